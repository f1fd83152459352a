"""include/lio_map_batch.h (the scan-to-map step of many sensors through one launch chain): the header, its binding, the argument checks
that need no device, and that the sensors of tests/map_batch_cases.py are what tests/test_gpu_map_batch.py takes them for, on the CPU
oracle's PointMapping.  No GPU needed."""
import ctypes
import os
import re
import subprocess

from lio_amd import capi
import map_batch_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SENSORS = capi.MAP_BATCH_MAX_SENSORS                         # (the binding's view of LIO_MAP_BATCH_MAX_SENSORS)
OTHER_HEADERS = ("lio_c.h", "lio_ext.h", "lio_test_hooks.h", "lio_full_cloud.h", "lio_odom_batch.h", "lio_frontend_batch.h")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_map_batch_header_is_bound_exported_and_apart_from_the_other_headers(oracle):
    mine = _declared("lio_map_batch.h")
    assert mine == ["lio_map_process_batch"]
    assert set(mine) == set(capi._MAP_BATCH_SIGS.keys())
    for other in OTHER_HEADERS:
        assert not set(mine) & set(_declared(other)), other
        assert "lio_map_batch.h" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert not set(mine) & (set(capi._SIGS) | set(capi._TEST_SIGS) | set(capi._EXT_SIGS) | set(capi._FULL_SIGS) | set(capi._ODOM_BATCH_SIGS)
                            | set(capi._FRONTEND_SIGS))
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in mine:
        assert hasattr(dll, s), s
        assert not hasattr(oracle.dll, s), s                    # the oracle does not implement it ...
    assert oracle.missing == []                                  # ... and loading it keeps working
    assert hasattr(capi.PointMapping, "process_batch")
    text = open(os.path.join(ROOT, "include", "lio_map_batch.h")).read()
    assert int(re.search(r"#define\s+LIO_MAP_BATCH_MAX_SENSORS\s+(\d+)", text).group(1)) == MAX_SENSORS
    assert "lio_est_map" in text and "LIO_ERR_STATE" in text     # the refusal of an estimator's handle is documented


def test_map_batch_header_is_plain_c_links_and_checks_its_arguments_without_a_device(tmp_path):
    src = tmp_path / "map_batch.c"
    call = "lio_map_process_batch"
    src.write_text('#include "lio_map_batch.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   "  lio_map *none[2] = {NULL, NULL};\n"
                   "  int marker = 0;\n"
                   "  lio_map *some[2] = {(lio_map *)&marker, NULL};   /* never dereferenced: an argument check refuses the call before */\n"
                   "  const float *clouds[2] = {NULL, NULL};\n"
                   "  size_t zero[2] = {0, 0}, five[2] = {5, 0};\n"
                   "  lio_transform_f Ts[2], Ta[2];\n"
                   "  int32_t it[2] = {7, 7}, sel[2] = {9, 9};\n"
                   "  Ta[0].p[0] = 4.5f; Ta[1].q[3] = 2.5f; Ts[0].q[3] = 1.f; Ts[1].q[3] = 1.f;\n"
                   f"  if ({call}(NULL, 2, clouds, zero, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 1;       /* no handle array */\n"
                   f"  if ({call}(some, 1, NULL, zero, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 2;         /* no corner array */\n"
                   f"  if ({call}(some, 1, clouds, NULL, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 3;       /* no corner counts */\n"
                   f"  if ({call}(some, 1, clouds, zero, NULL, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 4;         /* no surf array */\n"
                   f"  if ({call}(some, 1, clouds, zero, clouds, NULL, Ts, Ta, it, sel) != LIO_ERR_ARG) return 5;       /* no surf counts */\n"
                   f"  if ({call}(some, 1, clouds, zero, clouds, zero, NULL, Ta, it, sel) != LIO_ERR_ARG) return 6;     /* no transform_sum */\n"
                   f"  if ({call}(none, 0, clouds, zero, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 7;       /* n_sensors < 1 */\n"
                   f"  if ({call}(none, -3, clouds, zero, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 8;\n"
                   f"  if ({call}(none, 2, clouds, zero, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 9;       /* null entries */\n"
                   f"  if ({call}(some, 2, clouds, zero, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 10;      /* the second entry is null */\n"
                   f"  if ({call}(some, 1, clouds, five, clouds, zero, Ts, Ta, it, sel) != LIO_ERR_ARG) return 11;      /* a null cloud with a count */\n"
                   f"  if ({call}(some, 1, clouds, zero, clouds, five, Ts, Ta, it, sel) != LIO_ERR_ARG) return 12;\n"
                   f"  if ({call}(none, LIO_MAP_BATCH_MAX_SENSORS + 1, clouds, zero, clouds, zero, Ts, NULL, NULL, NULL) != LIO_ERR_CAPACITY) return 13;\n"
                   "  if (it[0] != 7 || it[1] != 7 || sel[0] != 9 || sel[1] != 9 || Ta[0].p[0] != 4.5f || Ta[1].q[3] != 2.5f) return 14;   /* outputs untouched */\n"
                   '  printf("%s %d\\n", lio_backend(), LIO_MAP_BATCH_MAX_SENSORS);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "map_batch_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
           "-l" + libname[3:-3], "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"hip-gfx950 {MAX_SENSORS}" in r.stdout


def test_python_binding_rejects_an_empty_or_uneven_batch():
    for handles, inputs in (([], []), ([None], [])):
        try:
            capi.PointMapping.process_batch(handles, inputs)
        except capi.LioError:
            continue
        raise AssertionError("a batch without an input per handle was accepted")


# ---------------------------------------------------------------- the sensors, on the oracle's PointMapping
def _observe(m):
    cen, _ = m.cube_state()
    return dict(cen=cen, stack=(len(m.cloud(0)), len(m.cloud(1))), from_map=(len(m.cloud(2)), len(m.cloud(3))))


def test_the_sensor_kinds_are_what_their_names_say_on_the_oracle(oracle):
    """per kind and step on the oracle: iterations, filtered stack sizes, from-map sizes, cube centre"""
    n_steps = 2
    sensors = {s["name"]: s for s in cases.all_kinds(oracle, n_steps)}
    assert {s["kind"] for s in sensors.values()} == set(cases.KINDS)
    runs = {name: cases.run_alone(oracle, s, _observe) for name, s in sensors.items()}
    for name, run in runs.items():
        print(f"{name:12s} " + "  ".join(f"it {r['iterations']:2d} sel {r['num_selected']:5d} stack {o['stack']} from-map {o['from_map']} cen {o['cen']}" for r, o in run))
    max_it = capi.PointMapping(oracle).cfg.num_max_iterations
    for name in ("first_call", "small_map", "shifted"):          # gated: no round (a first call and a shifted window have no from-map cloud)
        assert [r["iterations"] for r, _ in runs[name][:1]] == [0], name
    assert all(r["iterations"] == 0 for r, _ in runs["small_map"])
    assert all(o["from_map"][0] <= 10 or o["from_map"][1] <= 100 for _, o in runs["small_map"])
    assert all(r["iterations"] == 0 for r, _ in runs["shifted"])
    for name in ("empty", "dry"):                                # the loop runs dry
        assert all(r["iterations"] == max_it for r, _ in runs[name]), name
        assert all(o["from_map"][0] > 10 and o["from_map"][1] > 100 for _, o in runs[name]), name
    assert all(o["stack"] == (0, 0) for _, o in runs["empty"])
    assert all(0 < sum(o["stack"]) <= 23 for _, o in runs["dry"])
    assert all(o["stack"][0] == 0 and o["stack"][1] > 0 and r["iterations"] > 0 for r, o in runs["no_corner"])
    for j in range(3):                                           # an iterating sensor needs > 10 corner and > 100 surf from-map points
        assert all(o["from_map"][0] > 10 and o["from_map"][1] > 100 and 0 < r["iterations"] for r, o in runs[f"moving{j}"]), j
    assert all(r["iterations"] > 0 for r, _ in runs["imu_inited"]) and sensors["imu_inited"]["init"] and len(sensors["imu_inited"]["prep"]) == 2
    assert sensors["first_call"]["prep"] == [] and runs["first_call"][1][0]["iterations"] > 0
    # the shift moves the window: the cube centre changes from step to step, and from the centre a handle that stays has
    cens = [o["cen"] for _, o in runs["shifted"]]
    assert cens[0] != runs["moving0"][0][1]["cen"] and cens[1] != cens[0], cens
    assert sorted(sensors["full_cloud"]["full"]) == [0] and len(sensors["full_cloud"]["full"][0]) == 257
    # the two sides of the step of odom_rows_blocks, with the margin
    assert all(sum(o["stack"]) <= cases.ROW_STEP - cases.MARGIN and r["iterations"] > 0 for r, o in runs["one_block"]), runs["one_block"]
    assert all(cases.ROW_STEP + cases.MARGIN <= sum(o["stack"]) <= 2 * cases.ROW_STEP and r["iterations"] > 0 for r, o in runs["two_blocks"]), runs["two_blocks"]
    # sensors that converge after different numbers of rounds share a call
    its = [[runs[f"moving{j}"][k][0]["iterations"] for j in range(3)] for k in range(n_steps)]
    assert any(len(set(row)) > 1 for row in its), its


def test_moving_sensors_with_their_own_filters_differ_in_iterations_on_the_oracle(oracle):
    """the three sensors of the second GPU test (their own filter sizes, 3 steps): at some step their iteration counts are not all equal"""
    runs = [cases.run_alone(oracle, cases.moving(oracle, j, 3, own_filters=True)) for j in range(3)]
    its = [[runs[j][k][0]["iterations"] for j in range(3)] for k in range(3)]
    print(its)
    assert all(i > 0 for row in its for i in row)
    assert any(len(set(row)) > 1 for row in its), its
