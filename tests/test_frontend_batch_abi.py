"""include/lio_frontend_batch.h (the batched odometry fed from the feature extraction on the device): the header, its binding, its
argument checks, and that the inputs of tests/frontend_batch_cases.py are what tests/test_gpu_frontend_batch.py and
tests/test_gpu_odom_batch_grids.py take them for — the sensor kinds on the CPU oracle's PointProcessor (which the product equals bit for
bit), the crafted cell tables by restating grid_extent in numpy.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

from lio_amd import capi
import frontend_batch_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("lio_c.h", "lio_ext.h", "lio_test_hooks.h", "lio_full_cloud.h", "lio_odom_batch.h")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_frontend_header_is_bound_exported_and_apart_from_the_other_headers(oracle):
    front = _declared("lio_frontend_batch.h")
    assert front == ["lio_odom_process_batch_from_pp"]
    assert set(front) == set(capi._FRONTEND_SIGS.keys())
    for other in OTHER_HEADERS:
        assert not set(front) & set(_declared(other)), other
    assert not set(front) & (set(capi._SIGS) | set(capi._TEST_SIGS) | set(capi._EXT_SIGS) | set(capi._FULL_SIGS) | set(capi._ODOM_BATCH_SIGS))
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in front:
        assert hasattr(dll, s), s
        assert not hasattr(oracle.dll, s), s                    # the oracle does not implement it ...
    assert oracle.missing == []                                  # ... and loading it keeps working
    assert hasattr(capi.PointOdometry, "process_batch_from_pp")
    assert cases.grid_cells_max() >= 8 * 10 ** 4                 # an HDL-64E outdoor sweep (about 10^4 cells) is well inside
    for other in OTHER_HEADERS:
        assert "lio_frontend_batch.h" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_frontend_header_is_plain_c_links_and_checks_its_arguments_without_a_device(tmp_path):
    src = tmp_path / "frontend.c"
    src.write_text('#include "lio_frontend_batch.h"\n#include "lio_odom_batch.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   "  lio_odom *no_odom[2] = {NULL, NULL};\n"
                   "  lio_pp *no_pp[2] = {NULL, NULL};\n"
                   "  int marker = 0;\n"
                   "  lio_odom *some_odom[2] = {(lio_odom *)&marker, NULL};   /* never dereferenced: the entry behind it is null */\n"
                   "  lio_transform_f T[2];\n"
                   "  int32_t it[2] = {7, 7}, sel[2] = {9, 9};\n"
                   "  T[0].p[0] = 4.5f; T[1].q[3] = 2.5f;\n"
                   "  if (lio_odom_process_batch_from_pp(NULL, no_pp, 2, T, T, it, sel) != LIO_ERR_ARG) return 1;      /* no handle array */\n"
                   "  if (lio_odom_process_batch_from_pp(no_odom, NULL, 2, T, T, it, sel) != LIO_ERR_ARG) return 2;    /* no processor array */\n"
                   "  if (lio_odom_process_batch_from_pp(no_odom, no_pp, 0, T, T, it, sel) != LIO_ERR_ARG) return 3;   /* n_sensors < 1 */\n"
                   "  if (lio_odom_process_batch_from_pp(no_odom, no_pp, -3, T, T, it, sel) != LIO_ERR_ARG) return 4;\n"
                   "  if (lio_odom_process_batch_from_pp(no_odom, no_pp, 2, T, T, it, sel) != LIO_ERR_ARG) return 5;   /* null entries */\n"
                   "  if (lio_odom_process_batch_from_pp(some_odom, no_pp, 1, T, T, it, sel) != LIO_ERR_ARG) return 6; /* a null processor */\n"
                   "  if (lio_odom_process_batch_from_pp(no_odom, no_pp, LIO_ODOM_BATCH_MAX_SENSORS + 1, NULL, NULL, NULL, NULL) != LIO_ERR_CAPACITY) return 7;\n"
                   "  if (it[0] != 7 || it[1] != 7 || sel[0] != 9 || sel[1] != 9 || T[0].p[0] != 4.5f || T[1].q[3] != 2.5f) return 8;\n"
                   '  printf("%s %d %d\\n", lio_backend(), LIO_ODOM_BATCH_MAX_SENSORS, LIO_ODOM_BATCH_GRID_CELLS_MAX);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "frontend_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
           "-l" + libname[3:-3], "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"hip-gfx950 {capi.ODOM_BATCH_MAX_SENSORS} {cases.grid_cells_max()}" in r.stdout


def test_python_binding_rejects_an_empty_or_uneven_batch(hip):
    for handles, procs in (([], []), ([None], [])):
        try:
            capi.PointOdometry.process_batch_from_pp(handles, procs)
        except capi.LioError:
            continue
        raise AssertionError("a batch without a processor per handle was accepted")


# ---------------------------------------------------------------- the sensors, on the oracle's PointProcessor
def _counts(oracle, lid, sweep):
    pp = capi.PointProcessor(oracle, lid.lower_deg, lid.upper_deg, lid.rings)
    pp.process(sweep)
    return [len(pp.cloud(w)) for w in (1, 2, 3, 4)]


def test_the_sensor_kinds_are_what_their_names_say_on_the_oracle(oracle):
    """feature counts (sharp, less sharp, flat, less flat) of the sweeps every kind feeds, per kind"""
    sensors = {s["name"]: s for s in cases.mixed(2)}
    assert set(sensors) == {"moving0", "stationary", "first_call", "packer", "thin", "empty", "moving2", "hdl64"}
    counts = {name: dict(prep=[_counts(oracle, s["lidar"], x) for x in s["prep"]], steps=[_counts(oracle, s["lidar"], x) for x in s["steps"]])
              for name, s in sensors.items()}
    for name, c in counts.items():
        print(f"{name:12s} {c}")
    for j in range(3):                                           # an iterating sensor needs > 10 corner and > 100 surf points in its previous sweep
        s = cases.moving(j, 3)
        for x in s["prep"] + s["steps"]:
            c = _counts(oracle, s["lidar"], x)
            assert c[0] + c[2] == 768 and c[1] > 10 and c[3] > 100, (j, c)
    thin = counts["thin"]["prep"][0]
    assert 0 < thin[1] and 0 < thin[3] and (thin[1] <= 10 or thin[3] <= 100), thin   # some features, too few to iterate on
    assert all(c[1] > 10 and c[3] > 100 for c in counts["thin"]["steps"])
    assert len(sensors["empty"]["steps"][0]) == 0 and counts["empty"]["steps"][0] == [0, 0, 0, 0]
    assert counts["empty"]["steps"][1][1] > 10 and counts["empty"]["prep"][0][3] > 100
    assert sensors["first_call"]["prep"] == [] and sensors["packer"]["disable"] and not sensors["moving0"]["disable"]
    assert sensors["stationary"]["steps"][0] is sensors["stationary"]["prep"][0]
    assert sensors["hdl64"]["lidar"].rings == 64 and sensors["moving0"]["lidar"].rings == 16
    assert all(c[1] > 10 and c[3] > 100 and c[0] + c[2] == 3072 for c in counts["hdl64"]["prep"] + counts["hdl64"]["steps"])


# ---------------------------------------------------------------- the crafted cell tables, in numpy
def test_grid_extent_in_numpy_counts_the_cells_of_a_known_box():
    box = np.array([[0.1, 0.1, 0.1, 0], [9.9, 4.9, 0.2, 0], [np.nan, 1, 1, 0]], np.float32)   # cells 0..1 x 0..0 x 0..0, one border cell a side
    assert cases.grid_ncells(box) == 4 * 3 * 3
    assert cases.grid_ncells(box[:0]) == 27                      # a cloud without a finite point: bounds zeroed by the host


def test_the_crafted_previous_clouds_fall_on_their_side_of_the_limit(oracle):
    limit = cases.grid_cells_max()
    sensors = cases.grid_sensors(oracle, 3)
    assert [s["kind"] for s in sensors] == list(cases.GRID_KINDS)
    for s in sensors:
        for k, cl in enumerate(s["prep"] + s["steps"]):          # every sweep is the next step's previous sweep
            nc, ns = cases.grid_ncells(cl[1]), cases.grid_ncells(cl[3])
            print(f"{s['kind']:12s} sweep {k}: corner {nc} cells, surf {ns} cells, limit {limit}")
            assert cases.grid_side(s["kind"], nc, ns), (s["kind"], k, nc, ns, limit)
            assert len(cl[1]) > 10 and len(cl[3]) > 100          # every sensor iterates
    plain = cases.obc.sweeps(oracle, cases.T0S[1], 4)[0][3]
    long_x = sensors[1]["prep"][0][3]
    assert len(long_x) == len(plain) + 2 and np.array_equal(long_x[:-2], plain)
    assert np.array_equal(long_x[-2:, 3], np.repeat(plain[-1:, 3], 2))   # the outliers carry an existing point's intensity
    assert len(sensors[2]["prep"][0][3]) == len(cases.obc.sweeps(oracle, cases.T0S[2], 4)[0][3]) + 4
    assert len(sensors[3]["prep"][0][1]) == 11
