"""include/lio_odom_batch.h (the scan-to-scan odometry of many sensors through one launch chain): the header, its binding, its argument
checks, and — on the CPU oracle — that the sensors of tests/odom_batch_cases.py are what tests/test_gpu_odom_batch.py takes them for.
No GPU needed."""
import ctypes
import os
import re
import subprocess

from lio_amd import capi
import odom_batch_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_odom_batch_header_is_bound_exported_and_apart_from_the_other_headers(oracle):
    batch = _declared("lio_odom_batch.h")
    assert batch == ["lio_odom_process_batch"]
    assert set(batch) == set(capi._ODOM_BATCH_SIGS.keys())
    for other in ("lio_c.h", "lio_ext.h", "lio_test_hooks.h", "lio_full_cloud.h"):
        assert not set(batch) & set(_declared(other)), other
    assert not set(batch) & (set(capi._SIGS) | set(capi._TEST_SIGS) | set(capi._EXT_SIGS) | set(capi._FULL_SIGS))
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in batch:
        assert hasattr(dll, s), s
        assert not hasattr(oracle.dll, s), s                    # the oracle does not implement it ...
    assert oracle.missing == []                                  # ... and loading it keeps working
    text = open(os.path.join(ROOT, "include", "lio_odom_batch.h")).read()
    m = re.search(r"#define LIO_ODOM_BATCH_MAX_SENSORS (\d+)\b", text)
    assert m and int(m.group(1)) == capi.ODOM_BATCH_MAX_SENSORS >= 512
    assert '#include "lio_odom_batch.h"' not in open(os.path.join(ROOT, "include", "lio_c.h")).read()


def test_odom_batch_header_is_plain_c_links_and_checks_its_arguments_without_a_device(tmp_path):
    src = tmp_path / "batch.c"
    src.write_text('#include "lio_odom_batch.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   "  float p[4] = {1.f, 2.f, 3.f, 4.5f};\n"
                   "  const float *c[2] = {p, p};\n"
                   "  size_t n[2] = {1, 1};\n"
                   "  lio_odom *none[2] = {NULL, NULL};\n"
                   "  lio_transform_f T[2];\n"
                   "  int32_t it[2] = {7, 7};\n"
                   "  if (lio_odom_process_batch(NULL, 2, c, n, c, n, c, n, c, n, T, T, it, it) != LIO_ERR_ARG) return 1;   /* no handle array */\n"
                   "  if (lio_odom_process_batch(none, 0, c, n, c, n, c, n, c, n, T, T, it, it) != LIO_ERR_ARG) return 2;   /* n_sensors < 1 */\n"
                   "  if (lio_odom_process_batch(none, -3, c, n, c, n, c, n, c, n, T, T, it, it) != LIO_ERR_ARG) return 3;\n"
                   "  if (lio_odom_process_batch(none, 2, c, n, c, n, c, n, c, n, T, T, it, it) != LIO_ERR_ARG) return 4;   /* null entries */\n"
                   "  if (lio_odom_process_batch(none, 2, NULL, n, c, n, c, n, c, n, T, T, it, it) != LIO_ERR_ARG) return 5; /* a null array */\n"
                   "  if (lio_odom_process_batch(none, 2, c, n, c, n, c, NULL, c, n, T, T, it, it) != LIO_ERR_ARG) return 6;\n"
                   "  if (lio_odom_process_batch(none, LIO_ODOM_BATCH_MAX_SENSORS + 1, c, n, c, n, c, n, c, n, NULL, NULL, NULL, NULL) != LIO_ERR_CAPACITY) return 7;\n"
                   "  if (it[0] != 7 || it[1] != 7 || p[3] != 4.5f) return 8;\n"
                   '  printf("%s %d\\n", lio_backend(), LIO_ODOM_BATCH_MAX_SENSORS);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "batch_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
           "-l" + libname[3:-3], "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"hip-gfx950 {capi.ODOM_BATCH_MAX_SENSORS}" in r.stdout


def test_python_binding_rejects_an_empty_batch(hip):
    try:
        capi.PointOdometry.process_batch([], [])
    except capi.LioError:
        return
    raise AssertionError("an empty batch was accepted")


# ---------------------------------------------------------------- the sensors, on the oracle
def _steps(oracle, sensor):
    return [(r["iterations"], r["num_selected"], r["kz"]) for r in cases.run_alone(oracle, sensor)]


def test_the_sensor_kinds_do_on_the_oracle_what_the_gpu_test_takes_them_for(oracle):
    """iterations / selected rows / kz of lio_odom_process on the CPU oracle, per kind"""
    got = {s["name"]: _steps(oracle, s) for s in cases.mixed(oracle, 2)}
    for name, steps in got.items():
        print(f"{name:16s} {steps}")
    for j in range(3):                                           # all 25 iterations, 690 .. 755 rows
        for it, sel, kz in _steps(oracle, cases.moving(oracle, j, 3)):
            assert it == 25 and 690 <= sel <= 755 and kz == 0, (j, it, sel, kz)
    assert got["stationary"][0] == (1, 460, 0)                   # converges at once, then has to stay frozen for 24 iterations
    assert got["stationary"][1][0] == 1
    assert got["first_call"][0] == (0, 0, 0) and got["first_call"][1][0] == 25
    assert got["packer"] == [(0, 0, 0), (0, 0, 0)]
    assert got["short_previous"][0] == (0, 0, 0) and got["short_previous"][1][0] == 25
    assert got["minimal"] == [(25, 0, 0), (25, 0, 0)]            # fewer than 10 rows: no update, no convergence
    assert [len(c) for c in cases.minimal(oracle, 1)["steps"][0]] == [1, 11, 3, 101]
    assert got["no_queries"] == [(25, 0, 0), (25, 0, 0)]         # the iterations run, with zero selected rows
    for it, sel, kz in got["degenerate"]:
        assert it == 25 and sel >= 10 and kz > 0, (it, sel, kz)
    its = sorted(got[f"converging{i}"][0][0] for i in range(3))  # convergence in the middle of the loop, in three different peek intervals
    assert 5 < its[0] < 10 < its[1] < 15 and 20 < its[2] < 25, its


def test_short_previous_keeps_its_transform_es_on_the_oracle(oracle):
    s = cases.short_previous(oracle, 2)
    od = capi.PointOdometry(oracle, *s["params"])
    r0 = od.process(*s["prep"][0])
    r1 = od.process(*s["steps"][0])
    assert len(s["prep"][0][1]) == 10
    assert r1["T_es"][0].tobytes() == r0["T_es"][0].tobytes() and r1["T_es"][1].tobytes() == r0["T_es"][1].tobytes()


def test_partition_edges_have_the_query_counts_they_claim(oracle):
    ss = cases.partition_edges(oracle)
    nq = [len(s["steps"][0][0]) + len(s["steps"][0][2]) for s in ss]
    assert nq == [1, 255, 256, 257, 768, 16400] and nq[-1] > 64 * 256
    for s in ss:                                                 # previous clouds as they are: everybody iterates
        assert len(s["prep"][0][1]) > 10 and len(s["prep"][0][3]) > 100
        it, sel, kz = _steps(oracle, s)[0]
        assert it == 25 and sel <= nq[ss.index(s)], (s["name"], it, sel)
