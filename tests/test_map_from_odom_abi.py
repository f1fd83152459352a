"""include/lio_map_from_odom.h (the batched scan-to-map step fed from the odometry on the device): the header, its binding and the argument
checks that need no device.  No GPU needed."""
import ctypes
import os
import re
import subprocess

from lio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_HEADERS = ("lio_c.h", "lio_ext.h", "lio_test_hooks.h", "lio_full_cloud.h", "lio_odom_batch.h", "lio_frontend_batch.h", "lio_map_batch.h")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_map_from_odom_header_is_bound_exported_and_apart_from_the_other_headers(oracle):
    mine = _declared("lio_map_from_odom.h")
    assert mine == ["lio_map_process_batch_from_odom"]
    assert set(mine) == set(capi._MAP_FROM_ODOM_SIGS.keys())
    for other in OTHER_HEADERS:
        assert not set(mine) & set(_declared(other)), other
        assert "lio_map_from_odom.h" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert not set(mine) & (set(capi._SIGS) | set(capi._TEST_SIGS) | set(capi._EXT_SIGS) | set(capi._FULL_SIGS) | set(capi._ODOM_BATCH_SIGS)
                            | set(capi._FRONTEND_SIGS) | set(capi._MAP_BATCH_SIGS))
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in mine:
        assert hasattr(dll, s), s
        assert not hasattr(oracle.dll, s), s                    # the oracle does not implement it ...
    assert oracle.missing == []                                  # ... and loading it keeps working
    assert hasattr(capi.PointMapping, "process_batch_from_odom")
    text = open(os.path.join(ROOT, "include", "lio_map_from_odom.h")).read()
    for word in ("lio_est_map", "LIO_ERR_STATE", "LIO_ERR_CAPACITY", "io_ratio", "lio_odom_full_to_end"):   # the contract's refusals and limits are documented
        assert word in text, word


def test_map_from_odom_header_is_plain_c_links_and_checks_its_arguments_without_a_device(tmp_path):
    exe = tmp_path / "map_from_odom_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    assert libname.startswith("lib") and libname.endswith(".so")
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "map_from_odom_check.c"), "-o", str(exe), "-L", libdir, "-l" + libname[3:-3],
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"hip-gfx950 {capi.MAP_BATCH_MAX_SENSORS}" in r.stdout


def test_python_binding_rejects_an_empty_or_uneven_batch():
    for handles, odoms, pps in (([], [], None), ([None], [], None), ([None], [None], [])):
        try:
            capi.PointMapping.process_batch_from_odom(handles, odoms, pps)
        except capi.LioError:
            continue
        raise AssertionError("a batch without an odometry per handle was accepted")
