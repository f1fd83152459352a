"""include/lio_est_from_odom.h (the windows of an estimator batch fed from the odometry handles on the device): the header as C99, its
exports and binding, and the argument checks that need no device.  No GPU needed."""
import ctypes
import os
import re
import subprocess

from lio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["lio_est_batch_from_odom_stats", "lio_est_batch_process_compact_from_odom", "lio_est_batch_push_frames_from_odom"]
HEADER = "lio_est_from_odom.h"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_est_from_odom_header_is_bound_exported_and_apart_from_the_other_headers(oracle):
    assert _declared(HEADER) == CALLS
    assert set(CALLS) == set(capi._EST_FROM_ODOM_SIGS.keys())
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h") and f != HEADER)
    assert "lio_c.h" in others and "lio_est_push_batch.h" in others
    for other in others:                                         # every other header: no call twice, and none pulls this one in
        assert not set(CALLS) & set(_declared(other)), other
        assert HEADER not in open(os.path.join(ROOT, "include", other)).read(), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["lio_c.h"]   # it includes lio_c.h only
    for table in ("_SIGS", "_TEST_SIGS", "_EXT_SIGS", "_FULL_SIGS", "_ODOM_BATCH_SIGS", "_FRONTEND_SIGS", "_MAP_BATCH_SIGS", "_MAP_FROM_ODOM_SIGS",
                  "_EST_PUSH_SIGS", "_VOX_SORT_SIGS", "_SEG_BOUNDS_SIGS"):
        assert not set(CALLS) & set(getattr(capi, table)), table
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in CALLS:
        assert hasattr(dll, s), s
        assert not hasattr(oracle.dll, s), s                    # the oracle does not implement them ...
    assert oracle.missing == []                                  # ... and loading it keeps working
    hip = capi.load_hip()
    for s in CALLS:                                              # attached with their signatures
        assert getattr(hip.dll, s).restype is ctypes.c_int and getattr(hip.dll, s).argtypes == capi._EST_FROM_ODOM_SIGS[s][1], s
    for method in ("push_frames_from_odom", "process_compact_from_odom", "from_odom_stats"):
        assert callable(getattr(capi.EstimatorBatch, method)), method
    # the contract's refusals and limits are documented
    for word in ("LIO_ERR_ARG", "LIO_ERR_STATE", "LIO_ERR_CAPACITY", "LIO_ERR_DEVICE", "io_ratio", "lio_odom_full_to_end", "imu_factor"):
        assert word in text, word


def test_est_from_odom_header_is_plain_c_links_and_checks_its_arguments_without_a_device(tmp_path):
    exe = tmp_path / "est_from_odom_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    assert libname.startswith("lib") and libname.endswith(".so")
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "est_from_odom_check.c"), "-o", str(exe), "-L", libdir, "-l" + libname[3:-3],
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "hip-gfx950 8" in r.stdout


def test_null_arguments_are_refused_through_the_binding_without_a_device(hip):
    none = (ctypes.c_void_p * 1)(None)
    T, t = (capi.TransformF * 1)(), (ctypes.c_double * 1)(0.5)
    out = (ctypes.c_int * 8)(*([7] * 8))
    assert hip.dll.lio_est_batch_push_frames_from_odom(None, none, None, T, t) == -1
    assert hip.dll.lio_est_batch_process_compact_from_odom(None, none, None, t, None, None) == -1
    assert hip.dll.lio_est_batch_from_odom_stats(None, out) == -1 and list(out) == [7] * 8


class _Members:
    """what the binding's length checks read of an EstimatorBatch: they come before any handle is touched"""

    def __init__(self, n):
        self.members = [None] * n

    _sources = capi.EstimatorBatch._sources
    push_frames_from_odom = capi.EstimatorBatch.push_frames_from_odom
    process_compact_from_odom = capi.EstimatorBatch.process_compact_from_odom


def test_python_binding_rejects_uneven_array_lengths():
    b, T = _Members(2), capi.TransformF()
    calls = (lambda: b.push_frames_from_odom([], None, [T, T], [0.0, 0.1]),
             lambda: b.push_frames_from_odom([None], None, [T, T], [0.0, 0.1]),
             lambda: b.process_compact_from_odom([None, None, None], None, [0.0, 0.1]),
             lambda: b.process_compact_from_odom([], [], [0.0, 0.1]))
    for call in calls:
        try:
            call()
        except capi.LioError:
            continue
        raise AssertionError("arrays that do not hold one entry per window were accepted")


class _Handle:
    h = None


def test_python_binding_rejects_uneven_transforms_and_stamps():
    b, T, o = _Members(2), capi.TransformF(), _Handle()
    calls = (lambda: b.push_frames_from_odom([o, o], [o], [T, T], [0.0, 0.1]),
             lambda: b.push_frames_from_odom([o, o], None, [T], [0.0, 0.1]),
             lambda: b.push_frames_from_odom([o, o], None, [T, T], [0.0]),
             lambda: b.process_compact_from_odom([o, o], [o, o], [0.0]))
    for call in calls:
        try:
            call()
        except capi.LioError:
            continue
        raise AssertionError("arrays that do not hold one entry per window were accepted")
