"""include/lio_est_push_batch.h (PushFrame / SlideWindow / ProcessLaserOdom of the windows of a batch through one launch chain): the header as
C99, its exports and binding, the argument checks that need no device, what the product answers without a device, and that the crafted clouds of
tests/est_push_cases.py are what tests/test_gpu_est_push_batch.py takes them for, on the CPU oracle's filter.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

from lio_amd import capi
import est_push_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["lio_est_batch_process_laser_odom", "lio_est_batch_push_frames", "lio_est_batch_push_stats", "lio_est_batch_slide_windows"]
OTHER_HEADERS = ("lio_c.h", "lio_ext.h", "lio_test_hooks.h", "lio_full_cloud.h", "lio_odom_batch.h", "lio_frontend_batch.h", "lio_map_batch.h",
                 "lio_map_from_odom.h")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_header_is_bound_exported_and_apart_from_the_other_headers(oracle):
    assert _declared("lio_est_push_batch.h") == CALLS
    assert set(CALLS) == set(capi._EST_PUSH_SIGS.keys())
    for other in OTHER_HEADERS:
        assert not set(CALLS) & set(_declared(other)), other
        assert "lio_est_push_batch.h" not in open(os.path.join(ROOT, "include", other)).read(), other
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in CALLS:
        assert hasattr(dll, s), s
        assert not hasattr(oracle.dll, s), s                    # the oracle does not implement them ...
    assert oracle.missing == []                                  # ... and loading it keeps working
    hip = capi.load_hip()
    for s in CALLS:                                              # attached with their signatures
        assert getattr(hip.dll, s).restype is ctypes.c_int and getattr(hip.dll, s).argtypes == capi._EST_PUSH_SIGS[s][1], s
    for method in ("push_frames", "slide", "process_laser_odom", "push_stats"):
        assert callable(getattr(capi.EstimatorBatch, method)), method
    # the binding's frame is the header's: six fields in its order, no padding surprises
    text = open(os.path.join(ROOT, "include", "lio_est_push_batch.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} lio_est_frame;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in capi.EstFrame._fields_]
    assert ctypes.sizeof(capi.EstFrame) == ctypes.sizeof(capi.TransformF) + 4 + 4 * 8 + 8   # 7 floats, padding to 8, two pointers, two counts, the stamp


def test_header_is_plain_c_links_and_checks_its_arguments_without_a_device(tmp_path):
    exe = tmp_path / "est_push_batch_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "est_push_batch_check.c"), "-o", str(exe), "-L", libdir, "-l" + libname[3:-3],
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"hip-gfx950 {ctypes.sizeof(capi.EstFrame)}" in r.stdout


def test_binding_builds_the_frames_and_checks_their_number(hip):
    T = cases.ident_T()
    surf = np.arange(12, dtype=np.float32).reshape(3, 4)
    arr, keep = capi.EstimatorBatch.frames([(T, surf, np.zeros((0, 4), np.float32), 1.5), (T, np.zeros((0, 4)), surf[:2], 2.5)])
    assert (arr[0].n_surf, arr[0].n_corner, arr[1].n_surf, arr[1].n_corner) == (3, 0, 0, 2)
    assert not arr[0].corner_xyzi and not arr[1].surf_xyzi       # an empty cloud goes as a null pointer with a zero count
    assert [arr[0].surf_xyzi[i] for i in range(12)] == list(range(12)) and arr[1].corner_xyzi[7] == 7.0
    assert (arr[0].stamp, arr[1].stamp) == (1.5, 2.5) and arr[1].transform_in.q[3] == 1.0
    assert hip.dll.lio_est_batch_push_frames(None, arr) == -1 and hip.dll.lio_est_batch_process_laser_odom(None, arr, None) == -1


def test_without_a_device_no_batch_exists_and_nothing_is_computed(hip):
    """The new calls work on a lio_est_batch, and without a GPU the product makes neither an estimator nor a batch (lio_est_create and
    lio_est_batch_create answer null; the data path answers LIO_ERR_DEVICE, tests/test_abi.py): there is no handle on which they could compute
    on the CPU, and on no handle they answer LIO_ERR_ARG."""
    import torch

    if torch.cuda.is_available():
        return
    cfg = hip.default_est_config()
    assert not hip.dll.lio_est_create(ctypes.byref(cfg))
    none = (ctypes.c_void_p * 1)(None)
    assert not hip.dll.lio_est_batch_create(none, 1)
    out, n = np.zeros((4, 4), np.float32), ctypes.c_size_t(0)
    assert hip.dll.lio_voxel_grid(out.ctypes.data_as(capi.c_float_p), 4, 0.4, out.ctypes.data_as(capi.c_float_p), ctypes.byref(n)) == -3   # LIO_ERR_DEVICE
    arr, keep = capi.EstimatorBatch.frames([(cases.ident_T(), out, out, 0.0)])
    assert hip.dll.lio_est_batch_push_frames(None, arr) == -1
    assert hip.dll.lio_est_batch_slide_windows(None) == -1


# ---------------------------------------------------------------- the crafted clouds, on the oracle's filter
def test_the_crafted_clouds_are_what_their_names_say_on_the_oracle(oracle):
    leaf = cases.LEAF
    # the two clouds the chain flags: beyond the 9-bit z key the filter still is a filter; PCL's overflow hands the input back
    far = cases.beyond_the_key()
    out = oracle.voxel_grid(far, leaf)
    assert np.floor(150.0 / leaf) > 254 and len(out) < len(far) and np.sum(out[:, 2] > 149.0) == 1
    big = cases.pcl_overflow()
    out = oracle.voxel_grid(big, leaf)
    np.testing.assert_array_equal(cases.bits(out), cases.bits(big))
    span = np.floor(4e5 / leaf) + 1
    assert span ** 3 > 2 ** 31
    # the edges: sizes, one voxel, faces, non-finite coordinates
    assert [len(cases.room(n, 100 + n)) for n in cases.BLOCK_EDGES] == list(cases.BLOCK_EDGES)
    assert len(oracle.voxel_grid(cases.one_voxel(), leaf)) == 1
    lat = cases.face_lattice()
    cells = lat[:, :3].astype(np.float64) / float(np.float32(leaf))
    assert np.max(np.abs(cells - np.round(cells))) < 1e-6        # every point on a face (to float rounding: which side it falls is the filter's to say)
    assert 13 * 13 * 5 // 8 <= len(oracle.voxel_grid(lat, leaf)) <= len(lat) // 2   # every point is there twice
    nf = cases.non_finite()
    bad = int(np.sum(~np.all(np.isfinite(nf[:, :3]), axis=1)))
    out = oracle.voxel_grid(nf, leaf)
    assert bad == 6 and np.all(np.isfinite(out)) and 0 < len(out) <= len(nf) - bad
