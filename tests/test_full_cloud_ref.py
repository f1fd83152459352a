"""include/lio_full_cloud.h (the full-resolution sweep on the device) and the plain-Python references its GPU tests use
(tests/full_cloud_ref.py, tests/full_cloud_cases.py).  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

from lio_amd import capi
import full_cloud_cases as cases
import full_cloud_ref as ref
from full_cloud_ref import FULL_MAP_FRAME, FULL_SENSOR_END, FULL_SENSOR_RAW, FullRingModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_BOUND = ref.GPU_BOUND_FACTOR * ref.K_DESKEW


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


# ---------------------------------------------------------------- the header
def test_full_cloud_header_is_bound_exported_and_apart_from_the_other_headers(oracle):
    full = _declared("lio_full_cloud.h")
    assert set(full) == {"lio_odom_full_to_end", "lio_map_set_full_cloud", "lio_map_get_full_cloud", "lio_est_set_full_cloud",
                         "lio_est_get_full_stack", "lio_est_get_registered_full", "lio_est_get_full_transform_es", "lio_deskew_to_end"}
    assert set(full) == set(capi._FULL_SIGS.keys())
    for other in ("lio_c.h", "lio_ext.h", "lio_test_hooks.h"):
        assert not set(full) & set(_declared(other)), other
    assert not set(full) & (set(capi._SIGS) | set(capi._TEST_SIGS) | set(capi._EXT_SIGS))
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in full:
        assert hasattr(dll, s), s
        assert not hasattr(oracle.dll, s), s                    # the oracle does not implement them ...
    assert oracle.missing == []                                  # ... and loading it keeps working
    assert (capi.FULL_MAP_FRAME, capi.FULL_SENSOR_RAW, capi.FULL_SENSOR_END) == (FULL_MAP_FRAME, FULL_SENSOR_RAW, FULL_SENSOR_END)
    text = open(os.path.join(ROOT, "include", "lio_full_cloud.h")).read()
    for name, val in (("LIO_FULL_MAP_FRAME", 1), ("LIO_FULL_SENSOR_RAW", 2), ("LIO_FULL_SENSOR_END", 3)):
        assert re.search(rf"#define {name} {val}\b", text), name


def test_full_cloud_header_is_plain_c_and_links_against_the_product(tmp_path):
    src = tmp_path / "full.c"
    src.write_text('#include "lio_full_cloud.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   "  int state = 7;\n"
                   "  size_t n = 9;\n"
                   "  float p[4] = {1.f, 2.f, 3.f, 4.5f};\n"
                   "  lio_transform_f T = {{0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};\n"
                   "  if (lio_odom_full_to_end(NULL, p, 1, p) != LIO_ERR_ARG) return 1;\n"
                   "  if (lio_map_set_full_cloud(NULL, p, 1) != LIO_ERR_ARG) return 2;\n"
                   "  if (lio_map_get_full_cloud(NULL, NULL) != 0) return 3;\n"
                   "  if (lio_est_set_full_cloud(NULL, 1) != LIO_ERR_ARG) return 4;\n"
                   "  if (lio_est_get_full_stack(NULL, 0, NULL, &state) != 0 || state != 7) return 5;\n"
                   "  if (lio_est_get_registered_full(NULL, 0, NULL, &n, NULL) != LIO_ERR_ARG || n != 9) return 6;\n"
                   "  if (lio_est_get_full_transform_es(NULL, 0, &T) != LIO_ERR_ARG) return 7;\n"
                   "  if (lio_deskew_to_end(p, 1, NULL, 10.f, 1, p) != LIO_ERR_ARG) return 8;\n"
                   "  if (lio_deskew_to_end(p, 1, &T, 10.f, 2, p) != LIO_ERR_ARG) return 9;\n"
                   "  if (lio_deskew_to_end(NULL, 1, &T, 10.f, 1, p) != LIO_ERR_ARG) return 10;\n"
                   "  if (lio_deskew_to_end(NULL, 0, &T, 10.f, 1, NULL) != LIO_OK) return 11;   /* n == 0: nothing to do, no device needed */\n"
                   "  if (p[0] != 1.f || p[3] != 4.5f) return 12;\n"
                   '  printf("%s %d\\n", lio_backend(), LIO_FULL_SENSOR_END);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "full_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
           "-l" + libname[3:-3], "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "hip-gfx950 3" in r.stdout


# ---------------------------------------------------------------- the ring model on hand-written sequences
def test_pre_init_entries_are_map_frame_and_never_corrected():
    W, Wo = 4, 2
    m = FullRingModel(W, Wo)
    assert m.entry(0) is None and m.local_full_points() is None
    for k in range(3):
        m.push(f"reg{k}", inited=False)
        assert not m.solved()                                    # nothing to correct: the reference's call is a no-op there
    assert [m.entry(i)["state"] for i in range(3)] == [FULL_MAP_FRAME] * 3
    assert [m.entry(i)["cloud"] for i in range(3)] == ["reg0", "reg1", "reg2"]
    assert m.entry(3) is None and m.entry(-1) is None


def test_the_newest_entry_is_corrected_once():
    m = FullRingModel(4, 2)
    m.seed_window()
    m.push("raw0", inited=True, t_es="T0")
    assert m.entry(4)["state"] == FULL_SENSOR_RAW and m.entry(3) is None
    fix = lambda c, t: f"end({c},{t})"
    assert m.solved(fix)
    assert m.entry(4)["cloud"] == "end(raw0,T0)" and m.entry(4)["state"] == FULL_SENSOR_END
    assert not m.solved(fix) and not m.solved(fix)               # a repeated solve, solve_restored
    assert m.entry(4)["cloud"] == "end(raw0,T0)" and m.entry(4)["corrections"] == 1
    m.push("raw1", inited=True, t_es="T1")
    assert m.entry(3)["cloud"] == "end(raw0,T0)" and m.entry(4)["state"] == FULL_SENSOR_RAW
    assert m.solved(fix) and m.entry(3)["corrections"] == 1 and m.entry(4)["cloud"] == "end(raw1,T1)"


def test_local_full_points_is_pivot_plus_one_and_the_ring_wraps_after_w_plus_1_pushes():
    W, Wo = 4, 2
    m = FullRingModel(W, Wo)
    m.seed_window()
    for k in range(W + 1):
        m.push(f"c{k}", inited=True)
        m.solved()
        want = k - (W - (W - Wo + 1))                            # frame pivot + 1 is W - (pivot + 1) = 1 push behind the newest
        got = m.local_full_points()
        assert (got["cloud"] if got else None) == (f"c{want}" if want >= 0 else None)
    assert [m.entry(i)["cloud"] for i in range(W + 1)] == [f"c{k}" for k in range(W + 1)]
    m.push("c5", inited=True)                                    # push W + 2: c0 is evicted
    assert [m.entry(i)["cloud"] for i in range(W + 1)] == ["c1", "c2", "c3", "c4", "c5"]
    assert m.local_full_points()["cloud"] == "c4"


def test_entries_from_before_an_injected_window_stay_aligned_to_the_newest_frame_and_restore_drops():
    W, Wo = 4, 2
    m = FullRingModel(W, Wo)
    for k in range(3):
        m.push(f"reg{k}", inited=False)
    m.seed_window()
    assert [m.entry(i) and m.entry(i)["cloud"] for i in range(W + 1)] == [None, None, "reg0", "reg1", "reg2"]
    m.push("raw", inited=True)
    assert [m.entry(i) and m.entry(i)["cloud"] for i in range(W + 1)] == [None, "reg0", "reg1", "reg2", "raw"]
    m.restore()
    assert all(m.entry(i) is None for i in range(W + 1)) and not m.solved()


# ---------------------------------------------------------------- the arithmetic
def _ratios(form, keep):
    worst = {}
    for name, c, q, t in cases.all_cases():
        got = ref.to_end32(c, q, t, cases.TIME_FACTOR, form, keep)
        worst[name] = ref.worst_ratio(got[:, :3], c, q, t, time_factor=cases.TIME_FACTOR, form=form, keep_intensity=keep)
    return worst


def test_cases_cover_what_they_claim():
    fe = np.finfo(np.float32).eps
    names = [n for n, _, _ in cases.T_ES]
    assert names == ["identity", "below_threshold", "small", "large", "negative_w", "off_unit"]
    T = {n: (q, t) for n, q, t in cases.T_ES}
    assert abs(T["below_threshold"][0][3]) >= np.float32(1) - fe > abs(T["small"][0][3])
    assert T["negative_w"][0][3] < 0
    assert abs(np.linalg.norm(T["off_unit"][0].astype(np.float64)) - 1.001) < 1e-6
    assert abs(2 * np.arccos(T["large"][0][3]) - 1.0) < 1e-3 and abs(np.linalg.norm(T["large"][1]) - 3.0) < 0.1
    assert [len(cases.cloud(n)) for n in cases.SIZES] == [0, 1, 255, 256, 257, 2049]
    c = cases.cloud(2049)
    r = np.linalg.norm(c[:, :3].astype(np.float64), axis=1)
    assert abs(r.max() - 120.0) < 1e-3 and abs(r.min() - 0.5) < 1e-4
    ring = np.trunc(c[:, 3])
    assert ring.min() == 0 and ring.max() == 63
    s = np.float32(cases.TIME_FACTOR) * (c[:, 3] - ring)
    assert s.dtype == np.float32
    assert np.sum(s == 0) >= 10 and np.sum(s == 1) >= 5 and np.sum(s > 1) >= 10 and s.max() <= 1 + 1e-3 and s.min() >= 0


def test_fp32_restatement_stays_within_k_deskew():
    """the tolerance-setting run: numpy float32 in the kernel's operation order against float64, every case, both forms"""
    est, odo = _ratios("est", True), _ratios("odo", False)
    for name in est:
        print(f"{name:24s} est {est[name]:6.3f}  odo {odo[name]:6.3f}")
    print(f"worst: est {max(est.values()):.3f}  odo {max(odo.values()):.3f}  K_DESKEW {ref.K_DESKEW}")
    assert max(est.values()) <= ref.K_DESKEW and max(odo.values()) <= ref.K_DESKEW
    assert max(max(est.values()), max(odo.values())) > ref.K_DESKEW / 2     # the constant is the measured one, not a loose guess


def test_the_two_estimator_forms_share_xyz_and_differ_in_the_intensity_only():
    for name, c, q, t in cases.all_cases():
        a, b = ref.to_end32(c, q, t, cases.TIME_FACTOR, "est", True), ref.to_end32(c, q, t, cases.TIME_FACTOR, "est", False)
        assert a[:, :3].tobytes() == b[:, :3].tobytes(), name
        assert a[:, 3].tobytes() == c[:, 3].tobytes(), name
        np.testing.assert_array_equal(b[:, 3], c[:, 3] - np.trunc(c[:, 3]))
        o = ref.to_end32(c, q, t, cases.TIME_FACTOR, "odo")
        np.testing.assert_array_equal(o[:, 3], np.trunc(c[:, 3]))


def test_identity_with_integer_intensities_is_an_exact_no_op():
    """Estimator.cc:575 and both de-skew switches off: transform_es_ is the constructed identity and s = 0"""
    ident_q, ident_t = cases.T_ES[0][1], cases.T_ES[0][2]
    for n in cases.SIZES:
        c = cases.integer_intensity_cloud(n)
        for form, keep in (("est", True), ("odo", False)):
            assert ref.to_end32(c, ident_q, ident_t, cases.TIME_FACTOR, form, keep).tobytes() == c.tobytes(), (n, form)
    # ... and under the identity x y z survive ANY intensity (the slerp of two identities stays on the w axis)
    c = cases.cloud(257)
    assert ref.to_end32(c, ident_q, ident_t, cases.TIME_FACTOR, "est", True).tobytes() == c.tobytes()


def test_planted_errors_exceed_the_gpu_bound():
    """each error an implementation could make shows on at least one case under the bound the GPU tests use"""
    def worst(plant, form="est"):
        w = 0.0
        for name, c, q, t in cases.all_cases():
            got = ref.to_end32(c, q, t, cases.TIME_FACTOR, form, True, plant=plant)
            w = max(w, ref.worst_ratio(got[:, :3], c, q, t, time_factor=cases.TIME_FACTOR, form=form, keep_intensity=True))
        return w

    assert worst(None) <= ref.K_DESKEW < GPU_BOUND
    for plant in ("no_conj", "no_st"):
        w = worst(plant)
        print(plant, w)
        assert w > GPU_BOUND, plant
    # the odometry form's non-normalised conjugate in the estimator form: shows on the off-unit q_e
    name, q, t = cases.T_ES[5]
    c = cases.cloud(257)
    got = ref.to_end32(c, q, t, cases.TIME_FACTOR, "est", True, plant="no_norm")
    w = ref.worst_ratio(got[:, :3], c, q, t, time_factor=cases.TIME_FACTOR, form="est", keep_intensity=True)
    print("no_norm", w)
    assert name == "off_unit" and w > GPU_BOUND
    # the fraction stripped in keep mode: an exact check on w
    got = ref.to_end32(c, q, t, cases.TIME_FACTOR, "est", True, plant="strip_in_keep")
    assert got[:, 3].tobytes() != c[:, 3].tobytes()


def test_rigid_map_and_lidar_pose_restatements():
    rng = np.random.default_rng(2)
    c = cases.cloud(257)
    q = rng.normal(size=4)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    t = np.array([12.5, -3.25, 0.75], np.float32)
    got = ref.rigid_map32(c, q, t)
    assert got.dtype == np.float32 and got[:, 3].tobytes() == c[:, 3].tobytes()
    from map_refresh_ref import rot_from_quat

    want = c[:, :3].astype(np.float64) @ rot_from_quat(q.astype(np.float64)).T + t.astype(np.float64)
    assert np.max(np.abs(got[:, :3] - want)) < 1e-4              # 120 m x a few float ulps
    assert ref.rigid_map32(c, [0, 0, 0, 1], [0, 0, 0]).tobytes() == c.tobytes()
    W, Wo = 4, 2
    Rs = np.stack([rot_from_quat(v / np.linalg.norm(v)) for v in rng.normal(size=(W + 1, 4))])
    Ps = rng.normal(size=(W + 1, 3))
    q_lb, t_lb = np.array([0.02, -0.01, 0.03, 0.999], np.float32), np.array([0.1, -0.2, 0.05], np.float32)
    from map_refresh_ref import opt_pose0

    a, b = ref.lidar_pose(Rs, Ps, q_lb, t_lb, W - Wo), opt_pose0(Rs, Ps, q_lb, t_lb, W, Wo)
    np.testing.assert_array_equal(a[0], b[0]), np.testing.assert_array_equal(a[1], b[1])
    qi, pi = ref.lidar_pose(Rs, Ps, q_lb, t_lb, W)
    qn = q_lb.astype(np.float64) / np.linalg.norm(q_lb.astype(np.float64))
    np.testing.assert_allclose(rot_from_quat(qi.astype(np.float64)) @ rot_from_quat(qn), Rs[W], atol=1e-6)
    np.testing.assert_allclose(rot_from_quat(qi.astype(np.float64)) @ t_lb.astype(np.float64) + pi, Ps[W], atol=1e-6)
