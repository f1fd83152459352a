"""include/lio_ext.h (the product's entry points beyond the shared ABI: map refresh, surround map) and the plain-Python
model of the optimisation-window ring (tests/map_refresh_ref.py).  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

from lio_amd import capi
from map_refresh_ref import RefreshModel, opt_pose0, quat_from_rot, rot_from_quat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))


def test_ext_header_is_bound_exported_and_apart_from_the_shared_abi():
    ext = _declared("lio_ext.h")
    assert set(ext) == {"lio_est_map", "lio_est_set_map_refresh", "lio_est_refresh_map", "lio_map_get_surround", "lio_est_get_last_map_refresh"}
    assert set(ext) == set(capi._EXT_SIGS.keys())
    assert not set(ext) & set(_declared("lio_c.h"))
    assert not set(ext) & set(_declared("lio_test_hooks.h"))
    assert not set(ext) & (set(capi._SIGS) | set(capi._TEST_SIGS))
    dll = ctypes.CDLL(capi.HIP_LIB_PATH)
    for s in ext:
        assert hasattr(dll, s), s


def test_ext_symbols_are_not_demanded_of_the_oracle(oracle):
    """the oracle does not implement them, and loading it keeps working"""
    assert oracle.missing == [] and not oracle.has_ext
    for s in capi._EXT_SIGS:
        assert not hasattr(oracle.dll, s), s


def test_ext_header_is_plain_c_and_links_against_the_product(tmp_path):
    src = tmp_path / "ext.c"
    src.write_text('#include "lio_ext.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   "  int applied = 7;\n"
                   "  if (lio_est_map(NULL) != NULL) return 1;\n"
                   "  if (lio_est_set_map_refresh(NULL, 1) != LIO_ERR_ARG) return 2;\n"
                   "  if (lio_est_refresh_map(NULL) != LIO_ERR_ARG) return 3;\n"
                   "  if (lio_map_get_surround(NULL, 0.6f, NULL) != 0) return 4;\n"
                   "  if (lio_est_get_last_map_refresh(NULL, &applied, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != LIO_ERR_ARG || applied != 7) return 5;\n"
                   '  printf("%s\\n", lio_backend());\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "ext_check"
    libdir, libname = os.path.dirname(capi.HIP_LIB_PATH), os.path.basename(capi.HIP_LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
           "-l" + libname[3:-3], "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "hip-gfx950" in r.stdout


# ---------------------------------------------------------------- the model on hand-written sequences
def _ident():
    return (np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32))


def test_ring_fills_and_refresh_waits_for_a_full_ring():
    m = RefreshModel(W=4, Wo=2, deskew=False)
    m.seed_window([f"w{i}" for i in range(5)])
    assert m.refresh() is None and m.slot0() is None
    for k in range(2):
        m.push(_ident(), [10, 10, 5], [k], f"s{k}", f"c{k}")
        assert m.refresh() is None                       # :626 — two of three slots
    m.push(_ident(), [10, 10, 5], [2], "s2", "c2")
    a = m.refresh()
    assert a["surf"] == "s0" and a["corner"] == "c0" and a["valid_idx"] == [0]
    m.push(_ident(), [9, 10, 5], [3], "s3", "c3")
    a = m.refresh()
    assert a["surf"] == "s1" and a["cube_center"] == [10, 10, 5] and a["valid_idx"] == [1]     # the centre AT PUSH TIME, stale by now


def test_deskew_on_holds_the_previous_frames_stacks():
    """:484 runs before :689: an initialised step's slot holds what surf_stack_.last() was BEFORE this frame's stack went in"""
    m = RefreshModel(W=4, Wo=2, deskew=True)
    m.seed_window([f"w{i}" for i in range(5)])
    for k in range(3):
        m.push(_ident(), [10, 10, 5], [k], f"s{k}", f"c{k}")
    a = m.refresh()
    assert a["surf"] == "w4" and a["valid_idx"] == [0]          # frame 0's slot: the window's newest cloud before frame 0
    assert len(a["corner"]) == 0                                 # the injected window has no corner clouds
    m.push(_ident(), [10, 10, 5], [3], "s3", "c3")
    a = m.refresh()
    assert a["surf"] == "s0" and a["corner"] == "c0" and a["valid_idx"] == [1]
    # with de-skew off the same sequence pairs every slot with its own frame
    n = RefreshModel(W=4, Wo=2, deskew=False)
    n.seed_window([f"w{i}" for i in range(5)])
    for k in range(4):
        n.push(_ident(), [10, 10, 5], [k], f"s{k}", f"c{k}")
    assert n.refresh()["surf"] == "s1"


def test_uninitialised_steps_push_their_own_stacks_even_with_deskew_on():
    m = RefreshModel(W=4, Wo=2, deskew=True)
    for k in range(3):
        m.push(_ident(), [10, 10, 5], [k], f"s{k}", f"c{k}")   # :474: stage_flag_ != INITED
        m.end_uninitialised_step()
    assert m.slot0()["surf"] == "s0" and m.refresh() is None     # full, but masked


def test_initialising_steps_mask_reaches_slot_0_exactly_wo_solves_later():
    W, Wo = 4, 2
    m = RefreshModel(W, Wo, deskew=False)
    for k in range(W + 1):                                       # the last of them initialises (:542-577) and still ends at :616
        m.push(_ident(), [10, 10, 5], [k], f"s{k}", f"c{k}")
        m.end_uninitialised_step(initialised=(k == W))
    assert m.inited and m.refresh() is None                      # the initialising step does not refresh
    results = []
    for k in range(W + 1, W + 1 + Wo + 2):
        m.push(_ident(), [10, 10, 5], [k], f"s{k}", f"c{k}")
        results.append(m.refresh())
    # solve j (1-based) after the initialising one sees slot 0 = the slot pushed Wo frames earlier: masked for j <= Wo - 1, and for
    # j == Wo it is the INITIALISING step's own slot: still skipped.  The first refresh is solve Wo + 1.
    assert [r is None for r in results] == [True] * Wo + [False, False]
    assert results[Wo]["valid_idx"] == [W + 1] and results[Wo]["surf"] == f"s{W + 1}"


def test_in_place_edits_reach_the_slot_that_holds_the_cloud():
    W, Wo = 4, 2
    m = RefreshModel(W, Wo, deskew=False)
    m.seed_window([f"w{i}" for i in range(5)])
    for k in range(3):
        m.push(_ident(), [10, 10, 5], [k], f"s{k}", f"c{k}")
        if k == 0:
            m.fuse_pivot("fused")                                # :1434 on window slot W - Wo = 2, which is w3 after one push
        # after push k the window is [.., s_k]; pivot + 1 = 3 holds frame k - 1 (or w4 for k = 0)
        m.slide(f"slid{k}")
    # frame 0 sat at window slot 4 after its push, slot 3 = pivot + 1 after the next: slide 1 rewrote it in place
    assert m.refresh()["surf"] == "slid1"
    assert m.surf_stack[2].pts == "slid1"                        # and it is the pivot's cloud now: the same object


def test_slot_0_pose_is_overwritten_by_every_solve():
    W, Wo = 4, 2
    m = RefreshModel(W, Wo, deskew=False)
    m.seed_window([f"w{i}" for i in range(5)])
    m.push(("qin", "pin"), [10, 10, 5], [0], "s0", "c0")
    rng = np.random.default_rng(5)
    Rs = np.stack([rot_from_quat(q / np.linalg.norm(q)) for q in rng.normal(size=(W + 1, 4))])
    Ps = rng.normal(size=(W + 1, 3))
    q_lb = np.array([0.02, -0.01, 0.03, 0.999], np.float32)      # not unit: conjugate().normalized() matters
    t_lb = np.array([0.1, -0.2, 0.05], np.float32)
    m.solved(Rs, Ps, q_lb, t_lb)
    q, p = m.slot0()["T"]
    assert q.dtype == np.float32 and p.dtype == np.float32
    # T_l0 = T_b(W - Wo) * T_lb^-1: composing it with the (normalised) extrinsic gives the body pose back
    qn = q_lb.astype(np.float64) / np.linalg.norm(q_lb.astype(np.float64))
    np.testing.assert_allclose(rot_from_quat(q.astype(np.float64)) @ rot_from_quat(qn), Rs[W - Wo], atol=1e-6)
    np.testing.assert_allclose(rot_from_quat(q.astype(np.float64)) @ t_lb.astype(np.float64) + p, Ps[W - Wo], atol=1e-6)
    q2, p2 = opt_pose0(Rs, Ps, q_lb, t_lb, W, Wo)
    np.testing.assert_array_equal(q, q2), np.testing.assert_array_equal(p, p2)


def test_quaternion_extraction_takes_every_branch():
    for axis in range(3):
        v = np.zeros(4)
        v[axis], v[3] = 1.0, 0.05                                 # near-180-degree turns: trace < 0
        v /= np.linalg.norm(v)
        q = quat_from_rot(rot_from_quat(v))
        assert min(np.abs(q - v).max(), np.abs(q + v).max()) < 1e-12
