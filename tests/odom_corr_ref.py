"""Plain references of the scan-to-scan correspondence search (csrc/odometry.hip: k_ob_corr; test hook lio_odom_correspondences of
include/lio_test_hooks.h; PointOdometry.cc:237-259, :342-385, :440-494), written from the contract.  numpy only; no library of ours;
every previous point is looked at for every query, one query after the other.

  layer A   the contract in fp32 on a GIVEN sel (the one the implementation under test reports): equality with it is exact, no query
            left out.
  layer B   the same rule in fp64 on the same sel bits.  With u = 2^-24 an fp32 squared distance from fp32 inputs carries at most
            about 5 u relative error (one rounding per difference, squared; one per product; two additions of non-negative terms), so
            a comparison of two of them, or of one with the gate, can flip only below about 10 u = 6e-7 relative.  A slot is left out
            where the fp64 best and the runner-up, or the best and the gate 25, differ by less than MARGIN = 1e-5 relative and are NOT
            equal: an exact fp64 tie is decided by the tie rule, which both layers state (fp32 inputs make fp64 differences and
            squares exact, so an fp64 tie is a tie of the inputs — the same point twice, or a lattice).  A query whose closest is
            left out is left out whole.  Nothing else is exempt.
  to_start  TransformToStart in fp64 and in fp32, from the slerp and rotate helpers of tests/full_cloud_ref.py.
"""
import numpy as np

from full_cloud_ref import GPU_BOUND_FACTOR, K_DESKEW, _rotate, _slerp_from_identity, scale_of  # noqa: F401  (re-exported)

GATE = 25.0
MARGIN = 1e-5

# Worst |sel - to_start64|_inf / (2^-24 * (|p| + |t_es|)) of the ORACLE's lio_odom_correspondences over every case of
# tests/odom_corr_cases.py, as tests/test_odom_corr.py::test_oracle_sel_within_k_start measures it on the CPU (the run printed 2.154, in
# the case `deskew`), rounded up.  The product's k_odo_sel / k_ob_corr are held to GPU_BOUND_FACTOR x this, as the de-skew is to K_DESKEW
# (device acos, sin and the division each differ from libm by a few ulps).  Not measured on the code under test.
K_START = 2.2

PLANTS = ("runner_up", "behind_violation", "updown_tie_flip", "nn_tie_high", "gate_le", "round_ring", "surf_lt")


def _f32(a, cols=4):
    return np.ascontiguousarray(a, np.float32).reshape(-1, cols)


# ---------------------------------------------------------------- TransformToStart
def _to_start(xyzi, q_e, t_e, scan_period, no_deskew, dt):
    f32 = _f32(xyzi)
    w32 = f32[:, 3]
    with np.errstate(invalid="ignore"):
        ring32 = np.trunc(w32).astype(np.float32)
        tf32 = np.float32(1) / np.float32(scan_period)                 # time_factor_, a float member
        s32 = tf32 * (w32 - ring32)                                    # the ratio the pass-through test looks at is the fp32 one
        if no_deskew:
            s32 = np.zeros_like(s32)
        through = (s32 < 0) | (s32.astype(np.float64) > 1.001)
        a = f32.astype(dt)
        qe, te = np.asarray(q_e, np.float32).astype(dt), np.asarray(t_e, np.float32).astype(dt)
        s = dt(tf32) * (a[:, 3] - ring32.astype(dt))
        if no_deskew:
            s = np.zeros_like(s)
        p = a[:, :3] - s[:, None] * te[None, :]
        qs = _slerp_from_identity(s, qe, np.finfo(dt).eps)
        qc = np.concatenate([-qs[:, :3], qs[:, 3:4]], axis=1)          # the conjugate, not normalised (:254)
        v = _rotate(qc, p)
    v[through] = a[through, :3]
    return v, through


def to_start64(xyzi, q_e, t_e, scan_period=0.1, no_deskew=False):
    """-> (sel float64 n x 3, passes-through mask)"""
    return _to_start(xyzi, q_e, t_e, scan_period, no_deskew, np.float64)


def to_start32(xyzi, q_e, t_e, scan_period=0.1, no_deskew=False):
    v, through = _to_start(xyzi, q_e, t_e, scan_period, no_deskew, np.float32)
    assert v.dtype == np.float32
    return v, through


def start_ratio(sel, xyzi, q_e, t_e, scan_period=0.1, no_deskew=False):
    """max over the queries with a finite fp64 sel of |sel - to_start64|_inf / scale_of (0 when there is none)"""
    q = _f32(xyzi)
    want, _ = to_start64(q, q_e, t_e, scan_period, no_deskew)
    ok = np.isfinite(want).all(axis=1) & np.isfinite(q).all(axis=1)
    if not ok.any():
        return 0.0
    got = np.asarray(sel, np.float32).reshape(-1, 3).astype(np.float64)
    assert np.isfinite(got[ok]).all(), "a finite query has a non-finite sel"
    err = np.max(np.abs(got[ok] - want[ok]), axis=1)
    return float(np.max(err / scale_of(q[ok], t_e)))


# ---------------------------------------------------------------- the search, one query at a time
def _sqd(xyz, sel):
    d = xyz - sel[None, :]
    r = d[:, 0] * d[:, 0]
    r += d[:, 1] * d[:, 1]
    r += d[:, 2] * d[:, 2]
    return r


def _pick(dw, cand, le, skip=0):
    """the first minimum of the candidates' distances below the gate, in walk order -> position in the walk or -1; skip = 1: the runner-up"""
    with np.errstate(invalid="ignore"):
        ok = cand & ((dw <= GATE) if le else (dw < GATE))
    pos = np.nonzero(ok)[0]
    if pos.size <= skip:
        return -1
    order = pos[np.argsort(dw[pos], kind="stable")]
    return int(order[skip])


def _slot_sure(dw, cand):
    """layer B: is this slot's decision beyond rounding?"""
    d = dw[cand]
    if d.size == 0:
        return True
    best = d.min()
    if best != GATE and abs(best - GATE) < MARGIN * GATE:
        return False
    if best < GATE:
        rest = d[d > best]
        if rest.size and rest.min() - best < MARGIN * rest.min():
            return False
    return True


def search(cloud_xyzi, sel, corner, dt=np.float32, plant=None, query_ok=None, stats=None):
    """-> idx (m, 3) int32: closest, second, third (third is -1 for corner queries; -1 = missing).  dt = float64: layer B, which also
    returns sure (m, 3) bool.  sel: m x 3 float32, the bits under test.  query_ok: rows whose query was finite (default: all).
    stats: a dict that receives what the walks met (tests/odom_corr_cases.py asserts each case contains what it claims)."""
    c = _f32(cloud_xyzi)
    sel32 = np.ascontiguousarray(sel, np.float32).reshape(-1, 3)
    m, n = sel32.shape[0], c.shape[0]
    xyz = c[:, :3].astype(dt)
    with np.errstate(invalid="ignore"):
        ring = (np.rint(c[:, 3]) if plant == "round_ring" else np.trunc(c[:, 3])).astype(np.int64)
    idx = np.full((m, 3), -1, np.int32)
    sure = np.ones((m, 3), bool)
    ok_rows = np.isfinite(sel32).all(axis=1)
    if query_ok is not None:
        ok_rows &= np.asarray(query_ok, bool)
    le = plant == "gate_le"
    if stats is not None:
        for k in ("n_up", "n_down", "closest", "viol_up", "viol_down", "nn_tie", "tie_one_dir", "tie_two_dir", "tie_lanes", "tie_chunks",
                  "end_up", "end_down"):
            stats.setdefault(k, [])
    for i in range(m):
        if not ok_rows[i] or n == 0:
            continue
        d = _sqd(xyz, sel32[i].astype(dt))
        assert d.dtype == dt
        dmin = d.min()
        ties = np.nonzero(d == dmin)[0]
        closest = int(ties[-1] if plant == "nn_tie_high" else ties[0])
        if dt == np.float64:
            rest = d[d > dmin]
            if (dmin != GATE and abs(dmin - GATE) < MARGIN * GATE) or (dmin < GATE and rest.size and rest.min() - dmin < MARGIN * rest.min()):
                sure[i] = False
        if not (dmin <= GATE if le else dmin < GATE):
            continue
        cs = ring[closest]
        up, dn = ring[closest + 1:], ring[:closest][::-1]
        vu, vd = np.nonzero(up[:4096] > cs + 2.5)[0], np.nonzero(dn[:4096] < cs - 2.5)[0]     # (a window is rarely longer ...)
        if plant == "behind_violation" or (vu.size == 0 and up.size > 4096):
            vu = np.nonzero(up > cs + 2.5)[0]
        if plant == "behind_violation" or (vd.size == 0 and dn.size > 4096):
            vd = np.nonzero(dn < cs - 2.5)[0]
        if plant == "behind_violation":          # the violating points are skipped, the walk goes on
            ju = closest + 1 + np.nonzero(up[:8192] <= cs + 2.5)[0]
            jd = closest - 1 - np.nonzero(dn[:8192] >= cs - 2.5)[0]
        else:
            ju = closest + 1 + np.arange(vu[0] if vu.size else up.size)
            jd = closest - 1 - np.arange(vd[0] if vd.size else dn.size)
        if plant == "updown_tie_flip":
            walk, is_up = np.concatenate([jd, ju]), np.concatenate([np.zeros(jd.size, bool), np.ones(ju.size, bool)])
        else:
            walk, is_up = np.concatenate([ju, jd]), np.concatenate([np.ones(ju.size, bool), np.zeros(jd.size, bool)])
        rw, dw = ring[walk], d[walk]
        if corner:
            slots = [(is_up & (rw > cs)) | (~is_up & (rw < cs))]
        else:
            c2 = (is_up & ((rw < cs) if plant == "surf_lt" else (rw <= cs))) | (~is_up & (rw >= cs))
            slots = [c2, ~c2]
        idx[i, 0] = closest
        for k, cand in enumerate(slots):
            pos = _pick(dw, cand, le, 1 if (plant == "runner_up" and k == 0) else 0)
            if pos < 0 and plant == "runner_up" and k == 0:
                pos = _pick(dw, cand, le)
            idx[i, 1 + k] = walk[pos] if pos >= 0 else -1
            if dt == np.float64 and not _slot_sure(dw, cand):
                sure[i, 1 + k] = False
            if stats is not None and pos >= 0:
                tied = np.nonzero(cand & (dw == dw[pos]))[0]
                tied = tied[tied != pos]
                same = tied[is_up[tied] == is_up[pos]]
                off = lambda p: (walk[p] - closest - 1) if is_up[p] else (closest - 1 - walk[p])    # position inside its direction's walk
                stats["tie_one_dir"].append(same.size > 0)
                stats["tie_two_dir"].append((is_up[tied] != is_up[pos]).any())
                stats["tie_lanes"].append(any(off(p) % 64 != off(pos) % 64 for p in same))
                stats["tie_chunks"].append(any(off(p) // 64 != off(pos) // 64 for p in same))
        if stats is not None:
            stats["n_up"].append(ju.size); stats["n_down"].append(jd.size); stats["closest"].append(closest)
            stats["viol_up"].append(int(vu[0]) if vu.size else -1); stats["viol_down"].append(int(vd[0]) if vd.size else -1)
            stats["end_up"].append(vu.size == 0 and up.size > 0); stats["end_down"].append(vd.size == 0 and dn.size > 0)
            stats["nn_tie"].append(ties.size > 1)
    if corner:
        idx[:, 2] = -1
    if dt == np.float64:
        sure[~sure[:, 0]] = False
        return idx, sure
    return idx


def layer_a(case, sel, plant=None, stats=None):
    """-> (corner_idx (n_sharp, 2), surf_idx (n_flat, 3)) the hook must return for this sel"""
    nc = case.sharp.shape[0]
    ok = np.isfinite(np.concatenate([case.sharp, case.flat])[:, :3]).all(axis=1)
    sel = np.ascontiguousarray(sel, np.float32).reshape(-1, 3)
    sc = None if stats is None else stats.setdefault("corner", {})
    ss = None if stats is None else stats.setdefault("surf", {})
    a = search(case.last_corner, sel[:nc], True, plant=plant, query_ok=ok[:nc], stats=sc)
    b = search(case.last_surf, sel[nc:], False, plant=plant, query_ok=ok[nc:], stats=ss)
    return a[:, :2].copy(), b


def layer_b(case, sel):
    """-> ((corner idx (n_sharp, 2), sure), (surf idx (n_flat, 3), sure)) in fp64 on the same sel bits"""
    nc = case.sharp.shape[0]
    ok = np.isfinite(np.concatenate([case.sharp, case.flat])[:, :3]).all(axis=1)
    sel = np.ascontiguousarray(sel, np.float32).reshape(-1, 3)
    a, sa = search(case.last_corner, sel[:nc], True, dt=np.float64, query_ok=ok[:nc])
    b, sb = search(case.last_surf, sel[nc:], False, dt=np.float64, query_ok=ok[nc:])
    return (a[:, :2].copy(), sa[:, :2].copy()), (b, sb)


def compare(got, want):
    """got, want = (corner_idx, surf_idx).  Exact; raises AssertionError naming the first query that differs."""
    for kind, g, w in (("corner", got[0], want[0]), ("surf", got[1], want[1])):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == np.int32, (kind, g.shape, w.shape, g.dtype)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, f"{kind} indices differ at {bad.size} of {g.shape[0]} queries; first: query {bad[0]} got {g[bad[0]]} want {w[bad[0]]}"
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def compare_b(got, ref_b, cap):
    """got = (corner_idx, surf_idx) against layer_b(...) -> (queries, queries with a slot left out).  Raises when a compared slot is not
    the fp64 one, or when more than `cap` (a share) of the queries had a slot left out."""
    n, n_out = 0, 0
    for kind, g, (w, sure) in (("corner", got[0], ref_b[0]), ("surf", got[1], ref_b[1])):
        g = np.asarray(g)
        assert g.shape == w.shape
        wrong = sure & (g != w)
        bad = np.nonzero(wrong.any(axis=1))[0]
        assert bad.size == 0, f"{kind}: not the fp64 choice at {bad.size} queries; first: query {bad[0]} got {g[bad[0]]} fp64 {w[bad[0]]} sure {sure[bad[0]]}"
        n += g.shape[0]
        n_out += int((~sure).any(axis=1).sum())
    assert n_out <= cap * n, f"layer B leaves out {n_out} of {n} queries, more than the cap {cap}"
    return n, n_out
