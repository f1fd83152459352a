"""Plain references of the 6x6 Gauss-Newton loops from the rows onward (csrc/cloud_device.h: odom_row_form, fold_partials28_wide,
odom_update_from_sums; csrc/cloud_kernels.h: reduce_partials28; csrc/odometry.hip: odo_update_step; the test hooks lio_gn_rows_map,
lio_gn_fold, lio_gn_step and lio_gn_round of include/lio_test_hooks.h), written from the definition of each operation.  numpy fp64 only;
no library of ours.  tests/test_gn.py holds the oracle to them (and sets the two constants below from what the ORACLE shows),
tests/test_gpu_gn.py the product, with the same functions.

Rows of the scan-to-map family, for a residual with coefficients (w, c) at the point p under the pose (q, t), R = R(q):
    a[0..2] = -(w^T R skew(p))                        forms 0 and 1
    a[0..2] = -(w^T R skew(p)) R^-1 diag(5e-3, 5e-3, 1)   form 2
    a[3..5] = w                                       a copy: equal in bits
    b       = -(w . (R p + t) + c)                    form 0
    b       = -c                                      forms 1 and 2: a copy, equal in bits
R(q) is Eigen's toRotationMatrix formula on the quaternion as given (fp32 values, not re-normalised: the loops do not normalise
either), R p its _transformVector formula, R^-1 the same matrix formula on conj(q) / |q|^2.

Scales (what one fp32 rounding of the largest intermediate is worth), per element, times ONE constant for the family:
    rotation columns      EPS32 * |w| * |p|           (x 5e-3, 5e-3, 1 in form 2)
    b of form 0           EPS32 * (|w| * (|p| + |t|) + |c|)
    copies                0: bits
C_MAP_ROWS is 4 x the largest error / scale the oracle's statement (GaussNewtonMapRow, oracle/liomath.h) shows over every case of
tests/gn_cases.py (tests/test_gn.py::test_oracle_rows_meet_fp64 prints and asserts it).

Rows of the scan-to-scan loop: odom_rows_ref below states the formulas and the scales; C_ODOM_ROWS is 4 x the largest error / scale of the
oracle's statement (PointOdometry::EdgeCoefficients, PlaneCoefficients, OdometryRow) over the cases
(tests/test_gn.py::test_oracle_odom_rows_meet_fp64).  A weight within C_ODOM_ROWS x err(s) of 0.1 leaves its query out of the `ok` comparison
against fp64, at most 1 % of a case.

Sums: column 27 is the row count, exactly.  Every other column is a sum of fp32 products widened to fp64; the hook's partials, added
exactly (math.fsum), against the exact sum of the fp32 products of the hook's own rows: any order of fp64 additions of n terms is within
(n - 1) * 2^-53 * sum |terms| of the exact sum (Jeannerod and Rump 2013, for recursive summation in any order; a blocked sum is a sum of
such sums over disjoint subsets, so the bound adds up to the same expression).  Derived, not measured.

Step: X = lstsq(A, g) on the fp32-rounded A^T A and A^T b in fp64; kz = the number of eigenvalues (eigvalsh) below the family's threshold,
decided at iter 0 and carried otherwise; X[:kz] = 0; t += X[3:]; q = q * (1, X[:3] / 2) or (1, X[:3] / 2) * q; the abort test on the
rotation between normalised(q_in) and q_out in degrees and on 100 |X[3:]|.  A backward-stable fp32 solve has a forward error of order
EPS32 * cond * |X|; C_QR is 4 x the largest |X - X_ref|_2 / (EPS32 * cond_2 * |X_ref|_2) the oracle's step (GaussNewtonStep,
oracle/liomath.h: colpiv_qr_solve<float>) shows over the cases whose state is the identity with t = 0, where q_out = (1, X / 2) and
t_out = X exactly, the rank-5 systems with cond of the kept 5 x 5 block included (tests/test_gn.py::test_oracle_step_meets_fp64).  The
same systems at a general pose are held to the composition (which side, which translation) with a margin of 100, not to the accuracy
of X again."""
import math

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
U64 = 2.0 ** -53
# 4 x the oracle's largest error / scale (tests/test_gn.py asserts 0.9 C <= 4 * top <= C for each)
C_MAP_ROWS = 4 * 2.83
C_QR = 4 * 0.7
C_ODOM_ROWS = 4 * 0.5

THRESHOLD = {0: 100.0, 1: 10.0}     # eigenvalue threshold of the degeneracy mask
ABORT = {0: 0.05, 1: 0.1}           # degrees and centimetres
MIN_ROWS_ODOM = 10


# ------------------------------------------------------------------------------------------------ rows
def rot_of(q_xyzw):
    """Eigen's toRotationMatrix on the quaternion as given"""
    x, y, z, w = (float(v) for v in q_xyzw)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def rotate(q_xyzw, p):
    """Eigen's _transformVector: v + w * 2 (u x v) + u x 2 (u x v)"""
    q = np.asarray(q_xyzw, np.float64)
    u, w = q[:3], q[3]
    uv = 2 * np.cross(np.broadcast_to(u, p.shape), p)
    return p + w * uv + np.cross(np.broadcast_to(u, p.shape), uv)


def skew_rows(p):
    """skew(p) for every row of p: (m, 3, 3)"""
    S = np.zeros(p.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -p[..., 2], p[..., 1]
    S[..., 1, 0], S[..., 1, 2] = p[..., 2], -p[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -p[..., 1], p[..., 0]
    return S


def map_rows_ref(form, stack_xyzi, valid, coeff, q_xyzw, t):
    """-> ok (m,) bool, rows (m, 7) fp64, scale (m, 7) fp64 (0 where the entry is a copy), copies (m, 7) bool"""
    p = np.asarray(stack_xyzi, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    co = np.asarray(coeff, np.float32).reshape(-1, 4).astype(np.float64)
    w, c = co[:, :3], co[:, 3]
    q = np.asarray(q_xyzw, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    m = p.shape[0]
    ok = np.asarray(valid).reshape(m) != 0
    R = rot_of(q)
    rows, scale, copies = np.zeros((m, 7)), np.zeros((m, 7)), np.zeros((m, 7), bool)
    a = -np.einsum("mi,ij,mjk->mk", w, R, skew_rows(p))
    wn, pn = np.linalg.norm(w, axis=1), np.linalg.norm(p, axis=1)
    col = np.ones(3)
    if form == 2:
        n2 = float(q @ q)
        Rinv = rot_of(np.r_[-q[:3], q[3]] / n2)
        col = np.array([5e-3, 5e-3, 1.0])
        a = (a @ Rinv) * col
    rows[:, :3] = a
    scale[:, :3] = EPS32 * (wn * pn)[:, None] * col
    rows[:, 3:6] = w
    copies[:, 3:6] = True
    if form == 0:
        rp = rotate(q, p)
        rows[:, 6] = -((w * (rp + t)).sum(axis=1) + c)
        scale[:, 6] = EPS32 * (wn * (pn + np.linalg.norm(t)) + np.abs(c))
    else:
        rows[:, 6] = -c
        copies[:, 6] = True
    rows[~ok], scale[~ok] = 0, 0
    return ok, rows, scale, copies


def rows_ratio(got_rows, ref):
    """largest |error| / scale over the entries that are not copies (0 for an empty case)"""
    ok, rows, scale, copies = ref
    sel = ok[:, None] & ~copies & (scale > 0)
    if not sel.any():
        return 0.0
    return float((np.abs(np.asarray(got_rows, np.float64) - rows)[sel] / scale[sel]).max())


def compare_rows(got, ref, C, what="rows"):
    """got = (ok, rows fp32) of a hook against map_rows_ref's answer"""
    ok, rows, scale, copies = ref
    g_ok, g_rows = np.asarray(got[0]) != 0, np.asarray(got[1], np.float32)
    bad = np.nonzero(g_ok != ok)[0]
    assert bad.size == 0, f"{what}: ok differs at {bad.size} of {ok.size} queries; first: query {bad[0]}"
    off = np.nonzero(g_rows[~ok].view(np.uint32).any(axis=1))[0]
    assert off.size == 0, f"{what}: a query without a row does not return zeros; first: the {off[0]}th of them"
    r32 = rows.astype(np.float32)      # a copy of an fp32 input is that input
    cp = ok[:, None] & copies
    bad = np.argwhere(cp & (g_rows.view(np.uint32) != r32.view(np.uint32)))
    assert bad.size == 0, f"{what}: a copied entry is not equal in bits at {len(bad)} entries; first: query {bad[0][0]} column {bad[0][1]}"
    err = np.abs(g_rows.astype(np.float64) - rows)
    bad = np.argwhere(ok[:, None] & ~copies & ~(err <= C * scale))
    assert bad.size == 0, (f"{what}: {len(bad)} entries beyond {C:.3g} x scale; first: query {bad[0][0]} column {bad[0][1]}: "
                          f"{g_rows[tuple(bad[0])]!r} vs {rows[tuple(bad[0])]!r}, scale {scale[tuple(bad[0])]:.3g}")


def compare_bits(a, b, what="results"):
    """two tuples of arrays, equal in shape and in every bit"""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: array {k}: {x.shape} {x.dtype} vs {y.shape} {y.dtype}"
        bx, by = x.view(np.uint8), y.view(np.uint8)
        bad = np.nonzero((bx != by).reshape(x.shape[0], -1).any(axis=1))[0] if x.ndim and x.shape[0] else np.zeros(0, int)
        assert bad.size == 0, f"{what}: array {k} differs in bits at {bad.size} of {x.shape[0]} rows; first: row {bad[0]}: {x[bad[0]]!r} vs {y[bad[0]]!r}"


def compare_rows_bits(a, b, what="rows"):
    """(ok, rows) of two libraries: ok equal, every finite entry equal in bits, the same entries NaN / +inf / -inf (the payload and sign of a
    NaN are the machine's)"""
    (oka, ra), (okb, rb) = ((np.asarray(x[0]), np.asarray(x[1], np.float32)) for x in (a, b))
    bad = np.nonzero(oka != okb)[0]
    assert bad.size == 0, f"{what}: ok differs at {bad.size} of {oka.size} queries; first: query {bad[0]}"
    na, nb = np.isnan(ra), np.isnan(rb)
    bad = np.argwhere(na != nb)
    assert bad.size == 0, f"{what}: NaN in different entries; first: query {bad[0][0]} column {bad[0][1]}: {ra[bad[0][0]]} vs {rb[bad[0][0]]}"
    same = (ra.view(np.uint32) == rb.view(np.uint32)) | na
    bad = np.argwhere(~same)
    assert bad.size == 0, (f"{what}: {len(bad)} entries differ in bits; first: query {bad[0][0]} column {bad[0][1]}: "
                          f"{ra[tuple(bad[0])]!r} vs {rb[tuple(bad[0])]!r}")
    return int(na.sum())


# ------------------------------------------------------------------------------------------------ rows of the scan-to-scan loop
class OdomRows:
    pass


def odom_rows_ref(sel, queries, n_sharp, last_corner, last_surf, corner_idx, surf_idx, q_xyzw, t, it):
    """The scan-to-scan rows in fp64 on the fp32 inputs, evaluated on the `sel` bits lio_odom_correspondences reports for the same inputs (sel
    itself is held to to_start64 by tests/odom_corr_ref.py): PointOdometry.cc:391-435 (edge), :497-531 (plane), A.7 (weight), :548-571 (row).
    -> an object with has (a row can exist: the indices are there), s, s_err, ok (s > 0.1 and distance != 0), rows (nq, 7), scale (nq, 7).

    Scales, to first order, of an fp32 evaluation of the same formulas on the same inputs (EPS32 = one rounding of a value of size 1):
      edge   d1 = sel - t1, d2 = sel - t2, e = t1 - t2, M = |d1| |d2|, a = |d1 x d2|, l = |e|.  The three cross terms each carry EPS32 M, so the
             unit vector (e x (d1 x d2)) / (a l) carries EPS32 (M / a + 1) — the conditioning of a line through a point close to it —, the
             distance ld2 = a / l carries EPS32 (M / l + ld2), and the weight s = 1 - 1.8 ld2 (iterations >= 5) 1.8 x that plus EPS32
      plane  e1 = t2 - t1, e2 = t3 - t1, E = |e1| |e2|, K = E / |e1 x e2| + 1: the unit normal carries EPS32 K, pd (of size |t1|) 2 EPS32 |t1| K, and
             pd2 = n . sel + pd, a difference of numbers of size |sel| and |t1|, EPS32 (K + 1) (|sel| + 2 |t1|); s = 1 - 1.8 |pd2| / |sel|^(1/2)
             carries 1.8 / |sel|^(1/2) x that plus EPS32 (1 + 1.8 |pd2| / |sel|^(1/2))
      w = s n and c3 = s d carry |s| err(n) + err(s) + EPS32 |s| and |s| err(d) + |d| err(s) + EPS32 |c3|
      row    cc = R^T (p - t) carries 2 EPS32 (|p| + |t|); r[0..2] = w^T skew(cc): err(w) |cc| + 2 EPS32 |w| (|p| + |t|) + EPS32 |w| |cc|;
             r[3..5] = -(w^T R^T): err(w) + 2 EPS32 |w|; b = -0.1 c3: 0.1 err(c3) + EPS32 |b|
    One constant for the family multiplies them: C_ODOM_ROWS, 4 x the largest error / scale of the oracle."""
    r = OdomRows()
    sel = np.asarray(sel, np.float32).astype(np.float64).reshape(-1, 3)
    P = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 4)[:, :3]
    nq = P.shape[0]
    lc, ls = (np.asarray(c, np.float32).astype(np.float64).reshape(-1, 4)[:, :3] for c in (last_corner, last_surf))
    ci, si = np.asarray(corner_idx).reshape(-1, 2), np.asarray(surf_idx).reshape(-1, 3)
    q = np.asarray(q_xyzw, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    has = np.zeros(nq, bool)
    has[:n_sharp] = ci[:, 1] >= 0
    has[n_sharp:] = (si[:, 1] >= 0) & (si[:, 2] >= 0)
    n_vec, dist, err_n, err_d, s_extra = np.zeros((nq, 3)), np.zeros(nq), np.zeros(nq), np.zeros(nq), np.zeros(nq)
    norm = lambda v: np.linalg.norm(v, axis=1)
    with np.errstate(all="ignore"):
        k = np.nonzero(has[:n_sharp])[0]
        if k.size:
            x0, t1, t2 = sel[k], lc[ci[k, 0]], lc[ci[k, 1]]
            d1, d2, e = x0 - t1, x0 - t2, t1 - t2
            mxy = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
            mxz = d1[:, 0] * d2[:, 2] - d2[:, 0] * d1[:, 2]
            myz = d1[:, 1] * d2[:, 2] - d2[:, 1] * d1[:, 2]
            a012, l12 = np.sqrt(mxy * mxy + mxz * mxz + myz * myz), norm(e)
            n_vec[k, 0] = (e[:, 1] * mxy + e[:, 2] * mxz) / a012 / l12
            n_vec[k, 1] = -(e[:, 0] * mxy - e[:, 2] * myz) / a012 / l12
            n_vec[k, 2] = -(e[:, 0] * mxz + e[:, 1] * myz) / a012 / l12
            dist[k] = a012 / l12
            M = norm(d1) * norm(d2)
            err_n[k] = EPS32 * (M / a012 + 1)
            err_d[k] = EPS32 * (M / l12 + dist[k])
            s_extra[k] = 0.0
        k = np.nonzero(has[n_sharp:])[0]
        if k.size:
            g = k + n_sharp
            x0, t1, t2, t3 = sel[g], ls[si[k, 0]], ls[si[k, 1]], ls[si[k, 2]]
            e1, e2 = t2 - t1, t3 - t1
            nr = np.cross(e1, e2)
            ps = norm(nr)
            n = nr / ps[:, None]
            pd = -(nr * t1).sum(axis=1) / ps
            n_vec[g] = n
            dist[g] = (n * x0).sum(axis=1) + pd
            K = norm(e1) * norm(e2) / ps + 1
            err_n[g] = EPS32 * K
            err_d[g] = EPS32 * (K + 1) * (norm(x0) + 2 * norm(t1))
        s = np.ones(nq)
        err_s = np.zeros(nq)
        if it >= 5:
            div = np.ones(nq)
            div[n_sharp:] = np.sqrt(norm(sel[n_sharp:]))
            s = 1 - 1.8 * np.abs(dist) / div
            err_s = 1.8 * err_d / div + EPS32 * (1 + 1.8 * np.abs(dist) / div)
        r.has, r.s, r.s_err, r.dist = has, s, err_s, dist
        r.ok = has & (s > 0.1) & (dist != 0)
        w = s[:, None] * n_vec
        c3 = s * dist
        err_w = np.abs(s) * err_n + err_s + EPS32 * np.abs(s)
        err_c3 = np.abs(s) * err_d + np.abs(dist) * err_s + EPS32 * np.abs(c3)
        cc = rotate(np.r_[-q[:3], q[3]], P - t)
        Rt = rot_of(q).T
        rows, scale = np.zeros((nq, 7)), np.zeros((nq, 7))
        rows[:, :3] = np.einsum("mi,mij->mj", w, skew_rows(cc))
        rows[:, 3:6] = -(w @ Rt)
        rows[:, 6] = -0.1 * c3
        wn, ccn, pt = norm(w), norm(cc), norm(P) + np.linalg.norm(t)
        scale[:, :3] = (err_w * ccn + 2 * EPS32 * wn * pt + EPS32 * wn * ccn)[:, None]
        scale[:, 3:6] = (err_w + 2 * EPS32 * wn)[:, None]
        scale[:, 6] = 0.1 * err_c3 + EPS32 * np.abs(rows[:, 6])
    rows[~r.ok], scale[~r.ok] = 0, 0
    r.rows, r.scale = rows, scale
    return r


def odom_decided(ref, C):
    """the queries whose `ok` the reference settles: a row cannot exist, the distance is exactly 0 or not finite (`!= 0` is exact on both
    sides), or the weight is outside the band C x err(s) of 0.1"""
    with np.errstate(all="ignore"):
        return ~ref.has | (ref.dist == 0) | ~np.isfinite(ref.s) | ~(np.abs(ref.s - 0.1) <= C * ref.s_err)


def odom_rows_ratio(got, ref, C):
    ok = np.asarray(got[0]) != 0
    sel = (ok & ref.ok & odom_decided(ref, C))[:, None] & np.isfinite(ref.rows) & (ref.scale > 0)
    if not sel.any():
        return 0.0
    return float((np.abs(np.asarray(got[1], np.float64) - ref.rows)[sel] / ref.scale[sel]).max())


def compare_odom_rows(got, ref, C, cap=0.01, what="rows"):
    """(ok, rows) of a hook against odom_rows_ref's answer: ok equal wherever the reference settles it (at most `cap` of the case left out),
    zeros without a row, a non-finite reference row non-finite, every other entry within C x scale.  -> (checked, left out)"""
    ok, rows = np.asarray(got[0]) != 0, np.asarray(got[1], np.float32)
    dec = odom_decided(ref, C)
    left = int((~dec).sum())
    assert left <= cap * ok.size, f"{what}: {left} of {ok.size} weights within the band of 0.1, the cap is {cap:.0%}"
    bad = np.nonzero(dec & (ok != ref.ok))[0]
    assert bad.size == 0, f"{what}: ok differs at {bad.size} of {ok.size} queries; first: query {bad[0]} (s = {ref.s[bad[0]]!r})"
    off = np.nonzero(rows[~ok].view(np.uint32).any(axis=1))[0]
    assert off.size == 0, f"{what}: a query without a row does not return zeros; first: the {off[0]}th of them"
    both = ok & ref.ok
    fin = np.isfinite(ref.rows)
    bad = np.argwhere(both[:, None] & ~fin & np.isfinite(rows))
    assert bad.size == 0, f"{what}: finite where the reference is not; first: query {bad[0][0]} column {bad[0][1]}"
    with np.errstate(all="ignore"):
        err = np.abs(rows.astype(np.float64) - ref.rows)
        bad = np.argwhere(both[:, None] & fin & ~(err <= C * ref.scale))
    assert bad.size == 0, (f"{what}: {len(bad)} entries beyond {C:.3g} x scale; first: query {bad[0][0]} column {bad[0][1]}: "
                          f"{rows[tuple(bad[0])]!r} vs {ref.rows[tuple(bad[0])]!r}, scale {ref.scale[tuple(bad[0])]:.3g}")
    return int(dec.sum()), left


# ------------------------------------------------------------------------------------------------ sums
PAIRS = [(r, c) for r in range(6) for c in range(r, 6)]


def terms_of_rows(ok, rows32):
    """the fp32 products a row adds, widened: (n_ok, 27) fp64 — the 21 upper-triangle products a_r a_c, then a_r b"""
    r = np.asarray(rows32, np.float32)[np.asarray(ok) != 0]
    out = np.empty((r.shape[0], 27))
    for k, (i, j) in enumerate(PAIRS):
        out[:, k] = (r[:, i] * r[:, j]).astype(np.float64)       # the fp32 product, as the loops form it
    for i in range(6):
        out[:, 21 + i] = (r[:, i] * r[:, 6]).astype(np.float64)
    return out


def compare_sums(partials, ok, rows32, what="sums"):
    """the partials of a rows launch against the hook's own rows: the count exactly, every other column within the bound of any fp64
    summation order.  -> the largest |difference| / bound seen (0 where the bound is 0 and the difference too)"""
    P = np.asarray(partials, np.float64).reshape(-1, 28)
    n = int((np.asarray(ok) != 0).sum())
    count = math.fsum(P[:, 27]) if P.shape[0] else 0.0
    assert count == n, f"{what}: the count column holds {count!r}, {n} rows exist"
    T = terms_of_rows(ok, rows32)
    worst = 0.0
    for k in range(27):
        if not np.isfinite(T[:, k]).all():
            # a non-finite row (the collinear plane triple of the scan-to-scan loop) makes the column's sum non-finite, whatever the order
            assert not np.isfinite(P[:, k].sum()), f"{what}: column {k} holds a non-finite term, its partials add up to {P[:, k].sum()!r}"
            continue
        exact_p = math.fsum(P[:, k]) if P.shape[0] else 0.0
        exact_t = math.fsum(T[:, k])
        bound = max(n - 1, 0) * U64 * math.fsum(np.abs(T[:, k]))
        diff = abs(exact_p - exact_t)
        assert diff <= bound, f"{what}: column {k}: the partials add up to {exact_p!r}, the rows' products to {exact_t!r}: {diff:.3g} apart, bound {bound:.3g}"
        if bound > 0:
            worst = max(worst, diff / bound)
    return worst


def compare_sums_pair(partials_a, partials_b, ok, rows32, what="two sums"):
    """two sets of partials of the same rows (another partition, another number of lanes per query): each is within the bound of the exact
    sum, so the two are within twice the bound of each other, column by column; the counts are equal"""
    A, B = (np.asarray(p, np.float64).reshape(-1, 28) for p in (partials_a, partials_b))
    n = int((np.asarray(ok) != 0).sum())
    T = terms_of_rows(ok, rows32)
    assert math.fsum(A[:, 27]) == math.fsum(B[:, 27]) == n, f"{what}: counts {math.fsum(A[:, 27])!r}, {math.fsum(B[:, 27])!r}, rows {n}"
    for k in range(27):
        bound = 2 * max(n - 1, 0) * U64 * math.fsum(np.abs(T[:, k]))
        diff = abs(math.fsum(A[:, k]) - math.fsum(B[:, k]))
        assert diff <= bound, f"{what}: column {k}: {diff:.3g} apart, bound {bound:.3g}"


# ------------------------------------------------------------------------------------------------ folds
def fold_ref(partials):
    """integer-valued partials below 2^21 in magnitude: the sums of a few thousand rows stay far below 2^53, so every order adds exactly"""
    P = np.asarray(partials, np.float64).reshape(-1, 28)
    assert (P == np.rint(P)).all() and np.abs(P).max(initial=0) < 2 ** 21
    return P.astype(np.int64).sum(axis=0).astype(np.float64)


def position_coded(nblocks):
    """row b holds b + 1 in column 0 and ones in column 1 + (b mod 27): a wrong sum names the row that was dropped or doubled"""
    P = np.zeros((nblocks, 28))
    P[:, 0] = np.arange(1, nblocks + 1)
    P[np.arange(nblocks), 1 + np.arange(nblocks) % 27] = 1.0
    return P


def compare_fold(sums, partials, what="fold"):
    ref = fold_ref(partials)
    got = np.asarray(sums, np.float64).reshape(28)
    if (got.view(np.uint64) != ref.view(np.uint64)).any():
        d = got - ref
        k = int(np.nonzero(d)[0][0]) if np.nonzero(d)[0].size else int(np.nonzero(got.view(np.uint64) != ref.view(np.uint64))[0][0])
        hint = ""
        P = np.asarray(partials, np.float64).reshape(-1, 28)
        if P.shape[0] and (P[:, 0] == np.arange(1, P.shape[0] + 1)).all() and d[0] != 0 and abs(d[0]) <= P.shape[0]:
            hint = f"; row {int(abs(d[0])) - 1} was {'dropped' if d[0] < 0 else 'added twice'}"
        raise AssertionError(f"{what}: {P.shape[0]} rows: column {k} sums to {got[k]!r}, exactly {ref[k]!r}{hint}")


# ------------------------------------------------------------------------------------------------ step
def qmul(a, b):
    """Hamilton product, xyzw"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def sums_of(AtA, AtB, count):
    """the 28 sums of a symmetric 6x6 and a 6-vector"""
    s = np.zeros(28)
    for k, (i, j) in enumerate(PAIRS):
        s[k] = AtA[i, j]
    s[21:27] = AtB
    s[27] = count
    return s


def system_of(sums):
    """the fp32-rounded A^T A and A^T b of 28 sums, widened"""
    s = np.asarray(sums, np.float64)
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = np.float32(s[k])
    return A, s[21:27].astype(np.float32).astype(np.float64)


class Step:
    pass


def step_ref(family, sums, state_in, it, min_rows=0, left_update=0):
    """state_in: a record of capi.GN_STATE (or anything with those fields) -> the step in fp64 and its margins"""
    r = Step()
    s = np.asarray(sums, np.float64)
    q = np.asarray(state_in["T"], np.float64)[:4].copy()
    t = np.asarray(state_in["T"], np.float64)[4:7].copy()
    r.nsel = int(s[27])
    r.iters = it + 1
    r.kz, r.degenerate, r.converged = int(state_in["kz"]), int(state_in["degenerate"]), int(state_in["converged"])
    r.q, r.t, r.X, r.stepped = q, t, np.zeros(6), False
    r.pad = float(r.nsel) if family == 1 else float(np.asarray(state_in["T"])[7])
    if (family == 0 and min_rows > 0 and r.nsel < min_rows) or (family == 1 and r.nsel < MIN_ROWS_ODOM):
        return r
    r.stepped = True
    A, g = system_of(s)
    r.A, r.g = A, g
    X = np.linalg.lstsq(A, g, rcond=None)[0]
    r.eig = np.linalg.eigvalsh(A)
    # the condition number of the system the solve works on: largest over smallest singular value of the columns it keeps (an exactly
    # zero row and column — the rank-deficient cases — is dropped by the pivoting and by lstsq alike; 1e-12 is far below any kept value)
    sv = np.linalg.svd(A, compute_uv=False)
    r.rank = int((sv > 1e-12 * sv[0]).sum()) if sv[0] > 0 else 0
    r.cond = float(sv[0] / sv[r.rank - 1]) if r.rank else float("inf")
    if it == 0:
        r.kz = int((r.eig < THRESHOLD[family]).sum())
        r.degenerate = int(r.kz > 0)
    r.X_unmasked = X.copy()
    if r.degenerate:
        X[:r.kz] = 0
    r.X = X
    dq = np.r_[X[:3] / 2, 1.0]
    r.t = t + X[3:]
    r.q = qmul(dq, q) if left_update else qmul(q, dq)
    r.q_other_side = qmul(q, dq) if left_update else qmul(dq, q)
    R0 = q / np.linalg.norm(q)
    d = qmul(R0, qconj(r.q))
    r.delta_r = math.degrees(2 * math.atan2(np.linalg.norm(d[:3]), abs(d[3])))
    r.delta_t = 100 * float(np.linalg.norm(X[3:]))
    if r.delta_r < ABORT[family] and r.delta_t < ABORT[family]:
        r.converged = 1
    return r


def at_identity(state_in):
    T = np.asarray(state_in["T"], np.float64)
    return bool((T[:7] == np.array([0, 0, 0, 1, 0, 0, 0.0])).all())


def read_back_X(state_in, state_out, left_update=0):
    """the step a state pair stands for: t_out - t_in and q_in^-1 q_out = (1, X / 2) (q_out q_in^-1 with left_update), in fp64 from the
    fp32 states.  Exact for q_in = identity, t_in = 0 (the products are by 0 and 1), which is where X is held to its bound; away from the
    identity the fp32 rounding of q_in (1, X / 2) and of t_in + X comes on top and X is not read back for accuracy"""
    qi, qo = np.asarray(state_in["T"], np.float64)[:4], np.asarray(state_out["T"], np.float64)[:4]
    ti, to = np.asarray(state_in["T"], np.float64)[4:7], np.asarray(state_out["T"], np.float64)[4:7]
    qinv = qconj(qi) / (qi @ qi)
    dq = qmul(qo, qinv) if left_update else qmul(qinv, qo)
    return np.r_[2 * dq[:3], to - ti]


def x_ratio(state_in, state_out, ref, left_update=0):
    """|X - X_ref|_2 over EPS32 * cond * |X_ref|_2 (the quantity C_QR bounds); state_in is the identity with t = 0"""
    assert at_identity(state_in)
    X = read_back_X(state_in, state_out, left_update)
    return float(np.linalg.norm(X - ref.X)) / (EPS32 * ref.cond * float(np.linalg.norm(ref.X)))


SIDE_MARGIN = 100.0


def compare_step(state_in, state_out, ref, C=None, left_update=0, what="step", check_X=True):
    """the decisions exactly; T untouched (in bits) when no step was made; masked components exactly zero.
    At the identity (t = 0), where the state IS the step: X within C x EPS32 x cond x |X| (check_X: not for the non-finite cases).
    Away from the identity the accuracy of X is not asked again (every system there is also a case at the identity); what is asked is the
    composition: the rotation lies SIDE_MARGIN times nearer to the reference's update on the stated side than to the update on the other
    side, and t_out - (t_in + X[3:]) is below |X[3:]| / SIDE_MARGIN.  A wrong side, a missing, doubled or rotated translation are errors
    of order |X|; rounding and the solve are five orders below it.  -> the ratio where X was checked, else 0"""
    C = C_QR if C is None else C
    so = state_out
    assert int(so["nsel"]) == ref.nsel, f"{what}: nsel {int(so['nsel'])} vs {ref.nsel}"
    assert int(so["iters"]) == ref.iters, f"{what}: iters {int(so['iters'])} vs {ref.iters}"
    assert int(so["kz"]) == ref.kz, f"{what}: kz {int(so['kz'])} vs {ref.kz}"
    assert int(so["degenerate"]) == ref.degenerate, f"{what}: degenerate {int(so['degenerate'])} vs {ref.degenerate}"
    assert int(so["converged"]) == ref.converged, f"{what}: converged {int(so['converged'])} vs {ref.converged}"
    Ti, To = np.asarray(state_in["T"], np.float32), np.asarray(so["T"], np.float32)
    assert np.float32(To[7]).view(np.uint32) == np.float32(ref.pad).view(np.uint32), f"{what}: pad {To[7]!r} vs {ref.pad!r}"
    if not ref.stepped:
        assert (Ti[:7].view(np.uint32) == To[:7].view(np.uint32)).all(), f"{what}: T moved without a step: {Ti[:7]} -> {To[:7]}"
        return 0.0
    if not check_X:
        return 0.0
    if not at_identity(state_in):
        qo, to = To[:4].astype(np.float64), To[4:7].astype(np.float64)
        d_side, d_other = float(np.abs(qo - ref.q).max()), float(np.abs(qo - ref.q_other_side).max())
        assert np.abs(ref.q - ref.q_other_side).max() > 1e-4, f"{what}: the case does not tell the sides apart"
        assert SIDE_MARGIN * d_side < d_other, f"{what}: the rotation is {d_side:.3g} from the stated side's update and {d_other:.3g} from the other side's"
        d_t, xt = float(np.abs(to - ref.t).max()), float(np.linalg.norm(ref.X[3:]))
        assert SIDE_MARGIN * d_t < xt, f"{what}: t is {d_t:.3g} from t_in + X[3:], |X[3:]| = {xt:.3g}"
        return 0.0
    z = To[:3][:min(ref.kz, 3)] if ref.degenerate else To[:0]
    assert (z.view(np.uint32) == 0).all(), f"{what}: a masked rotation component is not zero: {To[:3]}"
    if ref.degenerate and ref.kz > 3:
        assert (To[4:4 + ref.kz - 3].view(np.uint32) == 0).all(), f"{what}: a masked translation component is not zero: {To[4:7]}"
    X = read_back_X(state_in, so, left_update)
    ratio = x_ratio(state_in, so, ref, left_update)
    assert ratio <= C, f"{what}: X {X} vs {ref.X}: {ratio:.3g} x EPS32 x cond ({ref.cond:.3g}) x |X|, allowed {C:.3g}"
    return ratio
