"""fp64 references of the two fits that turn a query's five neighbours into a residual (csrc/cloud_device.h: features_fit, csrc/cloud_kernels.hip:
line_features_fit; test hook lio_fit_five of include/lio_test_hooks.h), written from the definition of the operation.  numpy only; no
library of ours.  Everything is computed in fp64 from the fp32 inputs, for all queries of a case at once.

Plane (forms 0, 1, 2): x = argmin ||A x + 1|| over the five neighbours (SVD), n = x / |x|, d = 1 / |x|; the feature exists when the fifth
squared distance is below min_match_sq_dis, every neighbour lies within min_plane_dis of the plane, s = 1 - 0.9 |pd2| / |sel|^(1/2) > 0.1
(pd2 = n . sel + d) and sel lies in the field of view.  Form 0 returns s (n, d); forms 1 / 2 return s (n, pd2) and (n, d), form 1 with the
sign that makes pd2 positive.
Line (form 3): centroid c and covariance of the five, eigenvalues l0 <= l1 <= l2; the feature exists when l2 > 3 l1 (and the same distance,
score and field-of-view tests, s = 1 - 0.9 ld2); with w = sel - c and v the top eigenvector, ld2 = |w_perp|, nt = w_perp / ld2, coefficients
s (nt, ld2).

Error scales.  A result computed in fp32 cannot meet fp64 exactly; how far it may be off is estimated PER QUERY, from the query's own
conditioning, and one constant per fit multiplies the estimate:
  plane  E_rel = eps32 (kappa + kappa^2 ||A x + 1|| / (||A|| ||x||)), the first-order forward error of a backward-stable least-squares
         solve; |dn| <= E_rel, |dd| <= d E_rel; a point-plane distance, written n . (p - c) + (n . c + d) about the patch's centroid c,
         moves by E_rel |p - c| plus 8 eps32 (|p| + d) for the height at c and the fp32 evaluation (the errors of n and d are tied
         together: the computed plane still passes through the patch); sel itself carries 4 eps32 (|po| + |t|) from the fp32 transform.
  line   the reference algorithm forms the covariance in fp32 after an fp32 centroid subtraction.  The centroid's own error drops out of the
         covariance to first order (the differences sum to zero), so what is left is the rounding of each difference p - c, at most
         eps32 R / 2 (R the largest coordinate; for points within a factor two of c the subtraction is exact): delta = eps32 R for the
         two factors of a product, a covariance entry off by E_cov = 2 sigma delta + delta^2 + 8 eps32 sigma^2 (sigma^2 the trace), i.e.
         eps32 R / sigma relative; eigenvalues move by 3 E_cov, the top eigenvector by 3 E_cov / (l2 - l1).  Independent of the
         solver, the end points c +- 0.1 v are rounded to fp32 (direction noise 5 sqrt(3) eps32 R) and the cross products cancel
         (20 eps32 (|w| + 0.1)^2 on w_perp): the "solver-only" part of the scale, what remains when the covariance is taken as given.
A decision (a quantity against its threshold) is asserted where the fp64 margin exceeds C times the scale of that quantity; values are
asserted on every query whose decisions are all outside their bands.

The constants (tests/test_fit_five.py::test_oracle_meets_fp64 measures the ratios below on every run and asserts that the constants are
4 x their maxima):
  largest error / scale the oracle reaches, by family
    plane  1.30 (noisy_r50); noisy patches at 1 .. 400 m 0.80 .. 1.30 (axis-aligned 0.85 .. 1.19), equal column norms 0.22, planes near the
           origin 0.56, straddlers 0.58 .. 1.12, sign rule 0.61 .. 0.70, non-finite neighbours in the launch 0.88, 100 000 queries 1.27
    line   0.21 (straddle_fov_lo); noisy segments at 1 .. 400 m 0.04 .. 0.08, axis-aligned 0.05, ratio straddler 0.06, isotropic blobs 0.06,
           100 000 queries 0.10, field-of-view straddlers 0.15 .. 0.21 (their queries sit 5 cm from the line and metres from the sensor,
           where sel's own fp32 rounding is most of the error).  Even so the value comparison of the line is the coarse one — the
           covariance term is an upper estimate, and at the median query the tolerance is tens of times the oracle's error: it catches a wrong
           vector, a wrong sign, a wrong decision.  The SENSITIVE check of the eigen-solver is compare_direction below, which takes the
           fp32-formed covariance as given and leaves the solver only the fp32 cast of its vector and the noise of recovering it.
  The product on the MI355X (tests/test_gpu_fit_five.py prints its ratios): its plane forms equal the oracle in bits, so plane 1.30; line
  0.21 (straddle_fov_lo), noisy segments 0.04 .. 0.08, blobs 0.06: the oracle's figures to the digits shown, family by family (sel's rounding and the
  fp32 evaluation, not the solver, set them).
  C_PLANE = 4 x 1.31, C_LINE = 4 x 0.21 (maxima rounded up): the factor 4 lets an equally valid fp32 evaluation order, or another
  eigen-solver, land elsewhere inside the same rounding envelope.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
C_PLANE = 4 * 1.31
C_LINE = 4 * 0.21
SQRT3 = np.sqrt(3.0)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def quat_rotate(q_xyzw, p):
    """fp64: rotate the rows of p by the (not necessarily unit) quaternion the way a rotation matrix of the normalised one does"""
    q = np.asarray(q_xyzw, np.float64)
    q = q / np.linalg.norm(q)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.asarray(p, np.float64) @ R.T


class Ref:
    """what a reference returns: expected outputs (fp64), per-component scales, decision margins and scales"""


def _common(nbr, fifth, stack, q, t, pz, form, mm):
    r = Ref()
    r.form = form
    r.m = m = stack.shape[0]
    r.nbr = nbr.astype(np.float64).reshape(m, 5, 3)
    po = stack[:, :3].astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    r.t = t
    with np.errstate(invalid="ignore", over="ignore"):
        r.sel = quat_rotate(q, po) + t
    r.e_sel = 4 * EPS32 * (np.linalg.norm(np.nan_to_num(po, posinf=0, neginf=0), axis=1) + np.linalg.norm(t))
    r.finite = np.isfinite(r.nbr).all(axis=(1, 2)) & np.isfinite(po).all(axis=1)
    r.pz = (quat_rotate(q, np.array([[0.0, 0.0, 10.0]]))[0] + t) if form == 0 else np.asarray(pz, np.float32).astype(np.float64)
    # decision 1: the fifth squared distance, an exact fp32 comparison (no band); +inf stands for "fewer than five"
    r.mar_fifth = np.where(np.isfinite(fifth), fifth.astype(np.float64) - float(np.float32(mm)), np.inf)
    # decision 4: field of view, 100 + side1 - side2 -+ 10 sqrt(3) sqrt(side1)
    with np.errstate(invalid="ignore", over="ignore"):
        side1 = ((t - r.sel) ** 2).sum(axis=1)
        side2 = ((r.pz - r.sel) ** 2).sum(axis=1)
        k = 10.0 * float(np.float32(np.sqrt(np.float32(3.0))))
        r.check1 = 100.0 + side1 - side2 - k * np.sqrt(side1)
        r.check2 = 100.0 + side1 - side2 + k * np.sqrt(side1)
        r.e_fov = 8 * EPS32 * (100.0 + side1 + side2 + k * np.sqrt(side1)) + 2 * (np.sqrt(side1) + np.sqrt(side2) + k) * r.e_sel
    return r


def plane_ref(nbr_xyz, fifth_sqd, stack_xyzi, q_xyzw, t, fixed_pz, form, min_match_sq_dis, min_plane_dis):
    nbr, fifth, stack = _f32(nbr_xyz), _f32(fifth_sqd), _f32(stack_xyzi).reshape(-1, 4)
    assert form in (0, 1, 2)
    r = _common(nbr, fifth, stack, q_xyzw, t, fixed_pz, form, min_match_sq_dis)
    m = r.m
    A = np.where(r.finite[:, None, None], r.nbr, 1.0)
    with np.errstate(all="ignore"):
        U, S, Vt = np.linalg.svd(A, full_matrices=False) if m else (np.zeros((0, 5, 3)), np.zeros((0, 3)), np.zeros((0, 3, 3)))
        b = -np.ones((m, 5))
        y = np.einsum("mij,mi->mj", U, b) / S
        x = np.einsum("mji,mj->mi", Vt, y)
        r.S = S
        r.kappa = S[:, 0] / S[:, 2]
        res = np.linalg.norm(np.einsum("mij,mj->mi", A, x) + 1.0, axis=1)
        xn = np.linalg.norm(x, axis=1)
        r.e_rel = EPS32 * (r.kappa + r.kappa ** 2 * res / (S[:, 0] * xn))
        r.n = x / xn[:, None]
        r.d = 1.0 / xn
        pdist = np.einsum("mij,mj->mi", A, r.n) + r.d[:, None]
        # errors of n and d are tied together — the computed plane still passes through the patch — so a distance n . p + d is written
        # n . (p - c) + (n . c + d) about the centroid c: the first term turns with n, the second is the plane's height at c, known to the
        # rounding of the coordinates (and of the four-term fp32 evaluation)
        cen = A.mean(axis=1)
        e_pd = r.e_rel[:, None] * np.linalg.norm(A - cen[:, None], axis=2) + 8 * EPS32 * (np.linalg.norm(A, axis=2) + r.d[:, None])
        j = np.argmax(np.abs(pdist), axis=1)
        r.max_pd = np.abs(pdist)[np.arange(m), j]
        r.mar_plane = r.max_pd - float(np.float32(min_plane_dis))          # valid when <= 0
        r.e_plane = e_pd.max(axis=1)
        sn = np.linalg.norm(r.sel, axis=1)
        r.pd2 = (r.n * r.sel).sum(axis=1) + r.d
        r.e_pd2 = r.e_rel * np.linalg.norm(r.sel - cen, axis=1) + 8 * EPS32 * (sn + r.d) + r.e_sel
        r.s = 1.0 - 0.9 * np.abs(r.pd2) / np.sqrt(sn)
        r.e_s = 0.9 * r.e_pd2 / np.sqrt(sn) + 4 * EPS32 * (1.0 + np.abs(r.s)) + 0.9 * np.abs(r.pd2) * 0.5 * r.e_sel / sn ** 1.5
        r.e_s = np.where(sn > 0, r.e_s, 0.0)                            # sel at the origin: s = -inf whatever the rounding
        r.mar_score = r.s - 0.1
        r.valid = r.finite & (r.mar_fifth < 0) & (r.mar_plane <= 0) & (r.mar_score > 0) & (r.check1 < 0) & (r.check2 > 0)
        flip = (r.pd2 <= 0) if form == 1 else np.zeros(m, bool)
        sg = np.where(flip, -1.0, 1.0)
        nd = np.concatenate([r.n, r.d[:, None]], axis=1)
        e_nd = np.concatenate([np.repeat(r.e_rel[:, None], 3, axis=1), (r.d * r.e_rel)[:, None]], axis=1) + EPS32 * np.abs(nd)
        if form == 0:
            coeff = r.s[:, None] * nd
            e_coeff = r.e_s[:, None] * np.abs(nd) + np.abs(r.s)[:, None] * e_nd + 2 * EPS32 * np.abs(coeff)
            score, e_score = r.s.copy(), r.e_s.copy()
            ab, e_ab = np.zeros((m, 4)), np.zeros((m, 4))
        else:
            npd = np.concatenate([r.n, r.pd2[:, None]], axis=1)
            e_npd = np.concatenate([e_nd[:, :3], r.e_pd2[:, None]], axis=1)
            coeff = sg[:, None] * r.s[:, None] * npd
            e_coeff = r.e_s[:, None] * np.abs(npd) + np.abs(r.s)[:, None] * e_npd + 2 * EPS32 * np.abs(coeff)
            score, e_score = np.zeros(m), np.zeros(m)
            ab, e_ab = sg[:, None] * nd, e_nd
    z = ~r.valid
    coeff[z], score[z], ab[z] = 0, 0, 0
    r.coeff, r.score, r.abs = coeff, score, ab
    r.e_coeff, r.e_score, r.e_abs = e_coeff, e_score, e_ab
    r.sign_free = (np.abs(r.pd2) <= C_PLANE * r.e_pd2) if form == 1 else np.zeros(m, bool)
    return r


def line_cov32(nbr_xyz):
    """the covariance the way the reference algorithm forms it: fp32 centroid (sequential sums, / 5), fp32 differences, sequential fp32 sums of
    products, / 5 -> (cov (m, 3, 3) fp32, centroid (m, 3) fp32).  numpy's fp32 + - * / are the IEEE operations, one rounding each."""
    nb = _f32(nbr_xyz).reshape(-1, 5, 3)
    with np.errstate(all="ignore"):
        vc = np.zeros((nb.shape[0], 3), np.float32)
        for j in range(5):
            vc = vc + nb[:, j]
        vc = vc / np.float32(5.0)
        cov = np.zeros((nb.shape[0], 3, 3), np.float32)
        for j in range(5):
            a = nb[:, j] - vc
            cov = cov + a[:, :, None] * a[:, None, :]
        cov = cov / np.float32(5.0)
    assert cov.dtype == np.float32
    return cov, vc


def top_eig_of_cov32(nbr_xyz):
    """eigh (fp64) of the fp32-formed covariance: what an exact eigen-solver returns for the matrix the product's solver is handed
    -> (eigenvalues ascending (m, 3), top eigenvector (m, 3), centroid fp32 as fp64)"""
    cov, vc = line_cov32(nbr_xyz)
    c = np.where(np.isfinite(cov).all(axis=(1, 2))[:, None, None], cov.astype(np.float64), 0.0)
    lam, V = np.linalg.eigh(c) if c.shape[0] else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    return lam, V[:, :, 2], vc.astype(np.float64)


def line_ref(nbr_xyz, fifth_sqd, stack_xyzi, q_xyzw, t, fixed_pz, min_match_sq_dis):
    nbr, fifth, stack = _f32(nbr_xyz), _f32(fifth_sqd), _f32(stack_xyzi).reshape(-1, 4)
    r = _common(nbr, fifth, stack, q_xyzw, t, fixed_pz, 3, min_match_sq_dis)
    m = r.m
    P = np.where(r.finite[:, None, None], r.nbr, 0.0)
    with np.errstate(all="ignore"):
        c = P.mean(axis=1)
        a = P - c[:, None, :]
        cov = np.einsum("mji,mjk->mik", a, a) / 5.0
        lam, V = np.linalg.eigh(cov) if m else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
        r.lam, r.v, r.c = lam, V[:, :, 2], c
        R = np.abs(P).max(axis=(1, 2))
        sig = np.sqrt(np.trace(cov, axis1=1, axis2=2))
        dlt = EPS32 * R                  # per difference: one rounding, <= eps32 R / 2, doubled for the two factors of a product
        r.e_cov = 2 * sig * dlt + dlt ** 2 + 8 * EPS32 * sig ** 2
        r.mar_ratio = lam[:, 2] - 3 * lam[:, 1]                      # valid when > 0
        r.e_ratio = 4 * 3 * r.e_cov
        w = np.where(r.finite[:, None], r.sel, 0.0) - c
        wn = np.linalg.norm(w, axis=1)
        wpar = (w * r.v).sum(axis=1)
        wperp = w - wpar[:, None] * r.v
        r.ld2 = np.linalg.norm(wperp, axis=1)
        r.wn, r.wpar = wn, np.abs(wpar)
        r.nt = np.where(r.ld2[:, None] > 0, wperp / r.ld2[:, None], 0.0)
        # solver-independent evaluation noise of w_perp, and the eigenvector's scale
        r.e_eval = 4 * EPS32 * (R + wn) + 20 * EPS32 * (wn + 0.1) ** 2 + r.e_sel + 2 * wn * (5 * SQRT3 * EPS32 * R + 2 * EPS32)
        r.e_v = 3 * r.e_cov / (lam[:, 2] - lam[:, 1])
        e_wperp = 2 * r.e_v * wn + r.e_eval
        r.e_ld2 = e_wperp
        e_nt = np.where(r.ld2 > 0, e_wperp / r.ld2, np.inf) + 2 * EPS32
        r.s = 1.0 - 0.9 * r.ld2
        r.e_s = 0.9 * r.e_ld2 + 4 * EPS32
        r.mar_score = r.s - 0.1
        r.valid = r.finite & (r.mar_fifth < 0) & (r.mar_ratio > 0) & (r.mar_score > 0) & (r.check1 < 0) & (r.check2 > 0)
        nl = np.concatenate([r.nt, r.ld2[:, None]], axis=1)
        e_nl = np.concatenate([np.repeat(e_nt[:, None], 3, axis=1), r.e_ld2[:, None]], axis=1)
        coeff = r.s[:, None] * nl
        e_coeff = r.e_s[:, None] * np.abs(nl) + np.abs(r.s)[:, None] * e_nl + 2 * EPS32 * np.abs(coeff)
    coeff[~r.valid] = 0
    r.coeff, r.e_coeff = coeff, e_coeff
    r.score, r.e_score, r.abs, r.e_abs = np.zeros(m), np.zeros(m), np.zeros((m, 4)), np.zeros((m, 4))
    r.sign_free = np.zeros(m, bool)
    return r


def result_of(ref):
    """a clean result in the shape the hook returns: (valid uint8, coeff fp32 (m, 4), score fp32, abs_coeff fp32 (m, 4)), fresh arrays"""
    return ref.valid.astype(np.uint8), ref.coeff.astype(np.float32), ref.score.astype(np.float32), ref.abs.astype(np.float32)


def decisions(ref, C):
    """-> {name: (side bool (m,), outside-band bool (m,))}: on which side of its threshold every decision falls in fp64, and whether the
    margin exceeds C times the scale.  A decision that an earlier one has already settled towards "invalid" still appears here."""
    with np.errstate(invalid="ignore"):
        d = {"fifth": (ref.mar_fifth < 0, np.ones(ref.m, bool)),
             "score": (ref.mar_score > 0, np.abs(ref.mar_score) > C * ref.e_s),
             "fov_lo": (ref.check1 < 0, np.abs(ref.check1) > C * ref.e_fov),
             "fov_hi": (ref.check2 > 0, np.abs(ref.check2) > C * ref.e_fov)}
        if ref.form == 3:
            d["ratio"] = (ref.mar_ratio > 0, np.abs(ref.mar_ratio) > C * ref.e_ratio)
        else:
            d["plane"] = (ref.mar_plane <= 0, np.abs(ref.mar_plane) > C * ref.e_plane)
    return d


def decided(ref, C):
    """queries whose validity fp64 settles: every decision outside its band, or some decision outside its band on the invalid side (the
    feature does not exist whatever the others say), or a non-finite input (never valid)"""
    d = decisions(ref, C)
    all_out = np.ones(ref.m, bool)
    some_invalid = np.zeros(ref.m, bool)
    for side, out in d.values():
        all_out &= out
        some_invalid |= out & ~side
    return ~ref.finite | all_out | some_invalid


def finite_or_invalid(got):
    """what holds for every query of every case, the degenerate ones included: a valid query has finite numbers, an invalid one zeros"""
    valid, coeff, score, ab = got
    valid = np.asarray(valid).astype(bool)
    rows = np.concatenate([np.asarray(coeff, np.float64), np.asarray(score, np.float64)[:, None], np.asarray(ab, np.float64)], axis=1)
    bad = np.nonzero(valid & ~np.isfinite(rows).all(axis=1))[0]
    assert bad.size == 0, f"valid but not finite at {bad.size} of {valid.shape[0]} queries; first: query {bad[0]} {rows[bad[0]].tolist()}"
    bad = np.nonzero(~valid & (rows != 0).any(axis=1))[0]
    assert bad.size == 0, f"invalid but not zeros at {bad.size} of {valid.shape[0]} queries; first: query {bad[0]} {rows[bad[0]].tolist()}"


def ratios(got, ref, C):
    """largest |got - ref| / scale over the queries fp64 settles as valid (0 when there are none) — what sets the constants"""
    valid, coeff, score, ab = got
    chk = decided(ref, C) & ref.valid & np.asarray(valid).astype(bool)
    if not chk.any():
        return 0.0
    worst = 0.0
    for g, w, e in ((coeff, ref.coeff, ref.e_coeff), (np.asarray(score)[:, None], ref.score[:, None], ref.e_score[:, None]), (ab, ref.abs, ref.e_abs)):
        g = np.asarray(g, np.float64)
        err = np.abs(g - w)
        if ref.sign_free.any():
            err = np.where(ref.sign_free[:, None], np.minimum(err, np.abs(-g - w)), err)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e > 0, err / e, np.where(err > 0, np.inf, 0.0))
        q = np.where(np.isfinite(e), q, 0.0)
        worst = max(worst, float(q[chk].max()))
    return worst


def compare(got, ref, cap, C=None):
    """got = (valid, coeff, score, abs_coeff) of the hook; ref = plane_ref(...) / line_ref(...).  Raises AssertionError naming the first query
    that is off: a validity that differs where fp64 settles it, a value beyond C times its scale on a query fp64 settles as valid, numbers
    on an invalid query, or more than `cap` (a share) of the queries left out.  -> (n_checked, n_left_out)"""
    if C is None:
        C = C_LINE if ref.form == 3 else C_PLANE
    valid, coeff, score, ab = got
    m = ref.m
    valid = np.asarray(valid)
    assert valid.shape == (m,) and np.asarray(coeff).shape == (m, 4) and np.asarray(score).shape == (m,) and np.asarray(ab).shape == (m, 4)
    finite_or_invalid(got)
    chk = decided(ref, C)
    vb = valid.astype(bool)
    bad = np.nonzero(chk & (vb != ref.valid))[0]
    if bad.size:
        q = bad[0]
        why = {k: (bool(s[q]), bool(o[q])) for k, (s, o) in decisions(ref, C).items()}
        raise AssertionError(f"valid differs at {bad.size} of {m} queries; first: query {q} got {int(valid[q])} want {int(ref.valid[q])} "
                             f"(decision: (passes, outside band) {why}, finite {bool(ref.finite[q])})")
    val = chk & ref.valid
    for name, g, w, e in (("coeff", coeff, ref.coeff, ref.e_coeff), ("score", np.asarray(score)[:, None], ref.score[:, None], ref.e_score[:, None]),
                          ("abs_coeff", ab, ref.abs, ref.e_abs)):
        g = np.asarray(g, np.float64)
        err = np.abs(g - w)
        both = np.abs(-g - w)
        tol = C * e
        with np.errstate(invalid="ignore"):
            off = err > tol
            off_flipped = both > tol
        # a query whose pd2 cannot be told from zero may come with either sign — but with ONE sign for coeff and abs_coeff (checked below)
        off = np.where(ref.sign_free[:, None], off & off_flipped, off)
        bad = np.nonzero(val & off.any(axis=1))[0]
        assert bad.size == 0, (f"{name} beyond {C:.3g} x scale at {bad.size} of {m} queries; first: query {bad[0]} got {g[bad[0]].tolist()} "
                               f"want {w[bad[0]].tolist()} scale {e[bad[0]].tolist()}")
    sf = val & ref.sign_free
    if sf.any():
        c3, a3 = np.asarray(coeff, np.float64)[:, :3], np.asarray(ab, np.float64)[:, :3]
        bad = np.nonzero(sf & ((c3 * a3).sum(axis=1) <= 0))[0]
        assert bad.size == 0, f"coeff and abs_coeff carry different signs at {bad.size} of {m} queries; first: query {bad[0]}"
    n_left = int((~chk).sum())
    assert n_left <= cap * m, f"the comparison leaves out {n_left} of {m} queries, more than the cap {cap}"
    return int(chk.sum()), n_left


def asserted_sides(ref, name, C=None):
    """share of the queries on which decision `name` is asserted as passing / as failing: outside its band, with every OTHER decision
    passing outside its band (so that this decision alone makes the query valid or invalid)"""
    if C is None:
        C = C_LINE if ref.form == 3 else C_PLANE
    d = decisions(ref, C)
    others = ref.finite.copy()
    for k, (side, out) in d.items():
        if k != name:
            others &= side & out
    side, out = d[name]
    return float((others & out & side).sum()) / max(ref.m, 1), float((others & out & ~side).sum()) / max(ref.m, 1)


def recovered_direction(coeff, ref):
    """the line direction a form-3 result implies: nt = coeff[:3] / |coeff[:3]| is w_perp's direction, so the direction is w - (w . nt) nt,
    normalised (w = sel - centroid, known geometry) -> (m, 3); meaningful where w has a component along the line"""
    c = np.asarray(coeff, np.float64)
    with np.errstate(all="ignore"):
        nt = c[:, :3] / np.linalg.norm(c[:, :3], axis=1)[:, None]
        w = ref.sel - ref.c
        v = w - (w * nt).sum(axis=1)[:, None] * nt
        return v / np.linalg.norm(v, axis=1)[:, None]


def compare_direction(got, ref, nbr_xyz, C=None):
    """the eigen-solver on its own: on the queries fp64 settles as valid (and the result has as valid), the direction recovered from the
    result against eigh of the fp32-formed covariance, within C times the solver-only scale — the fp32 cast of the vector and the noise
    of recovering it (the evaluation noise of w_perp, seen from the component of w along the line).  -> number of queries checked"""
    if C is None:
        C = C_LINE
    valid, coeff = np.asarray(got[0]).astype(bool), got[1]
    lam, v32, _ = top_eig_of_cov32(nbr_xyz)
    chk = decided(ref, C) & ref.valid & valid & (ref.wpar > 0.5 * ref.wn) & (ref.ld2 > 0)
    vr = recovered_direction(coeff, ref)
    with np.errstate(all="ignore"):
        err = np.minimum(np.linalg.norm(vr - v32, axis=1), np.linalg.norm(vr + v32, axis=1))
        scale = 2 * EPS32 + 2 * ref.wn * (ref.e_eval / ref.ld2 + 4 * EPS32) / ref.wpar
        off = chk & ~(err <= C * scale)
    bad = np.nonzero(off)[0]
    assert bad.size == 0, (f"direction is not the top eigenvector of the fp32-formed covariance at {bad.size} of {ref.m} queries; first: query "
                           f"{bad[0]} recovered {vr[bad[0]].tolist()} eigh {v32[bad[0]].tolist()} (eigenvalues {lam[bad[0]].tolist()}) "
                           f"error {err[bad[0]]:.3g} scale {scale[bad[0]]:.3g}")
    return int(chk.sum())


def compare_bits(a, b, what="results"):
    """two results of the hook, bit for bit"""
    for name, x, y in zip(("valid", "coeff", "score", "abs_coeff"), a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape, x.dtype, y.dtype)
        if x.size == 0:
            continue
        xb, yb = x.view(np.uint8).reshape(x.shape[0], -1), y.view(np.uint8).reshape(y.shape[0], -1)
        bad = np.nonzero((xb != yb).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs in bits at {bad.size} of {x.shape[0]} queries; first: query {bad[0]} {x[bad[0]].tolist()!r} vs {y[bad[0]].tolist()!r}"


def line_coeff_from_direction(ref, v):
    """the form-3 coefficients s (nt, ld2) a given unit direction v (m, 3) implies for the reference's queries, fp64 (validity untouched)"""
    w = ref.sel - ref.c
    wperp = w - (w * v).sum(axis=1)[:, None] * v
    ld2 = np.linalg.norm(wperp, axis=1)
    with np.errstate(all="ignore"):
        nt = np.where(ld2[:, None] > 0, wperp / ld2[:, None], 0.0)
    s = 1.0 - 0.9 * ld2
    out = s[:, None] * np.concatenate([nt, ld2[:, None]], axis=1)
    out[~ref.valid] = 0
    return out
