"""The five-neighbour plane and line fits' references and checks, without a GPU: the oracle's statement of lio_fit_five
(include/lio_test_hooks.h) meets the fp64 references of tests/fit_ref.py on every case of tests/fit_cases.py — the run that sets the two
tolerance constants —, every case contains what it is there for, the caps hold for the references alone, and the comparisons the GPU
tests use (tests/test_gpu_fit_five.py) notice the errors a fit can make."""
import numpy as np
import pytest

import fit_cases
import fit_ref
from fit_cases import MM, MP
from lio_amd import capi

IDS = [f"{n}-form{f}" for n, f in fit_cases.RUNS]


# ------------------------------------------------------------------------------------------------ oracle against fp64
def test_oracle_meets_fp64(oracle):
    """every case and form under the comparison the product is held to; the largest error / scale per family is what the constants of
    fit_ref.py are 4 x of (printed; asserted here so that the recorded numbers cannot drift away from what the oracle does)"""
    worst = {"plane": {}, "line": {}}
    for name, form in fit_cases.RUNS:
        c = fit_cases.get(name)
        got, ref = c.run(oracle, form), c.ref(form)
        fit_ref.finite_or_invalid(got)
        if not c.exempt:
            fit_ref.compare(got, ref, c.cap)
            fam = worst[c.kind]
            fam[c.family] = max(fam.get(c.family, 0.0), fit_ref.ratios(got, ref, fit_ref.C_LINE if form == 3 else fit_ref.C_PLANE))
    for kind, C in (("plane", fit_ref.C_PLANE), ("line", fit_ref.C_LINE)):
        print(kind, "error / scale by family:", {k: round(v, 3) for k, v in worst[kind].items()}, "constant", C)
        top = max(worst[kind].values())
        assert 0.9 * C <= 4 * top <= C, (kind, top, C)   # the constant IS 4 x the measured maximum, rounded up to the digits written down


def test_oracle_direction_is_the_top_eigenvector(oracle):
    n = 0
    for name in fit_cases.NAMES:
        c = fit_cases.get(name)
        if c.kind == "line" and not c.exempt:
            n += fit_ref.compare_direction(c.run(oracle, 3), c.ref(3), c.nbr, C=4 * fit_ref.C_LINE)   # the oracle's solver is fp32: 4 x the scale
    assert n > 50000


def test_oracle_hook_checks_its_arguments(oracle):
    c = fit_cases.get("plane_m65")
    for form in (-1, 4, 17):
        with pytest.raises(capi.LioError):
            c.run(oracle, form)
    fit_cases.check_null_pointers(oracle, c)
    z = fit_cases.get("plane_m0")
    assert all(a.shape[0] == 0 for a in z.run(oracle, 0))


# ------------------------------------------------------------------------------------------------ the cases hold what they claim
@pytest.mark.parametrize("name,form", fit_cases.RUNS, ids=IDS)
def test_caps_hold_for_the_reference_alone(name, form):
    c = fit_cases.get(name)
    ref = c.ref(form)
    clean = fit_ref.result_of(ref)
    fit_ref.finite_or_invalid(clean)
    if c.exempt:
        return
    n_chk, n_left = fit_ref.compare(clean, ref, c.cap)
    assert n_chk + n_left == c.m and n_left <= c.cap * c.m
    if c.straddle:
        yes, no = fit_ref.asserted_sides(ref, c.straddle)
        assert yes >= 0.3 and no >= 0.3, (c.straddle, yes, no)
    elif c.family not in ("sel_at_origin", "nonfinite", "disc", "blob") and c.m >= 63:
        assert ref.valid[~c.bad].mean() > 0.95                   # an ordinary family is made of residuals that exist


def test_ranges_planes_and_ragged_sizes():
    for r in (1, 10, 50, 100, 400):
        for fam in (f"noisy_r{r}", f"noisy_axis_r{r}", f"line_noisy_r{r}"):
            c = fit_cases.get(fam)
            d = np.linalg.norm(c.nbr.astype(np.float64).mean(axis=1), axis=1)
            assert (np.abs(d - r) < 0.5 + 0.01 * r).all(), fam
    for r in (1, 400):
        ref = fit_cases.get(f"noisy_axis_r{r}").ref(0)
        assert (np.abs(np.abs(ref.n).max(axis=1) - 1) < 0.2).all()                  # axis-aligned up to the 5 cm noise
    ax = fit_cases.get("line_axis_aligned")
    cov, _ = fit_ref.line_cov32(ax.nbr)
    off = cov[:, [0, 0, 1], [1, 2, 2]]
    assert (off == 0).all() and ax.m == 600                                         # zero off-diagonals, exactly
    assert [fit_cases.get(f"plane_m{k}").m for k in (0, 1, 63, 64, 65)] == [0, 1, 63, 64, 65]
    assert [fit_cases.get(f"line_m{k}").m for k in (0, 1, 63, 64, 65)] == [0, 1, 63, 64, 65]
    assert fit_cases.get("plane_m100000").m >= 100000 and fit_cases.get("line_m100000").m >= 100000
    sig = fit_cases.get("noisy_r10").ref(0).max_pd
    assert sig.min() < 0.005 and sig.max() > 0.03                                   # noise from nothing to centimetres


def test_equal_column_norms_are_exactly_equal():
    c = fit_cases.get("equal_column_norms")
    n2 = np.zeros((c.m, 3), np.float32)
    for j in range(5):
        n2 = n2 + c.nbr[:, j] * c.nbr[:, j]                                          # the sequential fp32 sums of the pivot search
    assert (n2[:, 0] == n2[:, 1]).all() and (n2[:, 0] > n2[:, 2]).all()
    assert (c.nbr[:, :, 0] != c.nbr[:, :, 1]).any(axis=1).all()


def test_near_origin_and_degenerate_patches():
    ref = fit_cases.get("plane_through_origin").ref(0)
    assert ref.d.min() < 2e-3 and ref.d.max() > 5e-2 and (ref.d < 0.11).all() and (ref.d > 0.9e-3).all()
    sw = fit_cases.get("near_collinear_sweep").ref(0)
    rel = sw.S[:, 2] / sw.S[:, 0]
    eps = fit_ref.EPS32
    assert (rel < eps / 4).sum() > 50 and (rel > 4 * eps).sum() > 50 and ((rel > eps / 4) & (rel < 4 * eps)).sum() > 20   # across the rank threshold
    assert fit_cases.get("near_collinear_sweep").exempt and fit_cases.get("exactly_collinear").exempt
    col = fit_cases.get("exactly_collinear").nbr.astype(np.float64)
    d1, d2 = col[:, 1] - col[:, 0], col[:, 4] - col[:, 0]
    assert (np.cross(d1, d2) == 0).all() and (d1 != 0).any(axis=1).all()
    for dup in (2, 3, 4, 5):
        c = fit_cases.get(f"duplicates_{dup}")
        distinct = np.array([np.unique(p, axis=0).shape[0] for p in c.nbr])
        assert (distinct == 6 - dup).all() and c.exempt
    li = fit_cases.get("line_identical")
    assert (li.nbr == li.nbr[:, :1]).all()


def test_straddlers_sit_on_their_thresholds():
    c = fit_cases.get("straddle_fifth")
    mm = np.float32(MM)
    assert set(np.unique(c.fifth).tolist()) == {float(np.nextafter(mm, np.float32(0))), float(mm), float(np.nextafter(mm, np.float32(2))), float("inf")}
    assert (c.fifth == mm).sum() >= 100 and np.isinf(c.fifth).sum() >= 100
    ref = fit_cases.get("straddle_plane_dis").ref(0)
    assert (np.abs(ref.mar_plane) < 0.26 * MP).mean() > 0.8 and (ref.mar_plane > 0).sum() > 300 and (ref.mar_plane < 0).sum() > 300
    ref = fit_cases.get("straddle_score").ref(0)
    assert (np.abs(ref.mar_score) < 0.09).all() and (ref.mar_score > 0).sum() > 300 and (ref.mar_score < 0).sum() > 300
    for which, side in (("fov_lo", "check1"), ("fov_hi", "check2")):
        for suffix in ("", "_line"):
            ref = fit_cases.get(f"straddle_{which}{suffix}").ref(3 if suffix else 1)
            chk = getattr(ref, side)
            assert (chk > 0).sum() > 300 and (chk < 0).sum() > 300
    ref = fit_cases.get("straddle_ratio").ref(3)
    rat = ref.lam[:, 2] / ref.lam[:, 1]
    assert (rat > 3).sum() == 500 and (rat < 3).sum() == 500 and (np.abs(rat / 3 - 1) < 0.41).all()


def test_sign_cases_and_exact_geometry():
    ref = fit_cases.get("sign_both").ref(1)
    assert (ref.pd2 > 0.04).sum() > 250 and (ref.pd2 < -0.04).sum() > 250
    z = fit_cases.get("pd2_zero")
    assert (z.nbr[:, :, 2] == z.stack[:, None, 2]).all()                             # the query lies ON the dyadic plane z = const
    ref = z.ref(1)
    assert (np.abs(ref.pd2) < 1e-12).all() and ref.sign_free.all() and ref.valid.all()
    o = fit_cases.get("sel_at_origin")
    assert (o.stack[::2, :3] == 0).all() and not o.ref(0).valid[::2].any() and o.ref(0).valid[1::2].any()
    r1 = fit_cases.get("rank1_dyadic")
    ref = r1.ref(3)
    cov, _ = fit_ref.line_cov32(r1.nbr)
    assert (np.linalg.matrix_rank(cov.astype(np.float64)) == 1).all()
    assert (ref.ld2[::4] == 0).all() and (ref.ld2[1::4] > 0.1).all() and ref.valid.all()   # every fourth query lies exactly on the line
    b = fit_cases.get("blob").ref(3)
    assert not fit_cases.get("blob").exempt and 100 < b.valid.sum() < 300 and (b.lam[:, 0] > 1e-6).all()      # full rank, poorly separated, both outcomes
    d = fit_cases.get("disc").ref(3)
    assert (np.abs(d.lam[:, 2] / d.lam[:, 1] - 1) < 1e-5).all() and not d.valid.any()


@pytest.mark.parametrize("name", ["plane_nonfinite", "line_nonfinite"])
def test_every_wave_with_a_bad_query_holds_good_ones(name):
    c = fit_cases.get(name)
    assert c.bad.sum() >= 8
    rows = ~np.isfinite(c.nbr).all(axis=(1, 2)) | ~np.isfinite(c.stack).all(axis=1)
    assert (rows == c.bad).all()
    assert (~np.isfinite(c.nbr).all(axis=(1, 2))).sum() >= 3 and (~np.isfinite(c.stack).all(axis=1)).sum() >= 3
    assert np.isnan(c.nbr).any() and np.isinf(c.nbr).any() and np.isnan(c.stack).any() and np.isinf(c.stack).any()
    for w in range(0, c.m, 64):
        assert 0 < c.bad[w:w + 64].sum() < len(c.bad[w:w + 64]) / 2
    for form in c.forms:
        assert not c.ref(form).valid[c.bad].any()


# ------------------------------------------------------------------------------------------------ planted errors are noticed
def _raises(what, got, ref, cap=1.0):
    with pytest.raises(AssertionError, match=what):
        fit_ref.compare(got, ref, cap)


def _plane_outputs(ref, n, d, s, form):
    """reference-shaped outputs from a given normal, offset and score (fp64 -> the hook's arrays); sign rule of `form` applied"""
    pd2 = (n * ref.sel).sum(axis=1) + d
    sg = np.where((pd2 <= 0) & (form == 1), -1.0, 1.0)[:, None]
    if form == 0:
        co, sc, ab = s[:, None] * np.c_[n, d], s.copy(), np.zeros((ref.m, 4))
    else:
        co, sc, ab = sg * s[:, None] * np.c_[n, pd2], np.zeros(ref.m), sg * np.c_[n, d]
    z = ~ref.valid
    co[z], sc[z], ab[z] = 0, 0, 0
    return ref.valid.astype(np.uint8), co.astype(np.float32), sc.astype(np.float32), ab.astype(np.float32)


def test_pivoting_decides_the_answer_on_rank_two_patches(oracle):
    """a patch of two distinct points has rank 2: the oracle's answer is the basic solution on the two columns its pivot search picks, and
    where column 2 is one of them an unpivoted solve (columns 0 and 1) gives a normal that is off by more than 1e-2 — far beyond rounding.
    The degenerate families are held to product == oracle in bits (tests/test_gpu_fit_five.py), which therefore notices a product without
    pivoting; the fp64 comparison cannot (on full-rank patches an unpivoted Householder QR is as accurate)."""
    c = fit_cases.get("duplicates_4")
    got = c.run(oracle, 0)
    A = c.nbr.astype(np.float64)
    drop = np.argmin(np.abs(got[1][:, :3]), axis=1)
    moved = 0
    for i in range(c.m):
        if got[0][i] and drop[i] != 2:
            assert got[1][i, drop[i]] == 0
            keep = [k for k in range(3) if k != drop[i]]
            x = np.zeros(3)
            x[:2] = np.linalg.lstsq(A[i][:, :2], -np.ones(5), rcond=None)[0]
            n = x / np.linalg.norm(x)
            xp = np.zeros(3)
            xp[keep] = np.linalg.lstsq(A[i][:, keep], -np.ones(5), rcond=None)[0]
            npv = xp / np.linalg.norm(xp)
            s = np.linalg.norm(got[1][i, :3].astype(np.float64))
            assert np.abs(got[1][i, :3] / s - npv).max() < 1e-3          # the oracle's answer IS the pivoted basic solution
            moved += int(np.abs(n - npv).max() > 1e-2)
    assert moved > 100
    fit_ref.compare_bits(got, c.run(oracle, 0))


def test_planted_middle_eigenvector():
    c = fit_cases.get("line_noisy_r10")
    ref = c.ref(3)
    clean = fit_ref.result_of(ref)
    assert fit_ref.compare_direction(clean, ref, c.nbr) > 500
    cov, _ = fit_ref.line_cov32(c.nbr)
    mid = np.linalg.eigh(cov.astype(np.float64))[1][:, :, 1]
    bad = (clean[0], fit_ref.line_coeff_from_direction(ref, mid).astype(np.float32), clean[2], clean[3])
    _raises("coeff beyond", bad, ref)
    with pytest.raises(AssertionError, match="not the top eigenvector"):
        fit_ref.compare_direction(bad, ref, c.nbr)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_planted_plane_value_errors(form):
    c = fit_cases.get("noisy_r10")
    ref = c.ref(form)
    fit_ref.compare(_plane_outputs(ref, ref.n, ref.d, ref.s, form), ref, c.cap)                  # the helper itself is clean
    x = 1.0 / ref.d                                                                               # |x| of A x = -1
    _raises("beyond", _plane_outputs(ref, ref.n * x[:, None], ref.d * x, ref.s, form), ref)        # (x, 1): the normal not normalised
    sn = np.linalg.norm(ref.sel, axis=1)
    _raises("beyond", _plane_outputs(ref, ref.n, ref.d, 1 - 0.9 * np.abs(ref.pd2) / sn, form), ref)   # square root for fourth root


def test_planted_sign_rule_errors():
    c = fit_cases.get("sign_both")
    r1, r2 = c.ref(1), c.ref(2)
    v, co, sc, ab = fit_ref.result_of(r1)
    neg = r1.pd2 < 0
    co[neg], ab[neg] = -co[neg], -ab[neg]
    _raises("beyond", (v, co, sc, ab), r1)                    # mode 1 without its flip
    _raises("beyond", fit_ref.result_of(r1), r2)              # mode 2 with mode 1's flip: the suppression is missing
    fit_ref.compare(fit_ref.result_of(r2), r2, c.cap)


def test_planted_less_or_equal_at_the_match_distance():
    c = fit_cases.get("straddle_fifth")
    ref = c.ref(0)
    loose = fit_ref.plane_ref(c.nbr, np.where(c.fifth == np.float32(MM), np.float32(0.5), c.fifth), c.stack, c.q, c.t, c.pz, 0, MM, MP)
    assert (loose.valid & ~ref.valid).sum() >= 100
    _raises("valid differs", fit_ref.result_of(loose), ref)


@pytest.mark.parametrize("name,form", [("noisy_r10", 0), ("line_noisy_r10", 3)])
def test_planted_neighbours_of_the_next_query(name, form):
    c = fit_cases.get(name)
    ref = c.ref(form)
    shifted = tuple(np.roll(a, -1, axis=0) for a in fit_ref.result_of(ref))
    _raises("beyond", shifted, ref)


@pytest.mark.parametrize("name,form", [("plane_nonfinite", 0), ("plane_nonfinite", 1), ("line_nonfinite", 3)])
def test_planted_valid_flag_on_a_non_finite_query(name, form):
    c = fit_cases.get(name)
    ref = c.ref(form)
    v, co, sc, ab = fit_ref.result_of(ref)
    i = int(np.nonzero(c.bad)[0][2])
    v[i], co[i] = 1, (0.0, 0.9, -0.1, 3.0)
    _raises("valid differs", (v, co, sc, ab), ref)
    v[i] = 0
    with pytest.raises(AssertionError, match="invalid but not zeros"):
        fit_ref.compare((v, co, sc, ab), ref, c.cap)
    co[i] = (np.nan, 0, 0, 0)
    v[i - 1] = 1
    co[i - 1, 0] = np.nan
    with pytest.raises(AssertionError, match="valid but not finite"):
        fit_ref.compare((v, co, sc, ab), ref, c.cap)
