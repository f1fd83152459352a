"""The plane and line fits the product runs (csrc/cloud_device.h: features_fit<MAPPING>; csrc/cloud_kernels.hip: line_features_fit; through
the test hook lio_fit_five) against the fp64 references of tests/fit_ref.py on the cases of tests/fit_cases.py — the same comparison, constants
and caps the oracle meets in tests/test_fit_five.py, where the cases' contents and the comparisons' sensitivity are tested without a GPU —,
against the oracle, and against the production entry point."""
import numpy as np
import pytest

import fit_cases
import fit_ref
from lio_amd import capi, pipeline, synth

pytestmark = pytest.mark.gpu

IDS = [f"{n}-form{f}" for n, f in fit_cases.RUNS]
PLANE, LINE = fit_cases.PLANE_NAMES, fit_cases.LINE_NAMES


@pytest.mark.parametrize("name,form", fit_cases.RUNS, ids=IDS)
def test_product_meets_fp64(hip, name, form):
    c = fit_cases.get(name)
    got, ref = c.run(hip, form), c.ref(form)
    fit_ref.finite_or_invalid(got)
    if c.exempt:
        return
    C = fit_ref.C_LINE if form == 3 else fit_ref.C_PLANE
    print(f"{name} form {form}: largest error / scale {fit_ref.ratios(got, ref, C):.3f} (constant {C:.3g})")
    fit_ref.compare(got, ref, c.cap)


@pytest.mark.parametrize("name", PLANE)
def test_plane_forms_equal_the_oracle_in_bits(hip, oracle, name):
    """same statements, same order, -ffp-contract=off on both sides: every query of every case, the degenerate families included"""
    c = fit_cases.get(name)
    for form in c.forms:
        fit_ref.compare_bits(c.run(hip, form), c.run(oracle, form), f"{name} form {form}, product vs oracle")


@pytest.mark.parametrize("name", LINE)
def test_line_validity_equals_the_oracle_where_fp64_settles_it(hip, oracle, name):
    """two eigen-solvers by design: both are held to the reference; their validity agrees wherever the reference's decisions are outside
    their bands"""
    c = fit_cases.get(name)
    a, b, ref = c.run(hip, 3), c.run(oracle, 3), c.ref(3)
    fit_ref.finite_or_invalid(a)
    chk = fit_ref.decided(ref, fit_ref.C_LINE)
    bad = np.nonzero(chk & (a[0] != b[0]))[0]
    assert bad.size == 0, f"valid differs from the oracle's at {bad.size} of {c.m} queries; first: query {bad[0]}"


@pytest.mark.parametrize("name", [n for n in LINE if n not in fit_cases.EXEMPT])
def test_closed_form_direction_is_the_top_eigenvector(hip, name):
    c = fit_cases.get(name)
    ref = c.ref(3)
    n = fit_ref.compare_direction(c.run(hip, 3), ref, c.nbr)
    n_ref = fit_ref.compare_direction(fit_ref.result_of(ref), ref, c.nbr)      # what the reference alone offers for checking
    print(f"{name}: direction checked on {n} of {c.m} queries (the reference alone: {n_ref})")
    assert n >= 0.98 * n_ref
    # discs have no valid query by construction; the field-of-view straddlers' queries sit beside the centroid, with no component along
    # the line to recover a direction from (their values are held by test_product_meets_fp64)
    if name not in ("disc", "line_m0", "straddle_fov_lo_line", "straddle_fov_hi_line"):
        assert n_ref >= 0.2 * c.m and n_ref >= 1, (n_ref, c.m)


@pytest.mark.parametrize("name", ["plane_nonfinite", "line_nonfinite"])
def test_non_finite_queries_are_invalid_and_alone(hip, name):
    c = fit_cases.get(name)
    donor = np.nonzero(~c.bad)[0][0]
    nbr, stack = c.nbr.copy(), c.stack.copy()
    nbr[c.bad], stack[c.bad] = nbr[donor], stack[donor]
    for form in c.forms:
        got, clean = c.run(hip, form), c.run(hip, form, nbr=nbr, stack=stack)
        for a in got:
            assert not a[c.bad].any()                       # valid == 0 and zeros
        fit_ref.compare_bits(tuple(a[~c.bad] for a in got), tuple(a[~c.bad] for a in clean), f"{name} form {form}, with vs without the bad rows")


def test_hook_checks_its_arguments(hip):
    c = fit_cases.get("plane_m65")
    for form in (-1, 4):
        with pytest.raises(capi.LioError):
            c.run(hip, form)
    fit_cases.check_null_pointers(hip, c)
    assert all(a.shape[0] == 0 for a in fit_cases.get("plane_m0").run(hip, 0))


def test_hook_runs_what_production_runs(hip, oracle):
    """the neighbours lio_knn_walk returns for a realistic sweep, fed to the hook, give lio_calculate_features' answer bit for bit (identity
    transform: the fit sees the stack points themselves, which is what the walk is asked about)"""
    ds = synth.make_dataset("indoor", 2, 0.2)
    surf0, _ = pipeline.feature_clouds(oracle, ds.lidar, ds.frames[0].scan)
    surf1, _ = pipeline.feature_clouds(oracle, ds.lidar, ds.frames[1].scan)
    m, s = oracle.voxel_grid(surf0, 0.4), oracle.voxel_grid(surf1, 0.4)
    T = capi.TransformF.make((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
    va, ca, sa = hip.calculate_features(m, s, T)
    cell = np.float32(np.sqrt(np.float32(1.0))) * np.float32(1.0001) + np.float32(1e-6)      # knn_cell_edge(min_match_sq_dis)
    idx, sqd, nbr = hip.knn_walk(m, s, float(cell), 8)
    vb, cb, sb, ab = hip.fit_five(0, nbr, sqd[:, 4], s, T)
    assert va.sum() > 500 and (va == 0).sum() > 10
    fit_ref.compare_bits((va, ca, sa, np.zeros_like(ab)), (vb, cb, sb, ab), "lio_calculate_features vs walk + hook")
