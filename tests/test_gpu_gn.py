"""The Gauss-Newton rows, folds and step the product runs (csrc/cloud_device.h: odom_row_form, fold_partials28_wide, odom_update_from_sums;
csrc/cloud_kernels.h: reduce_partials28; csrc/odometry.hip: odo_update_step; the production launches launch_kf_rows and launch_odom_round;
through the test hooks lio_gn_rows_map, lio_gn_fold, lio_gn_step and lio_gn_round) against the references of tests/gn_ref.py on the cases of
tests/gn_cases.py — the same comparisons and constants the oracle meets in tests/test_gn.py, where the cases' contents and the comparisons'
sensitivity are tested without a GPU — and against the oracle."""
import numpy as np
import pytest

import gn_cases
import gn_ref
from lio_amd import capi

pytestmark = pytest.mark.gpu

MAP_IDS = [f"{n}-form{f}" for n, f in gn_cases.MAP_RUNS]
STEPS = [n for n in gn_cases.STEP_NAMES if not n.startswith("nan")]


# ------------------------------------------------------------------------------------------------ rows and their sums
@pytest.mark.parametrize("name,form", gn_cases.MAP_RUNS, ids=MAP_IDS)
def test_product_rows_and_sums(hip, name, form):
    """ONE launch_kf_rows (a table of one record) with the production block count: the rows against fp64, the count exactly, every other sum within the bound of
    any fp64 summation order of the fp32 products of the rows"""
    c = gn_cases.get_map(name)
    ok, rows, part = c.run(hip, form)
    ref = c.ref(form)
    assert part.shape == (gn_cases.rows_blocks(c.m), 28)
    print(f"{name} form {form}: largest row error / scale {gn_ref.rows_ratio(rows, ref):.3f} (constant {gn_ref.C_MAP_ROWS:.3g}), {part.shape[0]} blocks")
    gn_ref.compare_rows((ok, rows), ref, gn_ref.C_MAP_ROWS, f"{name} form {form}")
    worst = gn_ref.compare_sums(part, ok, rows, f"{name} form {form}")
    print(f"  sums: largest |difference| / bound {worst:.3g}")


@pytest.mark.parametrize("name", gn_cases.MAP_NAMES)
def test_rows_equal_the_oracle_in_bits(hip, oracle, name):
    """same statements, same order, -ffp-contract=off on both sides"""
    c = gn_cases.get_map(name)
    for form in (0, 1, 2):
        a, b = c.run(hip, form), c.run(oracle, form)
        gn_ref.compare_bits(a[:2], b[:2], f"{name} form {form}, product vs oracle")
        gn_ref.compare_sums_pair(a[2], b[2], a[0], a[1], f"{name} form {form}, product's partials vs the oracle's")


def test_rows_hook_checks_its_arguments(hip):
    gn_cases.check_rows_null_pointers(hip)
    ok, rows, part = gn_cases.get_map("m0").run(hip, 0)
    assert ok.shape == (0,) and rows.shape == (0, 7) and part.shape == (1, 28) and not part.any()


# ------------------------------------------------------------------------------------------------ rows of the scan-to-scan loop
@pytest.mark.parametrize("name", gn_cases.ODOM_NAMES)
def test_odom_rows_and_sums(hip, name):
    """ONE launch of k_ob_rows over the one-sensor table Process fills: the count exactly, every other sum within the bound of any fp64 summation
    order of the fp32 products of the rows the one-query-per-lane kernel returns (with and without de-skewing)"""
    c = gn_cases.get_odom(name)
    ok, rows, part = c.run(hip)
    assert ok.shape == (c.nq,) and rows.shape == (c.nq, 7) and part.shape == (gn_cases.odo_blocks(c.nq), 28)
    assert not rows[ok == 0].view(np.uint32).any()
    worst = gn_ref.compare_sums(part, ok, rows, name)
    print(f"{name}: {int(ok.sum())} rows of {c.nq} queries in {part.shape[0]} blocks; sums: largest |difference| / bound {worst:.3g}")


@pytest.mark.parametrize("name", gn_cases.ODOM_NAMES)
def test_odom_rows_meet_fp64(hip, name):
    """edge and plane coefficients, weight and row against fp64 on the sel the product reports — with de-skewing too, where bits are not asked
    for —; `ok` wherever the weight is outside its band of 0.1"""
    c = gn_cases.get_odom(name)
    got, ref = c.run(hip), c.ref(c.sel(hip))
    print(f"{name}: largest error / scale {gn_ref.odom_rows_ratio(got, ref, gn_ref.C_ODOM_ROWS):.3f} (constant {gn_ref.C_ODOM_ROWS:.3g})")
    n_chk, n_left = gn_ref.compare_odom_rows(got, ref, gn_ref.C_ODOM_ROWS, what=name)
    assert n_chk + n_left == c.nq


@pytest.mark.parametrize("name", gn_cases.ODOM_BITS)
def test_odom_rows_equal_the_oracle_in_bits(hip, oracle, name):
    """without de-skewing both sides hold the same statements (-ffp-contract=off): ok and every row, the -1 slots, ld2 == 0 and pd2 == 0, and
    the non-finite row of the collinear triple included"""
    c = gn_cases.get_odom(name)
    a, b = c.run(hip), c.run(oracle)
    n_nan = gn_ref.compare_rows_bits(a[:2], b[:2], f"{name}, product vs oracle")
    if c.special:
        assert (n_nan > 0) == (c.iter == 4)
    if n_nan == 0:
        gn_ref.compare_sums_pair(a[2], b[2], a[0], a[1], f"{name}, product's partials vs the oracle's")


def test_odom_rows_hook_checks_its_arguments(hip):
    gn_cases.check_odom_rows_arguments(hip)


def test_hooks_run_what_production_runs(hip, oracle):
    """lio_odom_create with num_max_iterations = 1 and two synthetic sweeps: the first entry of the second sweep's iteration trace is
    lio_gn_step(family 1, lio_gn_fold(partials of lio_gn_rows_odom at lio_odom_correspondences' indices and the transform_es the sweep starts
    from, narrow)) bit for bit, and the selected count is the hooks' count"""
    from lio_amd import synth
    sweeps, _, lid = synth.make_sweeps("indoor", 2)
    cl = []
    for sw in sweeps:
        pp = capi.PointProcessor(oracle, lid.lower_deg, lid.upper_deg, lid.rings)
        pp.process(sw)
        cl.append([pp.cloud(w) for w in (1, 2, 3, 4)])
    od = capi.PointOdometry(hip, 0.1, 2, 1, False)
    od.process(*cl[0])
    r = od.process(*cl[1])
    assert r["iterations"] == 1 and r["trace"].shape == (1, 7)
    T0 = capi.TransformF.make((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))          # transform_es_ before the first iterating sweep
    sharp, flat, last_corner, last_surf = cl[1][0], cl[1][2], cl[0][1], cl[0][3]
    ci, si, _ = hip.odom_correspondences(sharp, flat, last_corner, last_surf, T0, 0.1, False)
    ok, rows, part = hip.gn_rows_odom(sharp, flat, last_corner, last_surf, ci, si, T0, 0, 0.1, False)
    st = hip.gn_step(1, hip.gn_fold(part, 0), gn_cases.state(), 0)
    assert int(st["nsel"]) == int(ok.sum()) == r["num_selected"] > 100
    got = np.asarray(st["T"], np.float32)[:7]
    want = np.ascontiguousarray(r["trace"][0], np.float32)
    assert (want == r["trace"][0]).all()
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), (got, want)


# ------------------------------------------------------------------------------------------------ folds
@pytest.mark.parametrize("wide", [0, 1])
def test_product_folds_integers_exactly(hip, wide):
    """reduce_partials28 on 256 threads / fold_partials28_wide on 1024: integer partials add exactly in every order, so the sums are numpy's in
    bits; the position-coded set names a dropped or doubled row"""
    for nb in gn_cases.NBLOCKS:
        Q = gn_ref.position_coded(nb)
        gn_ref.compare_fold(hip.gn_fold(Q, wide), Q, f"fold of the position-coded set, wide {wide}")
        P = gn_cases.integer_partials(nb)
        gn_ref.compare_fold(hip.gn_fold(P, wide), P, f"fold, wide {wide}")


def test_fold_hook_checks_its_arguments(hip):
    gn_cases.check_fold_arguments(hip)


# ------------------------------------------------------------------------------------------------ step
@pytest.mark.parametrize("name", STEPS)
def test_product_step_meets_fp64(hip, oracle, name):
    c = gn_cases.step_case(name)
    ref, out = c.ref(), c.run(hip)
    ratio = gn_ref.compare_step(c.state_in, out, ref, left_update=c.left_update, what=name, check_X=c.check_X)
    print(f"{name}: |X - X_ref| / (EPS32 cond |X|) {ratio:.3f} (constant {gn_ref.C_QR:.3g})")
    if c.kind == "rankdef":
        # the dropped pivot's component is 0 in bits, on both sides
        j = c.expect["zero"]
        for lib in (hip, oracle):
            X = gn_ref.read_back_X(c.state_in, c.run(lib))
            assert X[j] == 0 and np.isfinite(X).all(), (name, X)


@pytest.mark.parametrize("name", [n for n in gn_cases.STEP_NAMES if n.startswith("nan")])
def test_step_on_a_nan_sum_equals_the_oracle_pattern(hip, oracle, name):
    c = gn_cases.step_case(name)
    a, b = c.run(hip), c.run(oracle)
    Ta, Tb = np.asarray(a["T"]), np.asarray(b["T"])
    assert (np.isfinite(Ta) == np.isfinite(Tb)).all(), (Ta, Tb)
    if name.endswith("one_rhs"):
        assert (Ta[4:7].view(np.uint32) == 0).all()                      # t resets to 0
    fin = np.isfinite(Tb)
    assert (Ta[fin].view(np.uint32) == Tb[fin].view(np.uint32)).all(), (Ta, Tb)
    for k in ("converged", "iters", "degenerate", "kz", "nsel"):
        assert int(a[k]) == int(b[k]), (k, int(a[k]), int(b[k]))


def test_step_hook_checks_its_arguments(hip):
    gn_cases.check_step_arguments(hip)


# ------------------------------------------------------------------------------------------------ one round through the production launch pair
@pytest.mark.parametrize("m", gn_cases.ROUND_M)
def test_round_is_rows_fold_and_step(hip, m):
    """launch_odom_round at round 0, keep 0, with 4 and 8 lanes per query: the partials' count and sums are those of the rows lio_gn_rows_map
    forms at lio_calculate_features' answer; the state is lio_gn_step(lio_gn_fold(partials, wide)) in bits; the sums hang on the lanes per query
    no further than the summation bound"""
    map_xyzi, stack, (q, t) = gn_cases.round_scene(m)
    T = capi.TransformF.make(q, t)
    valid, coeff, _ = hip.calculate_features(map_xyzi, stack, T)
    ok, rows, _ = hip.gn_rows_map(0, stack, valid, coeff, T)
    if m >= 63:
        assert valid.mean() > 0.8
    parts = {}
    for lpq in (4, 8):
        part, st = hip.gn_round(map_xyzi, stack, T, lpq)
        assert part.shape == (max(1, -(-m * lpq // 256)), 28)
        gn_ref.compare_sums(part, ok, rows, f"round, m {m}, {lpq} lanes per query")
        st2 = hip.gn_step(0, hip.gn_fold(part, 1), gn_cases.state(q, t), 0, 0, 0)
        gn_ref.compare_bits((np.array(st).reshape(1).view(np.uint32),), (np.array(st2).reshape(1).view(np.uint32),), f"round's state vs fold + step, m {m}, lpq {lpq}")
        assert int(st["nsel"]) == int(valid.sum()) and int(st["iters"]) == 1
        parts[lpq] = part
    gn_ref.compare_sums_pair(parts[4], parts[8], ok, rows, f"round, m {m}: 4 vs 8 lanes per query")
    assert parts[8].shape[0] == 625 if m == 20000 else True


def test_round_hook_checks_its_arguments(hip):
    map_xyzi, stack, (q, t) = gn_cases.round_scene(33)
    T = capi.TransformF.make(q, t)
    for lpq in (0, 1, 2, 16):
        with pytest.raises(capi.LioError):
            hip.gn_round(map_xyzi, stack, T, lpq)
    with pytest.raises(capi.LioError):
        hip.gn_round(map_xyzi, stack, capi.TransformF.make((0.0, 0.0, 0.0, float("nan")), t), 8)
    with pytest.raises(capi.LioError):
        hip.gn_round(map_xyzi, stack, T, 8, min_match_sq_dis=0.0)
    part, st = hip.gn_round(map_xyzi, stack[:0], T, 8)
    assert part.shape == (0, 28) and int(st["iters"]) == 0 and (np.asarray(st["T"])[:7] == np.r_[q, t].astype(np.float32)).all()
