"""Seven optimised frames on the device trust-region loop (include/lio_est_wide.h, docs/wide_window.md): window 12 / optimisation
window 7 of the reference's indoor_test_config.yaml — 126 tangent unknowns (120 with a constant extrinsic), n_pad = 128, the step
kernel's LDS shared between the lidar blocks and the arrays first written in P6.

* lio_est_set_device_solve_limit: 6 by default, 7 admits the window, anything else LIO_ERR_ARG; per handle, untouched by snapshot /
  restore / copy_snapshot; a handle left at 6 is solved by the single-window path next to one at 7 in the same batch;
* a batch of two 12 / 7 windows at limit 7 against two oracle estimators, teacher-forced over six steps: equal flags, iteration
  counts and terminations, windows within 1e-4 m / 1e-4 rad, priors within 1e-5 relative, at least four solves on the device loop;
* a device_solve = 1 handle at Wo = 7 equals, bit for bit, the same window inside a mixed batch of Wo 2, 5, 6 and 7 over solve + slide
  + five more frames; eight identical windows give equal digests of stages 5 .. 9 under loop_groups 1 / 2 and aux_threads 64 / 128 / 256;
* the first linearisation and the first step at Wo = 7 against tests/ds_ref.py, in the unit and with the margin (16 u) of
  tests/test_gpu_ds_linearization.py, free and constant extrinsic;
* the device loop against the host loop at Wo = 7, at the 1e-7 of tests/test_gpu_dev_solver.py.

(lio_dense_spd_solve at n = 120, 126 and 128 is tests/test_gpu_dev_solver.py's.)"""
import numpy as np
import pytest

import test_gpu_ds_linearization as L
from lio_amd import capi, pipeline, synth
from window_util import assert_priors_close, assert_windows_close, force_all, window_gap

pytestmark = pytest.mark.gpu

LIO_ERR_ARG, LIO_ERR_STATE = -1, -2
WINDOW_KEYS = ("Ps", "Rs", "Vs", "Bas", "Bgs", "q_lb", "t_lb")


@pytest.fixture(scope="module")
def world(hip):
    """one indoor scene for the whole module (19 frames: window 12 + the initial solve + six steps); the dict is also the `world` the
    helpers of tests/test_gpu_ds_linearization.py take, with a ratio table of this module's own"""
    ds = synth.make_dataset("indoor", 19, 0.2)
    clouds = [pipeline.feature_clouds(hip, ds.lidar, f.scan) for f in ds.frames]
    saved, L.WORST = L.WORST, {}
    w = dict(ds=ds, clouds=clouds, ctx={}, solved={}, refs={})
    yield w
    for c in w["ctx"].values():
        c["batch"].close()
    L.WORST = saved


def _est(lib, world, W, Wo, seed=3, opt_extrinsic=1, device_solve=0, limit=None, clouds=None):
    ds = world["ds"]
    clouds = clouds or world["clouds"]
    cfg = pipeline.config_indoor(lib, W, Wo)
    cfg.keep_features, cfg.prior_factor, cfg.cutoff_deskew, cfg.opt_extrinsic, cfg.device_solve = 0, 1, 1, opt_extrinsic, device_solve
    pipeline.set_extrinsic(cfg, ds)
    est = capi.Estimator(lib, cfg)
    pipeline.init_window(est, lib, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=seed)
    if limit is not None:
        est.set_device_solve_limit(limit)
    return est


def _push(est, world, k, clouds=None):
    c = (clouds or world["clouds"])[k]
    L._push(est, world["ds"], k, c[0], c[1])


def _rep_key(r):
    return (r.iterations, r.successful_steps, r.termination, r.n_lidar_residuals, r.n_local_map, r.laser_odom_iterations, r.turn_off, r.convergence_flag,
            r.marginalized, r.initial_cost, r.final_cost, tuple(r.cost_trace[:12]))


def _on_device(batch, w):
    """did the device loop solve window w in the batch's last solve (lio_est_batch_get_linearization: LIO_ERR_STATE otherwise)"""
    ni, npb, nst, nax = batch.DSL_SIZES
    ints = np.zeros(ni, np.int32)
    pbm, st, aux = np.zeros(npb), np.zeros(nst), np.zeros(nax)
    rc = batch.lib.dll.lio_est_batch_get_linearization(batch.h, int(w), ints.ctypes.data_as(capi.C.POINTER(capi.C.c_int32)), capi._dp(pbm), capi._dp(st), capi._dp(aux))
    assert rc in (0, LIO_ERR_STATE), rc
    return rc == 0


# ---------------------------------------------------------------------------------------------------- the limit
def test_limit_values_and_what_keeps_it(hip, world):
    est = _est(hip, world, 9, 7)
    assert est.device_solve_limit() == 6
    for bad in (5, 8, 0, -1):
        assert hip.dll.lio_est_set_device_solve_limit(est.h, bad) == LIO_ERR_ARG
        assert est.device_solve_limit() == 6
    assert hip.dll.lio_est_set_device_solve_limit(None, 7) == LIO_ERR_ARG
    est.set_device_solve_limit(7)
    assert est.device_solve_limit() == 7
    est.snapshot()
    est.set_device_solve_limit(6)
    est.restore()
    assert est.device_solve_limit() == 6                       # a choice of the handle, not part of the snapshot
    est.set_device_solve_limit(7)
    other = _est(hip, world, 9, 7)
    other.copy_snapshot_of(est)
    other.restore()
    assert other.device_solve_limit() == 6 and est.device_solve_limit() == 7


def test_a_handle_left_at_six_is_solved_by_the_fallback_beside_one_at_seven(hip, world):
    """two copies of one 9 / 7 window in one batch, constant extrinsic (the device loop takes the very first solve): the handle at limit 7
    runs the device loop, the one left at the default the single-window path; the two agree as the device and host loops do"""
    a, b = _est(hip, world, 9, 7, opt_extrinsic=0), _est(hip, world, 9, 7, opt_extrinsic=0, limit=7)
    batch = capi.EstimatorBatch(hip, [a, b])
    for step in range(3):
        if step > 0:
            for e in (a, b):
                e.slide()
                _push(e, world, 9 + step)
        ra, rb = batch.solve()
        clk = batch.clock()
        assert int(clk["n_device"]) == 1, clk
        assert not _on_device(batch, 0) and _on_device(batch, 1)
        with pytest.raises(capi.LioError, match=f"code {LIO_ERR_STATE}"):
            batch.linearization(0)
        assert batch.linearization(1)["n_pad"] == 128
        assert (ra.iterations, ra.termination, ra.marginalized) == (rb.iterations, rb.termination, rb.marginalized)
        assert_windows_close(a.get_window(), b.get_window())
    batch.close()


# ---------------------------------------------------------------------------------------------------- against the oracle
def test_wide_batch_matches_the_oracle(hip, oracle, world):
    """tests/test_gpu_batch.py::test_batch_matches_the_oracle at indoor 12 / 7 with the limit at 7: the same bounds, and the device loop
    takes the window (the first solves may go to the host while convergence_flag_ still changes the problem's shape)"""
    W, Wo = 12, 7
    ds = world["ds"]
    clouds = [pipeline.feature_clouds(oracle, ds.lidar, f.scan) for f in ds.frames]
    prod, orc = [], []
    for seed in (3, 11):
        prod.append(_est(hip, world, W, Wo, seed=seed, limit=7, clouds=clouds))
        orc.append(_est(oracle, world, W, Wo, seed=seed, clouds=clouds))
    batch = capi.EstimatorBatch(hip, prod)
    worst, on_device = 0.0, 0
    for step in range(6):
        if step > 0:
            k = W + step
            for ea, eb in zip(prod, orc):
                force_all(ea, eb, ds)
                _push(ea, world, k, clouds)
                _push(eb, world, k, clouds)
        ra = batch.solve()
        rb = [e.solve() for e in orc]
        on_device += int(batch.clock()["n_device"])
        for ea, eb, a, b in zip(prod, orc, ra, rb):
            assert (a.convergence_flag, a.turn_off, a.marginalized) == (b.convergence_flag, b.turn_off, b.marginalized), step
            assert a.iterations == b.iterations and a.termination == b.termination, (step, a.iterations, b.iterations)
            assert abs(a.n_lidar_residuals - b.n_lidar_residuals) <= max(5, 0.002 * b.n_lidar_residuals)
            assert_windows_close(ea.get_window(), eb.get_window())
            worst = max(worst, window_gap(ea.get_window(), eb.get_window())[0])
            if step > 0:
                assert_priors_close(ea, eb, a, b, rel_floor=1e-5)
            ea.slide(); eb.slide()
    print(f"batch vs oracle (indoor {W}/{Wo}, limit 7): worst |dP| over the teacher-forced steps {worst:.2e} m; {on_device} window-solves on the device loop")
    assert on_device >= 4
    assert all(_on_device(batch, w) for w in range(2))
    batch.close()


# ---------------------------------------------------------------------------------------------------- batch == alone
def test_wide_window_alone_equals_the_window_in_a_mixed_batch(hip, world):
    """a device_solve = 1 handle at 12 / 7 with the limit at 7 (a batch of one) and the same window as a member of a batch of Wo 2, 5, 6
    and 7, over solve + slide + five more frames: equal reports, equal windows, priors equal in bits"""
    W = 12
    solo = _est(hip, world, W, 7, device_solve=1, limit=7)
    others = [(Wo + 2, _est(hip, world, Wo + 2, Wo)) for Wo in (2, 5, 6)]
    member = _est(hip, world, W, 7, limit=7)
    batch = capi.EstimatorBatch(hip, [e for _, e in others] + [member])
    wide_on_device = 0
    for step in range(6):
        if step > 0:
            for Wk, e in others + [(W, solo), (W, member)]:
                _push(e, world, Wk + step)
        ra = solo.solve()
        rb = batch.solve()[3]
        wide_on_device += int(_on_device(batch, 3))
        assert _rep_key(ra) == _rep_key(rb), (step, _rep_key(ra), _rep_key(rb))
        wa, wb = solo.get_window(), member.get_window()
        for key in WINDOW_KEYS:
            np.testing.assert_array_equal(wa[key], wb[key], err_msg=f"step {step} {key}")
        for _, e in others + [(W, solo), (W, member)]:
            e.slide()
    pa, pb = solo.prior(), member.prior()
    assert pa is not None and pb is not None
    for key in ("JtJ", "Jtr", "x0"):
        np.testing.assert_array_equal(pa[key], pb[key], err_msg=key)
    assert pa["n"] == 57                                        # 6 poses + one speed-bias block + the extrinsic: k_bw_marg_schur at m = 15, n = 57
    print(f"Wo = 7 alone == in a mixed batch over 6 steps; {wide_on_device} of them on the device loop")
    assert wide_on_device >= 2                                  # (two in a row: the second reads the prior the first left on the device)
    batch.close()


def test_identical_wide_windows_agree_under_every_execution_choice(hip, world):
    """eight copies of one 9 / 7 window that holds a prior: digests of stages 5 .. 9 (solver state, moments, Jacobi scaling, scaled
    Hessian, new prior) equal across the windows and across loop_groups 1 / 2 and aux_threads 64 / 128 / 256"""
    W, Wo = 9, 7
    src = _est(hip, world, W, Wo, limit=7)
    b0 = capi.EstimatorBatch(hip, [src])
    for step in range(2):
        b0.solve()
        src.slide()
        _push(src, world, W + 1 + step)
    b0.close()
    src.snapshot()
    clones = []
    for _ in range(8):
        e = _est(hip, world, W, Wo)
        e.copy_snapshot_of(src)
        e.restore()
        e.set_device_solve_limit(7)
        clones.append(e)
    batch = capi.EstimatorBatch(hip, clones)
    first = None
    for groups in (1, 2):
        for aux in (64, 128, 256):
            batch.set_option("loop_groups", groups)
            batch.set_option("aux_threads", aux)
            reps = batch.solve_restored(1)
            assert int(batch.clock()["n_device"]) == 8
            assert reps[0].iterations >= 1 and reps[0].marginalized == 1
            dg = np.stack([batch.stage_digest(s) for s in range(5, 10)])
            for s in range(5):
                bad = np.nonzero(dg[s] != dg[s][0])[0]
                assert bad.size == 0, f"loop_groups {groups} aux_threads {aux}: stage {capi.EstimatorBatch.STAGES[5 + s]} of windows {bad.tolist()} differs from window 0"
            if first is None:
                first = dg
            np.testing.assert_array_equal(dg, first, err_msg=f"loop_groups {groups} aux_threads {aux}")
    batch.close()


# ---------------------------------------------------------------------------------------------------- against tests/ds_ref.py
def _ctx7(hip, world, name):
    """tests/test_gpu_ds_linearization.py's context at Wo = 7 (window 9), the handle's limit at 7"""
    key = (7, name)
    if key not in world["ctx"]:
        v = L.VARIANTS[name]
        est = L._make_est(hip, world, 7, v)
        est.set_device_solve_limit(7)
        batch = capi.EstimatorBatch(hip, [est])
        L._run_chain(world, batch, [est], [v])
        world["ctx"][key] = dict(est=est, batch=batch, v=v, Wo=7, name=name)
    return world["ctx"][key]


@pytest.mark.parametrize("name", ["free_extrinsic", "fixed_extrinsic"])
def test_first_linearisation_and_one_iteration_at_seven_frames(hip, oracle, world, name):
    """n_iter 0 and 1 at n = 126 / 120, n_pad = 128: aux row, scale, Hcur, g, costs0 within 16 u of the longdouble reference; the first
    candidate, the decision, alpha and the model change by the bounds of tests/test_gpu_ds_linearization.py"""
    c = _ctx7(hip, world, name)
    L._check_everything(hip, oracle, world, 7, name)
    lin = L._solve(world, c, 0)["lin"]
    assert (lin["Wo"], lin["n"], lin["n_pad"]) == (7, 126 if name == "free_extrinsic" else 120, 128)


def test_zz_report_wide_ratios(world):
    """the largest |Q - R| / u per array at Wo = 7 (docs/device_solve_pins.md records them)"""
    print("\nlargest |Q - R| / u per array at Wo = 7:", {k: round(v, 3) for k, v in L.WORST.items()})
    assert L.WORST and max(L.WORST.values()) <= L.R.GPU_MARGIN


# ---------------------------------------------------------------------------------------------------- against the host loop
def test_wide_device_loop_equals_host_loop(hip, world):
    """tests/test_gpu_dev_solver.py::test_device_loop_equals_host_loop at 9 / 7: the window in a batch of one at limit 7 and the same
    window through the host loop, in lockstep, the device one handed the host one's states, extrinsic and prior before every step.
    Identical iteration counts, accepted / rejected steps, termination codes and flags; cost traces within 1e-7; states within 1e-7
    after every step; priors equal to 1e-7."""
    W, Wo = 9, 7
    ea, eb = _est(hip, world, W, Wo, limit=7), _est(hip, world, W, Wo)
    batch = capi.EstimatorBatch(hip, [ea])

    def same(a, b):
        assert (a.iterations, a.successful_steps, a.termination) == (b.iterations, b.successful_steps, b.termination)
        assert (a.convergence_flag, a.turn_off, a.marginalized, a.n_lidar_residuals) == (b.convergence_flag, b.turn_off, b.marginalized, b.n_lidar_residuals)
        n = b.iterations + 1
        np.testing.assert_allclose(a.cost_trace[:n], b.cost_trace[:n], rtol=1e-7)
        np.testing.assert_allclose([a.cost_pim_before, a.cost_ppp_before, a.cost_marg_before], [b.cost_pim_before, b.cost_ppp_before, b.cost_marg_before],
                                   rtol=1e-9, atol=1e-12)

    on_device, worst = 0, 0.0
    for step in range(7):
        if step > 0:
            force_all(ea, eb, world["ds"])
            for e in (ea, eb):
                _push(e, world, W + step)
        ra, rb = batch.solve()[0], eb.solve()
        on_device += int(batch.clock()["n_device"])
        same(ra, rb)
        g = window_gap(ea.get_window(), eb.get_window())
        worst = max(worst, g[0])
        assert g[0] < 1e-7 and g[1] < 1e-7, (step, g)
        if rb.marginalized:
            pa, pb = ea.prior(), eb.prior()
            np.testing.assert_allclose(pa["JtJ"], pb["JtJ"], rtol=0, atol=1e-7 * np.abs(pb["JtJ"]).max())
        ea.slide(); eb.slide()
    print(f"device loop == host loop at Wo = 7 over 7 steps, worst |dP| {worst:.2e} m; {on_device} of them on the device loop")
    assert on_device >= 4
    batch.close()
