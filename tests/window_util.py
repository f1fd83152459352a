"""Helpers shared by the GPU parity tests that drive the product and the oracle through the same window."""
import numpy as np

from lio_amd import capi, pipeline, synth


def make_pair(libs, kind, W, Wo, n_frames, frame_dt, keep=0, deskew=False, prior_factor=1, seed=3, sigmas=(0.01, 0.001, 0.01), pp_lib=None,
              cfg_fields=None):
    """One estimator per library in `libs`, all initialised with the same window (frames 0..W of a seeded synthetic
    run, ground truth + the same perturbation) and the same stacks.  Feature clouds come from `pp_lib` (default: the
    last library, i.e. the oracle in (hip, oracle)).  cfg_fields: further lio_est_config fields (execution switches such as
    device_solve, which the oracle ignores)."""
    ds = synth.make_dataset(kind, n_frames, frame_dt)
    pp_lib = pp_lib or libs[-1]
    clouds = [pipeline.feature_clouds(pp_lib, ds.lidar, f.scan) for f in ds.frames]
    ests = []
    for lib in libs:
        cfg = pipeline.config_indoor(lib, W, Wo) if kind == "indoor" else pipeline.config_outdoor64(lib, W, Wo)
        cfg.keep_features = keep
        cfg.prior_factor = prior_factor
        cfg.cutoff_deskew = 0 if deskew else 1
        for k, v in (cfg_fields or {}).items():
            setattr(cfg, k, v)
        pipeline.set_extrinsic(cfg, ds)
        est = capi.Estimator(lib, cfg)
        pipeline.init_window(est, lib, ds, [c[0] for c in clouds], pos_sigma=sigmas[0], rot_sigma=sigmas[1], vel_sigma=sigmas[2], seed=seed)
        ests.append(est)
    return ds, clouds, ests


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1)))


def window_gap(wa, wb):
    """(max |dP| m, max rotation angle rad, max |dV|, max |dBa|, max |dBg|) between two get_window() results."""
    return (float(np.max(np.abs(wa["Ps"] - wb["Ps"]))), max(rot_angle(a, b) for a, b in zip(wa["Rs"], wb["Rs"])),
            float(np.max(np.abs(wa["Vs"] - wb["Vs"]))), float(np.max(np.abs(wa["Bas"] - wb["Bas"]))), float(np.max(np.abs(wa["Bgs"] - wb["Bgs"]))))


def assert_windows_close(wa, wb, tol_p=1e-4, tol_r=1e-4):
    dp, dr, dv, dba, dbg = window_gap(wa, wb)
    assert dp < tol_p, dp            # 1e-4 m (north_star)
    assert dr < tol_r, dr            # 1e-4 rad
    assert dv < 1e-3 and dba < 1e-3 and dbg < 1e-4, (dv, dba, dbg)


def assert_cost_trace_close(ra, rb, rtol_floor=1e-6):
    """Per-iteration cost trace (the summary Ceres prints, Estimator.cc:1990-2021) within 1e-6 relative (SURVEY.md §8d
    config 3), with the two effects that are NOT solver differences taken out explicitly:

    * newest-frame factor flips: the two newest-frame Gauss-Newton loops sum their fp32 rows in different orders, so a
      borderline feature of the NEWEST frame may be accepted by one side only; each such factor moves the total by about
      one residual's share (the bound is exactly 1e-6 whenever the factor sets are equal).  With keep_features the newest
      frame keeps the factor list of EVERY round (up to 10), each fitted at a round transform that differs at the fp32 level,
      and a factor gained in one round can offset one lost in another without changing the count: callers pass
      rtol_floor = 2e-4 there (measured: 7e-5 on one of six steps, 3e-8 on the others);
    * the marginalization prior's constant: `linearized_residuals = S^-1/2 V^T b` (MarginalizationFactor.cc:293-302)
      inverts every eigenvalue above the ABSOLUTE 1e-8 cut, including the gauge directions whose eigenvalues are rounding
      noise of a matrix with entries ~1e9; 0.5 |r0|^2 along those directions is a constant of the solve (their Jacobian
      rows are ~1e-4) that differs between two evaluations of the same prior at the 1e-4 level.  It is the same for every
      entry of the trace, equals the difference of the reported prior cost, and is bounded separately."""
    assert ra.iterations == rb.iterations
    n = min(rb.iterations + 1, 32)
    ta, tb = np.asarray(ra.cost_trace[:n]), np.asarray(rb.cost_trace[:n])
    flips = abs(ra.n_lidar_residuals - rb.n_lidar_residuals)
    tol = rtol_floor + 20.0 * flips / max(rb.n_lidar_residuals, 1)
    offset = ta[0] - tb[0]
    prior_gap = ra.cost_marg_before - rb.cost_marg_before
    if flips == 0 and rtol_floor <= 1e-6:
        assert abs(offset - prior_gap) <= 1e-6 * tb[0], (offset, prior_gap)      # the whole offset is the prior's constant
    assert abs(prior_gap) <= 2e-4 * tb[0], (prior_gap, tb[0])
    np.testing.assert_allclose(ta - prior_gap, tb, rtol=tol, atol=0)
    assert np.all(np.diff(tb) <= 0)  # the trace holds the cost of the ACCEPTED point: it never increases
    return float(np.max(np.abs(ta - prior_gap - tb) / np.abs(tb))), flips


def assert_priors_close(ea, eb, ra=None, rb=None, rel_floor=1e-6, tol_x0=1e-4, tol_ex=1e-4):
    """The marginalization prior each side produced ITSELF in the step just taken (before any teacher forcing overwrites
    it): same size, |dJtJ| / max|JtJ| <= 1e-6, linearisation point within 1e-4.  JtJ sums every lidar factor of the window
    (each PivotPointPlaneFactor touches the marginalised pivot pose), so a newest-frame factor accepted by one side only
    (see assert_cost_trace_close) moves it by about one residual's share: the bound widens by 20 / n_res per such flip.
    x0 = pose1, sb1, pose2 .. poseWo, extrinsic: the last 7 entries are the extrinsic, which has its own bound
    `tol_ex` — with prior_factor = 0 (the shipped indoor value) nothing anchors it and it is only weakly observable, so two
    solves that agree to 1e-5 m on every pose may differ by a few 1e-4 in it.
    Returns (relative JtJ gap, |dx0| over the states, flips)."""
    pa, pb = ea.prior(), eb.prior()
    if pb is None:
        assert pa is None
        return 0.0, 0.0, 0
    assert pa is not None and pa["n"] == pb["n"]
    flips = abs(ra.n_lidar_residuals - rb.n_lidar_residuals) if ra is not None else 0
    n_res = max(rb.n_lidar_residuals, 1) if rb is not None else 1
    rel = float(np.max(np.abs(pa["JtJ"] - pb["JtJ"])) / np.abs(pb["JtJ"]).max())
    relr = float(np.max(np.abs(pa["Jtr"] - pb["Jtr"])) / max(np.abs(pb["Jtr"]).max(), 1e-300))
    d = np.abs(pa["x0"] - pb["x0"])
    dx0, dex = float(np.max(d[:-7])), float(np.max(d[-7:]))
    assert rel <= rel_floor + 20.0 * flips / n_res, (rel, flips)
    assert dx0 <= tol_x0, dx0
    assert dex <= tol_ex, dex
    return max(rel, 0.0), dx0, flips


def force_window(dst, src_window, ds):
    """Teacher forcing: the states of `src_window` become the states of estimator `dst` (lio_est_set_window)."""
    dst.set_window(src_window["Ps"], src_window["Rs"], src_window["Vs"], src_window["Bas"], src_window["Bgs"], np.array([0, 0, -ds.g]))


def force_all(dst, src, ds):
    """Everything the next ProcessLaserOdom reads besides the clouds: window states, extrinsic, marginalization prior."""
    w = src.get_window()
    force_window(dst, w, ds)
    dst.set_extrinsic(w["q_lb"], w["t_lb"])
    pf = src.prior_factor()
    if pf is not None:
        dst.set_prior_factor(pf)
