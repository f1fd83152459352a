"""The device-resident dogleg (csrc/solve_step.h under DevExec: k_bw_aux and phases P1 - P6 of k_bw_solve_step) against the plain
longdouble references of tests/ds_ref.py, number by number (docs/device_solve_pins.md).

A normal chain runs until the window holds a marginalization prior and convergence_flag_ is set; the next solve is then stopped behind
its first linearisation (lio_est_set_max_num_iterations 0) or behind the decision on its first candidate (1), and
lio_est_batch_get_linearization reads the problem, the state and the aux row back.  The reference is evaluated on the very fp64 numbers
the device read; the assertion is |Q - R| <= 16 u entrywise, u from the reference alone (ds_ref.with_unit); integer outcomes, flags and
structural zeros are exact; the candidate step takes the bound of tests/test_gpu_dev_solver.py for a solve through a factorisation.

Shapes: window_size = Wo + 2, Wo = 2 (n 45 / 51, n_pad 48 / 64), 5 (90 / 96, 96) and 6 (105 / 111, 112) — the largest window the step
kernel's LDS holds.  Wo = 7 (n_pad 128) needs 183 KB of the 160 KB and is solved by the single-window path: asserted below."""
import os
import sys

import numpy as np
import pytest

import ds_ref as R
from lio_amd import capi, pipeline, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

WOS = (2, 5, 6)
BASE = dict(opt_extrinsic=1, prior_factor=1, empty_frame=False, absent_pim=False)
VARIANTS = {
    "free_extrinsic": BASE,
    "fixed_extrinsic": dict(BASE, opt_extrinsic=0),
    "no_extrinsic_prior": dict(BASE, prior_factor=0),
    "frame_without_residuals": dict(BASE, empty_frame=True),
    "absent_pim": dict(BASE, absent_pim=True),
}
WORST = {}   # largest |Q - R| / u per array over the module, printed by the last test


@pytest.fixture(scope="module")
def world(hip):
    ds = synth.make_dataset("indoor", 12, 0.2)
    clouds = [pipeline.feature_clouds(hip, ds.lidar, f.scan) for f in ds.frames]
    return dict(ds=ds, clouds=clouds, ctx={}, solved={}, refs={})


def _push(est, ds, k, surf, corner):
    f = ds.frames[k]
    for j in range(f.imu_dt.shape[0]):
        est.process_imu(float(f.imu_dt[j]), f.imu_acc[j], f.imu_gyr[j], float(f.imu_t[j]))
    est.push_frame(capi.TransformF.make([0, 0, 0, 1], [0, 0, 0]), surf, corner, f.t)


def _make_est(hip, world, Wo, v):
    ds, clouds = world["ds"], world["clouds"]
    W = Wo + 2
    cfg = pipeline.config_indoor(hip, W, Wo)
    cfg.keep_features, cfg.cutoff_deskew, cfg.device_solve = 0, 1, 0
    cfg.prior_factor, cfg.opt_extrinsic = v["prior_factor"], v["opt_extrinsic"]
    pipeline.set_extrinsic(cfg, ds)
    est = capi.Estimator(hip, cfg)
    pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=3)
    return est


def _run_chain(world, batch, ests, variants):
    """two solves and slides, the third frame pushed, the variant's change applied, a snapshot: the next solve is the one under test"""
    ds, clouds = world["ds"], world["clouds"]
    for step in range(2):
        batch.solve()
        for e in ests:
            e.slide()
            k = e.W + 1 + step
            _push(e, ds, k, clouds[k][0], clouds[k][1])
    for e, v in zip(ests, variants):
        pivot = e.W - e.cfg.opt_window_size
        if v["empty_frame"]:   # the newest frame's stack (the one frame that is not part of the local map) moved out of every neighbour's reach
            st = e.get_surf_stack(e.W).copy()
            st[:, 0] += 500.0
            e.set_surf_stack(e.W, st)
        if v["absent_pim"]:    # a pre-integration over more than ten seconds is left out of the problem (Estimator.cc:1693)
            f = ds.frames[e.W]
            reps = int(np.ceil(10.5 / f.imu_dt.sum()))
            e.set_preintegration(pivot + 1, f.imu_acc[0], f.imu_gyr[0], np.zeros(3), np.zeros(3), np.tile(f.imu_dt, reps), np.tile(f.imu_acc, (reps, 1)),
                                 np.tile(f.imu_gyr, (reps, 1)))
        e.snapshot()


def _ctx(hip, world, Wo, name):
    key = (Wo, name)
    if key not in world["ctx"]:
        v = VARIANTS[name]
        est = _make_est(hip, world, Wo, v)
        batch = capi.EstimatorBatch(hip, [est])
        _run_chain(world, batch, [est], [v])
        world["ctx"][key] = dict(est=est, batch=batch, v=v, Wo=Wo, name=name)
    return world["ctx"][key]


def _solve(world, c, n_iter, threads=0, w=0):
    """the snapshot solved once with max_num_iterations = n_iter -> dict(lin, S at the accepted point, report, prior before the solve)"""
    key = (c["Wo"], c["name"], n_iter, threads, id(c["batch"]), w)
    if key not in world["solved"]:
        est, batch = c["est"], c["batch"]
        est.restore()
        before = dict(prior=est.prior(), factor=est.prior_factor(), window=est.get_window())
        est.set_max_num_iterations(n_iter)
        batch.set_option("aux_threads", threads)
        rep = batch.solve_restored(1)[w]
        lin = batch.linearization(w)
        S, Rt = batch.moments(w)
        world["solved"][key] = dict(lin=lin, S=S, Rt=Rt, rep=rep, before=before, after=est.get_window())
        est.set_max_num_iterations(10)
        batch.set_option("aux_threads", 0)
    return world["solved"][key]


def _note(name, got, ref, unit):
    r = R.ratio(got, ref, unit)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"    {name}: |Q - R| / u = {r:.3f}")
    return r


def _ref(world, tag, lin, fn, inp, seed):
    """reference values and unit, computed once per distinct input (aux_threads variants and repeated solves share them)"""
    parts = [np.asarray(inp[k], np.float64).tobytes() for k in R.FLOAT_KEYS if k in inp]
    parts += [np.asarray(pm[k], np.float64).tobytes() for pm in inp["pim"] if pm is not None for k in R.PIM_KEYS]
    key = (tag, lin["Wo"], lin["n"], hash(b"".join(parts)))
    if key not in world["refs"]:
        world["refs"][key] = R.with_unit(fn, inp, seed=seed)
    return world["refs"][key]


def _check_aux_row(world, oracle, lin, v):
    """imu_out, lmap, prior_out, exprior_out and cand_Rt against the reference at the returned cand"""
    meta, inp = R.meta_of(lin), R.inputs_of(lin, "cand")
    ref, unit = _ref(world, "aux", lin, lambda q: R.aux_row(meta, q, oracle), inp, seed=lin["Wo"])
    Wo = lin["Wo"]
    assert list(lin["present"]) == [0 if (v["absent_pim"] and i == 0) else 1 for i in range(Wo)]
    np.testing.assert_array_equal(lin["imu_out"][:, 931], np.asarray(lin["present"], float))
    if v["absent_pim"]:
        assert not lin["imu_out"][0].any()            # a factor without a pre-integration gives zeros
    bad = []
    for name, got in (("imu_out", lin["imu_out"]), ("lmap", lin["lmap"][:, :247]), ("cand_Rt", lin["cand_Rt"])):
        if _note(name, got, ref[name], unit[name]) > R.GPU_MARGIN:
            bad.append(name)
    assert not lin["lmap"][:, 247].any()
    assert lin["have_prior"] == 1
    if _note("prior_out", lin["prior_out"], ref["prior_out"], unit["prior_out"]) > R.GPU_MARGIN:
        bad.append("prior_out")
    if lin["use_ex_prior"]:
        if _note("exprior_out", lin["exprior_out"][:43], ref["exprior_out"], unit["exprior_out"]) > R.GPU_MARGIN:
            bad.append("exprior_out")
    assert not bad, bad


def _check_problem(s, v, Wo):
    """the packed problem: layout integers and the prior the solve read equal the prior taken before the solve"""
    lin, before = s["lin"], s["before"]
    F = Wo + 1
    assert (lin["Wo"], lin["n"], lin["ex_col"]) == (Wo, 15 * F + 6 * v["opt_extrinsic"], 15 * F if v["opt_extrinsic"] else -1)
    assert lin["n_pad"] == (lin["n"] + 15) // 16 * 16 and lin["use_ex_prior"] == v["prior_factor"]
    assert lin["need_host"] == 0 and lin["started"] == 1 and lin["done"] == 1
    pf, pr = before["factor"], before["prior"]
    assert pf is not None and lin["n_prior"] == pf["n"]
    np.testing.assert_array_equal(lin["prior"]["lin_jac"], pf["lin_jac"])
    np.testing.assert_array_equal(lin["prior"]["lin_res"], pf["lin_res"])
    np.testing.assert_array_equal(lin["prior"]["JtJ"], pr["JtJ"])
    np.testing.assert_array_equal(lin["prior"]["Jtr0"], pr["Jtr"])
    np.testing.assert_array_equal(lin["prior_x0"][:pf["x0"].size], pf["x0"])
    sizes = [int(k[2]) for k in lin["keep"]]
    assert sum(6 if z == 7 else z for z in sizes) == pf["n"] and sum(sizes) == pf["x0"].size
    cols = lin["prior_col"]
    assert sorted(c for c in cols if c >= 0) == sorted(set(c for c in cols if c >= 0))     # no prior column twice


def _check_linearisation(world, oracle, s, tag, fixed_scale=None):
    """scale, Hcur, g (and at the first linearisation costs0) against the reference assembly at the returned x"""
    lin = s["lin"]
    meta = R.meta_of(lin)
    inp = R.inputs_of(lin, "x", S=s["S"], scale=fixed_scale)
    ref, unit = _ref(world, tag, lin, lambda q: R.assemble(meta, q, oracle), inp, seed=50 + lin["Wo"])
    bad = []
    names = [("Hcur", lin["Hcur"], "H"), ("g", lin["g"], "g")]
    if fixed_scale is None:
        names += [("scale", lin["scale"], "scale"), ("costs0", lin["costs0"], "costs")]
    for name, got, key in names:
        if _note(name, got, ref[key], unit[key]) > R.GPU_MARGIN:
            bad.append(name)
    zero = np.asarray(unit["H"] == 0)
    assert zero.any() and not lin["Hcur"][zero].any()          # entries no factor touches: exactly zero, pad rows never leak
    assert not bad, bad
    return ref


def _params_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("pose", "sb", "ex"))


def _tangent(x, cand, meta):
    """the tangent step that takes x to cand (the inverse of Plus): dp, 2 vec(q_x^-1 q_cand) / w, plain differences elsewhere"""
    d = np.zeros(meta["n"])

    def pose(a, b):
        qa, qb = R.q_of_pose(a), R.q_of_pose(b)
        dq = R.qmul(R.qinv(qa), qb)
        return np.r_[b[:3] - a[:3], np.asarray(2 * dq[1:] / dq[0], np.float64)]

    for f in range(meta["Wo"] + 1):
        d[15 * f:15 * f + 6] = pose(x["pose"][f], cand["pose"][f])
        d[15 * f + 6:15 * f + 15] = cand["sb"][f] - x["sb"][f]
    if meta["ex_col"] >= 0:
        d[meta["ex_col"]:] = pose(x["ex"], cand["ex"])
    return d


def _check_one_iteration(world, oracle, s0, s1, ref0):
    """cand against CeresDogleg's first step on the reference's normal equations; the decision, radius, mu and counters against
    CeresDogleg.decide at the device's own candidate cost; H, g at the point the hook returns with the scale fixed at the start"""
    from second_source import CeresDogleg

    l0, l1 = s0["lin"], s1["lin"]
    meta = R.meta_of(l1)
    n = meta["n"]
    assert _params_equal(l0["x"], l0["cand"])
    np.testing.assert_array_equal(l1["scale"], l0["scale"])                    # fixed at the first linearisation
    H0, g0 = np.asarray(ref0["H_unscaled"], np.float64), np.asarray(ref0["g_unscaled"], np.float64)
    cost0 = float(ref0["costs"].sum())
    dl = CeresDogleg(H0, g0, cost0)
    delta, model = dl.compute_step()
    assert delta is not None, "CeresDogleg: invalid first step"
    # the candidate: a solve through a factorisation (tests/test_gpu_dev_solver.py's bound), mapped back through the Jacobi scale
    A = dl.H + np.diag(dl.diag ** 2 * dl.mu)
    cond = np.linalg.cond(A)
    y = np.abs(dl.gn / dl.diag).max()
    bound = dl.scale * (1e-13 * cond * y + 1e-12 * y)
    x0 = l0["x"]
    got = _tangent(x0, l1["cand"], meta)
    ambient = np.concatenate([np.abs(np.r_[x0["pose"][f][:3], np.ones(3), x0["sb"][f]]) for f in range(meta["Wo"] + 1)] + ([np.abs(np.r_[x0["ex"][:3], np.ones(3)])] if meta["ex_col"] >= 0 else []))
    floor = 8 * R.EPS64 * np.maximum(ambient, 1.0)                                 # cand = x + step rounds once in the ambient space
    err = np.abs(got - delta)
    print(f"    candidate: cond {cond:.2e}  max |step| {np.abs(delta).max():.3e}  max err / bound {np.max(err / (bound + floor)):.3e}")
    assert np.all(err <= bound + floor), float(np.max(err / (bound + floor)))
    # the decision at the device's own candidate cost: the sums launch B forms, in its order
    pim = 0.0
    for i in range(meta["Wo"]):
        if l1["imu_out"][i, 931] != 0.0:
            pim += l1["imu_out"][i, 930]
    ppp = 0.0
    for f in range(meta["Wo"]):
        ppp += l1["cand_moments"][f, 256]
    marg = l1["prior_out"][l1["n_prior"]] if l1["have_prior"] else 0.0
    cand_cost = marg + pim + ppp + (l1["exprior_out"][42] if l1["use_ex_prior"] else 0.0)
    xs = [x0["pose"][: meta["Wo"] + 1].ravel(), x0["sb"][: meta["Wo"] + 1].ravel()] + ([x0["ex"]] if meta["ex_col"] >= 0 else [])
    x_norm = float(np.sqrt(np.sum(np.concatenate(xs) ** 2)))
    cs = [(l1["cand"]["pose"] - x0["pose"]).ravel(), (l1["cand"]["sb"] - x0["sb"]).ravel()] + ([l1["cand"]["ex"] - x0["ex"]] if meta["ex_col"] >= 0 else [])
    step_norm = float(np.sqrt(np.sum(np.concatenate(cs) ** 2)))
    np.testing.assert_allclose(l1["step_norm"], step_norm, rtol=1e-12)
    verdict = dl.decide(cand_cost, model, step_norm, x_norm)
    print(f"    decision {verdict}: cost {cost0:.9g} -> {cand_cost:.9g}, model change {model:.6g} (device {l1['model_change']:.6g}), radius {l1['radius']:.6g}, mu {l1['mu']:.3g}")
    # alpha and the model change go through ds_vHv: a dot product of n terms rounds by at most n eps times the sum of its absolute terms,
    # and the model moves with the step by its gradient g + H s times the factorisation's bound
    sstep = delta / dl.scale
    aH, B = np.abs(dl.H), 1e-13 * cond * y + 1e-12 * y
    M_model = np.abs(sstep) @ np.abs(dl.g) + 0.5 * np.abs(sstep) @ (aH @ np.abs(sstep))
    tol_model = n * R.EPS64 * M_model + np.abs(dl.g + dl.H @ sstep).sum() * B
    print(f"    model change |dev - ref| / tol {abs(l1['model_change'] - model) / tol_model:.3f}")
    assert abs(l1["model_change"] - model) <= tol_model, (l1["model_change"], model, tol_model)
    # alpha = |grad|^2 / (sg^T H sg) from the device's OWN scaled H and g of the first linearisation (the run stopped at n = 0 returned
    # them; same bits here): what is compared is ds_vHv and the sums around it, by the rounding bound of their dot products
    Hd, gd = R.ld(l0["Hcur"]), R.ld(l0["g"])
    dd = np.sqrt(np.clip(np.diag(Hd), 1e-6, 1e32))
    grad = gd / dd
    sg = grad / dd
    den = sg @ (Hd @ sg)
    alpha_ref = float((grad @ grad) / den)
    tol_alpha = alpha_ref * (n + 8) * R.EPS64 * float(1 + (np.abs(sg) @ (np.abs(Hd) @ np.abs(sg))) / den)
    print(f"    alpha {l1['alpha']:.15g}  |dev - ref| / tol {abs(l1['alpha'] - alpha_ref) / tol_alpha:.3f}")
    assert abs(l1["alpha"] - alpha_ref) <= tol_alpha, (l1["alpha"], alpha_ref, tol_alpha)
    assert l1["it"] == 1 and l1["done"] == 1
    if verdict == "accept":
        assert (l1["successful"], l1["termination"]) == (1, 0)
        assert _params_equal(l1["x"], l1["cand"]) and l1["x_cost"] == cand_cost
        np.testing.assert_array_equal(s1["S"], l1["cand_moments"])
    elif verdict == "reject":
        assert (l1["successful"], l1["termination"]) == (0, 0)
        assert _params_equal(l1["x"], x0) and not _params_equal(l1["x"], l1["cand"])
        np.testing.assert_array_equal(s1["S"], s0["S"])
    else:
        assert (l1["successful"], l1["termination"]) == (0, 2 if verdict == "func_tol" else 1)
        assert _params_equal(l1["x"], x0)
    if verdict in ("accept", "reject"):
        assert l1["mu"] == dl.mu
        # the radius is a multiple of the step's norm after a good step: the factorisation's bound, relative
        np.testing.assert_allclose(l1["radius"], dl.radius, rtol=1e-13 * cond + 1e-12)
    return verdict


def _check_everything(hip, oracle, world, Wo, name):
    c = _ctx(hip, world, Wo, name)
    print(f"\n  Wo = {Wo}, {name}")
    s0, s1 = _solve(world, c, 0), _solve(world, c, 1)
    for s in (s0, s1):
        _check_problem(s, c["v"], Wo)
    l0 = s0["lin"]
    # n = 0: one linearisation, nothing moves, and the host write-back takes it
    assert (l0["it"], l0["successful"], l0["termination"], l0["ntrace"]) == (0, 0, 0, 1)
    assert (s0["rep"].iterations, s0["rep"].successful_steps, s0["rep"].termination) == (0, 0, 0)
    assert _params_equal(l0["x"], l0["cand"])
    np.testing.assert_array_equal(l0["x"]["pose"][:, :3], s0["before"]["window"]["Ps"][c["est"].W - Wo:])
    for k in ("Ps", "Vs", "Bas", "Bgs", "Rs"):   # (the write-back re-anchors the yaw through Euler angles in degrees: 5e-11 on a rotation matrix)
        np.testing.assert_allclose(s0["after"][k], s0["before"]["window"][k], rtol=0, atol=1e-9 if k == "Rs" else 1e-12, err_msg=k)
    np.testing.assert_array_equal(s0["S"], l0["cand_moments"])
    assert l0["trace"][0] == l0["x_cost"] and s0["rep"].initial_cost == l0["x_cost"]
    if c["v"]["empty_frame"]:
        assert s0["S"][Wo - 1, 257] == 0 and not s0["S"][Wo - 1].any() and s0["S"][:Wo - 1, 257].all()
    else:
        assert s0["S"][:, 257].all()
    _check_aux_row(world, oracle, l0, c["v"])
    ref0 = _check_linearisation(world, oracle, s0, "lin0")
    _check_aux_row(world, oracle, s1["lin"], c["v"])
    verdict = _check_one_iteration(world, oracle, s0, s1, ref0)
    _check_linearisation(world, oracle, s1, "lin1", fixed_scale=s1["lin"]["scale"])
    return verdict


@pytest.mark.parametrize("threads", [64, 128, 256])
@pytest.mark.parametrize("Wo", WOS)
def test_aux_row(hip, oracle, world, Wo, threads):
    """the five jobs of aux_imu land on other waves at 64, 128 and 256 threads: each against the reference, at cand after one step"""
    c = _ctx(hip, world, Wo, "free_extrinsic")
    s = _solve(world, c, 1, threads)
    assert not _params_equal(s["lin"]["x"], s["lin"]["cand"]) or s["lin"]["successful"] == 1
    _check_aux_row(world, oracle, s["lin"], c["v"])
    base = _solve(world, c, 1)["lin"]
    for k in ("imu_out", "lmap", "prior_out", "exprior_out", "cand_Rt", "Hcur", "g"):
        np.testing.assert_array_equal(s["lin"][k], base[k], err_msg=k)


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("Wo", (2, 6))
def test_first_linearisation_and_one_iteration(hip, oracle, world, Wo, name):
    _check_everything(hip, oracle, world, Wo, name)


def test_first_linearisation_and_one_iteration_at_five_frames(hip, oracle, world):
    _check_everything(hip, oracle, world, 5, "free_extrinsic")


def test_first_solves_and_seven_frames_are_not_on_the_device(hip, world):
    """LIO_ERR_STATE for a window the device loop did not solve: the first solve with a free extrinsic (the problem changes shape:
    need_host), and a window of seven optimised frames (n_pad = 128: the step kernel's LDS does not hold it)"""
    est = _make_est(hip, world, 2, BASE)
    batch = capi.EstimatorBatch(hip, [est])
    rep = batch.solve()[0]
    assert rep.iterations >= 1 and rep.convergence_flag == 0
    with pytest.raises(capi.LioError):
        batch.linearization(0)
    with pytest.raises(capi.LioError):
        est.set_max_num_iterations(-1)
    batch.close()
    est = _make_est(hip, world, 7, dict(BASE, opt_extrinsic=0))
    batch = capi.EstimatorBatch(hip, [est])
    rep = batch.solve()[0]
    assert rep.iterations >= 1
    with pytest.raises(capi.LioError):
        batch.linearization(0)
    batch.close()


def test_mixed_batch(hip, oracle, world):
    """windows of 2, 5, 6 and 7 optimised frames in one batch: each device window meets the reference and equals, bit for bit, what it
    returns as a batch of one; the window of seven is solved by the single-window path"""
    wos = (2, 5, 6, 7)
    ests = [_make_est(hip, world, Wo, BASE) for Wo in wos]
    batch = capi.EstimatorBatch(hip, ests)
    _run_chain(world, batch, ests, [BASE] * len(wos))
    for n_iter in (0, 1):
        for e in ests:
            e.set_max_num_iterations(n_iter)
        batch.solve_restored(1)
        for w, Wo in enumerate(wos):
            if Wo == 7:
                with pytest.raises(capi.LioError):
                    batch.linearization(w)
                continue
            lin = batch.linearization(w)
            S, _ = batch.moments(w)
            solo = _solve(world, _ctx(hip, world, Wo, "free_extrinsic"), n_iter)
            for k in ("imu_out", "lmap", "prior_out", "exprior_out", "cand_Rt", "cand_moments", "Hcur", "g", "scale", "costs0", "trace"):
                np.testing.assert_array_equal(lin[k], solo["lin"][k], err_msg=f"Wo {Wo} n {n_iter} {k}")
            for k in ("it", "successful", "termination", "radius", "mu", "model_change", "step_norm", "x_cost"):
                assert lin[k] == solo["lin"][k], (Wo, n_iter, k)
            assert _params_equal(lin["x"], solo["lin"]["x"]) and _params_equal(lin["cand"], solo["lin"]["cand"])
            np.testing.assert_array_equal(S, solo["S"])
            _check_aux_row(world, oracle, lin, BASE)
            if n_iter == 0:
                _check_linearisation(world, oracle, dict(lin=lin, S=S), "lin0")
    batch.close()


def test_zz_report_ratios(world):
    """the largest |Q - R| / u per array over this module (docs/device_solve_pins.md records them); closes the module's batches"""
    print("\nlargest |Q - R| / u per array:", {k: round(v, 3) for k, v in WORST.items()})
    assert max(WORST.values(), default=0.0) <= R.GPU_MARGIN
    for c in world["ctx"].values():
        c["batch"].close()
