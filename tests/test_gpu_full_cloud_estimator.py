"""The estimator's full-cloud ring (include/lio_full_cloud.h; Estimator.cc:482, :2355-2420) on the GPU.

Window: window_size 4 / opt_window_size 2 on the `indoor` synthetic dataset, driven like tests/test_gpu_map_refresh.py: three frames while
the estimator is not initialised (each preceded by the map's own process, which registers the full cloud), the window injected through
the test hooks (pipeline.init_window), then W + 2 steps as set_full_cloud / push_frame / solve / slide — enough for the ring of W + 1
to wrap.  The ring's bookkeeping is held to tests/full_cloud_ref.py's FullRingModel (exact), the corrected clouds to the de-skew hook bit
for bit and to the float64 evaluation under the kernel tests' bound, the registered cloud to the float32 rigid map bit for bit and its
pose to the float64 evaluation within 4 float ulps (both sides round one double expression once; the margin covers a different
quaternion-extraction branch, as in tests/test_gpu_map_refresh.py).

Full clouds are every 14th point of a sweep's ring-ordered cloud (2058 -> cut to 2049 points, intensity = ring + rel_time).
"""
import functools

import numpy as np
import pytest

from lio_amd import capi, pipeline, replay, synth
import full_cloud_ref as ref
from full_cloud_ref import FULL_MAP_FRAME, FULL_SENSOR_END, FULL_SENSOR_RAW, FullRingModel

pytestmark = pytest.mark.gpu

W, WO = 4, 2
N_PRE, N_STEPS = 3, W + 2
PIVOT1 = W - WO + 1
IDENT = ([0, 0, 0, 1], [0, 0, 0])
GPU_BOUND = ref.GPU_BOUND_FACTOR * ref.K_DESKEW
REPORT_KEYS = [k for k, _ in capi.SolveReport._fields_ if not k.startswith("ms_")]


@functools.lru_cache(maxsize=None)
def _data():
    hip = capi.load_hip()
    ds = synth.make_dataset("indoor", W + 1 + N_STEPS, 0.2)
    clouds, fulls = [], []
    for f in ds.frames:
        pp = capi.PointProcessor(hip, ds.lidar.lower_deg, ds.lidar.upper_deg, ds.lidar.rings)
        pp.process(f.scan)
        clouds.append((pp.cloud(capi.PointProcessor.LESS_FLAT), pp.cloud(capi.PointProcessor.LESS_SHARP)))     # (surf, corner)
        fulls.append(np.ascontiguousarray(pp.cloud(capi.PointProcessor.RINGS)[::14][:2049]))
    assert all(1000 < len(c) <= 2049 for c in fulls)
    assert np.any(fulls[-1][:, 3] != np.trunc(fulls[-1][:, 3]))
    return ds, clouds, fulls


def _cfg(hip, ds, deskew, device_solve=0):
    cfg = pipeline.config_indoor(hip, W, WO)
    cfg.keep_features, cfg.prior_factor = 0, 1
    cfg.enable_deskew, cfg.cutoff_deskew = (1, 0) if deskew else (0, 0)
    cfg.init_window_factor = 1
    cfg.device_solve = device_solve
    pipeline.set_extrinsic(cfg, ds)
    return cfg


def _imu(est, f):
    for j in range(f.imu_dt.shape[0]):
        est.process_imu(float(f.imu_dt[j]), f.imu_acc[j], f.imu_gyr[j], float(f.imu_t[j]))


def _integral(c):
    c = c.copy()
    c[:, 3] = np.trunc(c[:, 3])
    return c


def _assert_T_within_4_ulps(got, want):
    for g, w_ in zip(got, want):
        assert g.dtype == np.float32 and w_.dtype == np.float32
        ulp = np.spacing(np.abs(w_))
        d = np.abs(g.astype(np.float64) - w_.astype(np.float64)) / ulp.astype(np.float64)
        print("  T ulps", d)
        assert np.all(d <= 4.0), (g, w_, d)


def _check_ring(est, model, what):
    """every window frame: the entry's bytes and state, or no entry"""
    for i in range(W + 1):
        e = model.entry(i)
        got, state = est.full_stack(i)
        if e is None:
            assert state is None and len(got) == 0, (what, i)
        else:
            assert state == e["state"], (what, i, state, e["state"])
            assert got.tobytes() == e["cloud"].tobytes(), (what, i)


def _drive(hip, deskew, full_on):
    ds, clouds, fulls = _data()
    est = capi.Estimator(hip, _cfg(hip, ds, deskew))
    if full_on:
        est.set_full_cloud(True)
    emap = est.map()
    ident_T = capi.TransformF.make(*IDENT)
    model = FullRingModel(W, WO)
    out = dict(est=est, windows=[], reports=[], worst=0.0, t_es=[])
    emap.process(clouds[0][1], clouds[0][0], IDENT)             # seeding, no full cloud yet
    assert len(emap.full_cloud()) == 0
    # ---- before initialisation: the odometry has carried the cloud to the sweep's end (integer intensities), the map registers it
    for k in range(N_PRE):
        _imu(est, ds.frames[k])
        if full_on:
            emap.set_full_cloud(_integral(fulls[k]))
        emap.process(clouds[k][1], clouds[k][0], IDENT)
        if full_on:
            registered = emap.full_cloud()
            assert registered.tobytes() == ref.rigid_map32(_integral(fulls[k]), *emap.transform_tobe_mapped()).tobytes()
            model.push(registered, inited=False)
        est.process_laser_odom(ident_T, clouds[k][0], clouds[k][1], ds.frames[k].t)
        assert est.stage()["event"] == "filling" and not est.stage()["inited"]
        _check_ring(est, model, f"pre {k}")
    if full_on:
        with pytest.raises(capi.LioError):
            est.registered_full(N_PRE - 1)                       # LIO_ERR_STATE before initialisation
    pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=3)
    model.seed_window()
    _check_ring(est, model, "injected window")
    for j in range(1, N_STEPS + 1):
        k = W + j
        f = ds.frames[k]
        _imu(est, f)
        pushed = fulls[k] if deskew else _integral(fulls[k])     # with both switches off the odometry stays enabled: integer intensities
        if full_on:
            emap.set_full_cloud(pushed)
        est.push_frame(ident_T, clouds[k][0], clouds[k][1], f.t)
        if full_on:
            q, t = est.full_transform_es(W)
            out["t_es"].append((q, t))
            model.push(pushed, inited=True, t_es=(q, t))
            _check_ring(est, model, f"step {j} pushed")
            assert est.full_stack(W)[1] == FULL_SENSOR_RAW
        rep = est.solve()
        w = est.get_window()
        out["windows"].append(w)
        out["reports"].append({key: (list(getattr(rep, key)) if key == "cost_trace" else getattr(rep, key)) for key in REPORT_KEYS})
        if full_on:
            T = capi.TransformF.make(q, t)
            assert model.solved(lambda c, t_es: hip.deskew_to_end(c, T, 10.0, True))
            _check_ring(est, model, f"step {j} solved")          # the newest entry == the hook on what was pushed, bit for bit
            got, state = est.full_stack(W)
            assert state == FULL_SENSOR_END and got[:, 3].tobytes() == pushed[:, 3].tobytes()
            r = ref.worst_ratio(got[:, :3], pushed, q, t, time_factor=10.0, form="est", keep_intensity=True)
            out["worst"] = max(out["worst"], r)
            assert r <= GPU_BOUND, (j, r)
            if not deskew:
                assert got.tobytes() == pushed.tobytes()         # identity transform_es_, s = 0: an exact no-op
            # ---- /local/full_points registered by its frame's pose
            e = model.local_full_points()
            if e is not None and e["state"] == FULL_SENSOR_END:
                (rq, rp), pts = est.registered_full(PIVOT1)
                _assert_T_within_4_ulps((rq, rp), ref.lidar_pose(w["Rs"], w["Ps"], w["q_lb"], w["t_lb"], PIVOT1))
                assert pts.tobytes() == ref.rigid_map32(e["cloud"], rq, rp).tobytes()
                assert len(pts) == len(e["cloud"]) > 1000 and not np.array_equal(pts[:, :3], e["cloud"][:, :3])
                out["registered"] = out.get("registered", 0) + 1
            else:
                with pytest.raises(capi.LioError):
                    est.registered_full(PIVOT1)                  # LIO_ERR_STATE on a map-frame entry / a frame without an entry
            _check_ring(est, model, f"step {j} registered")      # out of place: the ring is as it was
            if j == N_STEPS:                                     # a second solve of the same window corrects nothing
                est.solve()
                assert not model.solved()
                _check_ring(est, model, "second solve")
        est.slide()
    est.sync()
    out["model"] = model
    return out


_RUNS = {}


def _shared(hip, deskew, full_on):
    key = (deskew, full_on)
    if key not in _RUNS:
        _RUNS[key] = _drive(hip, deskew, full_on)
    return _RUNS[key]


def test_ring_follows_the_model_and_the_newest_entry_is_corrected_once(hip):
    out = _shared(hip, True, True)
    print(f"worst |entry - fp64| / (2^-24 (|p| + |t|)) over {N_STEPS} solves: {out['worst']:.3f} (bound {GPU_BOUND:.2f})")
    assert all(np.linalg.norm(t) > 1e-4 for _, t in out["t_es"])            # a real transform_es_ at every step
    assert out["registered"] == N_STEPS - 1                      # step 1 meets the last map-frame entry at pivot + 1
    m = out["model"]
    assert [m.entry(i)["state"] for i in range(W + 1)] == [FULL_SENSOR_END] * (W + 1)      # the ring has wrapped: no map-frame entry left
    assert N_PRE + N_STEPS > W + 1


def test_both_deskew_switches_off_the_correction_is_an_exact_no_op(hip):
    out = _shared(hip, False, True)
    for q, t in out["t_es"]:
        np.testing.assert_array_equal(q, np.array([0, 0, 0, 1], np.float32))
        np.testing.assert_array_equal(t, np.zeros(3, np.float32))
    assert out["worst"] == 0.0 and out["registered"] == N_STEPS - 1


@pytest.mark.parametrize("deskew", [True, False])
def test_switch_off_holds_nothing_and_the_solve_does_not_move(hip, deskew):
    on, off = _shared(hip, deskew, True), _shared(hip, deskew, False)
    for i in range(W + 1):
        pts, state = off["est"].full_stack(i)
        assert len(pts) == 0 and state is None
    with pytest.raises(capi.LioError):
        off["est"].registered_full(PIVOT1)
    assert len(on["windows"]) == len(off["windows"]) == N_STEPS
    for wa, wb in zip(on["windows"], off["windows"]):
        for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "q_lb", "t_lb"):
            np.testing.assert_array_equal(wa[key], wb[key], err_msg=key)
    assert on["reports"] == off["reports"]
    assert on["reports"][-1]["n_lidar_residuals"] > 100 and on["reports"][-1]["iterations"] > 0


def test_switching_off_and_restoring_drop_the_ring(hip):
    ds, clouds, fulls = _data()
    est = capi.Estimator(hip, _cfg(hip, ds, True))
    est.set_full_cloud(True)
    pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=3)
    ident_T = capi.TransformF.make(*IDENT)
    est.snapshot()
    _imu(est, ds.frames[W + 1])
    est.map().set_full_cloud(fulls[W + 1])
    est.push_frame(ident_T, clouds[W + 1][0], clouds[W + 1][1], ds.frames[W + 1].t)
    est.solve()
    assert est.full_stack(W)[1] == FULL_SENSOR_END
    est.restore()                                                # snapshots do not carry full clouds
    assert est.full_stack(W)[1] is None
    est.solve()                                                  # ... and a solve of the restored window has nothing to correct
    assert all(est.full_stack(i)[1] is None for i in range(W + 1))
    est.slide()
    _imu(est, ds.frames[W + 1])
    est.push_frame(ident_T, clouds[W + 1][0], clouds[W + 1][1], ds.frames[W + 1].t)
    assert est.full_stack(W)[1] == FULL_SENSOR_RAW and len(est.full_stack(W)[0]) == len(fulls[W + 1])
    est.set_full_cloud(False)                                    # turning it off drops the ring
    assert est.full_stack(W)[1] is None
    est.set_full_cloud(True)
    assert est.full_stack(W)[1] is None


def test_the_kept_transform_es_is_the_one_the_surf_cloud_was_deskewed_with(hip):
    """The hook's transform_es_ against the production path, not against itself: with a leaf too small for the cloud the VoxelGrid
    returns its input (pcl: "leaf size is too small"), so the pushed surf stack IS the de-skewed surf cloud, point for point, and
    must equal the production de-skew (keep = 0) of the surf input under the transform_es_ kept with the full-cloud entry."""
    ds, clouds, fulls = _data()
    cfg = _cfg(hip, ds, True)
    cfg.surf_filter_size = 1e-4                                  # 40 m / 1e-4 per axis: far beyond the filter's index range
    est = capi.Estimator(hip, cfg)
    est.set_full_cloud(True)
    pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=3)
    ident_T = capi.TransformF.make(*IDENT)
    seen = []
    for k in (W + 1, W + 2):
        _imu(est, ds.frames[k])
        est.map().set_full_cloud(fulls[k])
        est.push_frame(ident_T, clouds[k][0], clouds[k][1], ds.frames[k].t)
        q, t = est.full_transform_es(W)
        surf = est.get_surf_stack(W)
        assert len(surf) == len(clouds[k][0]) > 500              # nothing was filtered away
        want = hip.deskew_to_end(clouds[k][0], capi.TransformF.make(q, t), 10.0, False)
        assert surf.tobytes() == want.tobytes(), k
        assert not np.array_equal(surf[:, :3], clouds[k][0][:, :3])
        seen.append(np.concatenate([q, t]))
        est.solve()
        est.slide()
    assert not np.array_equal(seen[0], seen[1])                  # a transform per step, not a constant


def test_copy_snapshot_and_the_restored_solves_drop_the_ring(hip):
    ds, clouds, fulls = _data()
    ests = []
    for seed in (3, 5, 7):
        e = capi.Estimator(hip, _cfg(hip, ds, True))
        e.set_full_cloud(True)
        pipeline.init_window(e, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=seed)
        ests.append(e)
    ident_T = capi.TransformF.make(*IDENT)
    k = W + 1

    def step(e):
        _imu(e, ds.frames[k])
        e.map().set_full_cloud(fulls[k])
        e.push_frame(ident_T, clouds[k][0], clouds[k][1], ds.frames[k].t)
        e.solve()
        pts, state = e.full_stack(W)
        assert state == FULL_SENSOR_END and len(pts) == len(fulls[k])
        return pts

    a, b, c = ests
    corrected = step(a)
    a.solve()                                                    # a repeated solve of the same window: not corrected twice
    assert a.full_stack(W)[0].tobytes() == corrected.tobytes() and a.full_stack(W)[1] == FULL_SENSOR_END
    a.snapshot()
    assert a.full_stack(W)[1] == FULL_SENSOR_END                 # taking a snapshot leaves the ring alone
    # lio_est_copy_snapshot drops the DESTINATION's ring, the source keeps its own
    step(b)
    b.copy_snapshot_of(a)
    assert all(b.full_stack(i)[1] is None for i in range(W + 1))
    assert a.full_stack(W)[0].tobytes() == corrected.tobytes()
    # lio_est_solve_restored: every step restores first, so nothing is left to correct and nothing is held
    a.solve_restored(2)
    assert all(a.full_stack(i)[1] is None for i in range(W + 1))
    with pytest.raises(capi.LioError):
        a.registered_full(W)
    # lio_est_batch_solve_restored over two members that hold corrected entries
    step(c)
    c.snapshot()
    b.restore()
    step(b)
    b.snapshot()
    batch = capi.EstimatorBatch(hip, [b, c])
    batch.solve_restored(2)
    batch.sync()
    for e in (b, c):
        assert all(e.full_stack(i)[1] is None for i in range(W + 1))
    batch.close()


def test_a_batch_member_ends_with_the_bytes_of_the_handle_solved_alone(hip):
    ds, clouds, fulls = _data()
    ests = []
    for device_solve, seed in ((1, 3), (0, 3), (0, 5)):
        e = capi.Estimator(hip, _cfg(hip, ds, True, device_solve))
        e.set_full_cloud(True)
        pipeline.init_window(e, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=seed)
        ests.append(e)
    solo, member, other = ests
    batch = capi.EstimatorBatch(hip, [member, other])
    ident_T = capi.TransformF.make(*IDENT)
    for j in range(1, 3):
        k = W + j
        for e in ests:
            _imu(e, ds.frames[k])
            e.map().set_full_cloud(fulls[k])
            e.push_frame(ident_T, clouds[k][0], clouds[k][1], ds.frames[k].t)
        solo.solve()
        batch.solve()
        for i in range(W + 1):
            (a, sa), (b, sb) = solo.full_stack(i), member.full_stack(i)
            assert sa == sb and a.tobytes() == b.tobytes(), (j, i)
        assert solo.full_stack(W)[1] == FULL_SENSOR_END and other.full_stack(W)[1] == FULL_SENSOR_END
        assert not np.array_equal(solo.full_stack(W)[0][:, :3], fulls[k][:, :3])
        if j == 2:
            (qa, pa), ca = solo.registered_full(PIVOT1)
            (qb, pb), cb = member.registered_full(PIVOT1)
            np.testing.assert_array_equal(qa, qb), np.testing.assert_array_equal(pa, pb)
            assert ca.tobytes() == cb.tobytes() and len(ca) > 1000
        for e in ests:
            e.slide()
    batch.close()


def _replay(hip, n_sweeps, sweeps, full_cloud):
    sw, _, lid = sweeps
    cfg = pipeline.config_indoor(hip, 6, 3)
    cfg.transform_lb = capi.TransformF.make([0, 0, 0, 1], [0.0, 0.0, -0.081939])
    cfg.init_window_factor, cfg.extrinsic_stage = 1, 1
    msgs, sizes = [], []
    rp = replay.Replay(hip, cfg, lid, odom_io=2, tap=lambda kind, *m: msgs.append(m[1].copy()) if kind == "compact" else None, full_cloud=full_cloud)
    traj = synth.Trajectory()
    h, t_imu, t0 = 1.0 / 200.0, 1.0, 1.0
    steps = []
    for k, s in enumerate(sw[:n_sweeps]):
        t_end = t0 + 0.1 * (k + 1)
        while t_imu <= t_end + h + 1e-9:
            rp.add_imu(t_imu, traj.accel(t_imu), traj.gyro(t_imu))
            t_imu += h
        n0, m0 = len(rp.log), len(msgs)
        rp.add_sweep(s, t_end)
        if len(msgs) > m0:
            sizes.append(int(rp.pp.lib.dll.lio_pp_count(rp.pp.h, capi.PointProcessor.RINGS)))
        for e in rp.log[n0:]:
            steps.append((e["event"], rp.est.full_stack(min(len(rp.log) - 1, 6))))   # the newest frame: the window fills up to W + 1 frames
    return rp, msgs, sizes, steps


def test_replay_carries_the_full_cloud_and_the_default_stays_the_empty_block(hip):
    W6 = 6
    n = 2 * (W6 + 1 + 3) + 2                                     # odom_io 2: the initialisation plus three steps
    sweeps = synth.make_sweeps("indoor", n)
    rp, msgs, sizes, steps = _replay(hip, n, sweeps, True)
    events = [ev for ev, _ in steps]
    assert "initialised" in events
    k0 = events.index("initialised")
    post = steps[k0 + 1:]
    assert len(post) >= 3 and all(ev == "solved" for ev, _ in post)
    assert len(sizes) == len(steps)                              # every message is processed as it arrives
    for i, (ev, (pts, state)) in enumerate(steps):
        size = sizes[i]
        assert len(pts) == size > 20000, (i, ev)
        assert state == (FULL_SENSOR_END if i > k0 else FULL_MAP_FRAME), (i, ev, state)
    # the odometry is disabled once the estimator is initialised with a de-skew switch on: the pushed cloud is the raw sweep
    assert np.any(post[-1][1][0][:, 3] != np.trunc(post[-1][1][0][:, 3]))
    assert np.all(steps[k0][1][0][:, 3] == np.trunc(steps[k0][1][0][:, 3]))
    # ---- the default Replay: the empty full block, byte for byte what the same call encoded before the argument existed
    m = 4
    _, plain, _, _ = _replay(hip, 2 * m + 1, sweeps, False)
    assert len(plain) == m
    for a, b in zip(plain, msgs):
        T, corner, surf, full = hip.compact_decode(b)
        assert len(full) > 20000
        Ta, ca, sa, fa = hip.compact_decode(a)
        assert len(fa) == 0
        again = hip.compact_encode(capi.TransformF.make(*T), corner, surf, np.zeros((0, 4), np.float32))
        assert np.asarray(a).tobytes() == np.asarray(again).tobytes()
