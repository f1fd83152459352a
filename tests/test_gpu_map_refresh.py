"""The post-initialisation map-database refresh (include/lio_ext.h; Estimator.cc:703-708) on the GPU.

The ring of optimisation-window buffers is held to the plain-Python model of tests/map_refresh_ref.py (exact: bookkeeping and
buffer identity), slot 0's pose to the model's float64 evaluation of :2284-2286 (4 float ulps: both sides round one double expression
once; the margin covers a different quaternion-extraction branch), and the map itself to the ORACLE's UpdateMapDatabase fed with the
hook's arguments, compared as tests/test_gpu_mapping.py::test_update_map_database_rebases_valid_cubes compares that primitive.

Window: window_size 4 / opt_window_size 2, the smallest the step tests initialise with.  The sequence (one per parametrisation,
computed once and shared):
  * both maps take one lio_map_process of the first sweep (an empty map: no optimisation runs);
  * Wo + 1 frames go through lio_est_process_laser_odom while the estimator is NOT initialised: they fill the ring and the reference's
    :616 masks each of their slots;
  * the window is initialised through the test hooks (pipeline.init_window), then Wo + 3 steps are driven as push_frame /
    solve_optimization / refresh_map / slide_window: the first Wo meet a masked slot 0, the last three refresh;
  * after the first refresh both maps take a lio_map_process far away, which shifts the cube centre: the remaining refreshes carry
    a stale centre and a stale valid list.
"""
import functools
import hashlib

import numpy as np
import pytest

from lio_amd import capi, pipeline, synth
from map_refresh_ref import RefreshModel
import test_gpu_mapping as tgm

pytestmark = pytest.mark.gpu

W, WO = 4, 2
N_PRE, N_STEPS = WO + 1, WO + 3
IDENT = ([0, 0, 0, 1], [0, 0, 0])
L, WD = 21, 21


@functools.lru_cache(maxsize=None)
def _data():
    hip = capi.load_hip()
    ds = synth.make_dataset("indoor", W + 1 + N_STEPS, 0.2)
    clouds = [pipeline.feature_clouds(hip, ds.lidar, f.scan) for f in ds.frames]     # (surf, corner)
    return ds, clouds


def _cfg(hip, ds, deskew, same_cloud, device_solve=0):
    cfg = pipeline.config_indoor(hip, W, WO)
    cfg.keep_features, cfg.prior_factor = 0, 1
    cfg.enable_deskew, cfg.cutoff_deskew = (1, 0) if deskew else (0, 0)
    cfg.init_window_factor = 1
    cfg.device_solve = device_solve
    if same_cloud:
        cfg.corner_filter_size = cfg.surf_filter_size
    pipeline.set_extrinsic(cfg, ds)
    return cfg


def _near(cen, pos=(0.0, 0.0, 0.0), r=3):
    c = [int((pos[d] + 25.0) // 50.0) + cen[d] for d in range(3)]
    return [i + L * j + L * WD * k for i in range(c[0] - r, c[0] + r + 1) for j in range(c[1] - r, c[1] + r + 1) for k in range(c[2] - r, c[2] + r + 1)
            if 0 <= i < L and 0 <= j < WD and 0 <= k < 11]


FAR = (400.0, 0.0, 0.0)


def _cube_list(cen):
    """every cube the sequence can touch: three cubes around the origin (the indoor scene is < 100 m wide) and around the far sweep"""
    return sorted(set(_near(cen) + _near(cen, FAR)))


def _digest(m, cen):
    h = hashlib.sha256()
    n = 0
    for idx in _cube_list(cen):
        for cls in (0, 1):
            c = m.cube(cls, idx)
            h.update(c.tobytes())
            n += len(c)
    return h.hexdigest(), n


def _imu(est, f):
    for j in range(f.imu_dt.shape[0]):
        est.process_imu(float(f.imu_dt[j]), f.imu_acc[j], f.imu_gyr[j], float(f.imu_t[j]))


def _assert_T_within_4_ulps(got, want):
    for g, w_ in zip(got, want):
        assert g.dtype == np.float32 and w_.dtype == np.float32
        ulp = np.spacing(np.abs(w_))
        d = np.abs(g.astype(np.float64) - w_.astype(np.float64)) / ulp.astype(np.float64)
        print("  T ulps", d)
        assert np.all(d <= 4.0), (g, w_, d)


def _drive(hip, oracle, deskew, same_cloud, refresh_on=True, via="split", with_oracle=True, snapshot_at=None):
    ds, clouds = _data()
    cfg = _cfg(hip, ds, deskew, same_cloud)
    est = capi.Estimator(hip, cfg)
    if refresh_on:
        est.set_map_refresh(True)
    emap = est.map()
    kw = dict(corner_filter_size=cfg.corner_filter_size, surf_filter_size=cfg.surf_filter_size)
    omap = capi.PointMapping(oracle, **kw) if with_oracle else None
    ident_T = capi.TransformF.make(*IDENT)
    corner_of = (lambda k: clouds[k][0]) if same_cloud else (lambda k: clouds[k][1])
    # ---- seeding
    emap.process(clouds[0][1], clouds[0][0], IDENT)
    cen, valid = emap.cube_state()
    if omap:
        omap.process(clouds[0][1], clouds[0][0], IDENT)
        co, vo = omap.cube_state()
        assert cen == co
        np.testing.assert_array_equal(valid, vo)
        assert tgm._compare_cubes(emap, omap, _cube_list(cen), atol=5e-4, strict=False) > 500
    model = RefreshModel(W, WO, deskew)
    # ---- Wo + 1 frames while not initialised: ring filled, every slot masked (:616)
    for k in range(N_PRE):
        _imu(est, ds.frames[k])
        est.process_laser_odom(ident_T, clouds[k][0], corner_of(k), ds.frames[k].t)
        assert est.stage()["event"] == "filling" and not est.stage()["inited"]
        model.push(IDENT, cen, valid, clouds[k][0], corner_of(k))
        model.end_uninitialised_step()
    if refresh_on:
        with pytest.raises(capi.LioError):
            est.refresh_map()                                   # LIO_ERR_STATE before initialisation
        assert est.last_map_refresh() is None
    pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=3)
    model.seed_window([est.get_surf_stack(i) for i in range(W + 1)])
    out = dict(results=[], hooks=[], windows=[], stale=0, masked=0, est=est, emap=emap, omap=omap)
    digest0 = _digest(emap, cen)
    for j in range(1, N_STEPS + 1):
        k = W + j
        f = ds.frames[k]
        _imu(est, f)
        cen_now, valid_now = emap.cube_state()
        if via == "laser_odom":
            est.process_laser_odom(ident_T, clouds[k][0], corner_of(k), f.t)
            out["windows"].append(est.get_window())
        else:
            est.push_frame(ident_T, clouds[k][0], corner_of(k), f.t)
            pushed = est.get_surf_stack(W)
            if deskew:   # the de-skewed, filtered surf stack is pinned elsewhere; with equal leaves and the same cloud the corner stack must equal it
                model.push(IDENT, cen_now, valid_now, pushed, pushed if same_cloud else None)
            else:
                np.testing.assert_array_equal(pushed, clouds[k][0])
                model.push(IDENT, cen_now, valid_now, clouds[k][0], corner_of(k))
            est.solve()
            if j == 1:
                model.fuse_pivot(est.get_surf_stack(W - WO))
            w = est.get_window()
            out["windows"].append(w)
            model.solved(w["Rs"], w["Ps"], w["q_lb"], w["t_lb"])
            if snapshot_at == j:
                est.snapshot()
            if refresh_on:
                before = _digest(emap, cen_now)
                r = est.refresh_map()
                hook = est.last_map_refresh()
                want, slot = model.refresh(), model.slot0()
                print(f"step {j}: refresh -> {r}; model {'refresh' if want else 'skip'}; centre {slot['cube_center']} (now {cen_now}); "
                      f"{len(hook['corner'])} corner / {len(hook['surf'])} surf points")
                assert r == (1 if want else 0) and hook["applied"] == r
                assert hook["cube_center"] == slot["cube_center"]
                np.testing.assert_array_equal(hook["valid_idx"], np.asarray(slot["valid_idx"], np.uint32))
                np.testing.assert_array_equal(hook["surf"], slot["surf"])
                if slot["corner"] is not None:
                    np.testing.assert_array_equal(hook["corner"], slot["corner"])
                    assert not r or len(hook["corner"]) > 20
                _assert_T_within_4_ulps(hook["T"], slot["T"])
                out["results"].append(r)
                out["hooks"].append(hook)
                if r:
                    assert len(hook["surf"]) > 200
                    out["stale"] += int(hook["cube_center"] != cen_now)
                    if omap:
                        omap.update_map_database(hook["corner"], hook["surf"], hook["valid_idx"], hook["T"], hook["cube_center"])
                        assert tgm._compare_cubes(emap, omap, _cube_list(cen_now), atol=5e-4, strict=False) > 500
                    assert _digest(emap, cen_now) != before
                else:
                    out["masked"] += 1
                    assert _digest(emap, cen_now) == before          # a masked step leaves the map alone
            est.slide()
            model.slide(est.get_surf_stack(W - WO + 1))
        if j == WO + 1:   # a sweep far away: the cube centre moves; what the ring holds is stale from here on
            emap.process(clouds[1][1], clouds[1][0], (IDENT[0], list(FAR)))
            if omap:
                omap.process(clouds[1][1], clouds[1][0], (IDENT[0], list(FAR)))
                assert omap.cube_state()[0] == emap.cube_state()[0]
                np.testing.assert_array_equal(omap.cube_state()[1], emap.cube_state()[1])
            assert emap.cube_state()[0] != cen_now
    est.sync()
    out["prior"] = est.prior()
    out["cen"] = emap.cube_state()[0]
    out["digest0"], out["digest"] = digest0, _digest(emap, out["cen"])
    out["model"] = model
    return out


_RUNS = {}


def _shared(hip, oracle, deskew, same_cloud, refresh_on=True, via="split"):
    """one run per variant for the whole module"""
    key = (deskew, same_cloud, refresh_on, via)
    if key not in _RUNS:
        _RUNS[key] = _drive(hip, oracle, deskew, same_cloud, refresh_on, via, with_oracle=(refresh_on and via == "split"))
    return _RUNS[key]


@pytest.mark.parametrize("deskew,same_cloud", [(False, False), (True, True)])
def test_refresh_matches_the_model_and_the_oracles_update(hip, oracle, deskew, same_cloud):
    """every step: the hook against the model (exact; T within 4 ulps), then the oracle's UpdateMapDatabase with the hook's arguments
    against the product's cubes.  (True, True) also pins the corner path: the same cloud with equal leaves must give the surf stack."""
    out = _shared(hip, oracle, deskew, same_cloud)
    assert out["results"] == [0] * WO + [1] * 3                 # the masks of the uninitialised steps reach slot 0 for Wo solves
    assert out["masked"] == WO and out["stale"] >= 1            # ... and at least one refresh carried a centre that is no longer current
    assert out["digest"] != out["digest0"]
    # the whole map once, strictly cube by cube where both sides hold the same number of points
    assert tgm._compare_cubes(out["emap"], out["omap"], _cube_list(out["cen"]), atol=5e-4, strict=False) > 1000
    # the surround map through lio_est_map: the product's own cubes, concatenated here, through the oracle's VoxelGrid
    import test_gpu_surround_map as sur

    cloud, want = sur._expected(out["emap"], oracle, FAR, out["cen"], 0.6)
    assert len(cloud) > 100
    np.testing.assert_array_equal(out["emap"].surround(0.6), want)


def test_refresh_does_not_feed_back_and_off_means_off(hip, oracle):
    on, off = _shared(hip, oracle, False, False), _shared(hip, oracle, False, False, refresh_on=False)
    assert off["digest"] != off["digest0"]                      # (the far sweep's own Process adds its points)
    assert off["est"].last_map_refresh() is None
    # the same far sweep, no refresh: the cubes around the origin are what the seeding left
    cen = off["cen"]
    h0 = [off["emap"].cube(1, i).tobytes() for i in _near(cen)]
    m = capi.PointMapping(hip)
    ds, clouds = _data()
    m.process(clouds[0][1], clouds[0][0], IDENT)
    m.process(clouds[1][1], clouds[1][0], (IDENT[0], list(FAR)))
    assert m.cube_state()[0] == cen
    assert h0 == [m.cube(1, i).tobytes() for i in _near(cen)]
    for wa, wb in zip(on["windows"], off["windows"]):
        for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "q_lb", "t_lb"):
            np.testing.assert_array_equal(wa[key], wb[key], err_msg=key)
    for key in ("JtJ", "Jtr", "x0"):
        np.testing.assert_array_equal(on["prior"][key], off["prior"][key])


def test_process_laser_odom_refreshes_like_the_split_calls(hip, oracle):
    split, whole = _shared(hip, oracle, False, False), _shared(hip, oracle, False, False, via="laser_odom")
    assert whole["digest"] == split["digest"] and whole["digest"][1] > 1000
    hook = whole["est"].last_map_refresh()
    assert hook["applied"] == 1
    np.testing.assert_array_equal(hook["surf"], split["hooks"][-1]["surf"])
    np.testing.assert_array_equal(hook["T"][0], split["hooks"][-1]["T"][0]), np.testing.assert_array_equal(hook["T"][1], split["hooks"][-1]["T"][1])


def test_snapshot_restore_round_trips_the_ring(hip, oracle):
    out = _drive(hip, oracle, True, True, with_oracle=False, snapshot_at=N_STEPS - 1)
    est = out["est"]
    a = out["hooks"][N_STEPS - 2]                               # the refresh right after the snapshot
    last = out["hooks"][-1]
    assert a["applied"] == 1 and not np.array_equal(a["surf"], last["surf"])
    est.restore()
    assert est.refresh_map() == 1
    b = est.last_map_refresh()
    for key in ("valid_idx", "corner", "surf"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["cube_center"] == b["cube_center"]
    np.testing.assert_array_equal(a["T"][0], b["T"][0]), np.testing.assert_array_equal(a["T"][1], b["T"][1])


def test_refresh_of_a_batch_member_equals_the_window_alone(hip, oracle):
    ds, clouds = _data()
    ests = []
    for device_solve, seed in ((1, 3), (0, 3), (0, 5)):
        cfg = _cfg(hip, ds, False, False, device_solve)
        e = capi.Estimator(hip, cfg)
        e.set_map_refresh(True)
        e.map().process(clouds[0][1], clouds[0][0], IDENT)
        pipeline.init_window(e, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=seed)
        ests.append(e)
    solo, member, other = ests
    batch = capi.EstimatorBatch(hip, [member, other])
    ident_T = capi.TransformF.make(*IDENT)
    res = []
    for j in range(1, WO + 3):
        k = W + j
        for e in ests:
            _imu(e, ds.frames[k])
            e.push_frame(ident_T, clouds[k][0], clouds[k][1], ds.frames[k].t)
        solo.solve()
        batch.solve()
        ra, rb = solo.refresh_map(), member.refresh_map()        # the caller refreshes a member after lio_est_batch_solve; `other` is left alone
        res.append((ra, rb))
        ha, hb = solo.last_map_refresh(), member.last_map_refresh()
        for key in ("valid_idx", "corner", "surf"):
            np.testing.assert_array_equal(ha[key], hb[key], err_msg=f"step {j} {key}")
        np.testing.assert_array_equal(ha["T"][0], hb["T"][0]), np.testing.assert_array_equal(ha["T"][1], hb["T"][1])
        for e in ests:
            e.slide()
    assert res == [(0, 0)] * WO + [(1, 1)] * 2                  # ring not full for Wo steps (:626)
    cen = solo.map().cube_state()[0]
    assert _digest(solo.map(), cen) == _digest(member.map(), cen)
    assert other.last_map_refresh() is None
