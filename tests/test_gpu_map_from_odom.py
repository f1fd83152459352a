"""lio_map_process_batch_from_odom (include/lio_map_from_odom.h) against the host route its header states as the contract.  The rig of
tests/map_from_odom_cases.py steps the raw sweeps of tests/frontend_batch_cases.py through the product's PointProcessor and
lio_odom_process_batch_from_pp once per step, then feeds twin sets of map handles: one by the call under test, one by
lio_odom_get_last_cloud / lio_pp_get_cloud / lio_odom_full_to_end / lio_map_set_full_cloud / lio_map_process_batch.  Every comparison
is bit for bit (uint32 views) over every getter of every map handle after every step, the full cloud included, and every step also holds
every accessor of the odometry handles and the processors to what it answered before the call.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the product library is loaded: both bring a HIP runtime, torch must come first)

from lio_amd import capi, pipeline
import frontend_batch_cases as fbc
import map_batch_cases as mbc
import map_from_odom_cases as cases

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = -1, -2, -4   # include/lio_c.h


def test_one_sensor_with_the_full_cloud_on(hip):
    rig = cases.Rig(hip, [fbc.moving(0, 4)])
    res = [rig.step(k)[0] for k in range(4)]
    assert res[-1]["iterations"] > 0                             # the loop was entered
    nc, ns, nf = rig.counts[-1][0]
    registered, unregistered = rig.fed[0].full_cloud(), rig.unregistered_full(0)
    assert registered.shape == unregistered.shape == (nf, 4) and nf > 0
    assert not np.array_equal(cases.bits(registered), cases.bits(unregistered))   # the step registered what it took


def test_three_moving_sensors_from_pooled_storage(hip):
    """their own filter sizes; a step with every processor, one with pp_or_null == NULL, one with a single null entry"""
    fronts = [fbc.moving(j, 3) for j in range(3)]
    maps = [cases.map_handle(f["name"], j, corner_filter_size=mbc.MOVING_FILTERS[j][0], surf_filter_size=mbc.MOVING_FILTERS[j][1])
            for j, f in enumerate(fronts)]
    rig = cases.Rig(hip, fronts, maps)
    rig.step(0, cases.pooled)
    kept = [cases.bits(m.full_cloud()).copy() for m in rig.fed]
    assert all(len(x) > 0 for x in kept)
    res = rig.step(1, cases.pooled, no_pp_array=True)
    assert all(r["iterations"] > 0 for r in res)
    for m, x in zip(rig.fed, kept):                              # untouched full clouds stay what they were
        assert np.array_equal(cases.bits(m.full_cloud()), x)
    rig.step(2, cases.pooled, with_pp=[True, False, True])
    assert np.array_equal(cases.bits(rig.fed[1].full_cloud()), kept[1])
    for j in (0, 2):
        assert not np.array_equal(cases.bits(rig.fed[j].full_cloud()), kept[j])


def _all_kinds(four_dof):
    fronts = fbc.mixed(2)                                        # moving0, stationary, first_call, packer, thin, empty, moving2, hdl64
    names = [f["name"] for f in fronts]
    maps = cases.one_each(fronts)
    maps.append(cases.map_handle("inited", names.index("moving0"), init_at=1))
    maps.append(cases.map_handle("builder", names.index("moving2"), map_builder=1, enable_4d=1 if four_dof else 0, skip_count=2))
    return fronts, names, maps


@pytest.mark.parametrize("route", ["four_dof_one_after_the_other", "six_dof_one_chain"])
def test_all_kinds_in_one_call(hip, route):
    """odometry on its first call, packer, thin previous sweep, empty sweep, a map handle with the init flag, a MapBuilder handle on an
    optimising and on a skipped call and an HDL-64E in one call, two steps.  With the 4-DoF MapBuilder handle the call has no common launch
    parameters and processes its handles one after the other; with a 6-DoF MapBuilder handle in its place the same kinds share one chain."""
    four_dof = route.startswith("four_dof")
    fronts, names, maps = _all_kinds(four_dof)
    rig = cases.Rig(hip, fronts, maps)
    res = [rig.step(k, cases.pooled) for k in range(2)]
    mnames = [m["name"] for m in maps]
    assert rig.fed[mnames.index("builder")].cfg.enable_4d == (1 if four_dof else 0)
    # the packer's full cloud came through as a byte copy (the odometry is disabled), a moving sensor's through TransformToEnd
    j = names.index("packer")
    assert np.array_equal(cases.bits(rig.unregistered_full(j)), cases.bits(rig.pps[j].cloud(cases.RINGS)))
    j = names.index("moving0")
    assert not np.array_equal(cases.bits(rig.unregistered_full(j)), cases.bits(rig.pps[j].cloud(cases.RINGS)))
    # the empty sweep: zero stack points, and nF == 0 cleared the full cloud
    assert rig.counts[0][names.index("empty")] == (0, 0, 0) and rig.counts[1][names.index("empty")][2] > 0
    # the HDL-64E: a full cloud longer than both stack clouds, more than one block each
    nc, ns, nf = rig.counts[1][names.index("hdl64")]
    assert nf > ns > nc > 256
    # the second step iterates on the map the first one built
    for name in ("moving0", "moving2", "hdl64", "inited"):
        assert res[1][mnames.index(name)]["iterations"] > 0, name
    assert all(r["iterations"] == 0 for r in res[0])             # every handle's first call: no from-map cloud
    assert res[1][mnames.index("builder")]["iterations"] == 0    # skip_count = 2: the second call only updates the map


def test_one_odometry_and_one_processor_feed_a_6dof_and_a_4dof_handle(hip):
    """one call, no common launch parameters: one after the other, each taking its clouds on the device; the MapBuilder handle optimises
    (empty map), skips, optimises"""
    fronts = [fbc.moving(0, 3)]
    maps = [cases.map_handle("mapping", 0), cases.map_handle("builder", 0, map_builder=1, enable_4d=1, skip_count=2)]
    rig = cases.Rig(hip, fronts, maps)
    res = [rig.step(k) for k in range(3)]
    assert [r[1]["iterations"] > 0 for r in res] == [False, False, True]
    assert [r[0]["iterations"] > 0 for r in res] == [False, True, True]


def test_routes_mixed_over_a_handles_life(hip):
    fronts = [fbc.moving(0, 5), fbc.moving(1, 5), fbc.stationary(5)]
    rig = cases.Rig(hip, fronts)
    for k, how in enumerate(["new", "batch", "alone", "new"]):
        rig.step(k, how=how)
    res = rig.step(4, how="new", order=[2, 1, 0])
    assert all(r["iterations"] > 0 for r in res)


def test_the_sources_are_only_read(hip):
    """Rig.step holds every accessor of every odometry handle and processor to what it answered before the call (both last clouds, the
    trace and kz, lio_odom_full_to_end of a 257-point cloud; the five clouds and the picked indices); with twin odometry handles it also
    holds the next lio_odom_process_batch_from_pp to that of twins that never went through the call."""
    fronts = [fbc.moving(0, 3), fbc.moving(2, 3), fbc.packer(3)]
    rig = cases.Rig(hip, fronts, twin_odoms=True)
    for k in range(3):
        rig.step(k, cases.pooled)
    assert rig.last[0]["iterations"] == 25 and rig.last[2]["iterations"] == 0


def test_block_edges_of_the_take_launch(hip):
    """one call, one chain: stack clouds of 0 points, of fewer than 256, of more than 256 and no multiple of 256; a full cloud shorter than
    both stack clouds (a thin sweep's processor beside a whole sweep's odometry) and a cleared one.  The HDL-64E's full cloud, longer than
    both stack clouds, is asserted in test_all_kinds_in_one_call."""
    sw, lid = fbc.raw("indoor", fbc.T0S[0], 3)
    thin = [fbc.thin_sweep(x) for x in sw]
    fronts = [fbc.moving(0, 2),
              dict(fbc.moving(1, 2), name="thin_steps", steps=thin[1:3]),
              fbc.empty_sweep(2)]
    maps = [cases.map_handle("short_full", 0, pp=1), cases.map_handle("thin", 1), cases.map_handle("empty", 2)]
    rig = cases.Rig(hip, fronts, maps)
    rig.step(0, cases.pooled)
    rig.step(1, cases.pooled)
    print("counts (n_corner, n_surf, n_full) per step:", rig.counts)
    for k in range(2):
        nc, ns, nf = rig.counts[k][0]
        assert nc > 256 and ns > 256 and nc % 256 and ns % 256 and 0 < nf < min(nc, ns)
        nc, ns, nf = rig.counts[k][1]
        assert 0 < nc < 256 and 0 < ns < 256 and nf > 0
    assert rig.counts[0][2] == (0, 0, 0)
    assert len(rig.fed[0].full_cloud()) == rig.counts[1][0][2]


def test_refusals_leave_everything_as_it_was(hip):
    fronts = [fbc.moving(j, 2) for j in range(3)]
    rig = cases.Rig(hip, fronts)
    rig.step(0, cases.pooled)
    rig.feed(1, cases.pooled)                                    # the sweep the refused calls would have taken
    est = capi.Estimator(hip, pipeline.config_indoor(hip, 4, 2))
    borrowed = est.map()
    fresh_od = capi.PointOdometry(hip, *fronts[0]["params"])
    fresh_pp = capi.PointProcessor(hip, fronts[0]["lidar"].lower_deg, fronts[0]["lidar"].upper_deg, fronts[0]["lidar"].rings)
    maps_before = [cases.map_state(m) for m in rig.fed]
    borrowed_before = (cases.bits(borrowed.transform_tobe_mapped()).copy(), borrowed.cube_state()[0])
    assert all(len(st["full"]) > 0 for st in maps_before)
    state = dict(pps=list(range(3)))                             # the processors whose accessors still answer

    def light(st):                                               # all of a map handle's state but the per-cube clouds (those: once, below)
        return {k: v for k, v in st.items() if not k.startswith("cube")}

    def light_state(m):
        cen, valid = m.cube_state()
        score, point, coeff = m.score_point_coeff()
        st = dict(tobe=cases.bits(m.transform_tobe_mapped()), cen=np.array(cen, np.int32), valid=valid, score=score, point=point, coeff=coeff,
                  surround=m.surround(0.6), full=m.full_cloud())
        for w in range(4):
            st[f"cloud{w}"] = m.cloud(w)
        return st

    def sources():
        return [cases.odom_snapshot(od, rig.full) for od in rig.ods], [cases.pp_snapshot(rig.pps[p]) for p in state["pps"]]

    def arr(xs):
        return None if xs is None else (C.c_void_p * len(xs))(*[None if x is None else x.h for x in xs])

    def call(ms, ods, pps, n=None, expect=None):
        n = len(ms) if n is None else n
        before = sources()
        Ta = (capi.TransformF * 3)()
        it = np.full(3, 7, np.int32)
        rc = hip.dll.lio_map_process_batch_from_odom(arr(ms), arr(ods), arr(pps), n, Ta, it.ctypes.data_as(capi.c_int32_p), None)
        assert rc == expect, (rc, expect)
        assert list(it) == [7, 7, 7]                             # outputs untouched
        for j, m in enumerate(rig.fed):
            cases.assert_same(light(maps_before[j]), light_state(m), ("map after a refusal", j, expect))
        assert np.array_equal(cases.bits(borrowed.transform_tobe_mapped()), borrowed_before[0]) and borrowed.cube_state()[0] == borrowed_before[1]
        for b, a in zip(before, sources()):
            for j, (x, y) in enumerate(zip(b, a)):
                cases.assert_snapshots_equal(x, y, ("source after a refusal", j, expect))

    m, od, pp = rig.fed, rig.ods, rig.pps
    call(None, od, pp, n=3, expect=ERR_ARG)                      # no handle array
    call(m, None, pp, n=3, expect=ERR_ARG)                       # no odometry array
    call([m[0], None, m[2]], od, pp, expect=ERR_ARG)             # a null map handle
    call(m, [od[0], None, od[2]], pp, expect=ERR_ARG)            # a null odometry handle
    call(m, od, pp, n=0, expect=ERR_ARG)
    call([m[0], m[1], m[0]], od, pp, expect=ERR_ARG)             # the same map twice
    call(m, [od[0], fresh_od, od[2]], pp, expect=ERR_STATE)      # an odometry that never processed
    call(m, od, [pp[0], fresh_pp, pp[2]], expect=ERR_STATE)      # a processor that never processed
    call([m[0], borrowed, m[2]], od, pp, expect=ERR_STATE)       # an estimator's map
    call(m[:2], od[:2], pp[:2], n=capi.MAP_BATCH_MAX_SENSORS + 1, expect=ERR_CAPACITY)
    # the pooled sweep of the third processor overwritten by a later lio_pp_process_batch of its neighbours (the same sweeps again)
    capi.PointProcessor.process_batch(rig.pps[:2], [fronts[j]["steps"][1] for j in range(2)])
    assert hip.dll.lio_pp_get_cloud(rig.pps[2].h, 1, np.zeros((4096, 4), np.float32).ctypes.data_as(capi.c_float_p)) == ERR_STATE
    state["pps"] = [0, 1]
    call(m, od, pp, expect=ERR_STATE)
    call(m[2:], od[2:], pp[2:], expect=ERR_STATE)
    for j, m in enumerate(rig.fed):                              # every cube of every map too
        cases.assert_same(maps_before[j], cases.map_state(m), ("map after the refusals", j))
    # ... and the handles still step like their twins
    res = rig.step(1, cases.pooled)
    assert all(r["iterations"] > 0 for r in res)
