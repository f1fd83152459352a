"""include/lio_est_from_odom.h: lio_est_batch_push_frames_from_odom / lio_est_batch_process_compact_from_odom against the host route the
header states as the contract, bit for bit (rig: tests/est_from_odom_cases.py).

A: twin windows in a batch of their own, fed by lio_est_batch_push_frames with what lio_odom_get_last_cloud returns.  B: the windows under
test.  S: single handles with lio_est_config.device_solve = 1 (a batch of one) through lio_est_push_frame and lio_est_process_compact.
Compared after every call: what est_push_cases.observe reads of every window, lio_map_get_full_cloud and
lio_map_get_transform_tobe_mapped of lio_est_map, the reports, transform_to_init_out, and every accessor of the sources before and after."""
import ctypes

import numpy as np
import pytest

from lio_amd import capi, pipeline
import est_push_cases as epc
import est_from_odom_cases as cases
import frontend_batch_cases as fbc
from est_push_cases import assert_twins, bits
from ring_pick_cases import over_capacity_sweeps
from test_ring_pick import make_pp

pytestmark = pytest.mark.gpu


def _solve_slide(batches, singles):
    reps = [b.solve() for b in batches] + [[e.solve() for e in singles]]
    for b in batches:
        b.slide()
    for e in singles:
        e.slide()
    return reps


@pytest.mark.parametrize("deskew", ["cutoff", "imu"])
def test_push_and_composite_equal_the_host_route(hip, deskew):
    """Three different windows, each with a sensor of its own (an enabled odometry after a publishing step), over five steps of push from the
    odometry / batch solve / slide, then two steps of the composite.  deskew = "imu": k_bp_take_keys_dev de-skews."""
    def make(device_solve):
        return [cases.window(hip, W, Wo, seed, keep=keep, optex=optex, deskew=deskew, device_solve=device_solve) for _, W, Wo, keep, optex, seed in epc.SPECS]

    A, B, S = make(0), make(0), make(1)
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    Ws = [s[1] for s in epc.SPECS]
    srcs = [cases.Source(hip, prep=(W - 1, W)) for W in Ws]
    _solve_slide([batch_a, batch_b], S)
    assert_twins(A, B, "as built")
    for step in range(1, 8):
        for w, W in enumerate(Ws):
            srcs[w].frame(W + step)
            for e in (A[w], B[w], S[w]):
                epc.imu(e, W + step)
        k = Ws[0] + step                                         # (the stamp every window takes: frame k's)
        if step <= 5:
            cases.host_push_batch(batch_a, srcs, None, k)
            cases.host_push_single(S, srcs, None, k)
            st, fo = cases.fed_push(batch_b, srcs, None, k)
            assert st["host_waits"] == 1 and st["chain"] + st["redone"] == len(B) and st["as_is"] == 0, st
            assert fo == dict(device_sources=len(B), as_is_copies=0, full_clouds=0, uploads=0), fo   # every filtered cloud from a device source
            assert_twins(A, B, f"step {step} push")
            assert_twins(S, B, f"step {step} push, single handles")
            ra, rb, rs = _solve_slide([batch_a, batch_b], S)
            cases.same_reports(ra, rb, f"step {step}")
            cases.same_reports(rs, rb, f"step {step}, single handles")
            assert_twins(A, B, f"step {step} slide", prior=True)
            assert_twins(S, B, f"step {step} slide, single handles", prior=True)
        else:
            Ts, rs = cases.host_compact(S, srcs, None, k)
            Tb, rb, st, fo = cases.fed_compact(batch_b, srcs, None, k)
            assert st["host_waits"] == 1 and fo["device_sources"] == len(B) and fo["uploads"] == 0, (st, fo)
            cases.same_reports(rs, rb, f"composite step {step}")
            cases.assert_same_T(Ts, Tb, f"composite step {step}")
            assert_twins(S, B, f"composite step {step}", prior=True, event=True)
            cases.assert_maps(S, B, f"composite step {step}")
            assert all(e.stage()["event"] == "solved" for e in B)
    batch_a.close(); batch_b.close()


def test_block_edges_of_the_device_fed_kernel(hip, oracle):
    """Surf clouds of 0, 1, 255, 256, 257 and 3000 points and, the map refresh being on, corner clouds of 0 and 257 points, mixed over four windows
    and two calls: blocks beyond a short cloud's range leave while a long cloud's run.  The sources keep the clouds as they are (disabled
    odometries), so each filtered surf stack is also the oracle's voxel_grid of what lio_odom_get_last_cloud returns; none is redone.  A filtered
    corner cloud lives in the refresh ring and is read through lio_est_refresh_map once its slot is the ring's oldest: three more device-fed
    pushes follow, with a refresh on both twins behind every push, and the corner clouds of both calls are held to the twin's and to the
    oracle's voxel_grid at corner_filter_size."""
    sizes = [(0, 257), (3000, 0), (255, 257), (256, 0), (257, 0), (1, 257), (3000, 257), (0, 0)]   # (surf, corner) per window, call 0 then call 1
    later = [(300, 100), (129, 257), (64, 0)]                    # ... and of every window in the three pushes behind them
    A = [cases.window(hip, 4, 2, 3 + w, refresh=True, optex=0) for w in range(4)]
    B = [cases.window(hip, 4, 2, 3 + w, refresh=True, optex=0) for w in range(4)]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    leaf_c = B[0].cfg.corner_filter_size
    want_corner = {}                                             # push -> per window, the oracle's filter of the corner cloud that push took
    seen = set()
    for call in range(5):
        k = 5 + call
        mine = sizes[4 * call:4 * call + 4] if call < 2 else [later[call - 2]] * 4
        srcs = [cases.packer(hip, epc.room(nc, 300 + nc + w + 7 * call), epc.room(ns, 100 + ns + w + 7 * call)) for w, (ns, nc) in enumerate(mine)]
        for w, (ns, nc) in enumerate(mine):
            corner, surf = cases.host_clouds(srcs[w])
            assert (len(surf), len(corner)) == (ns, nc)
            np.testing.assert_array_equal(bits(surf), bits(epc.room(ns, 100 + ns + w + 7 * call)))
            np.testing.assert_array_equal(bits(corner), bits(epc.room(nc, 300 + nc + w + 7 * call)))
        want_corner[call] = [oracle.voxel_grid(cases.host_clouds(s)[0], leaf_c) if len(cases.host_clouds(s)[0]) else cases.EMPTY for s in srcs]
        cases.imu(A + B, k)
        cases.host_push_batch(batch_a, srcs, None, k)
        st, fo = cases.fed_push(batch_b, srcs, None, k)
        assert (st["chain"], st["redone"], st["as_is"], st["host_waits"]) == (8, 0, 0, 1), st   # a pass must not be hidden by the fallback
        assert fo == dict(device_sources=8, as_is_copies=0, full_clouds=0, uploads=0), fo
        assert_twins(A, B, f"call {call}")
        for w, s in enumerate(srcs):
            got, want = B[w].get_surf_stack(4), oracle.voxel_grid(cases.host_clouds(s)[1], epc.LEAF)
            assert got.shape == want.shape, (call, w, got.shape, want.shape)
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"call {call} window {w} against the oracle's filter")
        # the ring's oldest slot after push `call` (pushes counted from 0) is the slot of push max(0, call - 2); with the filter on it holds the
        # corner cloud of the push before its own (Estimator.cc:484-485 behind :689-693)
        recs = cases.refresh_both(A, B, f"call {call} refresh")
        held = max(0, call - 2) - 1
        for w, h in enumerate(recs):
            if held < 0:
                continue
            want = want_corner[held][w]
            assert h["corner"].shape == want.shape, (call, w, held, h["corner"].shape, want.shape)
            np.testing.assert_array_equal(bits(h["corner"]), bits(want), err_msg=f"corner cloud of push {held}, window {w}, against the oracle's filter")
            seen.add((held, sizes[4 * held + w][1]))
        assert_twins(A, B, f"call {call} refresh")
        batch_a.slide(); batch_b.slide()
        assert_twins(A, B, f"call {call} slide")
    assert seen == {(0, 0), (0, 257), (1, 0), (1, 257)}, seen    # the corner clouds of 0 and of 257 points of both calls were looked at
    batch_a.close(); batch_b.close()


def test_full_cloud_in_both_forms(hip, oracle):
    """Window 0: an enabled odometry after a publishing step (odo_to_end_body), its own processor.  Window 1: a disabled odometry (copy), pooled
    processor storage, a full cloud of 257 points and then of none.  Window 2: full cloud on, a null entry.  Window 3: full cloud off, given a
    processor all the same.  The push form leaves a map's full cloud where no processor is given, the composite clears it."""
    def make(device_solve):
        return [cases.window(hip, 4, 2, 3 + 2 * w, full=(w < 3), deskew="imu", optex=0, device_solve=device_solve) for w in range(4)]

    A, B, S = make(0), make(0), make(1)
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    srcs = [cases.Source(hip, prep=(3, 4)), cases.Source(hip, prep=(4,), enabled=False), cases.Source(hip, prep=(3, 4)), cases.Source(hip, prep=(3, 4))]
    pooled = [srcs[1].pp, srcs[3].pp]
    sweep = fbc.raw("indoor", fbc.T0S[0], 2)[0][1]
    lid = epc.data()[0].lidar
    for m in range(257, 300):                                    # the shortest head of the sweep whose ring cloud has 257 points, by the oracle's processor
        ref = capi.PointProcessor(oracle, lid.lower_deg, lid.upper_deg, lid.rings)
        ref.process(sweep[:m])
        if len(ref.cloud(cases.RINGS)) == 257:
            break
    s257 = sweep[:m]
    _solve_slide([batch_a, batch_b], S)
    for step, (form, with_pp, small) in enumerate([("push", True, s257), ("push", False, s257), ("compact", True, fbc.EMPTY_SWEEP),
                                                   ("compact", True, s257), ("compact", False, s257)], start=1):
        k = 4 + step
        for s in srcs:
            s.frame(k)
        capi.PointProcessor.process_batch(pooled, [small, cases.scan(k)])   # (behind the odometry's step: pooled storage holds the sweeps the full clouds come from)
        n_small = len(srcs[1].pp.cloud(cases.RINGS))
        assert n_small == (257 if len(small) else 0)                # a full row of two blocks, the second with one live lane; and one of no point
        pps = [srcs[0].pp, srcs[1].pp, None, srcs[3].pp] if with_pp else None
        cases.imu(A + B + S, k)
        before = [len(e.map().full_cloud()) for e in B]
        if form == "push":
            cases.host_push_batch(batch_a, srcs, pps, k)
            cases.host_push_single(S, srcs, pps, k)
            st, fo = cases.fed_push(batch_b, srcs, pps, k)
            assert fo == dict(device_sources=4, as_is_copies=0, full_clouds=2 if with_pp else 0, uploads=0), fo
            assert_twins(A, B, f"step {step} push")
            cases.assert_maps(A, B, f"step {step} push")
            assert_twins(S, B, f"step {step} push, single handles")
            after = [len(e.map().full_cloud()) for e in B]
            assert after[2:] == before[2:] and (with_pp or after == before)       # no processor, or the full cloud off: as it was
            if with_pp:
                assert after[0] == len(srcs[0].pp.cloud(cases.RINGS)) > 257 and after[1] == n_small
            ra, rb, rs = _solve_slide([batch_a, batch_b], S)
            cases.same_reports(ra, rb, f"step {step}")
            cases.same_reports(rs, rb, f"step {step}, single handles")
        else:
            Ts, rs = cases.host_compact(S, srcs, pps, k)
            Tb, rb, st, fo = cases.fed_compact(batch_b, srcs, pps, k)
            assert fo == dict(device_sources=4, as_is_copies=0, full_clouds=3, uploads=0), fo   # every window with the full cloud on: taken or cleared
            cases.same_reports(rs, rb, f"step {step}")
            cases.assert_same_T(Ts, Tb, f"step {step}")
            after = [len(e.map().full_cloud()) for e in B]
            assert after[2] == 0 and after[3] == before[3] and (with_pp or after[:3] == [0, 0, 0])   # an empty third block clears; full cloud off: ignored
            if with_pp:
                assert after[1] == n_small
        assert_twins(S, B, f"step {step}", prior=True, event=(form == "compact"))
        cases.assert_maps(S, B, f"step {step}")
    batch_a.close(); batch_b.close()


def test_a_flagged_cloud_from_a_device_source_is_redone(hip, oracle):
    """est_push_cases.beyond_the_key() as an odometry's last surf cloud: the handle's own filter redoes it from the chain's de-skewed copy."""
    A = [cases.window(hip, 4, 2, 3 + w, deskew="imu") for w in range(2)]
    B = [cases.window(hip, 4, 2, 3 + w, deskew="imu") for w in range(2)]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    for call in range(2):
        k = 5 + call
        srcs = [cases.packer(hip, cases.EMPTY, epc.beyond_the_key()), cases.packer(hip, cases.EMPTY, epc.room(3000, 23))]
        cases.imu(A + B, k)
        cases.host_push_batch(batch_a, srcs, None, k)
        st, fo = cases.fed_push(batch_b, srcs, None, k)
        assert (st["chain"], st["redone"], st["as_is"]) == (1, 1, 0) and fo["device_sources"] == 2 and fo["uploads"] == 0, (st, fo)
        assert_twins(A, B, f"call {call}")
        got = B[0].get_surf_stack(4)
        assert np.any(got[:, 2] > 140.0) and len(got) < 900
        batch_a.slide(); batch_b.slide()
    batch_a.close(); batch_b.close()


def test_both_deskew_switches_off_copies_device_to_device(hip):
    """Window 0 has the map refresh on: its corner cloud is copied as it is too, and the refresh behind every solve reads the ring's oldest slot,
    which holds the first push's corner cloud until the ring is full (step 3: the refresh is applied) — the bits lio_odom_get_last_cloud gave."""
    A = [cases.window(hip, 4, 2, 3, deskew="off", refresh=True, optex=0), cases.window(hip, 4, 2, 5, deskew="off")]
    B = [cases.window(hip, 4, 2, 3, deskew="off", refresh=True, optex=0), cases.window(hip, 4, 2, 5, deskew="off")]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    srcs = [cases.Source(hip, prep=(3, 4)), cases.packer(hip, epc.room(257, 7), epc.room(0, 8))]
    first = None
    applied = []
    for step in range(1, 4):
        k = 4 + step
        srcs[0].frame(k)
        if first is None:
            first = cases.host_clouds(srcs[0])
            assert len(first[0]) > 256 and len(first[1]) > 256
        cases.imu(A + B, k)
        cases.host_push_batch(batch_a, srcs, None, k)
        st, fo = cases.fed_push(batch_b, srcs, None, k)
        assert (st["chain"], st["redone"], st["as_is"], st["host_waits"]) == (0, 0, 3, 1), st
        assert fo == dict(device_sources=0, as_is_copies=3, full_clouds=0, uploads=0), fo
        assert_twins(A, B, f"step {step} push")
        cases.same_reports(batch_a.solve(), batch_b.solve(), f"step {step}")
        h = cases.refresh_both(A[:1], B[:1], f"step {step} refresh")[0]
        applied.append(h["applied"])
        np.testing.assert_array_equal(bits(h["corner"]), bits(first[0]), err_msg=f"step {step}: the corner cloud of the first push, copied as it is")
        if step == 1:                                            # (the slot's surf stack is the window's newest: no slide has touched it yet)
            np.testing.assert_array_equal(bits(h["surf"]), bits(first[1]), err_msg="the surf cloud of the first push, copied as it is")
        assert_twins(A, B, f"step {step} refresh", prior=True)
        batch_a.slide(); batch_b.slide()
        assert_twins(A, B, f"step {step} slide", prior=True)
    print("refresh applied per step:", applied)
    assert applied[-1] == 1, applied
    batch_a.close(); batch_b.close()


def test_composite_refreshes_the_map_from_device_fed_corner_clouds(hip):
    """lio_est_batch_process_compact_from_odom on windows with the map refresh on (corner clouds through k_bp_take_keys_dev, the refresh between solve
    and slide), de-skewed by the IMU poses, against lio_est_process_compact on device_solve = 1 twins: the last refresh's record — applied, pose,
    cube centre, valid cubes, corner and surf cloud — after every step, and the map it updated."""
    def make(device_solve):
        return [cases.window(hip, 4, 2, 3, refresh=True, deskew="imu", optex=0, device_solve=device_solve),
                cases.window(hip, 4, 2, 5, refresh=True, deskew="cutoff", optex=0, device_solve=device_solve)]

    S, B = make(1), make(0)
    batch = capi.EstimatorBatch(hip, B)
    srcs = [cases.Source(hip, prep=(3, 4)), cases.Source(hip, prep=(4,), enabled=False)]
    for e in S:
        e.solve(); e.slide()
    batch.solve(); batch.slide()
    applied = []
    for step in range(1, 6):
        k = 4 + step
        for s in srcs:
            s.frame(k)
        cases.imu(S + B, k)
        Ts, rs = cases.host_compact(S, srcs, None, k)
        Tb, rb, st, fo = cases.fed_compact(batch, srcs, None, k)
        assert (st["chain"], st["redone"], st["as_is"], st["host_waits"]) == (4, 0, 0, 1), st   # two surf and two corner clouds
        assert fo == dict(device_sources=4, as_is_copies=0, full_clouds=0, uploads=0), fo
        cases.same_reports(rs, rb, f"step {step}")
        cases.assert_same_T(Ts, Tb, f"step {step}")
        assert_twins(S, B, f"step {step}", prior=True, event=True)   # (observe reads the last refresh's record, clouds included)
        cases.assert_maps(S, B, f"step {step}")
        for w in range(2):
            hs, hb = S[w].last_map_refresh(), B[w].last_map_refresh()
            assert hs is not None and hb is not None and hs["applied"] == hb["applied"]
            np.testing.assert_array_equal(bits(hs["corner"]), bits(hb["corner"]), err_msg=f"step {step} window {w}: refresh corner cloud")
            for c in range(2):
                np.testing.assert_array_equal(bits(S[w].map().cloud(c)), bits(B[w].map().cloud(c)), err_msg=f"step {step} window {w}: map cloud {c}")
        applied.append(B[0].last_map_refresh()["applied"])
    print("refresh applied per step:", applied)
    assert applied[-1] == 1 and len(B[0].last_map_refresh()["corner"]) > 0, applied
    batch.close()


def test_two_parts_give_the_bits_of_one(hip):
    seeds = (3, 5, 7, 9)
    A = [cases.window(hip, 4, 2, s, optex=0, full=(s == 5), deskew="imu") for s in seeds]
    B = [cases.window(hip, 4, 2, s, optex=0, full=(s == 5), deskew="imu") for s in seeds]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    batch_a.set_option("parts", 1)
    batch_b.set_option("parts", 2)
    srcs = [cases.Source(hip, prep=(3, 4)) for _ in seeds]
    pps = [s.pp for s in srcs]
    for step in range(1, 3):
        k = 4 + step
        for s in srcs:
            s.frame(k)
        cases.imu(A + B, k)
        if step == 1:
            sa, fa = cases.fed_push(batch_a, srcs, pps, k)
            sb, fb = cases.fed_push(batch_b, srcs, pps, k)
            ra, rb = batch_a.solve(), batch_b.solve()
            batch_a.slide(); batch_b.slide()
        else:
            Ta, ra, sa, fa = cases.fed_compact(batch_a, srcs, pps, k)
            Tb, rb, sb, fb = cases.fed_compact(batch_b, srcs, pps, k)
            cases.assert_same_T(Ta, Tb, f"step {step}")
        assert sa["host_waits"] == 1 and sb["host_waits"] == 2, (sa, sb)   # one host wait per part
        assert fa == fb == dict(device_sources=4, as_is_copies=0, full_clouds=1, uploads=0), (fa, fb)
        cases.same_reports(ra, rb, f"step {step}")
        assert_twins(A, B, f"step {step}", prior=True)
        cases.assert_maps(A, B, f"step {step}")
    batch_a.close(); batch_b.close()


def test_one_odometry_feeds_two_windows_and_the_routes_mix(hip):
    """B alternates between the single calls, the host-fed batch and the device-fed batch from step to step, its windows fed by one odometry, by two,
    and by the two the other way round; A only ever sees the host-fed batch."""
    A = [cases.window(hip, 5, 2, 7, deskew="imu"), cases.window(hip, 4, 2, 3, deskew="imu")]
    B = [cases.window(hip, 5, 2, 7, deskew="imu"), cases.window(hip, 4, 2, 3, deskew="imu")]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    two = [cases.Source(hip, prep=(4, 5)), cases.Source(hip, prep=(4, 5), enabled=False)]
    cases.same_reports(batch_a.solve(), batch_b.solve(), "as built")
    batch_a.slide(); batch_b.slide()
    plans = [("fed", [0, 0]), ("single", [0, 1]), ("fed", [1, 0]), ("host", [1, 1]), ("fed", [0, 1]), ("fed", [1, 0])]
    for step, (route, feed) in enumerate(plans, start=1):
        k = 5 + step
        for s in two:
            s.frame(k)
        srcs = [two[j] for j in feed]
        cases.imu(A + B, k)
        cases.host_push_batch(batch_a, srcs, None, k)
        if route == "fed":
            st, fo = cases.fed_push(batch_b, srcs, None, k)
            assert fo["device_sources"] == 2 and fo["uploads"] == 0, fo
        elif route == "host":
            cases.host_push_batch(batch_b, srcs, None, k)
        else:
            cases.host_push_single(B, srcs, None, k)
        assert_twins(A, B, f"step {step} push ({route})")
        cases.same_reports(batch_a.solve(), batch_b.solve(), f"step {step}")
        batch_a.slide()
        if route == "single":
            for e in B:
                e.slide()
        else:
            batch_b.slide()
        assert_twins(A, B, f"step {step} slide", prior=True)
    batch_a.close(); batch_b.close()


def test_every_refusal_changes_nothing(hip):
    """LIO_ERR_ARG (-1) and LIO_ERR_STATE (-2) of the header, each before a window, a map or a source is touched; the valid call behind them all
    equals the twin's."""
    dll = hip.dll
    k = 5
    A = [cases.window(hip, 4, 2, 3, full=True), cases.window(hip, 4, 2, 5)]
    B = [cases.window(hip, 4, 2, 3, full=True), cases.window(hip, 4, 2, 5)]
    batch_a, batch = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    srcs = [cases.Source(hip, prep=(3, 4, 5)), cases.Source(hip, prep=(4, 5))]
    pps = [s.pp for s in srcs]
    cases.imu(A + B, k)
    fresh_od, fresh_pp = capi.PointOdometry(hip), cases._processor(hip)
    (ring_case, _), _ = over_capacity_sweeps()
    over_pp = make_pp(hip, ring_case[1], ring_case[2])
    over_pp.process_async(ring_case[3])
    assert dll.lio_pp_wait(over_pp.h) == -4
    lost = [cases._processor(hip) for _ in range(3)]              # pooled storage, then overwritten for the third by its neighbours' next batch
    capi.PointProcessor.process_batch(lost, [cases.scan(k)] * 3)
    capi.PointProcessor.process_batch(lost[:2], [cases.scan(k)] * 2)

    def arr(xs):
        return None if xs is None else (ctypes.c_void_p * len(xs))(*[None if x is None else x.h for x in xs])

    T2, t2 = (capi.TransformF * 2)(epc.ident_T(), epc.ident_T()), (ctypes.c_double * 2)(cases.stamp(k), cases.stamp(k))

    def both(b, wins, ods, ps, expect, what, T=T2, t=t2, compact_expect=None, watch=None):
        watch = srcs if watch is None else watch
        was = [epc.observe(e, prior=True, event=True) for e in wins]
        maps = [cases.map_view(e) for e in wins]
        src_was = cases.snapshot(watch, [s.pp for s in watch])
        reps = (capi.SolveReport * 2)()
        reps[0].iterations = reps[1].iterations = 41
        Tout = (capi.TransformF * 2)()
        Tout[1].p[0] = 5.0
        assert dll.lio_est_batch_push_frames_from_odom(b, arr(ods), arr(ps), T, t) == expect, what
        ce = expect if compact_expect is None else compact_expect
        assert dll.lio_est_batch_process_compact_from_odom(b, arr(ods), arr(ps), t, Tout, reps) == ce, what
        if ce != 0:
            assert reps[0].iterations == 41 and reps[1].iterations == 41 and Tout[1].p[0] == 5.0, what   # outputs untouched
            for w, e in enumerate(wins):
                epc.assert_same(was[w], epc.observe(e, prior=True, event=True), f"{what}, window {w}")
                epc.assert_same(maps[w], cases.map_view(e), f"{what}, map of window {w}")
        cases.assert_sources_unchanged(src_was, cases.snapshot(watch, [s.pp for s in watch]), what)

    od = [s.od for s in srcs]
    both(None, B, od, pps, cases.ERR_ARG, "no batch")
    both(batch.h, B, None, pps, cases.ERR_ARG, "no odometry array")
    both(batch.h, B, od, pps, cases.ERR_ARG, "no stamps", t=None)
    assert dll.lio_est_batch_push_frames_from_odom(batch.h, arr(od), arr(pps), None, t2) == cases.ERR_ARG   # no transforms
    both(batch.h, B, [od[0], None], pps, cases.ERR_ARG, "a null odometry entry")
    both(batch.h, B, [od[0], fresh_od], pps, cases.ERR_STATE, "an odometry that never processed")
    both(batch.h, B, od, [pps[0], fresh_pp], cases.ERR_STATE, "a processor that never processed")
    both(batch.h, B, od, [over_pp, pps[1]], cases.ERR_STATE, "a processor that ended over capacity")
    both(batch.h, B, od, [pps[0], lost[2]], cases.ERR_STATE, "a pooled sweep that was overwritten")
    assert dll.lio_est_batch_from_odom_stats(batch.h, None) == cases.ERR_ARG and dll.lio_est_batch_from_odom_stats(None, (ctypes.c_int * 8)()) == cases.ERR_ARG
    # an uninitialised window behind one that is
    mixed = [cases.window(hip, 4, 2, 3), capi.Estimator(hip, epc.config(hip, 4, 2))]
    epc.imu(mixed[0], k)
    bm = capi.EstimatorBatch(hip, mixed)
    both(bm.h, mixed[:1], od, pps, cases.ERR_STATE, "an uninitialised window")
    bm.close()
    # imu_factor off: the composite refuses as lio_est_process_compact does, the push does not (checked on a batch of its own: it pushes)
    cfg = epc.config(hip, 4, 2)
    cfg.imu_factor = 0
    ds, clouds, _ = epc.data()
    loam = [cases.window(hip, 4, 2, 3), capi.Estimator(hip, cfg)]
    pipeline.init_window(loam[1], hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=5)
    for e in loam:
        epc.imu(e, k)
    loam_was = [epc.observe(e, prior=True, event=True) for e in loam]
    loam_maps = [cases.map_view(e) for e in loam]
    bl = capi.EstimatorBatch(hip, loam)
    reps = (capi.SolveReport * 2)()
    assert dll.lio_est_batch_process_compact_from_odom(bl.h, arr(od), arr(pps), t2, None, reps) == cases.ERR_STATE
    for w, e in enumerate(loam):
        epc.assert_same(loam_was[w], epc.observe(e, prior=True, event=True), f"imu_factor off, window {w}")
        epc.assert_same(loam_maps[w], cases.map_view(e), f"imu_factor off, map of window {w}")
    bl.close()
    # lio_est_push_frame's own refusal: de-skew from the IMU poses and no IMU sample yet, in the second window
    dry = [cases.window(hip, 4, 2, 3, deskew="imu"), cases.window(hip, 4, 2, 5, deskew="imu")]
    epc.imu(dry[0], k)
    bd = capi.EstimatorBatch(hip, dry)
    both(bd.h, dry, od, pps, cases.ERR_STATE, "de-skew precondition")
    # a dissolved batch
    hip.dll.lio_est_destroy(dry[1].h)
    dry[1].h = None
    assert len(bd) == 0
    both(bd.h, dry[:1], od, pps, cases.ERR_STATE, "a dissolved batch")
    assert dll.lio_est_batch_from_odom_stats(bd.h, (ctypes.c_int * 8)()) == cases.ERR_STATE
    bd.close()
    # and the valid call behind all the refusals equals the twin's
    cases.host_push_batch(batch_a, srcs, pps, k)
    st, fo = cases.fed_push(batch, srcs, pps, k)
    assert fo == dict(device_sources=2, as_is_copies=0, full_clouds=1, uploads=0), fo
    assert_twins(A, B, "the valid call behind the refusals")
    cases.assert_maps(A, B, "the valid call behind the refusals")
    batch_a.close(); batch.close()
