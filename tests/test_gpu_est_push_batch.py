"""include/lio_est_push_batch.h: lio_est_batch_push_frames / _slide_windows / _process_laser_odom against the per-handle calls, bit for bit.

Twin handles are built from one seed (est_push_cases.window).  Twin A is driven by lio_est_push_frame / lio_est_slide_window (its solves by a
batch of its own), twin B by the new calls; where lio_est_process_laser_odom is the per-handle side, the twin is a single handle with
lio_est_config.device_solve = 1 — a batch of one, the solve that the batched composite runs.  Compared after every call: every surf stack and
its size, get_window, lio_est_get_stage, the full-cloud ring, the last map refresh, the reports and the priors, as uint32 / uint64 views."""
import ctypes

import numpy as np
import pytest

from lio_amd import capi
import est_push_cases as cases
from est_push_cases import assert_twins, bits, item, rep_key

pytestmark = pytest.mark.gpu


def _push_per_handle(ests, k, items=None):
    for w, e in enumerate(ests):
        cases.imu(e, k)
        cases.push_single(e, items[w] if items else item(k))


def _push_batched(batch, k, items=None):
    for e in batch.members:
        cases.imu(e, k)
    batch.push_frames(items if items else [item(k)] * len(batch.members))


def _same_reports(ra, rb, what):
    for w, (a, b) in enumerate(zip(ra, rb)):
        assert rep_key(a) == rep_key(b), (what, w, rep_key(a), rep_key(b))


@pytest.mark.parametrize("deskew", ["cutoff", "imu"])
def test_chains_of_push_solve_slide_equal_the_per_handle_calls(hip, deskew):
    """Three different windows over five steps of push, batch solve and slide, then two steps of the composite.  A: per-handle push and slide, a
    batch's solve; B: the new calls; S: single handles with device_solve = 1 through lio_est_push_frame / lio_est_solve_optimization /
    lio_est_slide_window and, in the composite steps, lio_est_process_laser_odom.  deskew = "imu": k_bp_take_keys de-skews."""
    def make(device_solve):
        return [cases.window(hip, W, Wo, seed, keep=keep, optex=optex, deskew=deskew, device_solve=device_solve) for _, W, Wo, keep, optex, seed in cases.SPECS]

    A, B, S = make(0), make(0), make(1)
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    Ws = [s[1] for s in cases.SPECS]
    assert_twins(A, B, "as built")
    chain = 0
    for step in range(6):
        if step > 0:
            items = [item(W + step) for W in Ws]
            for w, W in enumerate(Ws):
                for e in (A[w], S[w]):
                    cases.imu(e, W + step)
                    cases.push_single(e, items[w])
                cases.imu(B[w], W + step)
            batch_b.push_frames(items)
            st = batch_b.push_stats()
            assert st["host_waits"] == 1 and st["chain"] + st["redone"] == len(B) and st["as_is"] == 0, st
            chain += st["chain"]
            assert_twins(A, B, f"step {step} push")
            assert_twins(S, B, f"step {step} push, single handles")
        ra, rb, rs = batch_a.solve(), batch_b.solve(), [e.solve() for e in S]
        _same_reports(ra, rb, f"step {step}")
        _same_reports(rs, rb, f"step {step}, single handles")
        assert_twins(A, B, f"step {step} solve")
        for e in A + S:
            e.slide()
        batch_b.slide()
        assert_twins(A, B, f"step {step} slide", prior=True)
        assert_twins(S, B, f"step {step} slide, single handles", prior=True)
    assert chain >= 4 * len(B)          # (sweeps of an indoor room fit the chain's keys: the shared filter did the work)
    for step in range(6, 8):
        items = [item(W + step) for W in Ws]
        rs = []
        for w, W in enumerate(Ws):
            cases.imu(S[w], W + step)
            cases.imu(B[w], W + step)
            rs.append(S[w].process_laser_odom(*items[w]))
        rb = batch_b.process_laser_odom(items)
        _same_reports(rs, rb, f"composite step {step}")
        assert_twins(S, B, f"composite step {step}", prior=True, event=True)
        assert all(e.stage()["event"] == "solved" for e in B)
    batch_a.close(); batch_b.close()


def test_edges_of_the_chain(hip, oracle):
    """Crafted surf clouds into initialised windows, four per call: the block and sort-tile edges, one voxel, a lattice on voxel faces, NaN and inf,
    two leaf sizes.  Each against the twin and against the oracle's filter of the input; one host wait, every cloud through the shared chain."""
    leaves = (cases.LEAF, cases.LEAF, 0.3, 0.25)
    clouds = [cases.room(n, 100 + n) for n in cases.BLOCK_EDGES] + [cases.one_voxel(), cases.face_lattice(), cases.non_finite(), cases.face_lattice(0.3)]
    assert len(clouds) == 12
    A = [cases.window(hip, 4, 2, 3 + w, surf_leaf=leaf) for w, leaf in enumerate(leaves)]
    B = [cases.window(hip, 4, 2, 3 + w, surf_leaf=leaf) for w, leaf in enumerate(leaves)]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    order = [7, 5, 8, 9,   0, 1, 11, 10,   2, 6, 3, 4]          # per call: window 0 .. 3 (cloud 11, the 0.3 m lattice, meets the 0.3 m leaf)
    for call in range(3):
        k = 5 + call
        mine = [clouds[i] for i in order[4 * call:4 * call + 4]]
        items = [item(k, surf=c) for c in mine]
        _push_per_handle(A, k, items)
        _push_batched(batch_b, k, items)
        st = batch_b.push_stats()
        assert (st["chain"], st["redone"], st["as_is"], st["host_waits"]) == (4, 0, 0, 1), st
        assert st["sort_passes"] == (4 if call == 0 else 3), st  # four while unknown; then every window's previous push told the bits of its keys
        assert_twins(A, B, f"call {call}")
        for w, (c, leaf) in enumerate(zip(mine, leaves)):
            got, want = B[w].get_surf_stack(4), oracle.voxel_grid(c, leaf)
            assert got.shape == want.shape, (call, w, got.shape, want.shape)
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"call {call} window {w} against the oracle's filter")
            assert np.all(np.isfinite(got[:, :3]))
        for e in A:
            e.slide()
        batch_b.slide()
        assert_twins(A, B, f"call {call} slide")
    batch_a.close(); batch_b.close()


def test_flagged_clouds_are_redone_by_the_handle_s_own_filter(hip, oracle):
    """A point outside the chain's 9-bit z key, PCL's overflow (output = input) and a normal cloud in one call: equal bits, two clouds redone."""
    clouds = [cases.beyond_the_key(), cases.pcl_overflow(), cases.room(3000, 23)]
    A = [cases.window(hip, 4, 2, 3 + w) for w in range(3)]
    B = [cases.window(hip, 4, 2, 3 + w) for w in range(3)]
    batch_b = capi.EstimatorBatch(hip, B)
    for call in range(2):                                        # (the second call: the flags were left clear, the pass count follows the last push)
        k = 5 + call
        items = [item(k, surf=c) for c in clouds]
        _push_per_handle(A, k, items)
        _push_batched(batch_b, k, items)
        st = batch_b.push_stats()
        assert (st["chain"], st["redone"], st["as_is"]) == (1, 2, 0), st
        assert_twins(A, B, f"call {call}")
        got = [e.get_surf_stack(4) for e in B]
        np.testing.assert_array_equal(bits(got[1]), bits(clouds[1]))              # output = input
        assert np.any(got[0][:, 2] > 149.0) and len(got[0]) < len(clouds[0])
        for w in range(3):
            np.testing.assert_array_equal(bits(got[w]), bits(oracle.voxel_grid(clouds[w], cases.LEAF)), err_msg=f"window {w}")
        for e in A:
            e.slide()
        batch_b.slide()
    batch_b.close()


def test_map_refresh_and_full_cloud_ride_the_chain(hip):
    """A window with the map refresh on (its corner clouds through the chain) and one with the full cloud on, de-skewed by the IMU poses, over steps
    that include a refresh; split calls and the composite alternate.  S: single handles with device_solve = 1."""
    fulls = cases.data()[2]

    def make(device_solve):
        return [cases.window(hip, 4, 2, 3, refresh=True, deskew="imu", optex=0, device_solve=device_solve),
                cases.window(hip, 4, 2, 5, full=True, deskew="imu", optex=0, device_solve=device_solve)]

    S, B = make(1), make(0)
    batch = capi.EstimatorBatch(hip, B)
    refreshed = []
    for e in S:
        e.solve(); e.slide()
    batch.solve(); batch.slide()
    for step in range(1, 6):
        k = 4 + step
        for e in (S[1], B[1]):
            e.map().set_full_cloud(fulls[k])
        items = [item(k), item(k)]
        for e in S + B:
            cases.imu(e, k)
        if step % 2:
            for e, it in zip(S, items):
                cases.push_single(e, it)
            batch.push_frames(items)
            assert_twins(S, B, f"step {step} push")
            rs, rb = [e.solve() for e in S], batch.solve()
            refreshed.append((S[0].refresh_map(), B[0].refresh_map()))
            assert_twins(S, B, f"step {step} refresh")
            for e in S:
                e.slide()
            batch.slide()
        else:
            rs = [e.process_laser_odom(*it) for e, it in zip(S, items)]
            rb = batch.process_laser_odom(items)
            h = B[0].last_map_refresh()
            refreshed.append((None if h is None else h["applied"],) * 2)
        st = batch.push_stats()
        assert (st["chain"], st["redone"], st["as_is"], st["host_waits"]) == (3, 0, 0, 1), st      # two surf clouds and one corner cloud
        _same_reports(rs, rb, f"step {step}")
        assert_twins(S, B, f"step {step}", prior=True, event=True)
    print("refresh results per step:", refreshed)
    assert all(a == b for a, b in refreshed) and refreshed[-1][0] == 1 and refreshed[0][0] == 0
    assert len(B[1].full_stack(4)[0]) == len(fulls[9])
    assert S[0].refresh_map() == B[0].refresh_map()              # lio_est_refresh_map afterwards
    assert_twins(S, B, "refresh afterwards")
    batch.close()


def test_push_and_solve_leave_nothing_behind_in_the_filter_they_share(hip):
    """Solve's local maps and PushFrames' sweeps go through the part's one SegVoxFilter: a flag or a table that one leaves behind would reach the
    other.  Two windows with the map refresh on (four clouds, more than windows), sweeps of 257 points.  (a) a push whose first surf sweep has a
    return beyond the absolute key range: one cloud redone; (b) the solve behind it takes both windows on the device; (c) a solve whose first local
    map lies beyond the key range, then a push of ordinary sweeps: all four through the chain.  S: single handles with device_solve = 1."""
    n = cases.SHARED_SWEEP

    def make(device_solve):
        return [cases.window(hip, 4, 2, seed, refresh=True, optex=0, device_solve=device_solve) for seed in (3, 5)]

    def sweeps(k, first_surf=None):
        return [item(k, surf=cases.room(n, 40 + 4 * w) if (w or first_surf is None) else first_surf, corner=cases.room(n, 41 + 4 * w)) for w in range(2)]

    def push(k, items):
        for e in S + B:
            cases.imu(e, k)
        for e, it in zip(S, items):
            cases.push_single(e, it)
        batch.push_frames(items)
        return batch.push_stats()

    S, B = make(1), make(0)
    batch = capi.EstimatorBatch(hip, B)
    assert_twins(S, B, "as built")
    # (a)
    st = push(5, sweeps(5, cases.beyond_the_abs_range()))
    assert (st["chain"], st["redone"], st["as_is"], st["host_waits"]) == (3, 1, 0, 1), st
    assert_twins(S, B, "(a) push")
    # (b)
    _same_reports([e.solve() for e in S], batch.solve(), "(b)")
    assert int(batch.clock()["n_device"]) == 2, batch.clock()
    assert_twins(S, B, "(b) solve", prior=True)
    # (c)
    for e in S:
        e.slide()
    batch.slide()
    assert_twins(S, B, "(c) slide", prior=True)
    pivot = B[0].W - 2
    stray = cases.stray_above(B[0].get_surf_stack(pivot))
    for e in (S[0], B[0]):
        e.set_surf_stack(pivot, stray)
    _same_reports([e.solve() for e in S], batch.solve(), "(c)")
    assert int(batch.clock()["n_device"]) == 1, batch.clock()   # (window 0 was flagged: this solve did raise what the next push must not see)
    assert_twins(S, B, "(c) solve", prior=True)
    st = push(6, sweeps(6))
    assert (st["chain"], st["redone"], st["as_is"], st["host_waits"]) == (4, 0, 0, 1), st
    assert_twins(S, B, "(c) push", prior=True)
    batch.close()


def test_two_parts_give_the_bits_of_one(hip):
    """A batch of four with the option "parts" = 2 against its twin with "parts" = 1: equal bits, two host waits reported."""
    seeds = (3, 5, 7, 9)
    A = [cases.window(hip, 4, 2, s, optex=0) for s in seeds]
    B = [cases.window(hip, 4, 2, s, optex=0) for s in seeds]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    batch_a.set_option("parts", 1)
    batch_b.set_option("parts", 2)
    for step in range(1, 3):
        k = 4 + step
        for e in A + B:
            cases.imu(e, k)
        items = [item(k)] * 4
        if step == 1:
            batch_a.push_frames(items); batch_b.push_frames(items)
            ra, rb = batch_a.solve(), batch_b.solve()
            batch_a.slide(); batch_b.slide()
        else:
            ra, rb = batch_a.process_laser_odom(items), batch_b.process_laser_odom(items)
        sa, sb = batch_a.push_stats(), batch_b.push_stats()
        assert sa["host_waits"] == 1 and sb["host_waits"] == 2, (sa, sb)
        assert sa["chain"] == sb["chain"] == 4 and sb["redone"] == 0
        _same_reports(ra, rb, f"step {step}")
        assert_twins(A, B, f"step {step}", prior=True)
    batch_a.close(); batch_b.close()


def test_single_and_batched_calls_mix_over_a_handle_s_life(hip):
    """One handle alternates between lio_est_push_frame / lio_est_slide_window and the batched calls from step to step; its twin never sees them."""
    A, B = [cases.window(hip, 5, 2, 7, deskew="imu")], [cases.window(hip, 5, 2, 7, deskew="imu")]
    batch_a, batch_b = capi.EstimatorBatch(hip, A), capi.EstimatorBatch(hip, B)
    batch_a.solve(); A[0].slide()
    batch_b.solve(); batch_b.slide()
    for step in range(1, 5):
        k = 5 + step
        _push_per_handle(A, k)
        if step % 2:
            _push_batched(batch_b, k)
        else:
            _push_per_handle(B, k)
        assert_twins(A, B, f"step {step} push")
        _same_reports(batch_a.solve(), batch_b.solve(), f"step {step}")
        A[0].slide()
        if step % 2:
            B[0].slide()
        else:
            batch_b.slide()
        assert_twins(A, B, f"step {step} slide", prior=True)
    batch_a.close(); batch_b.close()


def test_refusals_change_nothing(hip):
    """LIO_ERR_ARG (-1) and LIO_ERR_STATE (-2) of the header, each before any window is touched: every window as it was, and a following valid call
    equal to the twin's.  (LIO_ERR_DEVICE: tests/test_est_push_batch_abi.py.)"""
    dll = hip.dll
    A, B = [cases.window(hip, 4, 2, 3), cases.window(hip, 4, 2, 5)], [cases.window(hip, 4, 2, 3), cases.window(hip, 4, 2, 5)]
    batch = capi.EstimatorBatch(hip, B)
    k = 5
    for e in A + B:
        cases.imu(e, k)
    before = [cases.observe(e, prior=True, event=True) for e in B]

    def unchanged(what):
        for w, e in enumerate(B):
            cases.assert_same(before[w], cases.observe(e, prior=True, event=True), f"{what}, window {w}")

    good, keep = capi.EstimatorBatch.frames([item(k), item(k)])
    reps = (capi.SolveReport * 2)()
    assert dll.lio_est_batch_push_frames(batch.h, None) == -1
    assert dll.lio_est_batch_process_laser_odom(batch.h, None, reps) == -1
    assert dll.lio_est_batch_push_frames(None, good) == -1 and dll.lio_est_batch_slide_windows(None) == -1
    assert dll.lio_est_batch_push_stats(batch.h, None) == -1
    for field in ("surf_xyzi", "corner_xyzi"):                   # a null cloud with a count, in the LAST window: the first one is not touched either
        bad, keep2 = capi.EstimatorBatch.frames([item(k), item(k)])
        setattr(bad[1], field, None)
        assert dll.lio_est_batch_push_frames(batch.h, bad) == -1, field
        assert dll.lio_est_batch_process_laser_odom(batch.h, bad, reps) == -1, field
    unchanged("LIO_ERR_ARG")
    # a window that is not initialised, behind one that is
    fresh = capi.Estimator(hip, cases.config(hip, 4, 2))
    mixed = [cases.window(hip, 4, 2, 3), fresh]
    cases.imu(mixed[0], k)
    was = cases.observe(mixed[0], event=True)
    bm = capi.EstimatorBatch(hip, mixed)
    assert dll.lio_est_batch_push_frames(bm.h, good) == -2 and dll.lio_est_batch_slide_windows(bm.h) == -2
    assert dll.lio_est_batch_process_laser_odom(bm.h, good, reps) == -2
    cases.assert_same(was, cases.observe(mixed[0], event=True), "an uninitialised window in the batch")
    bm.close()
    # lio_est_push_frame's own refusal: de-skew from the IMU poses and no IMU sample yet — in the second window
    dry = [cases.window(hip, 4, 2, 3, deskew="imu"), cases.window(hip, 4, 2, 5, deskew="imu")]
    cases.imu(dry[0], k)
    was = [cases.observe(e, event=True) for e in dry]
    bd = capi.EstimatorBatch(hip, dry)
    with pytest.raises(capi.LioError):
        dry[1].push_frame(*item(k))                              # (the single call refuses it too)
    assert dll.lio_est_batch_push_frames(bd.h, good) == -2
    assert dll.lio_est_batch_process_laser_odom(bd.h, good, reps) == -2
    for w, e in enumerate(dry):
        cases.assert_same(was[w], cases.observe(e, event=True), f"de-skew precondition, window {w}")
    # a dissolved batch
    hip.dll.lio_est_destroy(dry[1].h)
    dry[1].h = None
    assert len(bd) == 0
    assert dll.lio_est_batch_push_frames(bd.h, good) == -2 and dll.lio_est_batch_slide_windows(bd.h) == -2
    stats = (ctypes.c_int * 8)()
    assert dll.lio_est_batch_push_stats(bd.h, stats) == -2
    bd.close()
    # and the valid call behind all the refusals equals the twin's
    unchanged("all refusals")
    for e in A:                                                  # (A had its IMU samples above: push only)
        cases.push_single(e, item(k))
    return_code = dll.lio_est_batch_push_frames(batch.h, good)
    assert return_code == 0
    assert_twins(A, B, "the valid call behind the refusals")
    batch.close()
