"""The product's lidar moments S = sum rho' z z^T, cost and count (csrc/solve_kernels.h) against tests/moments_ref.py — exactly
rounded fp64 sums of the same per-residual terms — entry by entry, through every path that produces them:

* lio_est_eval_lidar_moments: the resident kernel (k_lidar_moments_resident<R>, R = 1 / 2 / 4 / 8 through
  lio_est_force_moments_per_lane), the MFMA launch pair (k_lidar_moments + k_moment_reduce) over the resident partition
  (resident_moments = 3) and its own (resident_moments = 2),
  stream_sync, and factor sharding (world 2, both ranks in this process: the shares add up);
  several passes at different poses inside one solve scope, as the doorbell sees them across a solve;
* lio_est_batch_get_moments: k_bw_moments' result at the point a batch solve accepted (one and two parts).

Bounds (tests/moments_ref.py): |S - S_ref| <= 1e-12 A entrywise (A = the sums of |rho' z_a z_b|), rows / columns 13..15 exactly 0,
S exactly symmetric, count exact, |cost - cost_ref| <= 1e-11 cost_ref + 1e-15 count.  tests/test_lidar_moments.py shows on the CPU
that a reference missing one residual fails them.  Not covered here: k_lidar_moments_dev (the single-window device loop) runs the
same lidar_moments_body as k_bw_moments."""
import numpy as np
import pytest

import moments_ref as mr

pytestmark = pytest.mark.gpu

# name -> (lio_est_config fields, residuals per lane to force or None, the path the hook must report: 0 MFMA pair, 2 resident)
PATHS = {
    "resident_r1": (dict(resident_moments=1), 1, 2),
    "resident_r2": (dict(resident_moments=1), 2, 2),
    "resident_r4": (dict(resident_moments=1), 4, 2),
    "resident_r8": (dict(resident_moments=1), 8, 2),
    "pair_resident_partition": (dict(resident_moments=3), None, 0),
    "pair_own_partition": (dict(resident_moments=2), None, 0),
    "stream_sync": (dict(resident_moments=1, stream_sync=1), None, 0),
}
SHAPES = [  # per optimised frame of the VLP-16 window (Wo 4): slot count; frames whose points are all far from the map; sparse last
    # chunk (only the newest frame's points stay out of the local map: frames pivot .. W-1 build it, Estimator.cc:1361-1646)
    ((0, 1, 63, 64), (), ()),
    ((65, 255, 256, 257), (), ()),
    ((300, 769, 1025, 40), (3,), ()),
    ((40, 769, 1025, 300), (), (3,)),   # 769: just over the stride of 3 blocks per frame (launch pair; resident at 2 and 4 per lane)
]
WORST = {}   # (path, case) -> (max |S - S_ref| / A, max |cost error|, max cost error / cost): printed at the end of the module


@pytest.fixture(scope="module")
def indoor(oracle):
    return mr.dataset("indoor", oracle)


@pytest.fixture(scope="module")
def outdoor(oracle):
    return mr.dataset("outdoor", oracle)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        s, c, cr = WORST[k]
        print(f"[moments] {k[0]:24s} {k[1]:28s} max|S-S_ref|/A {s:.2e}  max|cost err| {c:.2e}  rel {cr:.2e}")


def _window(hip, data, kind, path, **kw):
    fields, per_lane, expect = PATHS[path]
    est = mr.make_window(hip, data, kind, **kw, **fields)
    if per_lane is not None:
        est.force_moments_per_lane(per_lane)
    return est, expect


def _check(est, passes, path, case, expect_path):
    feats = mr.window_features(est)
    out, got = est.eval_lidar_moments(passes)
    assert got == expect_path, (path, got)   # a silent fallback to another path cannot pass
    worst = (0.0, 0.0, 0.0)
    for p in range(passes.shape[0]):
        w = mr.assert_moments(out[p], mr.window_moments(feats, passes[p]), f"{path} {case} pass {p}")
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    # the same poses again later in the same solve scope: the same bits (no stale register cache, no leftover of another pass)
    assert np.array_equal(out[4], out[1])
    assert not np.array_equal(out[2], out[1])
    WORST[(path, case)] = worst
    return feats, out


@pytest.mark.parametrize("path", list(PATHS))
def test_headline_window(hip, outdoor, path):
    """the HDL-64E window (W 15 / Wo 5, keep_features 0 so that the resident form takes it)"""
    est, expect = _window(hip, outdoor, "outdoor", path)
    passes = mr.make_passes(mr.window_rt(est.get_window(), 15, 5), 21)
    feats, _ = _check(est, passes, path, "headline", expect)
    assert sum(f[0].shape[0] for f in feats) > 20000


@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("path", ["resident_r1", "resident_r2", "resident_r4", "resident_r8", "pair_resident_partition", "pair_own_partition"])
def test_shapes(hip, oracle, indoor, path, shape):
    counts, far, sparse = SHAPES[shape]
    stacks = mr.shape_stacks(oracle, indoor, "indoor", counts, far, sparse)
    est, expect = _window(hip, indoor, "indoor", path, stacks=stacks)
    passes = mr.make_passes(mr.window_rt(est.get_window(), 8, 4), 30 + shape)
    feats, out = _check(est, passes, path, f"slots {counts}", expect)
    for f in far:
        assert feats[f][0].shape[0] == 0
        assert np.all(out[:, f, :] == 0.0)


def _keep_features_window(hip, indoor, outdoor, kind, path, expect):
    """keep_features = 1: the newest frame holds rounds x M slots (slot j's point: stack[j % M])"""
    data = indoor if kind == "indoor" else outdoor
    W, Wo = (8, 4) if kind == "indoor" else (15, 5)
    est, _ = _window(hip, data, kind, path, keep=1)
    passes = mr.make_passes(mr.window_rt(est.get_window(), W, Wo), 40)
    feats, _ = _check(est, passes, path, f"{kind} keep_features", expect)
    assert feats[-1][0].shape[0] > est.get_surf_stack(W).shape[0]
    return est, passes


@pytest.mark.parametrize("kind", ["indoor", "outdoor"])
@pytest.mark.parametrize("path,expect", [("resident_r8", 2)])
def test_keep_features_window(hip, indoor, outdoor, kind, path, expect):
    """the keep_features window at 8 residuals per lane: the resident kernel takes it (1 per lane: test_force_moments_per_lane)"""
    _keep_features_window(hip, indoor, outdoor, kind, path, expect)


@pytest.mark.parametrize("kind", ["indoor", "outdoor"])
def test_force_moments_per_lane(hip, indoor, outdoor, kind):
    """lio_est_force_moments_per_lane on the keep_features window.  At 1 residual per lane the window needs more blocks than the
    device keeps co-resident, and the launch pair must take the passes instead (path 0) — with the same sums.  0 hands the choice
    back to the rule, which finds a count whose blocks are co-resident (path 2).  Values other than 0 / 1 / 2 / 4 / 8 are refused."""
    from lio_amd import capi

    est, passes = _keep_features_window(hip, indoor, outdoor, kind, "resident_r1", 0)
    est.force_moments_per_lane(0)
    assert est.eval_lidar_moments(passes)[1] == 2
    for v in (-1, 3, 16):
        with pytest.raises(capi.LioError):
            est.force_moments_per_lane(v)


@pytest.mark.parametrize("case", ["headline", "shapes"])
def test_factor_sharding_shares_add_up(hip, oracle, indoor, outdoor, case):
    """world 2, both ranks in this process with a no-op all-reduce: each rank's hook returns its own share (slot_begin, slot_end),
    and the two shares add up to the whole window's moments"""
    outs = []
    for rank in range(2):
        if case == "headline":
            est, _ = _window(hip, outdoor, "outdoor", "resident_r1")
            W, Wo = 15, 5
        else:
            est, _ = _window(hip, indoor, "indoor", "resident_r1", stacks=mr.shape_stacks(oracle, indoor, "indoor", (1, 65, 257, 769)))
            W, Wo = 8, 4
        est.set_factor_sharding(rank, 2, lambda buf: None)
        passes = mr.make_passes(mr.window_rt(est.get_window(), W, Wo), 50)
        out, path = est.eval_lidar_moments(passes)
        assert path == 0   # factor sharding never uses the resident form
        outs.append(out)
        feats = mr.window_features(est)
    total = outs[0] + outs[1]
    assert not np.array_equal(outs[0], total)   # (both ranks hold residuals)
    worst = (0.0, 0.0, 0.0)
    for p in range(passes.shape[0]):
        w = mr.assert_moments(total[p], mr.window_moments(feats, passes[p]), f"sharded {case} pass {p}")
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    WORST[("sharding_world2", case)] = worst


def _batch_windows(hip, indoor, outdoor, copies):
    """the batch of 8: four HDL-64E and four VLP-16 windows (seeds 3..6), each `copies` times"""
    ests, kinds = [], []
    for c in range(copies):
        for k in range(8):
            kind = "outdoor" if k % 2 == 0 else "indoor"
            # (extrinsic held constant: a fresh window then goes to the device loop in its first solve, est_batch.h)
            ests.append(mr.make_window(hip, outdoor if kind == "outdoor" else indoor, kind, seed=3 + k // 2, build=False, opt_extrinsic=0))
            kinds.append((kind, k))
    return ests, kinds


def _check_batch(hip, b, ests, kinds, case, min_device):
    refs = {}
    worst = (0.0, 0.0, 0.0)
    n_device = 0
    for w, e in enumerate(ests):
        try:
            out, Rt = b.moments(w)
        except Exception:   # noqa: BLE001 - a window the device loop handed to the single-window path
            continue
        n_device += 1
        feats = mr.window_features(e)   # lio_est_get_features on an adopted handle: the batch's slots
        key = kinds[w][1]
        if key in refs:
            Rt0, feats0, ref = refs[key]
            assert np.array_equal(Rt, Rt0)   # a window gives the same bits in any batch position
            for (p, c), (p0, c0) in zip(feats, feats0):
                assert np.array_equal(p, p0) and np.array_equal(c, c0)
        else:
            ref = mr.window_moments(feats, Rt)
            refs[key] = (Rt, feats, ref)
        wr = mr.assert_moments(out, ref, f"{case} window {w}")
        worst = tuple(max(a, x) for a, x in zip(worst, wr))
    print(f"[moments] batch {case}: {n_device} of {len(ests)} windows solved on the device")
    assert n_device >= min_device, n_device
    WORST[("batch", case)] = worst
    return n_device


def test_batch_moments_one_part(hip, indoor, outdoor):
    from lio_amd import capi

    ests, kinds = _batch_windows(hip, indoor, outdoor, 1)
    b = capi.EstimatorBatch(hip, ests)
    b.set_option("parts", 1)
    b.solve()
    _check_batch(hip, b, ests, kinds, "8 windows, parts 1", len(ests))
    # a second solve from the point the first one reached: few steps (possibly none) are accepted, and the moments at the
    # accepted point must still be the ones of that point
    b.solve()
    _check_batch(hip, b, ests, kinds, "8 windows, re-solve", 0)
    b.close()


def test_batch_moments_two_parts(hip, indoor, outdoor):
    from lio_amd import capi

    ests, kinds = _batch_windows(hip, indoor, outdoor, 12)
    b = capi.EstimatorBatch(hip, ests)
    b.set_option("parts", 2)
    b.solve()
    _check_batch(hip, b, ests, kinds, "96 windows, parts 2", len(ests))
    b.close()
