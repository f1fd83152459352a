"""The lidar factor's normal-equation moments S = sum rho' z z^T, cost and count (csrc/solve_kernels.h) as the oracle's test hook
lio_est_eval_lidar_moments forms them — plain serial fp64 sums over its own feature slots — against tests/moments_ref.py, the
exactly rounded sums of the same per-residual terms.  The bounds are the ones the product's kernels are held to
(tests/test_gpu_lidar_moments.py); the second half shows that they are tight enough to notice one residual in 1e5: a reference
missing a residual, with one Cauchy weight off by 1e-9, with two frames' poses swapped, or with two passes exchanged fails them.
No GPU needed."""
import numpy as np
import pytest

import moments_ref as mr

SHAPES = [  # per optimised frame of the VLP-16 window (Wo 4): slot count; frames whose points are all far from the map; sparse last
    # chunk (only the newest frame's points stay out of the local map: frames pivot .. W-1 build it, Estimator.cc:1361-1646)
    ((0, 1, 63, 64), (), ()),
    ((65, 255, 256, 257), (), ()),
    ((300, 769, 1025, 40), (3,), ()),
    ((40, 769, 1025, 300), (), (3,)),
]


@pytest.fixture(scope="module")
def indoor(oracle):
    return mr.dataset("indoor", oracle)


@pytest.fixture(scope="module")
def headline(oracle):
    """the HDL-64E window (W 15 / Wo 5), one pass at its own poses and two perturbed ones, with the oracle's moments"""
    data = mr.dataset("outdoor", oracle)
    est = mr.make_window(oracle, data, "outdoor")
    feats = mr.window_features(est)
    Rt = mr.window_rt(est.get_window(), 15, 5)
    rng = np.random.default_rng(7)
    passes = np.stack([Rt, mr.perturbed_rt(Rt, rng), mr.perturbed_rt(Rt, rng)])
    out, path = est.eval_lidar_moments(passes)
    assert path == -1
    return feats, passes, out


@pytest.mark.parametrize("counts,far,sparse", SHAPES)
def test_oracle_moments_at_shapes(oracle, indoor, counts, far, sparse):
    est = mr.make_window(oracle, indoor, "indoor", stacks=mr.shape_stacks(oracle, indoor, "indoor", counts, far, sparse))
    feats = mr.window_features(est)
    for f in far:
        assert feats[f][0].shape[0] == 0
    Rt = mr.window_rt(est.get_window(), 8, 4)
    passes = mr.make_passes(Rt, 11)
    out, _ = est.eval_lidar_moments(passes)
    for p in range(passes.shape[0]):
        mr.assert_moments(out[p], mr.window_moments(feats, passes[p]), f"pass {p}")
    assert np.array_equal(out[4], out[1])
    for f in far:
        assert np.all(out[:, f, :] == 0.0)


def test_oracle_moments_keep_features(oracle, indoor):
    """keep_features = 1: the newest frame holds rounds x M slots, slot j's point is stack[j % M]"""
    est = mr.make_window(oracle, indoor, "indoor", keep=1)
    feats = mr.window_features(est)
    assert feats[-1][0].shape[0] > est.get_surf_stack(8).shape[0]   # more factors than points: slot indices wrap
    Rt = mr.window_rt(est.get_window(), 8, 4)
    passes = mr.make_passes(Rt, 12)
    out, _ = est.eval_lidar_moments(passes)
    for p in range(passes.shape[0]):
        mr.assert_moments(out[p], mr.window_moments(feats, passes[p]), f"pass {p}")


def test_oracle_moments_headline(headline):
    feats, passes, out = headline
    assert sum(f[0].shape[0] for f in feats) > 20000
    for p in range(passes.shape[0]):
        mr.assert_moments(out[p], mr.window_moments(feats, passes[p]), f"pass {p}")


def _most_exposed(feats, Rt):
    """(frame, residual) whose share of some entry's |terms| sum is the largest: where one residual moves S the most"""
    best = (0.0, 0, 0)
    for f, ((p, c), rt) in enumerate(zip(feats, Rt)):
        r, rho, z = mr.frame_terms(p, c, *mr.split_rt(rt))
        for a in range(13):
            for b in range(a, 13):
                t = np.abs(rho * z[:, a] * z[:, b])
                k = int(np.argmax(t))
                share = t[k] / t.sum()
                if share > best[0]:
                    best = (share, f, k)
    return best[1], best[2]


def test_sensitivity_one_residual_dropped(headline):
    feats, passes, out = headline
    ref = mr.window_moments(feats, passes[0])
    assert mr.frames_within(out[0], ref)
    f = 2
    bad = list(ref)
    bad[f] = mr.frame_moments(*feats[f], *mr.split_rt(passes[0][f]), drop=feats[f][0].shape[0] // 2)
    assert not mr.frames_within(out[0], bad)
    # and not only through the count: the S bound alone notices the missing residual
    bad[f]["count"] = ref[f]["count"]
    assert not mr.frames_within(out[0], bad)


def test_sensitivity_one_weight(headline):
    feats, passes, out = headline
    ref = mr.window_moments(feats, passes[0])
    f, k = _most_exposed(feats, passes[0])
    bad = list(ref)
    bad[f] = mr.frame_moments(*feats[f], *mr.split_rt(passes[0][f]), rho_scale=(k, 1.0 + 1e-9))
    assert not mr.frames_within(out[0], bad)


def test_sensitivity_frames_swapped(headline):
    feats, passes, out = headline
    Rt = passes[1].copy()
    Rt[[1, 3]] = Rt[[3, 1]]
    assert not mr.frames_within(out[1], mr.window_moments(feats, Rt))


def test_sensitivity_passes_exchanged(headline):
    feats, passes, out = headline
    assert mr.frames_within(out[2], mr.window_moments(feats, passes[2]))
    assert not mr.frames_within(out[1], mr.window_moments(feats, passes[2]))
    assert not mr.frames_within(out[2], mr.window_moments(feats, passes[1]))


def test_oracle_batch_moments_are_zeros(oracle, indoor):
    from lio_amd import capi

    ests = [mr.make_window(oracle, indoor, "indoor") for _ in range(2)]
    b = capi.EstimatorBatch(oracle, ests)
    b.solve()
    out, Rt = b.moments(1)
    assert out.shape == (4, 258) and Rt.shape == (4, 12)
    assert np.all(out == 0) and np.all(Rt == 0)
    b.close()


def test_oracle_force_moments_per_lane(oracle, indoor):
    """the hook checks its argument (0, 1, 2, 4, 8) and otherwise leaves the oracle's sums alone"""
    from lio_amd import capi

    est = mr.make_window(oracle, indoor, "indoor")
    passes = mr.make_passes(mr.window_rt(est.get_window(), 8, 4), 13)
    out, _ = est.eval_lidar_moments(passes)
    for v in (-1, 3, 16):
        with pytest.raises(capi.LioError):
            est.force_moments_per_lane(v)
    for v in (1, 2, 4, 8, 0):
        est.force_moments_per_lane(v)
        assert np.array_equal(est.eval_lidar_moments(passes)[0], out)
