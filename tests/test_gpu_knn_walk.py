"""The K-NN walk the product runs (csrc/cloud_device.h: knn_scan_group<5, LPQ>, through the test hook lio_knn_walk) against the exact
brute-force references of tests/knn_ref.py on the cases of tests/knn_cases.py, at 1, 4 and 8 lanes per query: equality with layer A
(indices, distance bits, the coordinates at the positions the plane fit loads — no tolerance, no query left out), then layer B (fp64,
no cells).  What every case contains, and that these checks notice planted errors, is tested without a GPU in tests/test_knn_walk.py."""
import numpy as np
import pytest

import knn_cases
import knn_ref
from lio_amd import capi, pipeline, synth

pytestmark = pytest.mark.gpu

_RUNS = [(name, lanes) for name in knn_cases.NAMES for lanes in (1, 4, 8)
         if not (name == "large" and lanes == 4)]      # the large case: the one-lane form the product picks at that size, and the eight-lane form


@pytest.mark.parametrize("name,lanes", _RUNS)
def test_walk_equals_brute_force(hip, name, lanes):
    c = knn_cases.get(name)
    assert lanes in c.lanes
    got = hip.knn_walk(c.map, c.query, c.cell, lanes)
    knn_ref.compare_a(got, c.ref_a, c.map)
    n_in, n_out = knn_ref.compare_b(got[0], c.ref_b, c.cell, c.cap)
    print(f"{name} lanes {lanes}: {c.query.shape[0]} queries, {knn_ref.rank56_ties(c.ref_a[:2])} exact rank-5/6 ties, layer B leaves out {n_out} of "
          f"{n_in} (cap {c.cap:.0%}), fifth neighbour outside the own row: {knn_ref.fifth_outside_own_row(c.ref_a)}")
    if c.lattice:
        assert n_out == 0


@pytest.mark.parametrize("lanes", [1, 4, 8])
def test_non_finite_query_finds_nothing_and_disturbs_nobody(hip, lanes):
    """the contract of include/lio_test_hooks.h, stated on its own: all -1 / +inf / zeros for a query with a NaN or inf coordinate, and
    the other queries of the launch (its wave's among them) get what they get without it"""
    c = knn_cases.get("non_finite_queries")
    idx, sqd, nbr = hip.knn_walk(c.map, c.query, c.cell, lanes)
    bad = c.bad_rows
    assert (idx[bad] == -1).all() and np.isposinf(sqd[bad]).all() and (nbr[bad] == 0).all()
    clean = c.query.copy()
    clean[bad, :3] = c.query[(bad + 1) % len(clean), :3]
    clean[bad, :3] = np.where(np.isfinite(clean[bad, :3]), clean[bad, :3], 0)
    idx2, sqd2, nbr2 = hip.knn_walk(c.map, clean, c.cell, lanes)
    good = np.setdiff1d(np.arange(len(clean)), bad)
    np.testing.assert_array_equal(idx[good], idx2[good])
    np.testing.assert_array_equal(sqd[good].view(np.uint32), sqd2[good].view(np.uint32))
    np.testing.assert_array_equal(nbr[good], nbr2[good])


def test_walk_hook_refuses_other_lane_counts(hip):
    c = knn_cases.get("small_map_5")
    for lanes in (0, 2, 3, 16, 64):
        with pytest.raises(capi.LioError):
            hip.knn_walk(c.map, c.query, c.cell, lanes)


def test_knn_entry_point_is_the_walk_with_a_radius_cut(hip):
    """lio_knn (k = 1 and 5) runs the same walk: its answers are layer A's, cut at the radius"""
    c = knn_cases.get("random_cell1.0001")
    r2 = np.float32(((c.cell - 1e-6) / 1.0001) ** 2)
    cellk = np.float32(np.sqrt(r2)) * np.float32(1.0001) + np.float32(1e-6)     # the cell lio_knn derives from the radius
    ref = knn_ref.layer_a(c.map, c.query, cellk)
    for k in (1, 5):
        idx, sqd = hip.knn(c.map, c.query, k, radius_sq=float(r2))
        inside = ref[1][:, :k] < r2
        assert inside.any() and not inside.all()
        np.testing.assert_array_equal(idx, np.where(inside, ref[0][:, :k], -1))
        np.testing.assert_array_equal(sqd, np.where(inside, ref[1][:, :k], np.float32(np.inf)))


def test_calculate_features_four_lane_form(hip, oracle):
    """lio_calculate_features takes four lanes per query from 50 000 queries (k_features<false, 4>); below that, eight.  One call of
    52 000 queries is bit-equal to the same queries in two calls of 26 000, and bit-equal to the oracle, like the eight-lane form
    (tests/test_gpu_parity.py::test_calculate_features_matches_oracle)."""
    ds = synth.make_dataset("indoor", 2, 0.2)
    surf0, _ = pipeline.feature_clouds(oracle, ds.lidar, ds.frames[0].scan)
    surf1, _ = pipeline.feature_clouds(oracle, ds.lidar, ds.frames[1].scan)
    m = oracle.voxel_grid(surf0, 0.4)
    s = oracle.voxel_grid(surf1, 0.4)
    R0 = ds.frames[0].R_wb @ ds.R_lb.T
    R1 = ds.frames[1].R_wb @ ds.R_lb.T
    p0 = ds.frames[0].p_wb - R0 @ ds.t_lb
    p1 = ds.frames[1].p_wb - R1 @ ds.t_lb
    T = capi.TransformF.make(synth.quat_from_rot(R0.T @ R1), R0.T @ (p1 - p0))
    rng = np.random.default_rng(31)
    n = 52000
    big = s[rng.integers(0, len(s), n)].copy()
    big[len(s):, :3] += rng.normal(0, 0.02, (n - len(s), 3)).astype(np.float32)
    big[:len(s)] = s
    va, ca, sa = hip.calculate_features(m, big, T)
    halves = [hip.calculate_features(m, big[a:a + n // 2], T) for a in (0, n // 2)]
    np.testing.assert_array_equal(va, np.concatenate([h[0] for h in halves]))
    np.testing.assert_array_equal(ca.view(np.uint32), np.concatenate([h[1] for h in halves]).view(np.uint32))
    np.testing.assert_array_equal(sa.view(np.uint32), np.concatenate([h[2] for h in halves]).view(np.uint32))
    vb, cb, sb = oracle.calculate_features(m, big, T)
    assert vb.sum() > 20000
    np.testing.assert_array_equal(va, vb)
    np.testing.assert_array_equal(ca.view(np.uint32), cb.view(np.uint32))
    np.testing.assert_array_equal(sa.view(np.uint32), sb.view(np.uint32))
