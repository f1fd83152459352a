"""The K-NN walk's references and checks, without a GPU: the oracle's serial statement of lio_knn_walk (include/lio_test_hooks.h) equals
layer A of tests/knn_ref.py on every case of tests/knn_cases.py, layer A satisfies layer B (fp64, no cells), every case contains what it
is there for, and the comparison the GPU tests use (tests/test_gpu_knn_walk.py) notices the errors a walk can make."""
import ctypes

import numpy as np
import pytest

import knn_cases
import knn_ref
from lio_amd import capi


def _ref_result(c):
    """layer A in the shape of a walk's result: (idx (m, 5), sqd (m, 5), nbr_xyz (m, 5, 3)), fresh copies"""
    idx, sqd = c.ref_a[0][:, :5].copy(), c.ref_a[1][:, :5].copy()
    nbr = np.concatenate([c.map[:, :3], np.zeros((1, 3), np.float32)])[np.where(idx >= 0, idx, -1)]
    return idx, sqd, nbr


@pytest.mark.parametrize("name", knn_cases.NAMES)
def test_oracle_walk_equals_layer_a(oracle, name):
    c = knn_cases.get(name)
    got = oracle.knn_walk(c.map, c.query, c.cell, 8)
    knn_ref.compare_a(got, c.ref_a, c.map)
    knn_ref.compare_a(_ref_result(c), c.ref_a, c.map)      # and the helper the planted errors start from is itself clean


@pytest.mark.parametrize("name", knn_cases.NAMES)
def test_layer_a_satisfies_layer_b(name):
    c = knn_cases.get(name)
    n_in, n_out = knn_ref.compare_b(c.ref_a[0], c.ref_b, c.cell, c.cap)
    print(f"{name}: {c.query.shape[0]} queries, {knn_ref.rank56_ties(c.ref_a[:2])} exact rank-5/6 ties, layer B leaves out {n_out} of {n_in} "
          f"in-radius query-rank pairs (cap {c.cap:.0%}), fifth neighbour outside the own row: {knn_ref.fifth_outside_own_row(c.ref_a)}")
    if c.lattice:
        assert n_out == 0
        # exact differences: the fp32 and fp64 distances are the same numbers
        f = np.isfinite(c.ref_b[1][:, :5])
        assert (c.ref_a[1][:, :5][f].astype(np.float64) == c.ref_b[1][:, :5][f]).all()


def test_oracle_hook_checks_its_arguments(oracle):
    c = knn_cases.get("small_map_5")
    for lanes in (0, 2, 3, 16, -1):
        with pytest.raises(capi.LioError):
            oracle.knn_walk(c.map, c.query, c.cell, lanes)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.LioError):
            oracle.knn_walk(c.map, c.query, cell, 8)
    for lanes in (1, 4, 8):
        knn_ref.compare_a(oracle.knn_walk(c.map, c.query, c.cell, lanes), c.ref_a, c.map)


# ------------------------------------------------------------------------------------------------ the cases hold what they claim
def test_random_cases_are_sparse_and_dense_enough():
    a, b = knn_cases.get("random_cell1.0001"), knn_cases.get("random_cell0.3")
    assert a.map.shape[0] == 40000 and a.query.shape[0] == 3000
    assert (a.ref_a[0][:, 4] >= 0).all()
    lo, hi = knn_ref.grid_of(b.map, b.cell)
    occupied = np.unique(b.ref_a[2], axis=0).shape[0]
    assert occupied < 0.5 * np.prod(hi - lo + 1)            # most cells of the small-cell grid are empty
    assert 0 < (b.ref_a[0][:, 4] < 0).sum() < 0.5 * b.query.shape[0]   # so some queries find fewer than five


@pytest.mark.parametrize("name", ["ties_cell0.5", "ties_cell1.0001"])
def test_tie_case_has_ties_everywhere(name):
    c = knn_cases.get(name)
    idx, sqd, pc, qc, _ = c.ref_a
    assert knn_ref.rank56_ties((idx, sqd)) >= 1000
    tied = (sqd[:, :4] == sqd[:, 1:5]) & (idx[:, 1:5] >= 0)
    assert tied.sum() >= 4000
    # a tie is broken by the ORIGINAL index ...
    assert (idx[:, :4][tied] < idx[:, 1:5][tied]).all()
    # ... also where the two points sit in different rows of cells (different sub-lanes / phases of the walk find them)
    pa, pb = pc[np.maximum(idx[:, :4], 0)], pc[np.maximum(idx[:, 1:5], 0)]
    assert (tied & ((pa[:, :, 1] != pb[:, :, 1]) | (pa[:, :, 2] != pb[:, :, 2]))).sum() >= 500
    # and index order is not the order of the cells: ascending cell id along a tied pair goes both ways
    cid = lambda p: p[..., 0] + 1000 * (p[..., 1] + 1000 * p[..., 2])
    assert (tied & (cid(pa) > cid(pb))).sum() >= 200 and (tied & (cid(pa) < cid(pb))).sum() >= 200
    # every point twice, at different indices
    u, cnt = np.unique(c.map[:, :3], axis=0, return_counts=True)
    assert (cnt == 2).all()


def test_dense_cases_fill_and_empty_the_runs():
    c = knn_cases.get("dense_cells")
    pc, qc = c.ref_a[2], c.ref_a[3]
    lo, _ = knn_ref.grid_of(c.map, c.cell)
    centre = qc[0]
    assert (qc[:1200] == centre).all()
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = int((pc == centre + np.array([dx, dy, dz])).all(axis=1).sum())
                assert (n == 5000) if (dx, dy, dz) == (0, 0, 0) else (200 <= n <= 600), (dx, dy, dz, n)
    s = knn_cases.get("single_run")
    pc, qc = s.ref_a[2], s.ref_a[3]
    centre = qc[0]
    assert (qc[:1500] == centre).all()
    rows = {(int(p[1] - centre[1]), int(p[2] - centre[2])) for p in pc[(np.abs(pc - centre) <= 1).all(axis=1)]}
    assert rows == {(1, -1)}                                   # one run of the nine holds points, and it is not the own row
    assert (s.ref_a[0][:1500, 4] >= 0).all()


def test_row_skip_case_needs_the_other_rows_and_can_skip_them():
    c = knn_cases.get("row_skip")
    idx, sqd, pc, qc, in_grid = c.ref_a
    n_face = c.n_face
    cellw = c.cell
    u = c.query[:n_face, 1:3].astype(np.float64) / cellw
    f = u - np.floor(u)
    edge = np.minimum(f, 1 - f)
    assert (edge.min(axis=1) < 2.5e-3).all()                   # within 2e-3 cell of a face (plus fp32 rounding of the coordinate)
    assert (c.query[:n_face, 1:3] < 0).any() and (c.query[:n_face, 1:3] > 0).any()
    assert ((f < 0.5) & (edge < 2.5e-3)).sum() > 500 and ((f > 0.5) & (edge < 2.5e-3)).sum() > 500    # both sides
    p5 = pc[idx[:n_face, 4]]
    dy, dz = p5[:, 1] != qc[:n_face, 1], p5[:, 2] != qc[:n_face, 2]
    assert (dy ^ dz).sum() > 1000, "true fifth neighbours in face rows"
    assert (dy & dz).sum() > 500, "true fifth neighbours in corner rows"
    # the other kind: the own row already holds five points closer than any other row can be
    own = idx[n_face:, :5]
    po = pc[own]
    assert ((po[:, :, 1] == qc[n_face:, None, 1]) & (po[:, :, 2] == qc[n_face:, None, 2])).all(axis=1).sum() > 1000
    assert (sqd[n_face:, 4] < (0.29 * cellw) ** 2).sum() > 1000    # the queries sit 0.3 cell or more from every face


def test_edge_cases_reach_the_edges():
    c = knn_cases.get("flat_map")
    lo, hi = knn_ref.grid_of(c.map, c.cell)
    assert hi[2] - lo[2] + 1 == 3
    qz = c.ref_a[3][:, 2]
    assert (qz == lo[2]).sum() > 100 and (qz == hi[2]).sum() > 100 and (~c.ref_a[4]).sum() > 100
    c = knn_cases.get("grid_margin")
    lo, hi = knn_ref.grid_of(c.map, c.cell)
    qc, in_grid = c.ref_a[3], c.ref_a[4]
    for ax in range(3):
        assert (in_grid & (qc[:, ax] == lo[ax])).sum() > 20 and (in_grid & (qc[:, ax] == hi[ax])).sum() > 20
    assert (~in_grid).sum() > 300
    assert (c.ref_a[0][~in_grid] == -1).all() and np.isinf(c.ref_a[1][~in_grid]).all()
    c = knn_cases.get("cell_corners")
    assert (c.query[:, :3] / np.float32(c.cell) == np.round(c.query[:, :3] / np.float32(c.cell))).all()
    c = knn_cases.get("far_400m")
    assert np.abs(c.query[:, :2]).min() > 380 and (c.query[:, 0] > 0).any() and (c.query[:, 0] < 0).any()
    assert (c.ref_a[0][:, 4] >= 0).all()


def test_small_ragged_and_non_finite_cases():
    for n in (0, 1, 4, 5):
        c = knn_cases.get(f"small_map_{n}")
        found = (c.ref_a[0][:, :5] >= 0).sum(axis=1)
        assert c.map.shape[0] == n and found.max() == n and (n == 0 or found.min() == 0)
    assert [knn_cases.get(f"ragged_m{m}").query.shape[0] for m in knn_cases.RAGGED_M] == list(knn_cases.RAGGED_M)
    c = knn_cases.get("non_finite_queries")
    bad = ~np.isfinite(c.query[:, :3]).all(axis=1)
    assert bad.sum() == 90 and (np.nonzero(bad)[0] == c.bad_rows).all()
    assert np.isnan(c.query[bad, :3]).any() and (c.query[bad, :3] == np.inf).any() and (c.query[bad, :3] == -np.inf).any()
    assert (np.isfinite(c.query[bad, :3]).sum(axis=1) == 2).all()      # one coordinate each
    assert (c.ref_a[0][bad] == -1).all() and (c.ref_a[0][~bad][:, 4] >= 0).sum() > 800
    # every wave of 64 one-lane queries and of 8 eight-lane queries that holds a bad query also holds good ones
    assert all((~bad[r // 64 * 64: r // 64 * 64 + 64]).any() for r in c.bad_rows)
    c = knn_cases.get("large")
    assert c.query.shape[0] >= 100000 and c.map.shape[0] == 80000 and c.lanes == (1, 8)


# ------------------------------------------------------------------------------------------------ the checks notice planted errors
def test_check_notices_two_tied_neighbours_exchanged():
    c = knn_cases.get("ties_cell0.5")
    idx, sqd, nbr = _ref_result(c)
    q, k = np.argwhere(sqd[:, :4] == sqd[:, 1:5])[7]
    idx[q, [k, k + 1]] = idx[q, [k + 1, k]]
    nbr[q, [k, k + 1]] = nbr[q, [k + 1, k]]                   # consistent with the exchanged indices: only the ORDER is wrong
    with pytest.raises(AssertionError, match=rf"indices differ at 1 of 4000 queries; first: query {q} "):
        knn_ref.compare_a((idx, sqd, nbr), c.ref_a, c.map)


def test_check_notices_a_dropped_candidate_row():
    c = knn_cases.get("row_skip")
    ridx, _, pc, qc, _ = c.ref_a
    q = 3
    p5 = pc[ridx[q, 4]]
    assert (p5[1], p5[2]) != (qc[q, 1], qc[q, 2])            # the fifth neighbour sits in a face or corner row: drop that row
    keep = ~((pc[:, 1] == p5[1]) & (pc[:, 2] == p5[2]))
    sub_idx, sub_sqd = knn_ref.layer_a(c.map[keep], c.query[q:q + 1], c.cell, grid_from=c.map)
    idx, sqd, nbr = _ref_result(c)
    idx[q] = np.where(sub_idx[0, :5] >= 0, np.nonzero(keep)[0][np.maximum(sub_idx[0, :5], 0)], -1)
    sqd[q] = sub_sqd[0, :5]
    nbr[q] = np.where((idx[q] >= 0)[:, None], c.map[np.maximum(idx[q], 0), :3], 0)
    with pytest.raises(AssertionError, match=rf"indices differ at 1 of 3600 queries; first: query {q} "):
        knn_ref.compare_a((idx, sqd, nbr), c.ref_a, c.map)
    # layer B sees it too: what came back is not the nearest
    with pytest.raises(AssertionError, match=rf"not the fp64 nearest at 1 queries; first: query {q} "):
        knn_ref.compare_b(idx, c.ref_b, c.cell, c.cap)


def test_check_notices_the_sixth_in_place_of_the_fifth():
    c = knn_cases.get("ties_cell1.0001")
    idx, sqd, nbr = _ref_result(c)
    q = int(np.nonzero(c.ref_a[1][:, 4] == c.ref_a[1][:, 5])[0][11])    # same distance: only the index tells them apart
    idx[q, 4] = c.ref_a[0][q, 5]
    nbr[q, 4] = c.map[idx[q, 4], :3]
    with pytest.raises(AssertionError, match=rf"indices differ at 1 of 4000 queries; first: query {q} "):
        knn_ref.compare_a((idx, sqd, nbr), c.ref_a, c.map)
    with pytest.raises(AssertionError, match=rf"not the fp64 nearest at 1 queries; first: query {q} "):
        knn_ref.compare_b(idx, c.ref_b, c.cell, c.cap)


def test_check_notices_neighbour_coordinates_of_another_point_at_the_same_distance():
    c = knn_cases.get("ties_cell0.5")
    idx, sqd, nbr = _ref_result(c)
    tied = (sqd[:, :4] == sqd[:, 1:5]) & (nbr[:, :4] != nbr[:, 1:5]).any(axis=2)     # same distance, a different place
    q, k = np.argwhere(tied)[5]
    nbr[q, k] = nbr[q, k + 1]
    with pytest.raises(AssertionError, match=rf"neighbour coordinates are not map\[idx\] at 1 queries; first: query {q} "):
        knn_ref.compare_a((idx, sqd, nbr), c.ref_a, c.map)


def test_check_notices_a_distance_off_by_one_ulp():
    c = knn_cases.get("random_cell1.0001")
    idx, sqd, nbr = _ref_result(c)
    sqd.view(np.uint32)[1234, 2] += 1
    with pytest.raises(AssertionError, match=r"distance bits differ at 1 queries; first: query 1234 "):
        knn_ref.compare_a((idx, sqd, nbr), c.ref_a, c.map)


def test_layer_b_cap_is_enforced():
    """the share left out is asserted, not reported: two points 1e-9 apart in distance are left out, and a cap of zero refuses that"""
    mp = knn_cases.xyzi([[1.0, 0, 0], [0, 1.0 + 2.0 ** -23, 0], [0.5, 0, 0]])
    q = knn_cases.xyzi([[0, 0, 0]])
    mp = np.concatenate([mp, knn_cases.xyzi([[3.0, 3.0, 3.0]])])
    ref = knn_ref.layer_a(mp, q, 2.0)
    ranks = knn_ref.layer_b_ranks(mp, q, 2.0)
    assert knn_ref.compare_b(ref[0], ranks, 2.0, 1.0) == (3, 2)
    with pytest.raises(AssertionError, match="leaves out 2 of 3"):
        knn_ref.compare_b(ref[0], ranks, 2.0, 0.01)
