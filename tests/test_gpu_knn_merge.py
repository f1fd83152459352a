"""The merge of the sub-lanes' K-NN lists (csrc/knn_merge.h inside knn_scan_group<5, LPQ>, through the test hook lio_knn_walk) at 4 and 8
lanes per query, on maps that put the winners on chosen sub-lanes and trips (tests/knn_merge_cases.py; that they do is tested without a
GPU in tests/test_knn_merge.py): equal to the one-lane walk, which has no merge, and to the brute force of tests/knn_ref.py — indices,
distance bits and the coordinates at the returned positions, no tolerance."""
import numpy as np
import pytest

import knn_merge_cases as cases
import knn_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def one_lane(hip):
    memo = {}

    def get(name):
        if name not in memo:
            c = cases.get(name)
            memo[name] = hip.knn_walk(c.map, c.query, c.cell, 1)
        return memo[name]
    return get


@pytest.mark.parametrize("lanes", cases.LANES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_merged_lists_equal_one_lane_walk_and_brute_force(hip, one_lane, name, lanes):
    c = cases.get(name)
    got = hip.knn_walk(c.map, c.query, c.cell, lanes)
    knn_ref.compare_a(got, c.ref, c.map)
    idx1, sqd1, nbr1 = one_lane(name)
    np.testing.assert_array_equal(got[0], idx1)
    np.testing.assert_array_equal(got[1].view(np.uint32), sqd1.view(np.uint32))
    np.testing.assert_array_equal(got[2].view(np.uint32), nbr1.view(np.uint32))
    missing = got[0] < 0
    assert np.isposinf(got[1][missing]).all() and (got[2][missing] == 0).all()
