"""The voxel filter's sort (docs/voxel_sort.md; include/lio_vox_sort.h): a sample sort in three launches, one direct launch up to one bucket's
capacity, the library's radix sort when a bucket overflows.

The sorted values are the points' own indices, so the result is the stable sort by key whichever path runs: the reference of the sort hook
is numpy.argsort(keys, kind="stable"), integers compared exactly, and every case asserts the path that served it.  The reference of the
filter is the oracle's voxel grid, bit for bit, as in test_gpu_parity.py.

The sizing rule the cases are built on (include/lio_vox_sort.h), modelled in numpy by _model_fills: n <= 4096 keys are sorted directly by one launch;
above, NB = ceil(n / 384) buckets hold 4096 pairs each, the sample is the S = 8 NB keys at floor((j + 0.5) n / S), splitter b is the sorted
sample's entry 8 b, and a key's bucket is the number of splitters <= key.
"""
import numpy as np
import pytest

from lio_amd import capi
from test_gpu_parity import _TILE_EDGE_CLOUDS, _random_cloud

pytestmark = pytest.mark.gpu

SAMPLE, SINGLE, LIBRARY = capi.VOX_SORT_SAMPLE, capi.VOX_SORT_SINGLE, capi.VOX_SORT_LIBRARY
LIMIT, CAP, MEAN, OVER = capi.VOX_SORT_SINGLE_MAX, capi.VOX_SORT_BUCKET_CAP, capi.VOX_SORT_MEAN_BUCKET, capi.VOX_SORT_OVERSAMPLE
NONE = np.uint32(0xFFFFFFFF)


def _sample_positions(n):
    nb = -(-n // MEAN)
    s = OVER * nb
    j = np.arange(s, dtype=np.int64)
    return nb, ((2 * j + 1) * n) // (2 * s)


def _model_fills(keys):
    """pairs per bucket of the sample sort, by the stated rule"""
    n = len(keys)
    nb, pos = _sample_positions(n)
    splitters = np.sort(keys[pos])[OVER * np.arange(1, nb)]
    return np.bincount(np.searchsorted(splitters, keys, side="right"), minlength=nb)


def _expected_path(keys):
    if len(keys) <= LIMIT:
        return SINGLE
    return SAMPLE if _model_fills(keys).max() <= CAP else LIBRARY


def _check_sort(hip, keys, path):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    assert _expected_path(keys) == path, "the case is not built as its name says"
    order = np.argsort(keys, kind="stable")
    ko, vo, got = hip.vox_sort_pairs(keys)
    assert got == path
    np.testing.assert_array_equal(vo, order.astype(np.uint32))
    np.testing.assert_array_equal(ko, keys[order])
    return ko, vo


def _voxel_like_keys(rng, n):
    return rng.integers(0, max(2, n // 3), n).astype(np.uint32)   # about three points per key: ties test the order inside a voxel


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, LIMIT - 1, LIMIT])
def test_direct_sort(hip, n):
    _check_sort(hip, _voxel_like_keys(np.random.default_rng(n), n), SINGLE)


@pytest.mark.parametrize("n", [LIMIT + 1, 10007, 50001])
def test_sample_sort_sizes(hip, n):
    """the first n with splitters; sizes that are no multiple of the sample size S (10007: S = 216, 50001: S = 1048)"""
    assert n == LIMIT + 1 or n % (OVER * -(-n // MEAN)) != 0
    _check_sort(hip, _voxel_like_keys(np.random.default_rng(n), n), SAMPLE)


def test_all_keys_equal_is_redone_through_the_library(hip):
    _check_sort(hip, np.full(CAP + 904, 7, np.uint32), LIBRARY)


def test_two_distinct_keys(hip):
    """balanced: the splitters are 5 ... 5, 9 ... 9 and the buckets between the two used ones stay empty"""
    rng = np.random.default_rng(2)
    keys = np.where(rng.permutation(6000) < 3000, 5, 9).astype(np.uint32)
    assert np.count_nonzero(_model_fills(keys)) == 2
    _check_sort(hip, keys, SAMPLE)
    # all splitters equal: 54 keys below them in bucket 0, exactly one capacity of the other key in the last bucket
    n = CAP + 54
    nb, pos = _sample_positions(n)
    keys = np.full(n, 9, np.uint32)
    keys[np.setdiff1d(np.arange(n), pos)[:: 70][:54]] = 1
    fills = _model_fills(keys)
    assert fills[0] == 54 and fills[-1] == CAP and fills[1:-1].sum() == 0
    _check_sort(hip, keys, SAMPLE)


@pytest.mark.parametrize("order", ["descending", "sorted"])
def test_ordered_keys(hip, order):
    n = 20011
    keys = np.arange(n, dtype=np.uint32)
    _check_sort(hip, keys[::-1] if order == "descending" else keys, SAMPLE)


@pytest.mark.parametrize("where", ["end", "scattered"])
def test_block_of_no_point_keys(hip, where):
    """3000 "no point" keys among 20000: more than a mean bucket (384), all in the last bucket"""
    rng = np.random.default_rng(3)
    n, holes = 20000, 3000
    keys = rng.integers(0, 1 << 20, n).astype(np.uint32)
    keys[n - holes:] = NONE
    if where == "scattered":
        keys = keys[rng.permutation(n)]
    assert _model_fills(keys)[-1] >= holes
    ko, _ = _check_sort(hip, keys, SAMPLE)
    assert np.all(ko[n - holes:] == NONE)


def _one_full_bucket(extra):
    """Small distinct keys at every sample position, one narrow key range everywhere else: every splitter is small, so all other keys and the
    last OVER samples share the last bucket, which receives n - S + OVER pairs: the capacity + extra."""
    nb = -(-CAP // MEAN)
    while -(-(CAP + extra + OVER * nb - OVER) // MEAN) != nb:   # NB is a function of n, and n of NB: a few steps settle it
        nb = -(-(CAP + extra + OVER * nb - OVER) // MEAN)
    n = CAP + extra + OVER * nb - OVER
    nb_of_n, pos = _sample_positions(n)
    assert nb_of_n == nb and len(np.unique(pos)) == OVER * nb
    rng = np.random.default_rng(5 + extra)
    keys = (1_000_000 + rng.integers(0, 100, n)).astype(np.uint32)
    keys[pos] = np.arange(OVER * nb, dtype=np.uint32)
    assert _model_fills(keys)[-1] == CAP + extra
    return keys


def test_constructed_overflow_and_its_neighbour(hip):
    _check_sort(hip, _one_full_bucket(1), LIBRARY)   # capacity + 1 pairs for one bucket
    _check_sort(hip, _one_full_bucket(0), SAMPLE)    # exactly the capacity: no overflow


def test_sample_sort_is_deterministic(hip):
    """The scatter's order inside a bucket differs from run to run; the result must not."""
    n = 177000
    keys = _voxel_like_keys(np.random.default_rng(177), n)
    ko0, vo0 = _check_sort(hip, keys, SAMPLE)
    for _ in range(19):
        ko, vo, path = hip.vox_sort_pairs(keys)
        assert path == SAMPLE
        np.testing.assert_array_equal(ko, ko0)
        np.testing.assert_array_equal(vo, vo0)


# ------------------------------------------------------------------------------------------------ the filter
def _filter_and_path(hip, pts, leaf):
    before = hip.vox_sort_stats()
    out = hip.voxel_grid(pts, leaf)
    after = hip.vox_sort_stats()
    delta = [a - b for a, b in zip(after, before)]
    assert sorted(delta) == [0, 0, 1], delta   # one run, one path
    return out, delta.index(1)


def _parity_cloud(n):
    rng = np.random.default_rng(n)
    pts = _random_cloud(rng, n)
    if n > 100:
        pts[rng.integers(0, n, 20), 0] = np.nan
    return pts


@pytest.mark.parametrize("n,leaf", [(1, 0.4), (37, 0.4), (5000, 0.4), (120000, 0.4), (30000, 0.2), (177000, 0.4), (260000, 0.4)])
def test_filter_matches_oracle_and_states_its_path(hip, oracle, n, leaf):
    pts = _parity_cloud(n)
    a, path = _filter_and_path(hip, pts, leaf)
    np.testing.assert_array_equal(a, oracle.voxel_grid(pts, leaf))
    assert path == (SINGLE if n <= LIMIT else SAMPLE)


@pytest.mark.parametrize("name", list(_TILE_EDGE_CLOUDS))
def test_filter_at_tile_edges_matches_oracle(hip, oracle, name):
    pts = _TILE_EDGE_CLOUDS[name]
    a, path = _filter_and_path(hip, pts, 0.4)
    np.testing.assert_array_equal(a, oracle.voxel_grid(pts, 0.4))
    assert path == SINGLE


def test_filter_overflow_then_a_normal_cloud(hip, oracle):
    """every point in one voxel, more of them than a bucket holds: redone through the library; the next cloud through the same handle is
    sample-sorted again"""
    rng = np.random.default_rng(11)
    n = CAP + 904
    pts = np.empty((n, 4), np.float32)
    pts[:, :3] = rng.uniform(0.85, 1.15, (n, 3))
    pts[:, 3] = rng.uniform(0, 64, n)
    a, path = _filter_and_path(hip, pts, 0.4)
    assert path == LIBRARY
    b = oracle.voxel_grid(pts, 0.4)
    assert len(b) == 1
    np.testing.assert_array_equal(a, b)
    normal = _random_cloud(rng, 6000)
    a, path = _filter_and_path(hip, normal, 0.4)
    assert path == SAMPLE
    np.testing.assert_array_equal(a, oracle.voxel_grid(normal, 0.4))
