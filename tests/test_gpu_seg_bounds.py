"""The bounds pass the sensor chains share (include/lio_seg_bounds.h; cloud_kernels.h: k_seg_bounds, k_seg_bounds_fold): every cloud of a call
reduced by its own max(1, min(ceil(n / 256), 512)) blocks, then folded by one block.

The reference is a numpy float32 statement of vox_fold_bounds (cloud_device.h), compared field by field with exact equality: minimum and
maximum do not depend on the order, the count is an integer, and minb / divb / overflow are single float32 operations on those.  A cloud
without a finite point has n_valid == 0 and nothing else defined.  The first two tests need no GPU: the header's binding, and that the
reference alone says of the built clouds what they were built for.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from lio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV_LEAF = 2.5
INT_MAX = np.int64(2**31 - 1)
BIG = 300001        # many strided passes: 512 blocks x 256 threads take 131072 points per pass
PASS = 131072


def _reference(cloud, inv_leaf):
    """vox_fold_bounds, word for word, in float32"""
    xyz = np.asarray(cloud, np.float32).reshape(-1, 4)[:, :3]
    fin = np.isfinite(xyz).all(axis=1)
    n_valid = int(fin.sum())
    if n_valid == 0:
        return dict(n_valid=0)
    il = np.float32(inv_leaf)
    mn, mx = xyz[fin].min(axis=0), xyz[fin].max(axis=0)
    assert mn.dtype == np.float32 and ((mx - mn) * il).dtype == np.float32
    dd = ((mx - mn) * il).astype(np.float32).astype(np.int64) + 1            # dd = int64(float32((mx - mn) * inv_leaf)) + 1
    minb = np.floor(mn * il).astype(np.int32)
    maxb = np.floor(mx * il).astype(np.int32)
    overflow = int(n_valid > 0 and dd[0] * dd[1] * dd[2] > INT_MAX)
    return dict(mn=mn, mx=mx, minb=minb, divb=maxb - minb + 1, overflow=overflow, n_valid=n_valid)


def _cube(rng, n, half):
    c = rng.uniform(-half, half, (n, 4)).astype(np.float32)
    if n >= 2:   # the span is exactly [-half, half] on every axis
        c[0, :3], c[n - 1, :3] = -half, half
    return c


@functools.lru_cache(maxsize=None)
def _segments():
    rng = np.random.default_rng(20)
    segs = []
    for n in (0, 1, 255, 256, 257, PASS, PASS + 1):
        segs.append((f"n{n}", rng.uniform(-50, 50, (n, 4)).astype(np.float32)))
    big = rng.uniform(-100, 100, (BIG, 4)).astype(np.float32)
    big[0, :3] = (-120.0, 119.5, 3.25)                # min x, max y at index 0
    big[BIG - 1, :3] = (118.75, -7.5, -120.0)         # max x, min z at index n - 1
    big[PASS, :3] = (1.5, -119.25, 120.0)             # min y, max z at the first point that only the second strided pass reaches
    segs.append(("planted", big))
    segs.append(("all_nan", np.full((300, 4), np.nan, np.float32)))
    dirty = rng.uniform(-50, 50, (5000, 4)).astype(np.float32)
    bad = rng.choice(5000, 600, replace=False)
    dirty[bad[:200], rng.integers(0, 3, 200)] = np.nan
    dirty[bad[200:400], rng.integers(0, 3, 200)] = np.inf
    dirty[bad[400:], rng.integers(0, 3, 200)] = -np.inf
    dirty[bad[:50], 3] = np.nan                       # (the intensity does not count)
    segs.append(("sprinkled", dirty))
    segs.append(("wide", _cube(rng, 1000, 1500.0)))   # 3000 m per axis: 7501 cells each, the product needs 64 bits
    # the two sides of the guard: 1290^3 = 2146689000 <= INT32_MAX < 1291^3 = 2151685171
    segs.append(("under_guard", _cube(rng, 700, 257.9)))   # 515.8 * 2.5 = 1289.5 -> 1290 per axis
    segs.append(("over_guard", _cube(rng, 700, 258.1)))    # 516.2 * 2.5 = 1290.5 -> 1291 per axis
    return tuple(segs)


@functools.lru_cache(maxsize=None)
def _expected():
    return tuple(_reference(c, INV_LEAF) for _, c in _segments())


def _assert_same(got, want, name):
    print(f"{name:12s} got {got}  want {want}")
    assert got["n_valid"] == want["n_valid"], name
    if want["n_valid"] == 0:
        return
    for key in ("mn", "mx", "minb", "divb"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name} {key}")
    assert got["overflow"] == want["overflow"], name


def test_seg_bounds_header_is_bound_and_exported_by_the_product_only(oracle):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lio_seg_bounds.h")).read(), flags=re.S)
    mine = sorted(set(re.findall(r"\b(lio_[a-z0-9_]+)\s*\(", text)))
    assert mine == ["lio_seg_bounds"] and set(mine) == set(capi._SEG_BOUNDS_SIGS.keys())
    assert not set(mine) & (set(capi._SIGS) | set(capi._TEST_SIGS) | set(capi._EXT_SIGS) | set(capi._VOX_SORT_SIGS))
    assert hasattr(ctypes.CDLL(capi.HIP_LIB_PATH), "lio_seg_bounds") and not hasattr(oracle.dll, "lio_seg_bounds")
    assert ctypes.sizeof(capi.SegBoundsOut) == 14 * 4


def test_the_reference_alone_says_what_the_clouds_were_built_for():
    exp = dict(zip((n for n, _ in _segments()), _expected()))
    assert [exp[f"n{n}"]["n_valid"] for n in (0, 1, 255, 256, 257, PASS, PASS + 1)] == [0, 1, 255, 256, 257, PASS, PASS + 1]
    assert exp["all_nan"] == dict(n_valid=0)
    p = exp["planted"]
    assert p["mn"].tolist() == [-120.0, -119.25, -120.0] and p["mx"].tolist() == [118.75, 119.5, 120.0] and p["n_valid"] == BIG
    assert p["minb"].tolist() == [-300, -299, -300] and p["divb"].tolist() == [597, 598, 601] and p["overflow"] == 0
    assert exp["sprinkled"]["n_valid"] == 5000 - 600 and np.isfinite(exp["sprinkled"]["mn"]).all() and np.abs(exp["sprinkled"]["mx"]).max() <= 50
    w = exp["wide"]
    assert w["mn"].tolist() == [-1500.0] * 3 and w["mx"].tolist() == [1500.0] * 3
    assert w["minb"].tolist() == [-3750] * 3 and w["divb"].tolist() == [7501] * 3 and w["overflow"] == 1
    assert 7501**3 > 2**32                                                    # more than 32 bits: the product is taken in 64
    assert exp["under_guard"]["divb"].tolist() == [1290] * 3 and exp["under_guard"]["overflow"] == 0
    assert exp["over_guard"]["divb"].tolist() == [1292] * 3 and exp["over_guard"]["overflow"] == 1


@pytest.mark.gpu
def test_one_call_over_all_segments_equals_the_reference(hip):
    got = hip.seg_bounds([c for _, c in _segments()], INV_LEAF)
    for (name, _), g, want in zip(_segments(), got, _expected()):
        _assert_same(g, want, name)


@pytest.mark.gpu
def test_the_segments_in_reverse_order_give_the_same_rows(hip):
    got = hip.seg_bounds([c for _, c in _segments()][::-1], INV_LEAF)[::-1]
    for (name, _), g, want in zip(_segments(), got, _expected()):
        _assert_same(g, want, name)


@pytest.mark.gpu
def test_each_segment_alone_gives_the_row_it_had_in_the_full_call(hip):
    full = hip.seg_bounds([c for _, c in _segments()], INV_LEAF)
    for (name, c), f, want in zip(_segments(), full, _expected()):
        alone = hip.seg_bounds([c], INV_LEAF)[0]
        _assert_same(alone, want, name)
        _assert_same(alone, f if f["n_valid"] else dict(n_valid=0), name)
