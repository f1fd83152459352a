"""Brute-force references for the product's five-nearest-neighbour walk (csrc/cloud_device.h: knn_scan_group, reached through the
test hook lio_knn_walk of include/lio_test_hooks.h).  numpy only; no library of ours; every map point is looked at for every query.

Layer A — the walk's definition, bit for bit.  Cells are int(floorf(v * inv_cell)) in float32, inv_cell = 1.0f / cell; the grid spans
cells c(min) - 1 .. c(max) + 1 of the map; a query whose cell lies in the grid sees the map points whose cell is within +-1 of its own
on every axis; they are ranked by (bit pattern of the fp32 distance d = dx*dx; d += dy*dy; d += dz*dz, original index).  The library
is built without fp contraction, so numpy's float32 arithmetic is the kernel's.  The comparison with a result is equality: all five
indices, the distances' bit patterns, and the neighbours' coordinates against map[idx].  No tolerance, no query left out.

Layer B — that the definition means "nearest".  fp64 squared distances to ALL map points, no cells.  For every query and rank k whose
fp64 distance is below R2 = (cell / 1.0001)^2 * (1 - EPS_B) the returned index must be the fp64 rank-k index (fp64 ties fall to the
index, as in the walk).  A point that close differs by less than a cell on every axis, so it is inside the 27-cell block; 1.0001 is
the head room the product's own cell sizes keep against the rounding of v * inv_cell.  EPS_B = 8 * 2^-24: three subtractions, three
products and two sums on exact fp32 inputs carry at most 5 * 2^-24 relative error into d, 8 is that with head room.  Two fp64 distances
closer than 2 * EPS_B relative (and not exactly equal) may legitimately swap in fp32, so a query-rank pair whose fp64 distance is that
close to the one at rank k - 1 or k + 1 is left out of layer B — and only of layer B; the share left out is returned and capped by the
caller (1 % on random clouds, nothing at all on lattices, whose fp32 distances are exact).
"""
import concurrent.futures
import os

import numpy as np

K = 5
KEEP = 6                    # the reference keeps one rank more than the walk returns: the rank-5/6 border is where ties matter
EPS_B = 8.0 * 2.0 ** -24
_PAIRS = 1 << 21            # query x map pairs per chunk of the broadcast (a few MB per temporary)


def _for_chunks(fn, m, step):
    """fn(a, b) for the query chunks [a, b) of [0, m): they write disjoint rows, numpy releases the GIL, so a few threads share them"""
    spans = [(a, min(a + step, m)) for a in range(0, m, step)]
    if len(spans) < 4:
        for a, b in spans:
            fn(a, b)
        return
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        for f in [pool.submit(fn, a, b) for a, b in spans]:
            f.result()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)


def cell_coords(xyz, cell):
    """int(floorf(v * inv_cell)) in float32, per axis; non-finite values give 0 (callers mask them)"""
    inv = np.float32(1.0) / np.float32(cell)
    u = np.floor(xyz.astype(np.float32) * inv)
    return np.where(np.isfinite(u), u, np.float32(0)).astype(np.int64)


def grid_of(map_xyzi, cell):
    """(lo, hi): first and last cell of the grid per axis — one cell of margin around the map's bounds; an empty map: bounds 0"""
    m = _f32(map_xyzi)
    assert np.isfinite(m[:, :3]).all(), "the reference is defined for finite maps"
    if m.shape[0] == 0:
        mn = mx = np.zeros(3, np.float32)
    else:
        mn, mx = m[:, :3].min(axis=0), m[:, :3].max(axis=0)
    return cell_coords(mn, cell) - 1, cell_coords(mx, cell) + 1


def _ranked(qi, pj, d, nq, keep, idx, dist):
    """pairs (query qi ascending, point pj, distance d) -> the first `keep` of every query by (d, pj) — for fp32 distances by their bit
    patterns, which order like the non-negative values — written into idx / dist"""
    if d.dtype == np.float32:
        assert nq <= 65536
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | pj.astype(np.uint64)
        order = np.argsort(key)                                                     # by (bits of d, index) ...
        order = order[np.argsort(qi[order].astype(np.uint16), kind="stable")]       # ... then stably by query
    else:
        order = np.lexsort((pj, d, qi))
    qs, ps, ds = qi[order], pj[order], d[order]
    start = np.searchsorted(qs, np.arange(nq))
    rank = np.arange(qs.shape[0]) - start[qs]
    sel = rank < keep
    idx[qs[sel], rank[sel]] = ps[sel]
    dist[qs[sel], rank[sel]] = ds[sel]


def layer_a(map_xyzi, query_xyzi, cell, keep=KEEP, grid_from=None, with_cells=False):
    """-> idx (m, keep) int32 (-1 = missing), sqd (m, keep) float32 (+inf = missing).  grid_from: the map whose bounds make the grid
    (default: map_xyzi itself).  with_cells: also the map points' and the queries' cells and the in-grid mask."""
    mp, q = _f32(map_xyzi), _f32(query_xyzi)
    n, m = mp.shape[0], q.shape[0]
    lo, hi = grid_of(mp if grid_from is None else grid_from, cell)
    pc = np.clip(cell_coords(mp[:, :3], cell), lo, hi).astype(np.int32)
    qc = cell_coords(q[:, :3], cell)
    in_grid = np.isfinite(q[:, :3]).all(axis=1) & (qc >= lo).all(axis=1) & (qc <= hi).all(axis=1)
    qc = np.clip(qc, lo - 2, hi + 2).astype(np.int32)
    idx = np.full((m, keep), -1, np.int32)
    sqd = np.full((m, keep), np.inf, np.float32)
    step = min(max(1, _PAIRS // max(n, 1)), 65536)

    def chunk(a, b):
        near = np.repeat(in_grid[a:b, None], n, axis=1)
        for ax in range(3):
            # |pc - qc| <= 1  <=>  0 <= pc - (qc - 1) <= 2, one unsigned comparison
            near &= (pc[None, :, ax] - (qc[a:b, None, ax] - 1)).view(np.uint32) <= 2
        qi, pj = np.nonzero(near)
        if qi.shape[0] == 0:
            return
        P, Q = mp[pj, :3], q[a + qi, :3]
        dx, dy, dz = P[:, 0] - Q[:, 0], P[:, 1] - Q[:, 1], P[:, 2] - Q[:, 2]
        d = dx * dx
        d += dy * dy
        d += dz * dz
        assert d.dtype == np.float32
        ok = d.view(np.uint32) <= np.uint32(0x7F800000)      # a NaN distance ranks nowhere
        _ranked(qi[ok], pj[ok].astype(np.int32), d[ok], b - a, keep, idx[a:b], sqd[a:b])

    if n:
        _for_chunks(chunk, m, step)
    if with_cells:
        return idx, sqd, pc, qc, in_grid
    return idx, sqd


def radius_sq(cell):
    return (float(np.float32(cell)) / 1.0001) ** 2 * (1.0 - EPS_B)


def layer_b_ranks(map_xyzi, query_xyzi, cell):
    """fp64 brute force, no cells -> idx (m, KEEP) int32, d (m, KEEP) float64 of the nearest points, for the ranks whose distance is
    below a threshold a little beyond radius_sq(cell) (what lies beyond it is -1 / +inf: farther than anything layer B asks about)"""
    mp, q = _f32(map_xyzi), _f32(query_xyzi)
    n, m = mp.shape[0], q.shape[0]
    P, Q = mp[:, :3].astype(np.float64), q[:, :3].astype(np.float64)
    thr = radius_sq(cell) * (1.0 + 8 * EPS_B)
    idx = np.full((m, KEEP), -1, np.int32)
    d64 = np.full((m, KEEP), np.inf, np.float64)
    step = max(1, _PAIRS // max(n, 1))

    def chunk(a, b):
        with np.errstate(invalid="ignore"):
            t = P[None, :, 0] - Q[a:b, None, 0]
            d = t * t
            t = P[None, :, 1] - Q[a:b, None, 1]
            d += t * t
            t = P[None, :, 2] - Q[a:b, None, 2]
            d += t * t
            qi, pj = np.nonzero(d < thr)
        if qi.shape[0]:
            _ranked(qi, pj.astype(np.int32), d[qi, pj], b - a, KEEP, idx[a:b], d64[a:b])

    if n:
        _for_chunks(chunk, m, step)
    return idx, d64


def compare_a(got, ref, map_xyzi):
    """got = (idx (m, 5), sqd (m, 5), nbr_xyz (m, 5, 3)) of the walk; ref = layer_a(...).  Raises AssertionError naming the first
    query that differs."""
    idx, sqd, nbr = got
    ridx, rsqd = ref[0][:, :K], ref[1][:, :K]
    mp = _f32(map_xyzi)
    assert idx.shape == ridx.shape and sqd.shape == rsqd.shape and nbr.shape == ridx.shape + (3,), (idx.shape, sqd.shape, nbr.shape, ridx.shape)
    bad = np.nonzero((idx != ridx).any(axis=1))[0]
    assert bad.size == 0, f"indices differ at {bad.size} of {idx.shape[0]} queries; first: query {bad[0]} got {idx[bad[0]]} ({sqd[bad[0]]}) want {ridx[bad[0]]} ({rsqd[bad[0]]})"
    gb, rb = np.ascontiguousarray(sqd, np.float32).view(np.uint32), np.ascontiguousarray(rsqd).view(np.uint32)
    bad = np.nonzero((gb != rb).any(axis=1))[0]
    assert bad.size == 0, f"distance bits differ at {bad.size} queries; first: query {bad[0]} got {sqd[bad[0]]!r} want {rsqd[bad[0]]!r}"
    pad = np.concatenate([mp[:, :3], np.zeros((1, 3), np.float32)])          # row -1: the zeros of a missing entry
    want = pad[np.where(ridx >= 0, ridx, -1)]
    bad = np.nonzero((np.ascontiguousarray(nbr, np.float32).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"neighbour coordinates are not map[idx] at {bad.size} queries; first: query {bad[0]} got {nbr[bad[0]].tolist()} want {want[bad[0]].tolist()}"


def compare_b(idx, ranks, cell, cap):
    """idx (m, 5) of the walk (or of layer A) against layer_b_ranks(...).  -> (pairs in radius, pairs left out).  Raises AssertionError
    when a checked rank is not the fp64 one, or when more than `cap` (a share) of the in-radius pairs had to be left out."""
    bidx, d = ranks
    r2 = radius_sq(cell)
    inside = d[:, :K] < r2
    with np.errstate(invalid="ignore"):
        gap_next = d[:, 1:KEEP] - d[:, :K]                    # to rank k + 1 (inf - x = inf: nothing there)
        close_next = (gap_next > 0) & (gap_next < 2 * EPS_B * d[:, 1:KEEP])
    close = close_next.copy()
    close[:, 1:] |= close_next[:, :-1]                        # ... and to rank k - 1
    check = inside & ~close
    wrong = check & (np.asarray(idx)[:, :K] != bidx[:, :K])
    bad = np.nonzero(wrong.any(axis=1))[0]
    assert bad.size == 0, (f"not the fp64 nearest at {bad.size} queries; first: query {bad[0]} got {np.asarray(idx)[bad[0]]} "
                           f"fp64 order {bidx[bad[0]]} at {d[bad[0]]}")
    n_in, n_out = int(inside.sum()), int((inside & close).sum())
    assert n_out <= cap * n_in, f"layer B leaves out {n_out} of {n_in} in-radius query-rank pairs, more than the cap {cap}"
    return n_in, n_out


def rank56_ties(ref):
    """queries whose fifth and sixth candidate have the same fp32 distance (the index alone decides which one is returned)"""
    idx, sqd = ref
    return int(((idx[:, K] >= 0) & (sqd[:, K - 1] == sqd[:, K])).sum())


def fifth_outside_own_row(ref_with_cells):
    """queries whose fifth neighbour lies in another (y, z) row of cells than the query — the rows the one-lane walk may skip"""
    idx, _, pc, qc, _ = ref_with_cells
    has = idx[:, K - 1] >= 0
    if pc.shape[0] == 0:
        return 0
    p5 = pc[np.maximum(idx[:, K - 1], 0)]
    return int((has & ((p5[:, 1] != qc[:, 1]) | (p5[:, 2] != qc[:, 2]))).sum())
