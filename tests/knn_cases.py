"""The cases the K-NN walk is pinned on (tests/test_knn_walk.py on the CPU: oracle and references; tests/test_gpu_knn_walk.py: the
product's kernel at 1, 4 and 8 lanes per query).  Every case is seeded; a case is (map xyzi, query xyzi, cell) plus what the checks need
to know about it: `lattice` (fp32 distances exact: layer B leaves out nothing), `lanes` (the lane counts it runs at on the GPU)."""
import functools

import numpy as np

import knn_ref

RAGGED_M = (0, 1, 7, 8, 9, 31, 33, 63, 64, 65, 257)
LARGE_QUERIES = 100_000      # the product picks one lane per query from 100 k queries in a batch; more is more than the brute-force references can afford


class Case:
    def __init__(self, name, map_xyzi, query_xyzi, cell, lattice=False, lanes=(1, 4, 8)):
        self.name, self.cell, self.lattice, self.lanes = name, float(np.float32(cell)), lattice, lanes
        self.map = np.ascontiguousarray(map_xyzi, np.float32).reshape(-1, 4)
        self.query = np.ascontiguousarray(query_xyzi, np.float32).reshape(-1, 4)

    @functools.cached_property
    def ref_a(self):
        return knn_ref.layer_a(self.map, self.query, self.cell, with_cells=True)

    @functools.cached_property
    def ref_b(self):
        return knn_ref.layer_b_ranks(self.map, self.query, self.cell)

    @property
    def cap(self):
        return 0.0 if self.lattice else 0.01


def xyzi(xyz, rng=None):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    out = np.zeros((xyz.shape[0], 4), np.float32)
    out[:, :3] = xyz
    if rng is not None:
        out[:, 3] = rng.uniform(0, 64, xyz.shape[0])
    return out


def random_cloud(rng, n, extent=20.0):
    """the cloud of tests/test_gpu_parity.py: points on a few planes plus clutter"""
    pts = np.zeros((n, 4), dtype=np.float32)
    pts[:, 0] = rng.uniform(-extent, extent, n)
    pts[:, 1] = rng.uniform(-extent, extent, n)
    pts[:, 2] = np.where(rng.random(n) < 0.7, rng.normal(0, 0.02, n), rng.uniform(0, 5, n))
    pts[:, 3] = rng.uniform(0, 64, n)
    return pts


def _random(cell):
    rng = np.random.default_rng(5)
    return Case(f"random_cell{cell}", random_cloud(rng, 40000), random_cloud(rng, 3000), cell)


def _ties(cell):
    """a lattice at multiples of 0.25, every point twice at different original indices; queries at multiples of 0.125"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(-12, 13), np.arange(-12, 13), np.arange(-4, 5), indexing="ij"), axis=-1).reshape(-1, 3) * 0.25
    pts = np.concatenate([g, g])
    pts = pts[rng.permutation(pts.shape[0])]          # a duplicate sits at an unrelated index, and index order is not cell order
    q = np.stack([rng.integers(-28, 29, 4000), rng.integers(-28, 29, 4000), rng.integers(-12, 13, 4000)], axis=1) * 0.125
    return Case(f"ties_cell{cell}", xyzi(pts, rng), xyzi(q), cell, lattice=True)


def _dense():
    """5000 points in one cell, 200..600 in each of its 26 neighbours: every run non-empty, the flat list far beyond LPQ * KNN_BATCH"""
    rng = np.random.default_rng(12)
    parts = []
    for cz in range(4, 7):
        for cy in range(4, 7):
            for cx in range(4, 7):
                n = 5000 if (cx, cy, cz) == (5, 5, 5) else int(rng.integers(200, 601))
                parts.append(np.array([cx, cy, cz]) + rng.uniform(0.001, 0.999, (n, 3)))
    parts.append(np.array([[0.5, 0.5, 0.5], [10.5, 10.5, 10.5]]))
    pts = np.concatenate(parts)
    pts = pts[rng.permutation(pts.shape[0])]
    q = np.concatenate([5 + rng.uniform(0, 1, (1200, 3)), 4 + rng.uniform(0, 3, (800, 3))])
    return Case("dense_cells", xyzi(pts, rng), xyzi(q), 1.0)


def _single_run():
    """the reverse: one non-empty run out of nine — the row (y, z) = (6, 4) — seen from the cell (5, 5, 5) and from inside the row"""
    rng = np.random.default_rng(13)
    pts = np.concatenate([np.array([4, 6, 4]) + rng.uniform(0.001, 0.999, (900, 3)) * np.array([3, 1, 1]),
                          np.array([[0.5, 0.5, 0.5], [10.5, 10.5, 10.5]])])
    q = np.concatenate([5 + rng.uniform(0, 1, (1500, 3)), np.array([4, 6, 4]) + rng.uniform(0, 1, (1500, 3)) * np.array([3, 1, 1])])
    return Case("single_run", xyzi(pts, rng), xyzi(q), 1.0)


def _row_skip():
    """the one-lane walk's row bound: (a) queries within 2e-3 cell of a face in y and / or z, on either side, at negative and positive
    coordinates, with their true neighbours just across that face (face and corner rows whose bound is near zero); (b) queries whose
    own row holds five close points, so that every other row is skippable"""
    rng = np.random.default_rng(14)
    cell = float(np.float32(1.0001))
    n_a, n_b = 2400, 1200
    base = rng.integers(-8, 8, (n_a, 3)).astype(np.float64)
    frac = rng.uniform(0.2, 0.8, (n_a, 3))
    kind = rng.integers(0, 3, n_a)                     # 0: y face, 1: z face, 2: both (corner row)
    side = rng.integers(0, 2, (n_a, 3))                # 0: just above the cell's lower face, 1: just below its upper face
    delta = rng.uniform(1e-5, 2e-3, (n_a, 3))
    near = np.zeros((n_a, 3), bool)
    near[:, 1] = kind != 1
    near[:, 2] = kind != 0
    frac = np.where(near, np.where(side == 1, 1.0 - delta, delta), frac)
    qa = (base + frac) * cell
    # six map points per query just across the face(s), up to 0.03 cell beyond, and close to the query in the free axes
    face = base + side
    eps = rng.uniform(1e-4, 0.03, (6, n_a, 3))
    pa = np.where(near, (face + np.where(side == 1, eps, -eps)) * cell, qa + rng.normal(0, 0.03, (6, n_a, 3)))
    qb = (rng.integers(-8, 8, (n_b, 3)) + rng.uniform(0.3, 0.7, (n_b, 3))) * cell
    pb = qb + rng.normal(0, 0.01, (6, n_b, 3))
    bg = rng.uniform(-8, 8, (20000, 3)) * cell
    pts = np.concatenate([pa.reshape(-1, 3), pb.reshape(-1, 3), bg])
    pts = pts[rng.permutation(pts.shape[0])]
    c = Case("row_skip", xyzi(pts, rng), xyzi(np.concatenate([qa, qb])), cell)
    c.n_face = n_a
    return c


def _flat():
    """all z equal: dims[2] == 3; queries in the slab, in the margin cells above / below and beyond them"""
    rng = np.random.default_rng(15)
    pts = np.concatenate([rng.uniform(-10, 10, (8000, 2)), np.full((8000, 1), 0.25)], axis=1)
    q = np.concatenate([rng.uniform(-10, 10, (2000, 2)), rng.uniform(-2.5, 2.5, (2000, 1))], axis=1)
    return Case("flat_map", xyzi(pts, rng), xyzi(q), 1.0001)


def _margin():
    """queries in the one-cell margin around the map's bounds (cell 0 and dims - 1 of the grid), and more than a cell outside"""
    rng = np.random.default_rng(16)
    pts = rng.uniform(0, 10, (12000, 3))
    q = rng.uniform(-2.6, 12.6, (3000, 3))
    keep_in = rng.random((3000, 3)) < 0.5              # most queries leave the map on one or two axes only
    q = np.where(keep_in, rng.uniform(0, 10, (3000, 3)), q)
    return Case("grid_margin", xyzi(pts, rng), xyzi(q), 1.0001)


def _corners():
    """queries exactly on cell corners (cell 0.5: v * inv_cell is exact), map points partly on cell faces"""
    rng = np.random.default_rng(17)
    pts = rng.uniform(-6, 6, (30000, 3))
    pts[:6000] = np.round(pts[:6000] * 8) / 8          # multiples of 0.125, every fourth value on a face
    q = rng.integers(-13, 14, (2500, 3)) * 0.5
    return Case("cell_corners", xyzi(pts, rng), xyzi(q), 0.5)


def _far():
    """coordinates around +-400 m at cell 1.0001 (fp32 spacing 3e-5 there)"""
    rng = np.random.default_rng(18)
    a, b = random_cloud(rng, 12000, 8.0), random_cloud(rng, 12000, 8.0)
    a[:, :3] += np.array([400, 397, -3], np.float32)
    b[:, :3] += np.array([-400, -403, 2], np.float32)
    qa, qb = random_cloud(rng, 1500, 8.0), random_cloud(rng, 1500, 8.0)
    qa[:, :3] += np.array([400, 397, -3], np.float32)
    qb[:, :3] += np.array([-400, -403, 2], np.float32)
    return Case("far_400m", np.concatenate([a, b]), np.concatenate([qa, qb]), 1.0001)


def _small(n_map):
    rng = np.random.default_rng(20 + n_map)
    pts = rng.uniform(-0.4, 0.4, (n_map, 3))
    q = rng.uniform(-1.2, 1.2, (300, 3))
    return Case(f"small_map_{n_map}", xyzi(pts, rng), xyzi(q), 1.0001)


def _ragged(m):
    rng = np.random.default_rng(5)
    mp, q = random_cloud(rng, 40000), random_cloud(rng, 3000)
    return Case(f"ragged_m{m}", mp, q[:m], 1.0001)


def _non_finite():
    """NaN / +inf / -inf in one coordinate of some queries: they find nothing and their wave's other queries are not disturbed"""
    rng = np.random.default_rng(19)
    mp, q = random_cloud(rng, 20000), random_cloud(rng, 1024)
    rows = rng.permutation(1024)[:90]
    for k, r in enumerate(rows):
        q[r, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    c = Case("non_finite_queries", mp, q, 1.0001)
    c.bad_rows = np.sort(rows)
    return c


def _large():
    """the regime in which the product itself picks one lane per query"""
    rng = np.random.default_rng(21)
    return Case("large", random_cloud(rng, 80000, 30.0), random_cloud(rng, LARGE_QUERIES, 30.0), 1.0001, lanes=(1, 8))


_MAKERS = {}
for _c in (1.0001, 0.3):
    _MAKERS[f"random_cell{_c}"] = functools.partial(_random, _c)
for _c in (0.5, 1.0001):
    _MAKERS[f"ties_cell{_c}"] = functools.partial(_ties, _c)
_MAKERS.update(dense_cells=_dense, single_run=_single_run, row_skip=_row_skip, flat_map=_flat, grid_margin=_margin, cell_corners=_corners,
               far_400m=_far, non_finite_queries=_non_finite)
for _n in (0, 1, 4, 5):
    _MAKERS[f"small_map_{_n}"] = functools.partial(_small, _n)
for _m in RAGGED_M:
    _MAKERS[f"ragged_m{_m}"] = functools.partial(_ragged, _m)
_MAKERS["large"] = _large
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def get(name):
    c = _MAKERS[name]()
    assert c.name == name, (c.name, name)
    return c
