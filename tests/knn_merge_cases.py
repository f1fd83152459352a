"""Maps that steer the candidates of the multi-lane K-NN walk (csrc/cloud_device.h: knn_scan_group<5, LPQ>, LPQ = 4 or 8) onto chosen
sub-lanes and trips, for the merge of the sub-lanes' lists (csrc/knn_merge.h).  numpy only.

What the walk fixes and what it does not.  A query's candidates are the points of the 27 cells around its own, read as ONE flat list: the
cells in the order (z, y, x) ascending, the order of the points inside a cell left to the atomics of the grid build.  Sub-lane s of a query
takes the flat positions s, s + LPQ, ...; a trip of the loop covers 4 LPQ positions.  So a point's position — and with it its sub-lane
(position mod LPQ) and its trip (position div 4 LPQ) — is fixed exactly when it is the ONLY point of its cell; cells in front of it may hold
any number.  `flat_positions` states this model on the cells of knn_ref.layer_a; tests/test_knn_merge.py holds every case below to what its
name says, without a GPU, so the GPU test (tests/test_gpu_knn_merge.py) compares results only.

A case is NQ = 72 queries (more than one 256-thread block at 4 and at 8 lanes per query), each at the centre of a cell with a block of 27
cells of its own (blocks lie four cells apart), cell = 1.  "Winners" sit on the near side of their cell (squared distance below 0.9),
everything else on the far side of a cell beside the query's (above 1.3); the query's own cell holds a winner or nothing.  The map's rows
are shuffled: original indices, which decide exact ties, run against nothing."""
import functools

import numpy as np

import knn_ref

CELL = 1.0
NQ = 72
LANES = (4, 8)
# the 27 cells of a block in the walk's flat order: index c = 9 (oz + 1) + 3 (oy + 1) + (ox + 1)
OFFS = np.array([(ox, oy, oz) for oz in (-1, 0, 1) for oy in (-1, 0, 1) for ox in (-1, 0, 1)], np.int64)
CENTRE = 13
NAMES = ("five_on_one_sublane", "four_on_one_sublane_of_eight", "one_winner_per_sublane", "winners_in_last_trip", "lattice_ties",
         "sparse_blocks", "trip_boundaries")


class Case:
    def __init__(self, name, map_, query, winners):
        self.name, self.map, self.query, self.cell = name, map_, query, np.float32(CELL)
        self.winners = winners      # per query: the map rows (after the shuffle) that must be the five nearest, or None
        self.ref = knn_ref.layer_a(map_, query, self.cell, with_cells=True)


def _origin(i):
    return np.array([4 * (i % 9) + 2, 4 * (i // 9) + 2, 2], np.float64)


def _near(off, eps):
    """a point of cell `off` on the side of the query (which sits at the block's (0.5, 0.5, 0.5)): 0.5 + eps away on the axes where off != 0"""
    return 0.5 + off * (0.5 + eps) + (off == 0) * eps * 0.5


def _far(off, eps):
    return 0.5 + off * (1.45 - eps) + (off == 0) * (0.4 * eps)


def _assemble(name, blocks, seed):
    """blocks: per query a list of (cell index, xyz relative to the block's corner, is_winner)"""
    rng = np.random.default_rng(seed)
    pts, owner, win = [], [], []
    for i, blk in enumerate(blocks):
        for c, xyz, w in blk:
            pts.append(_origin(i) + xyz)
            owner.append(i)
            win.append(w)
    n = len(pts)
    perm = rng.permutation(n)
    m = np.zeros((n, 4), np.float32)
    if n:
        m[:, :3] = np.asarray(pts, np.float64)[perm]
        m[:, 3] = rng.uniform(0, 1, n)     # intensity: not read by the walk
    owner, win = np.asarray(owner, np.int64)[perm], np.asarray(win, bool)[perm]
    q = np.zeros((len(blocks), 4), np.float32)
    q[:, :3] = np.array([_origin(i) + 0.5 for i in range(len(blocks))])
    winners = [np.nonzero((owner == i) & win)[0] for i in range(len(blocks))]
    return Case(name, m, q, winners)


def _block(counts, winner_cells, rng):
    blk = []
    for c in range(27):
        for k in range(int(counts[c])):
            w = c in winner_cells
            assert not (w and counts[c] != 1) and not (c == CENTRE and not w)
            eps = rng.uniform(0.01, 0.04) if w else rng.uniform(0.0, 0.3)
            blk.append((c, (_near if w else _far)(OFFS[c].astype(np.float64), eps), w))
    return blk


def _positions(counts):
    """flat position of the first point of every cell"""
    return np.concatenate([[0], np.cumsum(counts)[:-1]])


def _steered(name, seed, counts_of, pick):
    """counts_of(i, rng) -> 27 counts; pick(i, rng, pos, single) -> winner cells, chosen by their flat positions"""
    rng = np.random.default_rng(seed)
    blocks = []
    for i in range(NQ):
        counts = np.asarray(counts_of(i, rng), np.int64)
        assert counts[CENTRE] == 0
        pos = _positions(counts)
        cells = [int(c) for c in pick(i, rng, pos, counts == 1)]
        assert len(set(cells)) == 5 and all(counts[c] == 1 for c in cells)
        blocks.append(_block(counts, set(cells), rng))
    return _assemble(name, blocks, seed + 1)


_ONE_EACH = np.array([0 if c == CENTRE else 1 for c in range(27)])


def _five_on_one_sublane():
    # seven points in cell 9 and two in cell 14 put single cells at the positions 0, 8, 16, 24 and 32: sub-lane 0 at eight lanes and at four
    counts = _ONE_EACH.copy()
    counts[9], counts[14] = 7, 2

    def pick(i, rng, pos, single):
        cells = [c for c in range(27) if single[c] and pos[c] % 8 == 0]
        assert len(cells) == 5, (cells, pos)
        return cells
    return _steered("five_on_one_sublane", 11, lambda i, rng: counts, pick)


def _four_on_one_sublane_of_eight():
    # one point per cell: sub-lane s of eight sees the positions s, s + 8, s + 16, s + 24 (s <= 1); the fifth winner is on another one
    def pick(i, rng, pos, single):
        s = i % 2
        cells = [c for c in range(27) if single[c] and pos[c] % 8 == s]
        assert len(cells) == 4
        other = [c for c in range(27) if single[c] and pos[c] % 8 != s]
        return cells + [int(rng.choice(other))]
    return _steered("four_on_one_sublane_of_eight", 12, lambda i, rng: _ONE_EACH, pick)


def _one_winner_per_sublane():
    def pick(i, rng, pos, single):
        avail = [c for c in range(27) if single[c]]
        while True:
            cells = rng.choice(avail, 5, replace=False)
            if len(set(pos[cells] % 8)) == 5 and len(set(pos[cells] % 4)) == 4:
                return cells
    return _steered("one_winner_per_sublane", 13, lambda i, rng: _ONE_EACH, pick)


def _winners_in_last_trip():
    # 33 far points in the block's first cell: 58 candidates, the single cells at 33 .. 57; the last trip starts at 32 (eight lanes) / 48 (four)
    counts = _ONE_EACH.copy()
    counts[0] = 33

    def pick(i, rng, pos, single):
        avail = [c for c in range(27) if single[c] and pos[c] >= 48]
        return rng.choice(avail, 5, replace=False)
    return _steered("winners_in_last_trip", 14, lambda i, rng: counts, pick)


def _lattice_ties():
    """points at +-0.75 from the query along one axis (six, squared distance 0.5625 exactly), along two (twelve, 1.125) and along three
    (eight, 1.6875): one point per cell, exact fp32 distances, the original index decides inside a shell.  Query i keeps 6, 3 or 0 of the
    face points, so the fifth neighbour is decided inside the first, the second or (no face, five of twelve kept edges) the second shell."""
    rng = np.random.default_rng(15)
    blocks = []
    for i in range(NQ):
        keep_faces = (6, 3, 0)[i % 3]
        faces = [c for c in range(27) if np.abs(OFFS[c]).sum() == 1]
        faces = set(rng.choice(faces, keep_faces, replace=False).tolist()) if keep_faces else set()
        blk = []
        for c in range(27):
            nz = int(np.abs(OFFS[c]).sum())
            if nz == 0 or (nz == 1 and c not in faces):
                continue
            blk.append((c, 0.5 + 0.75 * OFFS[c].astype(np.float64), False))
        blocks.append(blk)
    case = _assemble("lattice_ties", blocks, 16)
    case.winners = [None] * NQ
    return case


def _random_blocks(name, seed, totals):
    """blocks of totals[i] points at random places of random cells, one per cell up to 26, the rest in the block's first cell"""
    rng = np.random.default_rng(seed)
    blocks = []
    for i in range(NQ):
        t = totals[i % len(totals)]
        cells = rng.choice([c for c in range(27) if c != CENTRE], min(t, 26), replace=False).tolist() + [0] * max(t - 26, 0)
        blocks.append([(c, OFFS[c] + rng.uniform(0.05, 0.95, 3), False) for c in cells])
    case = _assemble(name, blocks, seed + 1)
    case.winners = [None] * NQ
    case.totals = [totals[i % len(totals)] for i in range(NQ)]
    return case


_BUILDERS = {
    "five_on_one_sublane": _five_on_one_sublane,
    "four_on_one_sublane_of_eight": _four_on_one_sublane_of_eight,
    "one_winner_per_sublane": _one_winner_per_sublane,
    "winners_in_last_trip": _winners_in_last_trip,
    "lattice_ties": _lattice_ties,
    # 0, 1, 4, 5, 6 points and full blocks side by side: a wave of 64 lanes holds 8 or 16 consecutive queries, so every wave has queries
    # without a candidate beside full ones, and lists with 5, 4, 1 and 0 missing entries
    "sparse_blocks": lambda: _random_blocks("sparse_blocks", 17, (0, 26, 1, 4, 26, 5, 6, 0)),
    # a trip is 16 positions at four lanes and 32 at eight
    "trip_boundaries": lambda: _random_blocks("trip_boundaries", 19, (15, 16, 17, 31, 32, 33)),
}


@functools.lru_cache(maxsize=None)
def get(name):
    return _BUILDERS[name]()


def flat_positions(case, i):
    """query i's candidates by the model above -> (rows of case.map, flat position of the first point of the row's cell, cell holds one point)"""
    _, _, pc, qc, in_grid = case.ref
    assert in_grid[i]
    rows = np.nonzero((np.abs(pc.astype(np.int64) - qc[i].astype(np.int64)) <= 1).all(axis=1))[0]
    key = (pc[rows, 2].astype(np.int64) << 40) | (pc[rows, 1].astype(np.int64) << 20) | pc[rows, 0].astype(np.int64)
    order = np.argsort(key, kind="stable")
    rows, key = rows[order], key[order]
    first = np.searchsorted(key, key, side="left")
    count = np.searchsorted(key, key, side="right") - first
    return rows, first, count == 1
