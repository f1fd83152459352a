"""The cases the scan-to-scan correspondence search is pinned on (tests/test_odom_corr.py on the CPU: oracle and references;
tests/test_gpu_odom_corr.py: the product's k_ob_corr through lio_odom_correspondences).  Every case is seeded and small: at most about
45 k previous points and 2 k queries.  A case is the four clouds of one hook call, transform_es, and what the checks need to know about
it: `lattice` (every fp32 distance exact: layer B leaves out nothing).  What each case must contain is asserted in
tests/test_odom_corr.py::test_case_contains_what_it_claims.

Most synthetic cases are made of BLOCKS: neighbourhoods 16 m apart (farther than the 5 m gate reaches), each with one designated closest
point 0.04 m from its query, written into the previous cloud one after the other in index order.  Identity transform and no_deskew make
sel the query itself, so the geometry below is the geometry the search sees."""
import functools
import hashlib

import numpy as np

import odom_corr_ref as ref

CHUNK_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
VIOLATION_OFFSETS = tuple(64 * q + l for q in range(4) for l in (0, 1, 63)) + (256, 512)
CELL = np.float32(5.0) * np.float32(1.0001)       # the grids of csrc/odometry.hip
GRID_CELLS_MAX = 131072                           # LIO_ODOM_BATCH_GRID_CELLS_MAX (include/lio_frontend_batch.h)


class Case:
    def __init__(self, name, sharp, flat, last_corner, last_surf, q=(0, 0, 0, 1), p=(0, 0, 0), scan_period=0.1, no_deskew=False, lattice=False,
                 **info):
        f = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1, 4)
        self.name, self.sharp, self.flat, self.last_corner, self.last_surf = name, f(sharp), f(flat), f(last_corner), f(last_surf)
        self.q, self.p = np.asarray(q, np.float32), np.asarray(p, np.float32)
        self.scan_period, self.no_deskew, self.lattice = scan_period, no_deskew, lattice
        self.__dict__.update(info)
        self._refs = {}

    @property
    def cap(self):
        return 0.0 if self.lattice else 0.01

    @property
    def queries(self):
        return np.concatenate([self.sharp, self.flat])

    def run(self, lib, sharp=None, flat=None):
        from lio_amd import capi
        T = capi.TransformF.make(self.q, self.p)
        return lib.odom_correspondences(self.sharp if sharp is None else sharp, self.flat if flat is None else flat, self.last_corner,
                                        self.last_surf, T, self.scan_period, self.no_deskew)

    def refs(self, sel):
        """(layer A, layer B, stats) for this sel, computed once per distinct sel"""
        key = hashlib.sha1(np.ascontiguousarray(sel, np.float32).tobytes()).hexdigest()
        if key not in self._refs:
            stats = {}
            a = ref.layer_a(self, sel, stats=stats)
            self._refs[key] = (a, ref.layer_b(self, sel), stats)
        return self._refs[key]

    def start_ratio(self, sel):
        return ref.start_ratio(sel, self.queries, self.q, self.p, self.scan_period, self.no_deskew)


# ---------------------------------------------------------------- blocks
Q_OFF = np.array([0.03125, 0.015625, 0.015625])     # the query's offset from its block's closest point (dyadic)


class Blocks:
    def __init__(self, per_row=24, pitch=16.0):
        self.per_row, self.pitch, self.k = per_row, pitch, 0
        self.pts, self.queries, self.closest = [], [], []
        self.n = 0

    def add(self, offsets, rings, i_closest, q_at=None, found=True):
        """one block: points at centre + offsets (index order), rings (may be fractional), the designated closest among them; the
        block's query sits at that point + Q_OFF (or at centre + q_at); found = False: the gate must reject the closest"""
        c = np.array([(self.k % self.per_row - self.per_row // 2) * self.pitch, (self.k // self.per_row - 8) * self.pitch, 0.0])
        self.k += 1
        off = np.asarray(offsets, np.float64).reshape(-1, 3)
        blk = np.zeros((off.shape[0], 4), np.float32)
        blk[:, :3] = c + off
        blk[:, 3] = rings
        self.pts.append(blk)
        self.queries.append(np.concatenate([c + (off[i_closest] + Q_OFF if q_at is None else q_at), [0.0]]))
        self.closest.append(self.n + i_closest if found else -1)
        self.n += off.shape[0]

    def cloud(self):
        return np.concatenate(self.pts) if self.pts else np.zeros((0, 4), np.float32)

    def query_cloud(self):
        return np.asarray(self.queries, np.float32).reshape(-1, 4)


def _dirs(rng, n, radius):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * np.broadcast_to(np.asarray(radius, np.float64), (n,))[:, None]


def _window(rng, k, r, sign, variant):
    """k in-window points in walk order: rings r, r +- 1, r +- 2 in that order, 0.5 .. 3 m away; variant 'far' / 'near' puts the
    nearest one (0.2 m) at the last / first place of the walk"""
    rings = r + sign * (3 * np.arange(k) // max(k, 1))
    rad = rng.uniform(0.5, 3.0, k)
    if k and variant == "far":
        rad[-1] = 0.2
    if k and variant == "near":
        rad[0] = 0.2
    return _dirs(rng, k, rad), rings


def _chunk_layout(rng, first, last):
    """blocks for every pairing of CHUNK_COUNTS; `first` = (kd, ku) of a block with NO violator in front of it (the walk runs to index
    0), `last` likewise at the end of the cloud"""
    K = CHUNK_COUNTS
    pairs = [(K[i], K[(i + 4) % len(K)]) for i in range(len(K))] + [(k, k) for k in K]
    specs = [(first[0], first[1], "rand", False, True)] + [(kd, ku, v, True, True) for kd, ku in pairs for v in ("rand", "far", "near")]
    specs.append((last[0], last[1], "rand", True, False))
    b, r = Blocks(), 10
    for kd, ku, variant, lead, trail in specs:
        dn, rdn = _window(rng, kd, r, -1, variant)
        up, rup = _window(rng, ku, r, +1, variant)
        off = ([_dirs(rng, 1, 0.1)] if lead else []) + [dn[::-1], np.zeros((1, 3)), up] + ([_dirs(rng, 1, 0.1)] if trail else [])
        rings = ([[r - 3]] if lead else []) + [rdn[::-1], [r], rup] + ([[r + 3]] if trail else [])
        b.add(np.concatenate(off), np.concatenate(rings), (1 if lead else 0) + kd)
    return b


def _chunk_edges(swapped):
    rng = np.random.default_rng(21)
    ends = _chunk_layout(rng, (0, 65), (65, 0))           # closest at index 0 and at n - 1
    runs = _chunk_layout(rng, (257, 64), (64, 257))       # windows that run to both ends of the array without a violation
    c, s = (runs, ends) if swapped else (ends, runs)
    return Case("chunk_edges_swapped" if swapped else "chunk_edges", c.query_cloud(), s.query_cloud(), c.cloud(), s.cloud(), no_deskew=True,
                want_closest=(c.closest, s.closest))


def _violation_then_valid():
    rng = np.random.default_rng(22)
    b, r = Blocks(), 20
    for o in VIOLATION_OFFSETS:
        parts, rings = [], []
        for sign in (-1, +1):
            seen = _dirs(rng, o, rng.uniform(0.5, 3.0, o))
            rseen = r + sign * rng.integers(0, 3, o)                 # not monotone
            viol = _dirs(rng, 1, 0.1)
            behind = _dirs(rng, 30, rng.uniform(0.15, 0.3, 30))      # in-window rings with the smallest distances, never to be seen
            rbehind = r + sign * rng.integers(0, 3, 30)
            end = _dirs(rng, 1, 0.1)
            walk = np.concatenate([seen, viol, behind, end])
            rw = np.concatenate([rseen, [r + sign * int(rng.integers(3, 6))], rbehind, [r + sign * 6]])
            parts.append(walk[::-1] if sign < 0 else walk)
            rings.append(rw[::-1] if sign < 0 else rw)
        b.add(np.concatenate([parts[0], np.zeros((1, 3)), parts[1]]), np.concatenate([rings[0], [r], rings[1]]), o + 32)
    return Case("violation_then_valid", b.query_cloud(), b.query_cloud(), b.cloud(), b.cloud(), no_deskew=True, want_closest=(b.closest, b.closest))


def _ties():
    """multiples of 0.25 (points) and 0.125 (queries): every distance exact.  Ring r lies at height 0.5 r; every point is present twice
    inside its ring at unrelated indices, so every 1-NN, and most seconds and thirds, are decided by the tie rule alone"""
    rng = np.random.default_rng(23)

    def cloud():
        g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), axis=-1).reshape(-1, 2) * 0.25
        out = []
        for r in range(12):
            xy = g[rng.random(g.shape[0]) < 0.7]
            pts = np.concatenate([xy, np.full((xy.shape[0], 1), 0.5 * r), np.full((xy.shape[0], 1), float(r))], axis=1)
            pts = np.concatenate([pts, pts])
            out.append(pts[rng.permutation(pts.shape[0])])
        return np.concatenate(out)

    def queries(n):
        return np.stack([rng.integers(-2, 42, n) * 0.125, rng.integers(-2, 42, n) * 0.125, rng.integers(0, 45, n) * 0.125, np.zeros(n)], axis=1)

    return Case("ties", queries(1000), queries(1000), cloud(), cloud(), no_deskew=True, lattice=True)


def _gate():
    """3-4-0 offsets: squared distance exactly 25, and 1/64 m inside and outside it, for closest and for second / third"""
    b = Blocks()
    e = 1.0 / 64
    q = Q_OFF
    trip = [(3, 4, 0), (0, 3, 4), (4, 0, 3), (-3, 4, 0), (0, -4, -3), (5, 0, 0), (0, 0, -5)]
    shifts = (0.0, -e, +e)
    n_exact = 0
    for t in trip:
        t = np.asarray(t, np.float64)
        ax = int(np.argmax(np.abs(t)))
        for sh in shifts:
            far = t.copy()
            far[ax] += np.sign(t[ax]) * sh
            # (a) the only point of the block: closest at exactly / inside / outside the gate
            b.add([q + far], [5], 0, q_at=q, found=sh < 0)
            # (b) closest 0.04 m away; ring 5 above and ring 6 above at the gate (surf second, corner second / surf third)
            b.add([np.zeros(3), q + far, q - far], [5, 5, 6], 0)
            # (c) the same below
            b.add([q - far, q + far, np.zeros(3)], [4, 5, 5], 2)
            n_exact += sh == 0.0
    return Case("gate", b.query_cloud(), b.query_cloud(), b.cloud(), b.cloud(), no_deskew=True, lattice=True, want_closest=(b.closest, b.closest),
                n_blocks_exact=3 * n_exact)


def _ring_rules():
    """fractional intensities (ring + a fraction up to 0.95: int() is truncation); rings cs +- 2 seen, cs +- 3 ending the walk"""
    rng = np.random.default_rng(25)
    b, kinds = Blocks(), []
    fr = lambda n: rng.uniform(0.0, 0.95, n)
    for rep in range(40):
        r = int(rng.integers(3, 60))
        # A: rings r-3 .. r+3 in order; r +- 1 far (4 m), r +- 2 near (1 m), r +- 3 nearer (0.5 m) but behind the end of the walk
        off, rings = [], []
        for dr, rad in ((-3, 0.5), (-2, 1.0), (-1, 4.0), (0, None), (1, 4.0), (2, 1.0), (3, 0.5)):
            if dr == 0:
                same = _dirs(rng, 6, rng.uniform(0.3, 2.0, 6))
                off += [same[:3], np.zeros((1, 3)), same[3:]]
                rings += [r + fr(3), [r + fr(1)[0]], r + fr(3)]
            else:
                off.append(_dirs(rng, 5, rad * rng.uniform(1.0, 1.1, 5)))
                rings.append(r + dr + fr(5))
        b.add(np.concatenate(off), np.concatenate(rings), 18)
        kinds.append("A")
        # B: the only near points share the ring of closest; the other rings of the window lie beyond the gate
        off = [_dirs(rng, 4, 5.5), _dirs(rng, 3, rng.uniform(0.3, 2.0, 3)), np.zeros((1, 3)), _dirs(rng, 3, rng.uniform(0.3, 2.0, 3)), _dirs(rng, 4, 5.5)]
        rings = [r - 1 + fr(4), r + fr(3), [r + fr(1)[0]], r + fr(3), r + 1 + fr(4)]
        b.add(np.concatenate(off), np.concatenate(rings), 7)
        kinds.append("B")
    return Case("ring_rules", b.query_cloud(), b.query_cloud(), b.cloud(), b.cloud(), no_deskew=True, want_closest=(b.closest, b.closest),
                kinds=np.array(kinds))


def ring_cloud(rng, rings=16, per_ring=300, centre=(0.0, 0.0, 0.0), frac=0.1):
    """a ring-ordered sweep-like cloud: ring r at elevation -15 + 2 r degrees, azimuth ascending inside a ring, range 5 .. 11 m;
    intensity = ring + relative time (frac * azimuth / 2 pi)"""
    out = []
    for r in range(rings):
        az = np.sort(rng.uniform(0, 2 * np.pi, per_ring))
        rad = 8 + 3 * np.sin(3 * az + 0.1 * r) + rng.normal(0, 0.02, per_ring)
        el = np.deg2rad(-15 + 2.0 * r)
        xyz = np.stack([rad * np.cos(az) * np.cos(el), rad * np.sin(az) * np.cos(el), rad * np.sin(el)], axis=1) + np.asarray(centre)
        out.append(np.concatenate([xyz, (r + frac * az / (2 * np.pi))[:, None]], axis=1))
    return np.concatenate(out).astype(np.float32)


def _near_queries(rng, cloud, n, sigma):
    q = cloud[rng.integers(0, cloud.shape[0], n)].astype(np.float64)
    q[:, :3] += rng.normal(0, 1, (n, 3)) * np.broadcast_to(np.asarray(sigma), (n,))[:, None]
    return q.astype(np.float32)


def _grid_edges():
    rng = np.random.default_rng(26)

    def cloud():
        return np.concatenate([ring_cloud(rng, 8, 150, c) for c in ((112.0, 112.0, 1.0), (0.0, 0.0, 0.0), (-112.0, -112.0, -1.0))])

    def queries(cl):
        out = [_near_queries(rng, cl, 400, rng.choice([0.2, 1.0, 3.0, 6.0], 400))]
        xyz = cl[:, :3].astype(np.float64)
        outside = []
        for ax in range(3):
            for side, ext in ((+1, np.argmax(xyz[:, ax])), (-1, np.argmin(xyz[:, ax]))):
                for delta in (0.5, 4.9, 4.999, 5.001, 5.2, 9.0, 11.0, 30.0):
                    p = cl[ext].astype(np.float64)
                    p[ax] += side * delta
                    outside.append(p)
        faces = []
        cell = float(CELL)
        for ax in range(3):
            k = np.rint(xyz[:, ax] / cell)
            near = np.nonzero(np.abs(xyz[:, ax] - k * cell) < 3.0)[0]
            for i in rng.choice(near, 40):
                for side in (-1, +1):
                    p = cl[i].astype(np.float64)
                    p[:3] += rng.normal(0, 0.3, 3)
                    p[ax] = k[i] * cell + side * 1e-3 * cell
                    faces.append(p)
        return np.concatenate([out[0], np.asarray(outside, np.float32), np.asarray(faces, np.float32)]), len(outside), len(faces)

    lc, ls = cloud(), cloud()
    (qc, no, nf), (qs, _, _) = queries(lc), queries(ls)
    return Case("grid_edges", qc, qs, lc, ls, no_deskew=True, n_outside=no, n_faces=nf)


def grid_cells(cloud):
    """cells of the 5 m grid the product lays over a previous cloud (csrc/cloud_kernels.h: grid_extent, one border cell on every side)"""
    inv = np.float32(1.0) / CELL
    lo = np.floor(cloud[:, :3].min(axis=0) * inv).astype(np.int64) - 1
    hi = np.floor(cloud[:, :3].max(axis=0) * inv).astype(np.int64) + 1
    return int(np.prod(hi - lo + 1))


def _grid_oversize():
    """two tight clusters 300 m apart along every axis: the grid over them has about 61^3 cells, more than GRID_CELLS_MAX, so the product
    builds it by KnnGrid::build and not by the segmented build every other case's grids go through"""
    rng = np.random.default_rng(31)
    centres = np.array([[-150.0, -150.0, -150.0], [150.0, 150.0, 150.0]])

    def cloud():
        out = []
        for c in centres:   # rings 0 .. 9 at heights 0.3 m apart, ten points each on a 3 m patch
            ring = np.repeat(np.arange(10.0), 10)
            xyz = c + np.concatenate([rng.uniform(-1.5, 1.5, (100, 2)), 0.3 * ring[:, None] + rng.normal(0, 0.02, (100, 1))], axis=1)
            out.append(np.concatenate([xyz, ring[:, None]], axis=1))
        return np.concatenate(out).astype(np.float32)

    lc, ls = cloud(), cloud()
    near = lambda cl: np.concatenate([_near_queries(rng, cl[:100], 64, 0.2), _near_queries(rng, cl[100:], 64, 0.2)])
    return Case("grid_oversize", near(lc), near(ls), lc, ls, no_deskew=True)


def _tiny(kind):
    rng = np.random.default_rng(27)
    q = np.concatenate([rng.normal(0, 2.0, (70, 3)), np.zeros((70, 1))], axis=1)
    q[:5, :3] += 9.0
    one = np.array([[1.0, 2.0, 0.5, 3.02]])
    two_rings = np.array([[1.0, 2.0, 0.5, 3.02], [1.5, 1.0, 0.0, 4.07]])
    two_same = np.array([[1.0, 2.0, 0.5, 3.02], [1.5, 1.0, 0.0, 3.5]])
    none = np.zeros((0, 4))
    if kind == "prev_0":
        lc, ls = none, none
    elif kind == "prev_1":
        lc, ls = one, two_same
    elif kind == "prev_2":
        lc, ls = two_rings, one
    else:   # all previous points identical: rings 0 .. 9, twenty points each
        lc = np.concatenate([np.tile([[0.5, -0.25, 0.125]], (200, 1)), np.repeat(np.arange(10.0), 20)[:, None]], axis=1)
        ls = lc
    return Case(kind, q, q, lc, ls, no_deskew=True)


def _motion():
    ang = np.deg2rad(3.0)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]]), np.array([0.6, -0.5, 0.17])      # 3 degrees, 0.8 m


def _bad_queries():
    rng = np.random.default_rng(28)
    lc, ls = ring_cloud(rng), ring_cloud(rng)
    q, p = _motion()

    def queries(cl):
        qs = _near_queries(rng, cl, 300, 0.2)
        qs[:, 3] = np.trunc(qs[:, 3]) + rng.uniform(0, 0.1, 300)
        rows = np.array([0, 5, 31, 63, 64, 65, 100, 127, 128, 129, 191, 192, 200, 255, 256, 299])
        nothing, through = [], []
        for k, i in enumerate(rows):
            t = k % 8
            if t == 0: qs[i, 0] = np.nan
            elif t == 1: qs[i, 1] = np.inf
            elif t == 2: qs[i, 2] = -np.inf
            elif t == 3: qs[i, 3] = np.nan
            elif t == 4: qs[i, 3] = -0.05                       # ratio -0.5
            elif t == 5: qs[i, 3] = np.trunc(qs[i, 3]) + 0.15   # ratio 1.5
            elif t == 6: qs[i, 3] = np.inf
            else: qs[i, 3] = -np.inf
            (nothing if t < 4 else through).append(i)
        return qs, np.array(nothing), np.array(through)

    (qc, nc_, tc), (qs, ns_, ts) = queries(lc), queries(ls)
    return Case("bad_queries", qc, qs, lc, ls, q=q, p=p, nothing=(nc_, ns_), through=(tc, ts))


def _deskew():
    rng = np.random.default_rng(29)
    lc, ls = ring_cloud(rng, per_ring=400), ring_cloud(rng, per_ring=400)
    q, p = _motion()

    def queries(cl):
        qs = _near_queries(rng, cl, 800, rng.choice([0.05, 0.3], 800))
        qs[:, 3] = np.trunc(qs[:, 3]) + rng.uniform(0, 0.1, 800).astype(np.float32)      # relative times over the whole sweep
        return qs

    return Case("deskew", queries(lc), queries(ls), lc, ls, q=q, p=p)


def _sweep(kind, it, oracle):
    """two consecutive synthetic sweeps through the oracle's PointProcessor; the previous clouds are the first sweep's less-sharp and
    less-flat clouds as the first Process keeps them (ring + relative time); transform_es is what the oracle's odometry holds when
    iteration `it` (0 or 5) searches: the identity, or the end of iteration 4"""
    from lio_amd import capi, synth

    sweeps, _, lid = synth.make_sweeps("indoor" if kind == "vlp16" else "outdoor", 2)
    cl = []
    for sw in sweeps:
        pp = capi.PointProcessor(oracle, lid.lower_deg, lid.upper_deg, lid.rings)
        pp.process(sw)
        cl.append([pp.cloud(w) for w in (1, 2, 3, 4)])
    q, p = np.array([0, 0, 0, 1.0]), np.zeros(3)
    if it:
        od = capi.PointOdometry(oracle, 0.1, 2, 25, False)
        od.process(*cl[0])
        trace = od.process(*cl[1])["trace"]
        assert trace.shape[0] >= it, trace.shape
        q, p = trace[it - 1, :4], trace[it - 1, 4:7]
    sharp, flat = cl[1][0], cl[1][2]
    if kind == "hdl64":
        sharp, flat = sharp[:: max(1, -(-sharp.shape[0] // 512))], flat[:: max(1, -(-flat.shape[0] // 512))]
    return Case(f"sweep_{kind}_iter{it}", sharp, flat, cl[0][1], cl[0][3], q=q, p=p)


_BUILDERS = {
    "chunk_edges": lambda o: _chunk_edges(False), "chunk_edges_swapped": lambda o: _chunk_edges(True),
    "violation_then_valid": lambda o: _violation_then_valid(), "ties": lambda o: _ties(), "gate": lambda o: _gate(),
    "ring_rules": lambda o: _ring_rules(), "grid_edges": lambda o: _grid_edges(), "grid_oversize": lambda o: _grid_oversize(),
    "prev_0": lambda o: _tiny("prev_0"), "prev_1": lambda o: _tiny("prev_1"), "prev_2": lambda o: _tiny("prev_2"),
    "prev_identical": lambda o: _tiny("prev_identical"), "bad_queries": lambda o: _bad_queries(), "deskew": lambda o: _deskew(),
    "sweep_vlp16_iter0": lambda o: _sweep("vlp16", 0, o), "sweep_vlp16_iter5": lambda o: _sweep("vlp16", 5, o),
    "sweep_hdl64_iter0": lambda o: _sweep("hdl64", 0, o), "sweep_hdl64_iter5": lambda o: _sweep("hdl64", 5, o),
}
NAMES = tuple(_BUILDERS)
LATTICE = ("ties", "gate")


@functools.lru_cache(maxsize=None)
def _get(name):
    return _BUILDERS[name](_get.oracle)


def get(name, oracle):
    """the case, built once per process; `oracle` (the CPU library) makes the sweep cases' clouds and transforms"""
    _get.oracle = oracle
    return _get(name)


# ---------------------------------------------------------------- checks both libraries are held to
def check_bad_queries(c, lib):
    """the statement of include/lio_test_hooks.h on its own (oracle: tests/test_odom_corr.py; product: tests/test_gpu_odom_corr.py)"""
    ci, si, sel = c.run(lib)
    nc = c.sharp.shape[0]
    assert (ci[c.nothing[0]] == -1).all() and (si[c.nothing[1]] == -1).all()
    # a ratio outside [0, 1.001] passes through unchanged, and is searched for
    np.testing.assert_array_equal(sel[c.through[0]], c.sharp[c.through[0], :3])
    np.testing.assert_array_equal(sel[nc + c.through[1]], c.flat[c.through[1], :3])
    assert (ci[c.through[0], 0] >= 0).all() and (si[c.through[1], 0] >= 0).all()
    clean = []
    for q, rows in ((c.sharp, np.concatenate([c.nothing[0], c.through[0]])), (c.flat, np.concatenate([c.nothing[1], c.through[1]]))):
        q = q.copy()
        q[rows] = q[(rows + 3) % q.shape[0]]
        assert np.isfinite(q).all()
        clean.append((q, np.setdiff1d(np.arange(q.shape[0]), rows)))
    ci2, si2, sel2 = c.run(lib, clean[0][0], clean[1][0])
    np.testing.assert_array_equal(ci[clean[0][1]], ci2[clean[0][1]])
    np.testing.assert_array_equal(si[clean[1][1]], si2[clean[1][1]])
    np.testing.assert_array_equal(sel[:nc][clean[0][1]], sel2[:nc][clean[0][1]])
    np.testing.assert_array_equal(sel[nc:][clean[1][1]], sel2[nc:][clean[1][1]])
    assert (ci2[:, 0] >= 0).all() and (si2[:, 0] >= 0).all()


def check_arguments(lib):
    """a null required pointer or a scan_period that is not positive and finite: LIO_ERR_ARG, before anything is written"""
    import ctypes

    from lio_amd import capi

    f = lambda n: np.zeros((n, 4), np.float32)
    sharp, flat, lc, ls = f(2), f(3), f(4), f(5)
    ci, si, sel = np.full((2, 2), 7, np.int32), np.full((3, 3), 7, np.int32), np.full((5, 3), 7, np.float32)
    T = capi.TransformF.make([0, 0, 0, 1], [0, 0, 0])
    fp, ip = (lambda a: None if a is None else a.ctypes.data_as(capi.c_float_p)), (lambda a: None if a is None else a.ctypes.data_as(capi.c_int32_p))

    def call(sharp=sharp, flat=flat, lc=lc, ls=ls, T=T, period=0.1, ci=ci, si=si, sel=sel, counts=(2, 3, 4, 5)):
        return lib.dll.lio_odom_correspondences(fp(sharp), counts[0], fp(flat), counts[1], fp(lc), counts[2], fp(ls), counts[3],
                                                None if T is None else ctypes.byref(T), period, 0, ip(ci), ip(si), fp(sel))

    for bad in (dict(sharp=None), dict(flat=None), dict(lc=None), dict(ls=None), dict(T=None), dict(ci=None), dict(si=None), dict(sel=None),
                dict(period=0.0), dict(period=-0.1), dict(period=float("inf")), dict(period=float("nan"))):
        assert call(**bad) == -1, bad
    assert (ci == 7).all() and (si == 7).all() and (sel == 7).all()


def check_no_queries(lib):
    """n_sharp == n_flat == 0 is fine, with and without previous clouds"""
    rng = np.random.default_rng(30)
    none = np.zeros((0, 4), np.float32)
    for prev in (none, ring_cloud(rng, 4, 50)):
        ci, si, sel = Case("no_queries", none, none, prev, prev).run(lib)
        assert ci.shape == (0, 2) and si.shape == (0, 3) and sel.shape == (0, 3)
