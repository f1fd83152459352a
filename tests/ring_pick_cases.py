"""Seeded sweeps for lio_pp_process_rings that put k_ring_pick, k_lf_ring and k_pp_pack at their edges (tests/test_ring_pick.py holds
every family to the conditions it is built for, from the counters of tests/ring_pick_ref.py alone; tests/test_gpu_ring_pick.py runs
them through the product).  A ring is an arc of increasing azimuth (step <= 0.003 rad, range about 8 m: the beam-parallel test of
PrepareRing stays silent unless a case wants it) whose range zigzags: every kink is a corner candidate.  The rings of a sweep are
interleaved point by point as a spinning sensor delivers them, a few stray returns carry a ring outside [0, rings), and no jump
above 0.1 m^2 lies in the last nc + 2 points of a ring (there the reference writes past its mask vector).  All default-config
families use a 64-ring sensor, so that they can share one launch chain of lio_pp_process_rings_batch.
"""
import numpy as np

from ring_pick_ref import config, ring_picks, subregion_bounds

F = np.float32
RINGS = 64
SLOPE = 0.03      # range step per point of the zigzag (m): the apex of a kink has curvature (30 x 0.03)^2 = 0.81 at nc = 5


def arc(n, kinks=(), seed=0, ring=0, slope=SLOPE, noise=1e-4, step=None, az0=0.3, steps=(), spikes=(), z=None, r0=8.0, profile=None):
    """n x 4 float32: range r0 + zigzag (the slope changes sign at every kink) + steps (pos, dr: everything from pos on moves by dr)
    + spikes (pos, dr: that point alone) + seeded noise (`profile`, in units of the slope, replaces the zigzag); azimuth az0 + i * step (2 pi - atan2(y, x) increases with i)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    sign = np.ones(n)
    for k in sorted(kinks):
        sign[k:] *= -1.0
    shape = np.r_[0.0, np.cumsum(sign[:-1])] if profile is None else np.asarray(profile, np.float64)
    r = r0 + shape * slope + rng.normal(0.0, noise, n)
    for pos, dr in steps:
        r[pos:] += dr
    for pos, dr in spikes:
        r[pos] += dr
    if step is None:
        step = min(0.003, 5.4 / max(n, 1))
    az = az0 + 1e-5 * ring + i * step                  # a higher ring starts a little later: the sweep's first return has the smallest azimuth
    zc = (-0.3 + 0.05 * (ring % 13)) if z is None else None
    out = np.zeros((n, 4), F)
    out[:, 0] = r * np.cos(az)
    out[:, 1] = -r * np.sin(az)
    out[:, 2] = (zc * r / 8.0) if z is None else z
    out[:, 3] = (i % 7) + 0.25
    return out


def interleave(ring_points, rings, seed=0, strays=5):
    """{ring: n x 4} -> (scan, ring field): round robin over the rings that still have points, strays with a ring outside [0, rings)
    sprinkled in.  The first kept return has the sweep's smallest azimuth (no ring is unwrapped by 2 pi)."""
    rng = np.random.default_rng(1000 + seed)
    ids = sorted(ring_points)
    pts, rf = [], []
    depth = max(len(ring_points[r]) for r in ids)
    cols_p, cols_r = [], []
    for r in ids:
        p = ring_points[r]
        pad = np.full((depth, 4), np.nan, F)
        pad[:len(p)] = p
        cols_p.append(pad)
        cols_r.append(np.full(depth, r, np.int64))
    P = np.stack(cols_p, 1).reshape(-1, 4)
    R = np.stack(cols_r, 1).reshape(-1)
    have = ~np.isnan(P[:, 0])
    pts.append(P[have])
    rf.append(R[have])
    scan, ring = np.concatenate(pts), np.concatenate(rf)
    azi = (-np.arctan2(scan[:, 1].astype(np.float64), scan[:, 0])) % (2 * np.pi)
    assert azi[0] > 0 and np.all(azi[1:] > azi[0] + 5e-6) and azi.max() < 6.2
    # strays: finite points whose ring is outside the sensor's
    at = np.sort(rng.integers(1, len(scan), strays))
    for k, a in enumerate(at):
        scan = np.insert(scan, a, np.array([7.5, -2.0 - k, 0.3, 3.0], F), 0)
        ring = np.insert(ring, a, [rings, 65535, rings + 1, 200, 4000][k % 5])
    return np.ascontiguousarray(scan, F), ring.astype(np.uint16)


def _drift_kinks(n, fixed, every=24, clear=10):
    """kinks that keep the zigzag's range near its start: one every `every` points, none within `clear` points of a fixed kink"""
    fixed = np.asarray(sorted(fixed), np.int64)
    out = []
    for k in range(every // 2, n - 8, every):
        if len(fixed) == 0 or np.abs(fixed - k).min() > clear:
            out.append(k)
    return out


# ------------------------------------------------------------------------------------------------ boundary
BOUNDARY = [(8, 5), (16, 8), (9, 3), (1, 5), (3, 1), (16, 1)]
BOUNDARY_TH = {5: 0.1, 8: 0.1, 3: 0.002, 1: 0.002}     # small nc: only the apex of a kink would pass 0.1
_OFFSETS = [-1, 1, -3, 2, -2, 0, 3, -4]


def boundary_case(ns, nc):
    lengths = [397, 411, 522, 463, 505, 436]
    pts = {}
    for q, n in enumerate(lengths):
        ring = [0, 1, 17, 31, 32, 63][q]
        kinks = []
        for j, (sp, _) in enumerate(subregion_bounds(n, ns, nc)[1:], 1):
            off = -1 if q == 0 else _OFFSETS[(q + j) % len(_OFFSETS)]
            off = int(np.clip(off, -nc, nc - 1))
            k = sp + off
            if nc + 1 < k < n - nc - 3:
                kinks.append(k)
                if nc <= 1 and (q + j) % 2 == 0:
                    kinks.append(k + 1)              # nc = 1: only the apex has curvature, so two apexes side by side
        kinks = sorted(set(kinks))
        pts[ring] = arc(n, kinks + _drift_kinks(n, kinks, every=max(12, 3 * nc + 6), clear=nc + 3), seed=100 * ns + nc + q, ring=ring)
    over = {} if (ns, nc) == (8, 5) else {"num_scan_subregions": ns, "num_curvature_regions": nc, "surf_curv_th": BOUNDARY_TH[nc]}
    scan, ring = interleave(pts, RINGS, seed=ns * 10 + nc)
    return (f"boundary_ns{ns}_nc{nc}", RINGS, over, scan, ring)


# ------------------------------------------------------------------------------------------------ tiny
def tiny_case(ns):
    pts = {}
    for r in range(50):
        n = 11 + r                                     # 2 nc + 1 (skipped), 2 nc + 2, ... 60
        rng = np.random.default_rng(7000 + 64 * ns + r)
        kinks = sorted(set(rng.integers(2, max(3, n - 2), max(1, n // 4)).tolist()))
        pts[r] = arc(n, kinks, seed=7100 + 64 * ns + r, ring=r, slope=0.035)
    over = {} if ns == 8 else {"num_scan_subregions": ns}
    scan, ring = interleave(pts, RINGS, seed=ns)
    return (f"tiny_ns{ns}", RINGS, over, scan, ring)


# ------------------------------------------------------------------------------------------------ chunks
def chunks_case(name, sizes, seed):
    pts = {}
    for q, size in enumerate(sizes):
        n = 10 + 8 * size
        ring = 3 + 9 * q
        pts[ring] = arc(n, _drift_kinks(n, [], every=14 + q), seed=seed + q, ring=ring)
    scan, ring = interleave(pts, RINGS, seed=seed)
    return (name, RINGS, {}, scan, ring)


def all_masked_case():
    """every point of the ring fails the beam-parallel test (both neighbours farther than sqrt(0.0002) x range), so every candidate is
    masked by PrepareRing and both pick loops of both subregions run through all their 64-candidate chunks without a pick"""
    n = 10 + 2 * 130
    p = arc(n, _drift_kinks(n, [], every=9), seed=4242, ring=5, step=0.0148)
    scan, ring = interleave({5: p}, RINGS, seed=42)
    return ("chunks_all_masked", RINGS, {"num_scan_subregions": 2}, scan, ring)


# ------------------------------------------------------------------------------------------------ ties
TIES_TH = 0.140625     # (24 / 64)^2: the curvature two points from the apex of a kink of slope 2 / 64


def lattice_ring(n, period, m, k0, x0=8.0, z=-0.25, phase=0):
    """points on the 1/64 lattice: y = -(k0 + i) / 64, x = x0 + (m / 64) x triangle wave of the given period (0: straight), z fixed.
    Every sum of PrepareSubregion is exact in fp32, so equal shapes give equal curvatures."""
    i = np.arange(n)
    if period:
        t = (i + phase) % period
        tri = np.where(t < period // 2, t, period - t)
    else:
        tri = np.zeros(n)
    out = np.zeros((n, 4), F)
    out[:, 0] = x0 + tri * (m / 64.0)
    out[:, 1] = -(k0 + i) / 64.0
    out[:, 2] = z
    out[:, 3] = (i % 5) + 0.5
    assert np.all(out[:, :3] * 64 == np.round(out[:, :3] * 64))
    return out


def ties_case():
    n = 10 + 8 * 70
    pts = {0: lattice_ring(n, 16, 2, 200), 1: lattice_ring(n, 2, 6, 215, x0=8.5), 2: lattice_ring(n, 0, 0, 232, x0=9.0), 3: lattice_ring(n, 24, 2, 203, x0=7.5, phase=5)}
    scan, ring = interleave(pts, 4, seed=77, strays=3)
    return ("ties_lattice", 4, {"surf_curv_th": TIES_TH}, scan, ring)


# ------------------------------------------------------------------------------------------------ gaps
def gaps_case():
    pts = {}
    # ring 2: range steps whose squared length is just above / just below 0.05 m^2, right behind and right in front of kinks
    n = 400
    kinks = [60, 120, 180, 240, 300, 350]
    steps = [(63, 0.225), (117, -0.225), (183, 0.215), (237, -0.215), (302, 0.24), (348, 0.23)]
    pts[2] = arc(n, kinks + _drift_kinks(n, kinks), seed=51, ring=2, steps=steps)
    # ring 9: one occlusion of each direction (a jump above 0.1 m^2 to a closer / to a farther surface) and beam-parallel points
    n = 380
    kinks = [90, 200, 290]
    pts[9] = arc(n, kinks + _drift_kinks(n, kinks), seed=52, ring=9, steps=[(100, -1.0), (210, 1.2)], spikes=[(150, 0.15), (250, -0.15), (251, 0.15)])
    # ring 40: both at subregion boundaries
    n = 522
    b = [sp for sp, _ in subregion_bounds(n, 8, 5)]
    kinks = [b[2] - 2, b[4] + 1, b[6] - 1]
    pts[40] = arc(n, kinks + _drift_kinks(n, kinks), seed=53, ring=40, steps=[(b[2] - 1, 0.23), (b[4] + 3, -0.23), (b[5], -0.9), (b[6] + 1, 0.21)])
    scan, ring = interleave(pts, RINGS, seed=5)
    return ("gaps", RINGS, {}, scan, ring)


# ------------------------------------------------------------------------------------------------ capacity edges that must work
def capacity_case(name, n, over, extra=()):
    pts = {20: arc(n, _drift_kinks(n, [], every=31), seed=n, ring=20)}
    for q, m in enumerate(extra):
        pts[22 + 2 * q] = arc(m, [m // 2], seed=n + 1 + q, ring=22 + 2 * q)
    scan, ring = interleave(pts, RINGS, seed=n % 97)
    return (name, RINGS, over, scan, ring)


def capacity_cases():
    return [capacity_case("cap_ring4080_ns8", 4080, {}, extra=(11, 12)),
            capacity_case("cap_7x512_ns7", 7 * 512 + 10, {"num_scan_subregions": 7}),
            capacity_case("cap_7x512_nc8", 7 * 512 + 16, {"num_scan_subregions": 7, "num_curvature_regions": 8})]


def over_capacity_sweeps():
    """(name, config overrides, scan, ring field, the exact-limit case that follows it through the same handle)"""
    a = capacity_case("over_ring4081_ns8", 4081, {})
    b = capacity_case("over_subregion513_ns7", 7 * 512 + 11, {"num_scan_subregions": 7})
    return [(a, "cap_ring4080_ns8"), (b, "cap_7x512_ns7")]


# ------------------------------------------------------------------------------------------------ quotas
def quota_case(less_sharp, flat, jagged):
    """nc = 2, two subregions of 500 points: `jagged` of each is a zigzag with a kink every 6 points (a pick masks 5), the rest an arc of constant range"""
    over = {"num_scan_subregions": 2, "num_curvature_regions": 2, "surf_curv_th": 1e-4, "max_corner_sharp": less_sharp,
            "max_corner_less_sharp": less_sharp, "max_surf_flat": flat}
    n = 4 + 2 * 500
    pts = {}
    for q, ring in enumerate((7, 8)):
        profile = np.zeros(n)
        for sp, ep in subregion_bounds(n, 2, 2):
            t = np.arange(12 * int(jagged * 500 / 12))           # whole periods: the range is back where it was when the straight part begins
            profile[sp + 3 + q:sp + 3 + q + len(t)] = np.where(t % 12 < 6, t % 12, 12 - t % 12)
        pts[ring] = arc(n, seed=900 + less_sharp + q, ring=ring, noise=2e-5, profile=profile)
    scan, ring = interleave(pts, RINGS, seed=less_sharp)
    return (f"quota_{less_sharp}_{flat}", RINGS, over, scan, ring)


# ------------------------------------------------------------------------------------------------ rings
def rings_cases():
    out = []
    pts = {}
    for q, r in enumerate((0, 1, 63, 64, 65, 100, 127)):
        n = 300 - 13 * q
        pts[r] = arc(n, _drift_kinks(n, [], every=20 + q), seed=600 + r, ring=r)
    scan, ring = interleave(pts, 128, seed=128)
    out.append(("rings_128_sparse", 128, {}, scan, ring))
    pts = {r: arc(260 + 30 * r, _drift_kinks(260 + 30 * r, [], every=17), seed=650 + r, ring=r) for r in (0, 1)}
    scan, ring = interleave(pts, 2, seed=2, strays=4)
    out.append(("rings_2", 2, {}, scan, ring))
    return out


# ------------------------------------------------------------------------------------------------ less-flat
def less_flat_ring(members, ring, seed, cfg, z):
    """a ring with exactly `members` points handed to the voxel filter: the length starts at members + 2 nc and grows until the CPU
    reference reports that count (every pick that is not a flat one takes a member away).  Negative coordinates (az0 = 2.2 rad), z
    exactly on a voxel face."""
    nc = cfg["num_curvature_regions"]
    for n in range(members + 2 * nc, members + 2 * nc + 400):
        p = arc(n, _drift_kinks(n, [], every=33), seed=seed, ring=ring, az0=2.2, z=z, step=min(0.003, 3.0 / n))
        if len(ring_picks(p[:, :3], cfg)["members"]) == members:
            return p
    raise AssertionError(f"no ring length gives {members} less-flat members")


def less_flat_case(name, leaf, wanted):
    over = {} if leaf == 0.2 else {"less_flat_filter_size": leaf}
    cfg = config(over)
    pts = {}
    for q, m in enumerate(wanted):
        ring = 4 + 5 * q
        pts[ring] = less_flat_ring(m, ring, 300 + m, cfg, z=F(-leaf) * (1 + q % 3))
    scan, ring = interleave(pts, RINGS, seed=int(leaf * 100))
    return (name, RINGS, over, scan, ring)


LESS_FLAT_MEMBERS = {"less_flat_leaf02": (128, 129, 240, 256, 257, 2048, 2049), "less_flat_leaf005": (240, 256, 2048)}

_CASES = None


def cases():
    """-> list of (name, rings, config overrides, scan [N x 4 float32], ring field [N uint16]); built once"""
    global _CASES
    if _CASES is None:
        out = [boundary_case(ns, nc) for ns, nc in BOUNDARY]
        out += [tiny_case(8), tiny_case(16)]
        out += [chunks_case("chunks_63_64", (63, 64), 300), chunks_case("chunks_65_128_129", (65, 128, 129), 310), all_masked_case()]
        out += [ties_case(), gaps_case()]
        out += capacity_cases()
        out += [quota_case(40, 24, 0.62), quota_case(64, 0, 0.85), quota_case(1, 63, 0.2)]
        out += rings_cases()
        out += [less_flat_case("less_flat_leaf02", 0.2, LESS_FLAT_MEMBERS["less_flat_leaf02"]),
                less_flat_case("less_flat_leaf005", 0.05, LESS_FLAT_MEMBERS["less_flat_leaf005"])]
        assert sum(len(c[3]) for c in out) < 70000
        _CASES = out
    return _CASES


def case(name):
    return next(c for c in cases() if c[0] == name)


DEFAULT_BATCH = ["boundary_ns8_nc5", "tiny_ns8", "chunks_65_128_129", "gaps", "cap_ring4080_ns8", "less_flat_leaf02"]   # one launch chain, rings up to 4080
SMALL_BATCH = ["boundary_ns8_nc5", "tiny_ns8", "gaps", "chunks_63_64"]                                                    # longest ring: 522 points
