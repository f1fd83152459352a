"""The cases of the Gauss-Newton tests (tests/test_gn.py: the oracle and the comparisons themselves, without a GPU; tests/test_gpu_gn.py: the
product through lio_gn_rows_map, lio_gn_fold, lio_gn_step and lio_gn_round).  Every case is seeded; the references are tests/gn_ref.py.

Rows of the scan-to-map family: the sizes at which the rows launch changes shape — 0, 1, around a wave (63, 64, 65) and a block (255, 256,
257), one and two blocks of eight slots per thread (2048, 2049), nine blocks (16385: past the eight groups of reduce_partials28) and
524289 (past the 256-block cap: the grid-stride loop wraps) — with every, no, every 64th and all-but-one-wave valid queries, at ranges of
1, 50 and 400 m, at the identity and at a general pose, in the three forms.
Folds: integer partials, which every order adds exactly, at the counts around each of the two folds' strides, and a position-coded set.
Steps: well-conditioned systems from synthetic rows, decisions built with margin, a rank-deficient system, a NaN sum."""
import functools
import math

import numpy as np

import gn_ref
from lio_amd import capi

# ------------------------------------------------------------------------------------------------ rows of the scan-to-map family
IDENTITY = ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
_g = np.array([0.21, -0.37, 0.55, 0.72])
GENERAL = (tuple(float(v) for v in (_g / np.linalg.norm(_g)).astype(np.float32)), (3.25, -7.5, 1.125))

#        name                 m       range  valid          pose
_MAP = [("m0",                0,      50.0,  "all",         GENERAL),
        ("m1",                1,      50.0,  "all",         GENERAL),
        ("m63",               63,     50.0,  "all",         GENERAL),
        ("m64",               64,     50.0,  "all",         IDENTITY),
        ("m65",               65,     50.0,  "all",         GENERAL),
        ("m255",              255,    1.0,   "all",         GENERAL),
        ("m256",              256,    400.0, "all",         GENERAL),
        ("m257",              257,    50.0,  "all",         IDENTITY),
        ("none_m257",         257,    50.0,  "none",        GENERAL),
        ("wave_out_m257",     257,    50.0,  "wave_out",    GENERAL),
        ("r1_m2048",          2048,   1.0,   "all",         IDENTITY),
        ("every64_m2049",     2049,   400.0, "every64",     GENERAL),
        ("r400_m2049",        2049,   400.0, "all",         GENERAL),
        ("m16385",            16385,  50.0,  "most",        GENERAL),
        ("m524289",           524289, 50.0,  "half",        GENERAL)]
MAP_NAMES = [c[0] for c in _MAP]
MAP_RUNS = [(n, f) for n in MAP_NAMES for f in (0, 1, 2)]


class MapCase:
    def __init__(self, name, m, rng_m, valid_kind, pose):
        self.name, self.m, self.range, self.valid_kind = name, m, rng_m, valid_kind
        self.q, self.t = (np.asarray(v, np.float32) for v in pose)
        rng = np.random.default_rng(1000 + MAP_NAMES.index(name))
        d = rng.normal(size=(m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        self.stack = np.zeros((m, 4), np.float32)
        self.stack[:, :3] = d * rng_m * rng.uniform(0.98, 1.02, (m, 1))
        self.stack[:, 3] = rng.uniform(0, 16, m)
        n = rng.normal(size=(m, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        s = rng.uniform(0.1, 1.0, (m, 1))                       # the residual's weight
        sel = gn_ref.rotate(self.q, self.stack[:, :3].astype(np.float64)) + self.t.astype(np.float64)
        dist = rng.normal(0, 0.05, m)                           # point-to-plane distances of centimetres: b cancels, as in a real sweep
        self.coeff = np.zeros((m, 4), np.float32)
        self.coeff[:, :3] = s * n
        self.coeff[:, 3] = s[:, 0] * (dist - (n * sel).sum(axis=1))
        v = np.ones(m, np.uint8)
        if valid_kind == "none":
            v[:] = 0
        elif valid_kind == "every64":
            v[:] = 0
            v[::64] = 1
        elif valid_kind == "wave_out":
            v[64:128] = 0
        elif valid_kind == "most":
            v[rng.random(m) < 0.3] = 0
        elif valid_kind == "half":
            v[rng.random(m) < 0.5] = 0
        self.valid = v

    def T(self):
        return capi.TransformF.make(tuple(float(x) for x in self.q), tuple(float(x) for x in self.t))

    def run(self, lib, form, valid=None, coeff=None):
        return lib.gn_rows_map(form, self.stack, self.valid if valid is None else valid, self.coeff if coeff is None else coeff, self.T())

    @functools.lru_cache(maxsize=None)
    def ref(self, form):
        return gn_ref.map_rows_ref(form, self.stack, self.valid, self.coeff, self.q, self.t)


@functools.lru_cache(maxsize=None)
def get_map(name):
    return MapCase(*_MAP[MAP_NAMES.index(name)])


def rows_blocks(m):
    """odom_rows_blocks of csrc/cloud_kernels.hip: eight slots per thread of 256, at most 256 blocks"""
    return max(1, min(-(-m // 2048), 256))


def check_rows_null_pointers(lib):
    """lio_gn_rows_map with each required pointer null, an unknown form and a non-finite pose: LIO_ERR_ARG"""
    import ctypes as C
    c = get_map("m65")
    ok, rows = np.zeros(c.m, np.uint8), np.zeros((c.m, 7), np.float32)
    nb, part = np.zeros(1, np.int32), np.zeros((256, 28))
    T = c.T()
    u8, f32, i32, f64 = (C.POINTER(t) for t in (C.c_uint8, C.c_float, C.c_int32, C.c_double))
    args = [1, c.stack.ctypes.data_as(f32), c.m, c.valid.ctypes.data_as(u8), c.coeff.ctypes.data_as(f32), C.byref(T), ok.ctypes.data_as(u8),
            rows.ctypes.data_as(f32), nb.ctypes.data_as(i32), part.ctypes.data_as(f64)]
    assert lib.dll.lio_gn_rows_map(*args) == 0
    for k in (1, 3, 4, 5, 6, 7, 8, 9):
        bad = list(args)
        bad[k] = None
        assert lib.dll.lio_gn_rows_map(*bad) == -1, k
    for form in (-1, 3, 17):
        assert lib.dll.lio_gn_rows_map(*([form] + args[1:])) == -1, form
    for bad_T in (capi.TransformF.make((0.0, 0.0, float("nan"), 1.0), (0.0, 0.0, 0.0)), capi.TransformF.make((0.0, 0.0, 0.0, 1.0), (float("inf"), 0.0, 0.0))):
        bad = list(args)
        bad[5] = C.byref(bad_T)
        assert lib.dll.lio_gn_rows_map(*bad) == -1
    # m == 0 with null inputs is fine
    z = [0, None, 0, None, None, C.byref(T), None, None, nb.ctypes.data_as(i32), part.ctypes.data_as(f64)]
    assert lib.dll.lio_gn_rows_map(*z) == 0


# ------------------------------------------------------------------------------------------------ folds
NBLOCKS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 223, 224, 225, 255, 256, 257, 606, 1023, 1024, 1025]


@functools.lru_cache(maxsize=None)
def integer_partials(nblocks):
    rng = np.random.default_rng(7000 + nblocks)
    return rng.integers(0, 2 ** 20, (nblocks, 28)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ steps
def state(q=(0.0, 0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0), pad=0.0, converged=0, iters=0, degenerate=0, kz=0, nsel=0):
    s = np.zeros((), capi.GN_STATE)
    s["T"][:4], s["T"][4:7], s["T"][7] = q, t, pad
    s["converged"], s["iters"], s["degenerate"], s["kz"], s["nsel"] = converged, iters, degenerate, kz, nsel
    return s


class StepCase:
    def __init__(self, name, kind, family, sums, state_in, it, min_rows=0, left_update=0, check_X=True, expect=None):
        self.name, self.kind, self.family, self.sums, self.state_in, self.iter = name, kind, family, np.asarray(sums, np.float64), state_in, it
        self.min_rows, self.left_update, self.check_X, self.expect = min_rows, left_update, check_X, expect or {}

    def run(self, lib):
        return lib.gn_step(self.family, self.sums, self.state_in, self.iter, self.min_rows, self.left_update)

    def ref(self):
        return gn_ref.step_ref(self.family, self.sums, self.state_in, self.iter, self.min_rows, self.left_update)


def _orthogonal(rng):
    return np.linalg.qr(rng.normal(size=(6, 6)))[0]


def _spd(rng, lam):
    Q = _orthogonal(rng)
    A = (Q * np.asarray(lam)) @ Q.T
    return (A + A.T) / 2


def _well_conditioned():
    """rows of a synthetic problem: A = U diag(s) V^T with the singular values spread so that cond(A^T A) is 1e2 .. 1e4, b = A x + noise"""
    out = []
    k = 0
    for cond in (1e2, 1e3, 1e4):
        for rep in range(4):
            rng = np.random.default_rng(8000 + k)
            n = 400 + 37 * rep
            U = np.linalg.qr(rng.normal(size=(n, 6)))[0]
            sv = np.sqrt(cond) ** np.linspace(0, 1, 6) * 30.0            # eigenvalues of A^T A from 900 up: above both thresholds
            A = ((U * sv) @ _orthogonal(rng).T).astype(np.float32).astype(np.float64)
            x = rng.normal(0, 0.01, 6)
            b = (A @ x + rng.normal(0, 1e-3, n)).astype(np.float32).astype(np.float64)
            sums = gn_ref.sums_of(A.T @ A, A.T @ b, n)
            family = k % 2
            name = f"well_cond{int(cond)}_{rep}"
            out.append(StepCase(name, "well", family, sums, state(), rep % 2))          # the state is the step: X held to its bound
            if rep == 3:                                                # the same system away from the identity, updated on either side
                st = state(GENERAL[0], GENERAL[1])
                for left in (0, 1):
                    out.append(StepCase(f"{name}_general_{'left' if left else 'right'}", "side", 0, sums, st, rep % 2, left_update=left))
            k += 1
    return out


def _diag_system(x, count=500):
    d = np.array([400.0, 500.0, 600.0, 700.0, 800.0, 900.0])
    return gn_ref.sums_of(np.diag(d), d * np.asarray(x), count)


def _abort_cases():
    out = []
    for family in (0, 1):
        thr = gn_ref.ABORT[family]
        rng = np.random.default_rng(8100 + family)
        for r_side in (-1, +1):
            for t_side in (-1, +1):
                dr, dt = rng.normal(size=3), rng.normal(size=3)
                dr, dt = dr / np.linalg.norm(dr), dt / np.linalg.norm(dt)
                ang = thr * (1 + 0.02 * r_side)
                xr = dr * 2 * math.tan(math.radians(ang) / 2)
                xt = dt * thr * (1 + 0.02 * t_side) / 100
                name = f"abort_f{family}_r{'lo' if r_side < 0 else 'hi'}_t{'lo' if t_side < 0 else 'hi'}"
                out.append(StepCase(name, "decision", family, _diag_system(np.r_[xr, xt]), state(), 0,
                                    expect={"converged": int(r_side < 0 and t_side < 0), "kz": 0}))
        # each alone: the other far inside
        for which in ("r", "t"):
            for side in (-1, +1):
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                xr = d * 2 * math.tan(math.radians(thr * (1 + 0.02 * side)) / 2) if which == "r" else np.zeros(3)
                xt = d * thr * (1 + 0.02 * side) / 100 if which == "t" else np.zeros(3)
                out.append(StepCase(f"abort_f{family}_{which}_alone_{'lo' if side < 0 else 'hi'}", "decision", family, _diag_system(np.r_[xr, xt]), state(), 0,
                                    expect={"converged": int(side < 0), "kz": 0}))
    return out


def _spectrum(thr, kz):
    return [thr * 0.99] * kz + list(thr * 1.01 * 300.0 ** np.linspace(0, 1, 6 - kz))


def _spectrum_cases():
    out = []
    for family in (0, 1):
        thr = gn_ref.THRESHOLD[family]
        for kz in (0, 1, 2, 3):
            rng = np.random.default_rng(8200 + 10 * family + kz)
            A = _spd(rng, _spectrum(thr, kz))
            x = rng.normal(0, 0.2, 6)                                    # far outside the abort box: no second decision in play
            out.append(StepCase(f"spectrum_f{family}_kz{kz}", "decision", family, gn_ref.sums_of(A, A @ x, 500), state(), 0, expect={"kz": kz, "converged": 0}))
        # iter 3: the spectrum is not looked at; degenerate and kz are carried in
        rng = np.random.default_rng(8250 + family)
        A = _spd(rng, _spectrum(thr, 2))
        x = rng.normal(0, 0.2, 6)
        s = gn_ref.sums_of(A, A @ x, 500)
        out.append(StepCase(f"carried_f{family}_deg1_kz1", "decision", family, s, state(degenerate=1, kz=1), 3, expect={"kz": 1, "degenerate": 1}))
        out.append(StepCase(f"carried_f{family}_deg1_kz3", "decision", family, s, state(degenerate=1, kz=3), 3, expect={"kz": 3, "degenerate": 1}))
        out.append(StepCase(f"carried_f{family}_deg0_kz0", "decision", family, s, state(degenerate=0, kz=0), 3, expect={"kz": 0, "degenerate": 0}))
    return out


def _count_cases():
    x = np.array([0.01, -0.02, 0.015, 0.03, -0.01, 0.02])
    st = state(GENERAL[0], GENERAL[1], pad=-3.0)
    out = [StepCase("odom_nsel9", "decision", 1, _diag_system(x, 9), st, 2, expect={"stepped": False}),
           StepCase("odom_nsel10", "decision", 1, _diag_system(x, 10), state(pad=-3.0), 2, expect={"stepped": True}),
           StepCase("map_min50_nsel49", "decision", 0, _diag_system(x, 49), st, 2, min_rows=50, expect={"stepped": False}),
           StepCase("map_min50_nsel50", "decision", 0, _diag_system(x, 50), st, 2, min_rows=50, expect={"stepped": True}),
           StepCase("map_min0_nsel3", "decision", 0, _diag_system(x, 3), st, 2, min_rows=0, expect={"stepped": True}),
           StepCase("map_min50_nsel49_left", "decision", 0, _diag_system(x, 49), st, 2, min_rows=50, left_update=1, expect={"stepped": False})]
    return out


def _rank_deficient_cases():
    out = []
    for family in (0, 1):
        for j in (0, 2, 4):
            rng = np.random.default_rng(8300 + 10 * family + j)
            keep = [k for k in range(6) if k != j]
            Q = np.linalg.qr(rng.normal(size=(5, 5)))[0]
            B = (Q * (200.0 * 50.0 ** np.linspace(0, 1, 5))) @ Q.T
            A = np.zeros((6, 6))
            A[np.ix_(keep, keep)] = (B + B.T) / 2
            x = rng.normal(0, 0.2, 6)
            x[j] = 0
            out.append(StepCase(f"rank5_f{family}_col{j}", "rankdef", family, gn_ref.sums_of(A, A @ x, 500), state(), 2, expect={"zero": j}))
    return out


def _nan_cases():
    out = []
    for family in (0, 1):
        s = _diag_system([0.01, -0.02, 0.015, 0.03, -0.01, 0.02])
        s[21 + 4] = np.nan
        out.append(StepCase(f"nan_f{family}_one_rhs", "nan", family, s, state(GENERAL[0], GENERAL[1]), 1, check_X=False))
        s2 = s.copy()
        s2[:27] = np.nan
        out.append(StepCase(f"nan_f{family}_all", "nan", family, s2, state(GENERAL[0], GENERAL[1]), 1, check_X=False))
    return out


@functools.lru_cache(maxsize=None)
def step_cases():
    return tuple(_well_conditioned() + _abort_cases() + _spectrum_cases() + _count_cases() + _rank_deficient_cases() + _nan_cases())


def step_case(name):
    return next(c for c in step_cases() if c.name == name)


STEP_NAMES = [c.name for c in step_cases()]


def check_step_arguments(lib):
    import ctypes as C
    c = step_case("well_cond100_0")
    si, so = np.array(c.state_in, capi.GN_STATE).reshape(1), np.zeros(1, capi.GN_STATE)
    f64 = C.POINTER(C.c_double)
    args = [0, c.sums.ctypes.data_as(f64), si.ctypes.data, 0, 0, 0, so.ctypes.data]
    assert lib.dll.lio_gn_step(*args) == 0
    for k in (1, 2, 6):
        bad = list(args)
        bad[k] = None
        assert lib.dll.lio_gn_step(*bad) == -1, k
    for k, v in ((0, 2), (0, -1), (3, -1), (4, -1)):
        bad = list(args)
        bad[k] = v
        assert lib.dll.lio_gn_step(*bad) == -1, (k, v)
    for k, v in ((4, 50), (5, 1)):                  # the scan-to-scan step has neither a row gate of the caller's nor a left update
        bad = [1] + args[1:]
        bad[k] = v
        assert lib.dll.lio_gn_step(*bad) == -1, (k, v)
    nf = si.copy()
    nf["T"][0, 5] = np.nan
    bad = list(args)
    bad[2] = nf.ctypes.data
    assert lib.dll.lio_gn_step(*bad) == -1


def check_fold_arguments(lib):
    import ctypes as C
    p, s = np.ones((3, 28)), np.zeros(28)
    f64 = C.POINTER(C.c_double)
    assert lib.dll.lio_gn_fold(p.ctypes.data_as(f64), 3, 0, s.ctypes.data_as(f64)) == 0 and (s == 3).all()
    assert lib.dll.lio_gn_fold(None, 3, 0, s.ctypes.data_as(f64)) == -1
    assert lib.dll.lio_gn_fold(p.ctypes.data_as(f64), 3, 0, None) == -1
    assert lib.dll.lio_gn_fold(p.ctypes.data_as(f64), -1, 0, s.ctypes.data_as(f64)) == -1
    for wide in (-1, 2):
        assert lib.dll.lio_gn_fold(p.ctypes.data_as(f64), 3, wide, s.ctypes.data_as(f64)) == -1
    assert lib.dll.lio_gn_fold(None, 0, 1, s.ctypes.data_as(f64)) == 0 and (s == 0).all()


# ------------------------------------------------------------------------------------------------ one round of the newest-frame loop
ROUND_M = [1, 31, 32, 33, 63, 64, 65, 1025, 20000]


@functools.lru_cache(maxsize=None)
def round_scene(m):
    """a room of six walls (10 x 8 x 3 m) sampled at about 10 cm as the map, m queries on the walls with millimetres of noise, seen from a
    pose a few centimetres and a fraction of a degree off: most queries find five neighbours within a metre and a plane through them"""
    rng = np.random.default_rng(9000 + m)

    def on_walls(n):
        half = np.array([5.0, 4.0, 1.5])
        p = rng.uniform(-1, 1, (n, 3)) * half
        ax = rng.integers(0, 3, n)
        p[np.arange(n), ax] = np.where(rng.random(n) < 0.5, -1, 1) * half[ax]
        return p

    n_map = 40000
    map_xyzi = np.zeros((n_map, 4), np.float32)
    map_xyzi[:, :3] = on_walls(n_map) + rng.normal(0, 0.002, (n_map, 3))
    q = np.array([0.002, -0.001, 0.003, 1.0])
    q /= np.linalg.norm(q)
    q32, t32 = q.astype(np.float32), np.array([0.03, -0.02, 0.01], np.float32)
    world = on_walls(m) + rng.normal(0, 0.002, (m, 3))
    Rm = gn_ref.rot_of(q32)
    stack = np.zeros((m, 4), np.float32)
    stack[:, :3] = (world - t32.astype(np.float64)) @ Rm                 # R^T (x - t)
    return map_xyzi, stack, (tuple(float(v) for v in q32), tuple(float(v) for v in t32))


# ------------------------------------------------------------------------------------------------ rows of the scan-to-scan loop
PER_RING = 300


def _ring_neighbours(cloud, j, rng):
    """for points j of a ring_cloud (ring-major, azimuth ascending inside a ring): a neighbour on the same ring and the point of an adjacent
    ring nearest in azimuth"""
    ring = j // PER_RING
    same = np.where(j % PER_RING == PER_RING - 1, j - 1, j + 1)
    other_ring = np.where(ring == 15, ring - 1, ring + 1)
    az = np.arctan2(cloud[:, 1].astype(np.float64), cloud[:, 0].astype(np.float64)) % (2 * np.pi)
    adj = np.empty_like(j)
    for k, (jj, r) in enumerate(zip(j, other_ring)):
        a = az[r * PER_RING:(r + 1) * PER_RING]
        adj[k] = r * PER_RING + min(int(np.searchsorted(a, az[jj])), PER_RING - 1)
    return same, adj


#          name                 n_sharp n_flat iter no_deskew pose
_ODOM = [("odo_m0",             0,      0,     4,   True,     "general"),
         ("odo_m1",             1,      0,     4,   True,     "general"),
         ("odo_m63",            30,     33,    5,   True,     "general"),
         ("odo_m64",            32,     32,    4,   True,     "identity"),
         ("odo_m65",            33,     32,    5,   True,     "general"),
         ("odo_m255",           100,    155,   5,   True,     "general"),
         ("odo_m256",           128,    128,   4,   True,     "general"),
         ("odo_m257",           129,    128,   5,   True,     "identity"),
         ("odo_corner_only",    700,    0,     5,   True,     "general"),
         ("odo_surf_only",      0,      700,   5,   True,     "general"),
         ("odo_m16384",         4000,   12384, 5,   True,     "general"),
         ("odo_m16385",         4001,   12384, 4,   True,     "general"),
         ("odo_specials_iter4", 200,    200,   4,   True,     "general"),
         ("odo_specials_iter5", 200,    200,   5,   True,     "general"),
         ("odo_deskew_iter4",   500,    1500,  4,   False,    "general"),
         ("odo_deskew_iter5",   500,    1500,  5,   False,    "general")]
ODOM_NAMES = [c[0] for c in _ODOM]
ODOM_BITS = [c[0] for c in _ODOM if c[4]]
# dyadic points appended to the previous surf cloud: an exact plane z = 4 and a collinear triple
_PLANE = np.array([[1.0, 2.0, 4.0, 3.0], [3.0, 2.0, 4.0, 3.0], [1.0, 5.0, 4.0, 4.0]], np.float32)
_LINE3 = np.array([[2.0, 1.0, 1.0, 5.0], [4.0, 2.0, 2.0, 5.0], [8.0, 4.0, 4.0, 6.0]], np.float32)


class OdomCase:
    def __init__(self, name, n_sharp, n_flat, it, no_deskew, pose):
        from odom_corr_cases import _motion, ring_cloud
        self.name, self.iter, self.no_deskew = name, it, no_deskew
        rng = np.random.default_rng(5000 + ODOM_NAMES.index(name))
        self.last_corner = ring_cloud(rng, per_ring=PER_RING)
        ls = ring_cloud(rng, per_ring=PER_RING)
        n_ring = ls.shape[0]
        self.last_surf = np.concatenate([ls, _PLANE, _LINE3])
        q, p = _motion()
        if pose == "identity":
            q, p = np.array([0, 0, 0, 1.0]), np.zeros(3)
        self.q, self.p = q.astype(np.float32), p.astype(np.float32)

        def queries(cloud, n):
            j = rng.integers(0, n_ring, n)
            pts = cloud[j].astype(np.float64)
            # distances from millimetres to a metre and more: the weight 1 - 1.8 d of iterations >= 5 falls on both sides of 0.1
            pts[:, :3] += rng.normal(0, 1, (n, 3)) * rng.choice([0.003, 0.05, 0.3, 1.0], (n, 1))
            pts[:, 3] = np.trunc(pts[:, 3]) + rng.uniform(0, 0.1, n)
            return pts.astype(np.float32), j

        self.sharp, jc = queries(self.last_corner, n_sharp)
        self.flat, js = queries(self.last_surf[:n_ring], n_flat)
        _, adj_c = _ring_neighbours(self.last_corner, jc, rng)
        same_s, adj_s = _ring_neighbours(self.last_surf, js, rng)
        self.corner_idx = np.stack([jc, adj_c], axis=1).astype(np.int32).reshape(-1, 2)
        self.surf_idx = np.stack([js, same_s, adj_s], axis=1).astype(np.int32).reshape(-1, 3)
        self.special = {}
        if "specials" in name:
            c, s = self.corner_idx, self.surf_idx
            c[0:8] = -1                                         # nothing found
            c[64:70, 1] = -1                                    # closest alone
            s[0:8] = -1
            s[64:70, 1] = -1                                    # no second
            s[70:76, 2] = -1                                    # no third
            s[76:80, 1:] = -1                                   # closest alone
            self.sharp[10:14, :3] = self.last_corner[c[10:14, 0], :3]       # the query ON its closest point: ld2 == 0 exactly
            base = n_ring
            s[20:24] = (base, base + 1, base + 2)              # the dyadic plane z = 4 ...
            self.flat[20:24, :3] = [[2.0, 3.0, 4.0], [1.5, 2.5, 4.0], [1.0, 2.0, 4.0], [7.0, -3.0, 4.0]]   # ... and queries on it: pd2 == 0 exactly
            s[30:34] = (base + 3, base + 4, base + 5)          # a collinear triple: 0 / 0 in the normal
            self.flat[30:34, :3] = [[2.0, 1.5, 1.0], [3.0, 0.0, 2.0], [0.5, 0.5, 0.5], [5.0, 5.0, 1.0]]
            self.special = {"ld2_zero": np.arange(10, 14), "pd2_zero": n_sharp + np.arange(20, 24), "collinear": n_sharp + np.arange(30, 34)}

    def T(self):
        return capi.TransformF.make(tuple(float(x) for x in self.q), tuple(float(x) for x in self.p))

    def run(self, lib, corner_idx=None, surf_idx=None):
        return lib.gn_rows_odom(self.sharp, self.flat, self.last_corner, self.last_surf, self.corner_idx if corner_idx is None else corner_idx,
                                self.surf_idx if surf_idx is None else surf_idx, self.T(), self.iter, 0.1, self.no_deskew)

    def sel(self, lib):
        """TransformToStart of every query as `lib` computes it (lio_odom_correspondences' sel_out; the indices it finds are not used)"""
        return lib.odom_correspondences(self.sharp, self.flat, self.last_corner, self.last_surf, self.T(), 0.1, self.no_deskew)[2]

    def ref(self, sel):
        return gn_ref.odom_rows_ref(sel, np.concatenate([self.sharp, self.flat]), self.sharp.shape[0], self.last_corner, self.last_surf, self.corner_idx,
                                    self.surf_idx, self.q, self.p, self.iter)

    @property
    def nq(self):
        return self.sharp.shape[0] + self.flat.shape[0]


@functools.lru_cache(maxsize=None)
def get_odom(name):
    return OdomCase(*_ODOM[ODOM_NAMES.index(name)])


def odo_blocks(nq):
    """the rows launch of csrc/odometry.hip: a query per thread of 256, at most 64 blocks"""
    return max(1, min(-(-nq // 256), 64))


def check_odom_rows_arguments(lib):
    c = get_odom("odo_m65")
    assert c.run(lib)[0].shape == (65,)
    for which, col, val in (("corner", 0, c.last_corner.shape[0]), ("corner", 1, -2), ("surf", 2, c.last_surf.shape[0]), ("surf", 0, 10 ** 9)):
        ci, si = c.corner_idx.copy(), c.surf_idx.copy()
        (ci if which == "corner" else si)[3, col] = val        # outside its cloud
        with pytest_raises(capi.LioError):
            c.run(lib, ci, si)
    ci = c.corner_idx.copy()
    ci[5, 0] = -1                                               # a second point without a closest one
    with pytest_raises(capi.LioError):
        c.run(lib, ci, None)
    si = c.surf_idx.copy()
    si[5, 0] = -1
    with pytest_raises(capi.LioError):
        c.run(lib, None, si)
    for bad in (dict(scan_period=0.0), dict(scan_period=float("nan")), dict(iter=-1)):
        kw = dict(scan_period=0.1, iter=c.iter)
        kw.update(bad)
        with pytest_raises(capi.LioError):
            lib.gn_rows_odom(c.sharp, c.flat, c.last_corner, c.last_surf, c.corner_idx, c.surf_idx, c.T(), kw["iter"], kw["scan_period"], True)
    with pytest_raises(capi.LioError):
        lib.gn_rows_odom(c.sharp, c.flat, c.last_corner, c.last_surf, c.corner_idx, c.surf_idx, capi.TransformF.make((0.0, float("nan"), 0.0, 1.0), (0.0, 0.0, 0.0)),
                         c.iter, 0.1, True)
    # each required pointer null: LIO_ERR_ARG, nothing written
    import ctypes as C
    u8, f32, i32, f64 = (C.POINTER(t) for t in (C.c_uint8, C.c_float, C.c_int32, C.c_double))
    ok, rows = np.full(c.nq, 7, np.uint8), np.full((c.nq, 7), 7, np.float32)
    nb, part = np.full(1, 7, np.int32), np.full((64, 28), 7.0)
    T = c.T()
    args = [c.sharp.ctypes.data_as(f32), c.sharp.shape[0], c.flat.ctypes.data_as(f32), c.flat.shape[0], c.last_corner.ctypes.data_as(f32),
            c.last_corner.shape[0], c.last_surf.ctypes.data_as(f32), c.last_surf.shape[0], c.corner_idx.ctypes.data_as(i32), c.surf_idx.ctypes.data_as(i32),
            C.byref(T), 0.1, 1, c.iter, ok.ctypes.data_as(u8), rows.ctypes.data_as(f32), nb.ctypes.data_as(i32), part.ctypes.data_as(f64)]
    for k in (0, 2, 4, 6, 8, 9, 10, 14, 15, 16, 17):
        bad = list(args)
        bad[k] = None
        assert lib.dll.lio_gn_rows_odom(*bad) == -1, k
    assert (ok == 7).all() and (rows == 7).all() and nb[0] == 7 and (part == 7).all()
    assert lib.dll.lio_gn_rows_odom(*args) == 0 and nb[0] == odo_blocks(c.nq)
    ok, rows, part = get_odom("odo_m0").run(lib)
    assert ok.shape == (0,) and rows.shape == (0, 7) and part.shape == (1, 28) and not part.any()


def pytest_raises(exc):
    import pytest
    return pytest.raises(exc)
