"""The cases the two five-neighbour fits are pinned on (tests/test_fit_five.py on the CPU: oracle and references;
tests/test_gpu_fit_five.py: the product).  Seeded, numpy only.  A case: name, kind ("plane": run in forms 0, 1, 2; "line": form 3), the
hook's inputs, what it is there for (family, straddle = the decision it straddles, exempt = held to product == oracle and "finite or
invalid" only: the rank-threshold and exactly-degenerate patches, where rounding decides the rank cut of the plane fit and whether five
identical points have a direction at all), and the cap on what the fp64 comparison may leave out.
The names are known at import; the cases are built on first use, their references on first use of each, and kept."""
import functools

import numpy as np

import fit_ref

MM, MP = 1.0, 0.2            # min_match_sq_dis, min_plane_dis of the product's defaults
CAP = 0.02                   # every family that does not straddle a threshold
CAP_STRADDLE = 0.40          # a straddler family asserts at least 30 % on each side
IDENT = (0.0, 0.0, 0.0, 1.0)


class Case:
    def __init__(self, name, kind, family, nbr, fifth, stack, q=IDENT, t=(0, 0, 0), pz=None, straddle=None, exempt=False, bad=None):
        self.name, self.kind, self.family, self.straddle, self.exempt = name, kind, family, straddle, exempt
        self.nbr = np.ascontiguousarray(nbr, np.float32).reshape(-1, 5, 3)
        self.m = self.nbr.shape[0]
        self.fifth = np.ascontiguousarray(fifth, np.float32).reshape(self.m)
        self.stack = np.ascontiguousarray(stack, np.float32).reshape(self.m, 4)
        self.q, self.t = tuple(float(np.float32(v)) for v in q), tuple(float(np.float32(v)) for v in t)
        z = fit_ref.quat_rotate(self.q, np.array([[0.0, 0.0, 10.0]]))[0] + np.asarray(self.t)
        self.pz = tuple(float(np.float32(v)) for v in (z if pz is None else pz))   # forms 1 - 3: the apex a fixed transform would give
        self.bad = np.zeros(self.m, bool) if bad is None else bad                    # queries with a NaN / inf input
        self.cap = CAP_STRADDLE if straddle else CAP
        self.forms = (0, 1, 2) if kind == "plane" else (3,)
        self._ref = {}

    def ref(self, form):
        if form not in self._ref:
            if form == 3:
                self._ref[form] = fit_ref.line_ref(self.nbr, self.fifth, self.stack, self.q, self.t, self.pz, MM)
            else:
                self._ref[form] = fit_ref.plane_ref(self.nbr, self.fifth, self.stack, self.q, self.t, self.pz, form, MM, MP)
        return self._ref[form]

    def transform(self):
        from lio_amd import capi
        T = capi.TransformF()
        for k in range(4):
            T.q[k] = self.q[k]
        for k in range(3):
            T.p[k] = self.t[k]
        return T

    def run(self, lib, form, nbr=None, fifth=None, stack=None):
        return lib.fit_five(form, self.nbr if nbr is None else nbr, self.fifth if fifth is None else fifth, self.stack if stack is None else stack,
                            self.transform(), self.pz, MM, MP)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rand_quat(rng):
    return tuple(_unit(rng.normal(size=4)))


def _dirs(rng, m, q, lo=50.0, hi=130.0):
    """unit directions from the sensor whose angle to the sensor's z axis lies in [lo, hi] degrees (the field of view is 30 .. 150)"""
    th = np.radians(rng.uniform(lo, hi, m))
    ph = rng.uniform(0, 2 * np.pi, m)
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
    return fit_ref.quat_rotate(q, d)


def _stack_of(sel, q, t):
    """the sensor-frame points whose image under (q, t) is sel (up to the rounding of the fp32 stack)"""
    qi = (-q[0], -q[1], -q[2], q[3])
    po = fit_ref.quat_rotate(qi, np.asarray(sel, np.float64) - np.asarray(t, np.float64))
    return np.concatenate([po, np.zeros((po.shape[0], 1))], axis=1)


def _frame(n):
    """two unit vectors spanning the plane of normal n (rows)"""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    u = _unit(np.cross(n, a))
    return u, np.cross(n, u)


def _normals(rng, c0, axis_aligned):
    """plane normals that keep the plane away from the origin: |n . c0| >= 0.3 |c0|"""
    ch = _unit(c0)
    m = c0.shape[0]
    if axis_aligned:
        k = np.argmax(np.abs(ch), axis=1)
        n = np.zeros((m, 3))
        n[np.arange(m), k] = 1.0
        return n
    n = _unit(rng.normal(size=(m, 3)))
    for _ in range(50):
        badn = np.abs((n * ch).sum(axis=1)) < 0.3
        if not badn.any():
            break
        n[badn] = _unit(rng.normal(size=(int(badn.sum()), 3)))
    return n


def _patch(rng, c0, n, sigma, half=0.4):
    """five points around c0 in the plane of normal n, spread +-half, with out-of-plane noise sigma (rows)"""
    m = c0.shape[0]
    u, v = _frame(n)
    ab = rng.uniform(-half, half, (m, 5, 2))
    ab[:, :3] = np.array([[-0.35, -0.3], [0.35, -0.25], [0.0, 0.38]]) * (half / 0.4) + rng.uniform(-0.03, 0.03, (m, 3, 2))   # never near-collinear
    o = rng.normal(size=(m, 5)) * np.asarray(sigma).reshape(-1, 1)
    return c0[:, None] + ab[..., :1] * u[:, None] + ab[..., 1:] * v[:, None] + o[..., None] * n[:, None]


def _plane_case(name, family, seed, m, rng_range, sigma, axis_aligned=False, height=None, **kw):
    rng = np.random.default_rng(seed)
    q = _rand_quat(rng)
    t = rng.uniform(-0.3, 0.3, 3)
    r = np.broadcast_to(np.asarray(rng_range, np.float64), (m,)) if np.ndim(rng_range) else np.full(m, float(rng_range))
    c0 = np.asarray(t) + r[:, None] * _dirs(rng, m, q)
    n = _normals(rng, c0, axis_aligned)
    sig = rng.uniform(0, 1, m) * sigma
    nbr = _patch(rng, c0, n, sig)
    h = rng.uniform(0.02, 0.12, m) * rng.choice([-1.0, 1.0], m) if height is None else height(rng, m)
    u, v = _frame(n)
    sel = c0 + rng.uniform(-0.2, 0.2, (m, 1)) * u + rng.uniform(-0.2, 0.2, (m, 1)) * v + h[:, None] * n
    return Case(name, "plane", family, nbr, np.full(m, 0.5), _stack_of(sel, q, t), q, t, **kw)


def _with_bad(c, rng_seed):
    """NaN / inf planted in one neighbour coordinate or in the query of every 37th query: every wave of 64 keeps good ones"""
    rng = np.random.default_rng(rng_seed)
    nbr, stack = c.nbr.copy(), c.stack.copy()
    bad = np.zeros(c.m, bool)
    for k, i in enumerate(range(5, c.m, 37)):
        val = [np.nan, np.inf, -np.inf][k % 3]
        if (k // 3) % 2 == 0:
            nbr[i, rng.integers(5), rng.integers(3)] = val
        else:
            stack[i, rng.integers(3)] = val
        bad[i] = True
    return Case(c.name + "_nonfinite", c.kind, "nonfinite", nbr, c.fifth, stack, c.q, c.t, c.pz, bad=bad)


def _dyadic(rng, shape, lo, hi, step=0.125):
    return rng.integers(int(lo / step), int(hi / step) + 1, shape) * step


# ------------------------------------------------------------------------------------------------ plane families
def _plane_cases():
    out = []
    for k, r in enumerate((1, 10, 50, 100, 400)):
        out.append(_plane_case(f"noisy_r{r}", f"noisy_r{r}", 100 + k, 600, r, 0.05))
        out.append(_plane_case(f"noisy_axis_r{r}", f"noisy_axis_r{r}", 110 + k, 600, r, 0.05, axis_aligned=True))
    # axis-aligned, dyadic, the x and y columns the same multiset of numbers: two column norms exactly equal in the pivot search
    rng = np.random.default_rng(120)
    m = 400
    xs = _dyadic(rng, (m, 5), 2.0, 4.0)
    xs[:, :3] = np.array([2.0, 4.0, 3.0]) + _dyadic(rng, (m, 3), 0.0, 0.25)
    perm = np.array([1, 2, 0, 4, 3])
    nbr = np.stack([xs, xs[:, perm], np.repeat(_dyadic(rng, (m, 1), 1.0, 2.0), 5, axis=1)], axis=2)
    sel = np.stack([xs.mean(axis=1), xs.mean(axis=1), nbr[:, 0, 2] + rng.uniform(0.02, 0.1, m) * rng.choice([-1.0, 1.0], m)], axis=1)
    out.append(Case("equal_column_norms", "plane", "equal_column_norms", nbr, np.full(m, 0.5), _stack_of(sel, IDENT, (0, 0, 0))))
    # planes passing 1e-3 .. 1e-1 m from the origin: |x| = 1 / d is large, the right-hand side -1 nearly unreachable
    rng = np.random.default_rng(121)
    m = 600
    q = _rand_quat(rng)
    c0 = rng.uniform(1.5, 3.0, (m, 1)) * _dirs(rng, m, q)
    dist = 10.0 ** rng.uniform(-3, -1, m)
    nperp = _unit(np.cross(c0, rng.normal(size=(m, 3))))
    n = _unit(nperp + (dist / np.linalg.norm(c0, axis=1))[:, None] * _unit(c0))
    nbr = _patch(rng, c0, n, np.zeros(m))
    u, v = _frame(n)
    sel = c0 + rng.uniform(-0.2, 0.2, (m, 1)) * u + rng.uniform(0.03, 0.1, (m, 1)) * n
    out.append(Case("plane_through_origin", "plane", "plane_through_origin", nbr, np.full(m, 0.5), _stack_of(sel, q, (0, 0, 0)), q))
    # ---- exempt: the rank cut is rounding-determined
    rng = np.random.default_rng(122)
    m = 640
    c0 = rng.uniform(2.0, 4.0, (m, 1)) * _dirs(rng, m, IDENT)
    u = _unit(rng.normal(size=(m, 3)))
    w = _unit(np.cross(u, rng.normal(size=(m, 3))))
    a = np.array([-0.4, -0.2, 0.0, 0.2, 0.4])
    b = np.array([1.0, -2.0, 2.0, -2.0, 1.0])
    eps = 10.0 ** rng.uniform(-9, -3, m)
    nbr = c0[:, None] + a[None, :, None] * u[:, None] + (eps[:, None] * b[None, :])[..., None] * w[:, None]
    out.append(Case("near_collinear_sweep", "plane", "near_collinear_sweep", nbr, np.full(m, 0.5), _stack_of(c0 + 0.05 * w, IDENT, (0, 0, 0)), exempt=True))
    base = _dyadic(rng, (m, 3), 1.0, 3.0)
    step = _dyadic(rng, (m, 3), 0.125, 0.5)
    nbr = base[:, None] + np.arange(5)[None, :, None] * step[:, None]
    out.append(Case("exactly_collinear", "plane", "exactly_collinear", nbr, np.full(m, 0.5), _stack_of(base + 0.05, IDENT, (0, 0, 0)), exempt=True))
    good = _plane_case("tmp", "tmp", 123, m, 3.0, 0.0)
    for dup in (2, 3, 4, 5):
        nbr = good.nbr.copy()
        nbr[:, 5 - dup:] = nbr[:, 5 - dup:5 - dup + 1]
        out.append(Case(f"duplicates_{dup}", "plane", f"duplicates_{dup}", nbr, good.fifth, good.stack, good.q, good.t, exempt=True))
    # ---- straddlers, one per decision
    g = _plane_case("tmp", "tmp", 130, 1000, 3.0, 0.01)
    mm32 = np.float32(MM)
    vals = np.array([np.nextafter(mm32, np.float32(0)), mm32, np.nextafter(mm32, np.float32(2)), np.float32(np.inf)], np.float32)
    fifth = vals[np.array([0, 0, 1, 2, 3])[np.arange(g.m) % 5]]
    out.append(Case("straddle_fifth", "plane", "straddle_fifth", g.nbr, fifth, g.stack, g.q, g.t, straddle="fifth"))
    out.append(_straddle_plane_dis())
    out.append(_straddle_score())
    out.append(_straddle_fov("fov_lo", 30.0, 132))
    out.append(_straddle_fov("fov_hi", 150.0, 133))
    # the sign rule of the mapping modes: pd2 positive, negative ...
    out.append(_plane_case("sign_both", "sign_both", 134, 600, 5.0, 0.01,
                           height=lambda rng, m: rng.uniform(0.05, 0.3, m) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)))
    # ... and exactly zero: a query lying on a dyadic-coordinate plane z = const
    rng = np.random.default_rng(135)
    m = 320
    xy = _dyadic(rng, (m, 5, 2), 1.0, 3.0)
    xy[:, :3] = np.array([[1.0, 1.0], [3.0, 1.25], [2.0, 3.0]]) + _dyadic(rng, (m, 3, 2), 0.0, 0.25)
    z = _dyadic(rng, (m, 1), 0.5, 2.0)
    nbr = np.concatenate([xy, np.repeat(z[:, None], 5, axis=1)], axis=2)
    sel = np.concatenate([xy.mean(axis=1).round(2), z], axis=1)
    out.append(Case("pd2_zero", "plane", "pd2_zero", nbr, np.full(m, 0.5), _stack_of(sel, IDENT, (0, 0, 0))))
    # sel at the origin: the score divides by |sel|^(1/2) = 0
    g = _plane_case("tmp", "tmp", 136, 128, 2.0, 0.0)
    stack = g.stack.copy()
    stack[::2] = 0
    out.append(Case("sel_at_origin", "plane", "sel_at_origin", g.nbr, g.fifth, stack, IDENT, (0, 0, 0)))
    out.append(_with_bad(_plane_case("plane", "tmp", 137, 300, 5.0, 0.02), 138))
    for mm_ in (0, 1, 63, 64, 65):
        out.append(_plane_case(f"plane_m{mm_}", "ragged_m", 140 + mm_, mm_, 5.0, 0.02))
    out.append(_plane_case("plane_m100000", "large_m", 141, 100000, np.random.default_rng(142).uniform(1, 60, 100000), 0.03))
    return out


def _straddle_plane_dis():
    """the farthest neighbour's distance to the fitted plane at min_plane_dis (1 +- 3 .. 25 %)"""
    rng = np.random.default_rng(131)
    m = 1000
    g = _plane_case("tmp", "tmp", 131, m, 3.0, 0.0)
    P = g.nbr.astype(np.float64)
    c0 = P.mean(axis=1)
    n = _unit(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]))
    pat = rng.normal(size=(m, 5))
    target = MP * (1 + rng.uniform(0.03, 0.25, m) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0))
    scale = np.full(m, 0.1)
    for _ in range(6):
        nb = (P + (scale[:, None] * pat)[..., None] * n[:, None]).astype(np.float32)
        r = fit_ref.plane_ref(nb, g.fifth, g.stack, g.q, g.t, g.pz, 0, MM, MP)
        scale *= target / r.max_pd
    nb = (P + (scale[:, None] * pat)[..., None] * n[:, None]).astype(np.float32)
    r = fit_ref.plane_ref(nb, g.fifth, g.stack, g.q, g.t, g.pz, 0, MM, MP)
    sel = c0 + r.n * (0.05 - ((r.n * c0).sum(axis=1) + r.d))[:, None]          # 5 cm off the fitted plane: the score is far from 0.1
    return Case("straddle_plane_dis", "plane", "straddle_plane_dis", nb, g.fifth, _stack_of(sel, g.q, g.t), g.q, g.t, straddle="plane")


def _straddle_score():
    """s = 1 - 0.9 |pd2| / |sel|^(1/2) at 0.1 (+- 0.01 .. 0.08): the query |sel|^(1/2) above or below its plane"""
    rng = np.random.default_rng(139)
    m = 1000
    g = _plane_case("tmp", "tmp", 139, m, 3.0, 0.0)
    r = g.ref(0)
    s_t = 0.1 + rng.uniform(0.01, 0.08, m) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    sg = rng.choice([-1.0, 1.0], m)
    foot = r.sel - r.pd2[:, None] * r.n
    h = np.full(m, 1.7)
    for _ in range(30):
        sel = foot + (sg * h)[:, None] * r.n
        h = (1 - s_t) / 0.9 * np.sqrt(np.linalg.norm(sel, axis=1))
    sel = foot + (sg * h)[:, None] * r.n
    return Case("straddle_score", "plane", "straddle_score", g.nbr, g.fifth, _stack_of(sel, g.q, g.t), g.q, g.t, straddle="score")


def _straddle_fov(which, edge_deg, seed, kind="plane"):
    """queries whose angle to the sensor's z axis is edge (1 +- 0.5 .. 5 %): 30 degrees is check1's edge, 150 degrees check2's"""
    rng = np.random.default_rng(seed)
    m = 1000
    q = _rand_quat(rng)
    t = rng.uniform(-0.3, 0.3, 3)
    ang = edge_deg + rng.uniform(0.3, 2.5, m) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    ph = rng.uniform(0, 2 * np.pi, m)
    th = np.radians(ang)
    d = fit_ref.quat_rotate(q, np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1))
    sel = t + rng.uniform(2.0, 6.0, (m, 1)) * d
    if kind == "line":
        u = _unit(rng.normal(size=(m, 3)))
        nbr = _segment(rng, sel - 0.05 * _unit(np.cross(u, d)), u, 0.0)
    else:
        n = _normals(rng, sel, False)
        nbr = _patch(rng, sel - 0.05 * n, n, np.zeros(m))
    return Case(f"straddle_{which}" + ("_line" if kind == "line" else ""), kind, f"straddle_{which}", nbr, np.full(m, 0.5), _stack_of(sel, q, t), q, t,
                straddle=which)


# ------------------------------------------------------------------------------------------------ line families
A5 = np.array([-2.0, -1.0, 0.0, 1.0, 2.0]) * 0.15          # along the line
B5 = np.array([2.0, -1.0, -2.0, -1.0, 2.0])                # sum 0 and orthogonal to A5: a second, independent direction of spread


def _segment(rng, c0, u, sigma):
    m = c0.shape[0]
    a = A5[None, :] + rng.uniform(-0.02, 0.02, (m, 5))
    return c0[:, None] + a[..., None] * u[:, None] + rng.normal(size=(m, 5, 3)) * np.asarray(sigma).reshape(-1, 1, 1)


def _line_case(name, family, seed, m, r, sigma, axis_aligned=False, **kw):
    rng = np.random.default_rng(seed)
    q = _rand_quat(rng)
    t = rng.uniform(-0.3, 0.3, 3)
    c0 = t + np.broadcast_to(np.asarray(r, np.float64), (m,))[:, None] * _dirs(rng, m, q)
    if axis_aligned:
        u = np.eye(3)[rng.integers(3, size=m)]
        c0 = np.round(c0 * 8) / 8          # 5 c0 is exact in fp32: the centroid's off-axis coordinates are c0's, the off-diagonals zero
    else:
        u = _unit(rng.normal(size=(m, 3)))
    nbr = _segment(rng, c0, u, rng.uniform(0, 1, m) * sigma) if not axis_aligned else c0[:, None] + (A5[None, :] + _dyadic(rng, (m, 5), 0, 0.0625, 1 / 64))[..., None] * u[:, None]
    w = _unit(np.cross(u, rng.normal(size=(m, 3))))
    sel = c0 + rng.uniform(0.25, 0.45, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1)) * u + rng.uniform(0.05, 0.3, (m, 1)) * w
    return Case(name, "line", family, nbr, np.full(m, 0.5), _stack_of(sel, q, t), q, t, **kw)


def _line_cases():
    out = []
    for k, r in enumerate((1, 10, 50, 100, 400)):
        out.append(_line_case(f"line_noisy_r{r}", f"line_noisy_r{r}", 200 + k, 600, r, 0.02))
    out.append(_line_case("line_axis_aligned", "line_axis_aligned", 210, 600, np.random.default_rng(211).uniform(1, 100, 600), 0.0, axis_aligned=True))
    # eigenvalue ratio l2 / l1 swept across 3 (+- 5 .. 40 %): spread k B5 along a second direction
    rng = np.random.default_rng(212)
    m = 1000
    g = _line_case("tmp", "tmp", 212, m, 4.0, 0.0)
    u = _unit(rng.normal(size=(m, 3)))
    w = _unit(np.cross(u, rng.normal(size=(m, 3))))
    ratio = 3.0 * (1 + rng.uniform(0.05, 0.4, m) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0))
    k = np.sqrt((A5 ** 2).sum() / (ratio * (B5 ** 2).sum()))
    c0 = g.nbr.astype(np.float64).mean(axis=1)
    nbr = c0[:, None] + A5[None, :, None] * u[:, None] + (k[:, None] * B5[None, :])[..., None] * w[:, None]
    sel = c0 + 0.3 * u + 0.1 * np.cross(u, w)
    out.append(Case("straddle_ratio", "line", "straddle_ratio", nbr, g.fifth, _stack_of(sel, g.q, g.t), g.q, g.t, straddle="ratio"))
    out.append(_straddle_fov("fov_lo", 30.0, 213, kind="line"))
    out.append(_straddle_fov("fov_hi", 150.0, 214, kind="line"))
    g = _line_case("tmp", "tmp", 215, 1000, 3.0, 0.0)
    mm32 = np.float32(MM)
    vals = np.array([np.nextafter(mm32, np.float32(0)), mm32, np.nextafter(mm32, np.float32(2)), np.float32(np.inf)], np.float32)
    out.append(Case("straddle_fifth_line", "line", "straddle_fifth", g.nbr, vals[np.array([0, 0, 1, 2, 3])[np.arange(g.m) % 5]], g.stack, g.q, g.t,
                    straddle="fifth"))
    # exactly rank-1 covariance on dyadic coordinates; a query exactly on the line is every fourth one (n2 == 0 branch)
    rng = np.random.default_rng(216)
    m = 400
    base = _dyadic(rng, (m, 3), 1.0, 3.0)
    base[:, 2] = _dyadic(rng, m, -1.0, 1.0)
    ax = rng.integers(2, size=m)
    u = np.eye(3)[ax]
    a = np.array([-0.5, -0.25, 0.0, 0.25, 0.5])
    nbr = base[:, None] + a[None, :, None] * u[:, None]
    off = np.where((np.arange(m) % 4 == 0)[:, None], 0.0, np.eye(3)[(ax + 1) % 3] * _dyadic(rng, (m, 1), 0.125, 0.25))
    sel = base + 0.375 * u + off
    out.append(Case("rank1_dyadic", "line", "rank1_dyadic", nbr, np.full(m, 0.5), _stack_of(sel, IDENT, (0, 0, 0))))
    # discs (l2 == l1: a regular pentagon), isotropic blobs
    rng = np.random.default_rng(217)
    m = 400
    g = _line_case("tmp", "tmp", 217, m, 3.0, 0.0)
    c0 = g.nbr.astype(np.float64).mean(axis=1)
    n = _unit(rng.normal(size=(m, 3)))
    e1, e2 = _frame(n)
    ang = 2 * np.pi * np.arange(5) / 5
    nbr = c0[:, None] + 0.3 * (np.cos(ang)[None, :, None] * e1[:, None] + np.sin(ang)[None, :, None] * e2[:, None])
    out.append(Case("disc", "line", "disc", nbr, g.fifth, g.stack, g.q, g.t))
    nbr = c0[:, None] + 0.15 * rng.normal(size=(m, 5, 3))
    out.append(Case("blob", "line", "blob", nbr, g.fifth, g.stack, g.q, g.t))
    nbr = np.repeat(c0[:, None], 5, axis=1)
    out.append(Case("line_identical", "line", "line_identical", nbr, g.fifth, g.stack, g.q, g.t, exempt=True))
    out.append(_with_bad(_line_case("line", "tmp", 218, 300, 5.0, 0.01), 219))
    for mm_ in (0, 1, 63, 64, 65):
        out.append(_line_case(f"line_m{mm_}", "ragged_m", 220 + mm_, mm_, 5.0, 0.01))
    out.append(_line_case("line_m100000", "large_m", 221, 100000, np.random.default_rng(222).uniform(1, 60, 100000), 0.01))
    return out


PLANE_NAMES = tuple([f"noisy{a}_r{r}" for r in (1, 10, 50, 100, 400) for a in ("", "_axis")] +
                    ["equal_column_norms", "plane_through_origin", "near_collinear_sweep", "exactly_collinear", "duplicates_2", "duplicates_3",
                     "duplicates_4", "duplicates_5", "straddle_fifth", "straddle_plane_dis", "straddle_score", "straddle_fov_lo", "straddle_fov_hi",
                     "sign_both", "pd2_zero", "sel_at_origin", "plane_nonfinite", "plane_m0", "plane_m1", "plane_m63", "plane_m64", "plane_m65",
                     "plane_m100000"])
LINE_NAMES = tuple([f"line_noisy_r{r}" for r in (1, 10, 50, 100, 400)] +
                   ["line_axis_aligned", "straddle_ratio", "straddle_fov_lo_line", "straddle_fov_hi_line", "straddle_fifth_line", "rank1_dyadic",
                    "disc", "blob", "line_identical", "line_nonfinite", "line_m0", "line_m1", "line_m63", "line_m64", "line_m65", "line_m100000"])
EXEMPT = ("near_collinear_sweep", "exactly_collinear", "duplicates_2", "duplicates_3", "duplicates_4", "duplicates_5", "line_identical")
NAMES = PLANE_NAMES + LINE_NAMES                                   # known without building anything: importing this module is free
RUNS = tuple((n, f) for n in PLANE_NAMES for f in (0, 1, 2)) + tuple((n, 3) for n in LINE_NAMES)   # every (case, form) the hook is run on


@functools.lru_cache(maxsize=None)
def _all():
    """the cases, built on first use"""
    cs = _plane_cases() + _line_cases()
    d = {c.name: c for c in cs}
    assert tuple(d) == NAMES, [n for n in d if n not in NAMES] + [n for n in NAMES if n not in d]
    assert tuple(n for n in NAMES if d[n].exempt) == EXEMPT
    return d


def get(name):
    return _all()[name]


def check_null_pointers(lib, c):
    """the hook's argument checks on library `lib`: a null pointer in any pointer argument is LIO_ERR_ARG (-1), the full call LIO_OK"""
    import ctypes as C

    def f(a):
        return a.ctypes.data_as(C.POINTER(C.c_float))

    T = c.transform()
    v, co, sc, ab = np.zeros(c.m, np.uint8), np.zeros((c.m, 4), np.float32), np.zeros(c.m, np.float32), np.zeros((c.m, 4), np.float32)
    pz = np.zeros(3, np.float32)
    args = [0, f(c.nbr), f(c.fifth), f(c.stack), c.m, C.byref(T), f(pz), MM, MP, v.ctypes.data_as(C.POINTER(C.c_uint8)), f(co), f(sc), f(ab)]
    assert lib.dll.lio_fit_five(*args) == 0
    for k in (1, 2, 3, 5, 6, 9, 10, 11, 12):
        bad = list(args)
        bad[k] = None
        assert lib.dll.lio_fit_five(*bad) == -1, k
