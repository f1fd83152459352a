"""fp64 reference of the lidar factor's normal-equation moments (csrc/solve_kernels.h):

    S = sum_k rho'_k z_k z_k^T,  z = [w (x) [p; 1]; d] (13 values, padded to 16),  rho' = 1 / (1 + r^2),
    r = w . (R p + t) + d,  cost = 0.5 sum log(1 + r^2),  count = number of residuals,

per frame i of the optimised window at T_{pivot<-i} = (R, t).  Every entry is an exactly rounded sum (math.fsum) of the fp64
per-residual terms, so the reference carries no summation error of its own; `A` holds the same sums of |rho' z_a z_b|, the
scale an entry's rounding error is measured against.  The points and coefficients are what lio_est_get_features returns:
exactly the valid slots of a frame, the point of slot j being stack[j % M]."""
import math

import numpy as np

S_RTOL = 1e-12       # |S - S_ref| <= S_RTOL * A, entrywise
COST_RTOL = 1e-11    # |cost - cost_ref| <= COST_RTOL * cost_ref + COST_PER_RES * count
COST_PER_RES = 1e-15


def frame_terms(p, co, R, t):
    """Per-residual pieces: r, rho' and z (n x 13), in the order of the kernels' arithmetic (solve_kernels.hip: moment_z)."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    co = np.asarray(co, dtype=np.float64).reshape(-1, 4)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    w0, w1, w2, d = co[:, 0], co[:, 1], co[:, 2], co[:, 3]
    qx = R[0, 0] * px + R[0, 1] * py + R[0, 2] * pz + t[0]
    qy = R[1, 0] * px + R[1, 1] * py + R[1, 2] * pz + t[1]
    qz = R[2, 0] * px + R[2, 1] * py + R[2, 2] * pz + t[2]
    r = w0 * qx + w1 * qy + w2 * qz + d
    rho = 1.0 / (1.0 + r * r)
    one = np.ones_like(px)
    z = np.stack([w0 * px, w0 * py, w0 * pz, w0, w1 * px, w1 * py, w1 * pz, w1, w2 * px, w2 * py, w2 * pz, w2, d * one], axis=1)
    return r, rho, z


def frame_moments(p, co, R, t, drop=None, rho_scale=None):
    """-> dict(S (16 x 16), A (16 x 16), cost, count, r).  drop: index of a residual to leave out; rho_scale: (index, factor)
    multiplying one residual's rho' — both only to show that the comparison notices such changes."""
    r, rho, z = frame_terms(p, co, R, t)
    if rho_scale is not None:
        rho = rho.copy()
        rho[rho_scale[0]] *= rho_scale[1]
    if drop is not None:
        keep = np.ones(r.shape[0], dtype=bool)
        keep[drop] = False
        r, rho, z = r[keep], rho[keep], z[keep]
    S, A = np.zeros((16, 16)), np.zeros((16, 16))
    for a in range(13):
        za = rho * z[:, a]
        for b in range(a, 13):
            terms = za * z[:, b]
            S[a, b] = S[b, a] = math.fsum(terms.tolist())
            A[a, b] = A[b, a] = math.fsum(np.abs(terms).tolist())
    cost = 0.5 * math.fsum(np.log1p(r * r).tolist())
    return dict(S=S, A=A, cost=cost, count=int(r.shape[0]), r=r)


def split_rt(Rt):
    """(12,) R row-major then t -> (R 3 x 3, t 3)"""
    Rt = np.asarray(Rt, dtype=np.float64)
    return Rt[:9].reshape(3, 3), Rt[9:12]


def window_features(est):
    """[(points, coefficients)] of the optimised frames pivot+1 .. W (lio_est_get_features)"""
    W, Wo = est.W, est.cfg.opt_window_size
    out = []
    for i in range(W - Wo + 1, W + 1):
        pt, co, _ = est.features(i)
        out.append((pt, co))
    return out


def window_moments(feats, Rt_pass, **kw):
    """feats: window_features(); Rt_pass: (Wo, 12) -> [frame_moments] per frame"""
    return [frame_moments(p, c, *split_rt(Rt), **kw) for (p, c), Rt in zip(feats, Rt_pass)]


def compare(dev, ref):
    """dev: (258,) one frame's moments from a library; ref: frame_moments().  -> (max |S - S_ref| / A over the entries with A > 0,
    |cost - cost_ref|, problems: a list of strings, empty when the frame is within every bound)."""
    dev = np.asarray(dev, dtype=np.float64)
    S = dev[:256].reshape(16, 16)
    cost, count = float(dev[256]), float(dev[257])
    bad = []
    if np.any(S[13:, :] != 0.0) or np.any(S[:, 13:] != 0.0):
        bad.append("rows / columns 13..15 are not exactly 0")
    if not np.array_equal(S, S.T):
        bad.append("S is not exactly symmetric")
    if count != ref["count"]:
        bad.append(f"count {count} != {ref['count']}")
    if not np.all(np.isfinite(dev)):
        bad.append("not finite")
    err = np.abs(S - ref["S"])
    A = ref["A"]
    over = err > S_RTOL * A
    if np.any(over):
        a, b = np.argwhere(over)[0]
        bad.append(f"|S - S_ref| > {S_RTOL} A at ({a}, {b}): {err[a, b]:.3e} vs A {A[a, b]:.3e}")
    rel = float(np.max(np.where(A > 0, err / np.where(A > 0, A, 1.0), 0.0)))
    cerr = abs(cost - ref["cost"])
    if not cerr <= COST_RTOL * ref["cost"] + COST_PER_RES * ref["count"]:
        bad.append(f"cost {cost!r} vs {ref['cost']!r}: error {cerr:.3e}")
    return rel, cerr, bad


def assert_moments(dev_frames, ref_frames, what=""):
    """Every frame of one pass within the bounds -> (max S error / A, max cost error, max cost error / cost_ref)"""
    worst, worst_c, worst_cr = 0.0, 0.0, 0.0
    for f, (dev, ref) in enumerate(zip(dev_frames, ref_frames)):
        rel, cerr, bad = compare(dev, ref)
        assert not bad, f"{what} frame {f}: " + "; ".join(bad)
        worst, worst_c = max(worst, rel), max(worst_c, cerr)
        if ref["cost"] > 0:
            worst_cr = max(worst_cr, cerr / ref["cost"])
    return worst, worst_c, worst_cr


def frames_within(dev_frames, ref_frames):
    """True when every frame is within the bounds (the sensitivity checks expect False)"""
    return all(not compare(dev, ref)[2] for dev, ref in zip(dev_frames, ref_frames))


def perturbed_rt(Rt, rng, rot=0.05, trans=0.2):
    """(Wo, 12) -> a copy with every frame rotated by up to `rot` rad and moved by up to `trans` m (uniform per axis)"""
    out = np.array(Rt, dtype=np.float64, copy=True)
    for f in range(out.shape[0]):
        R, t = split_rt(out[f])
        v = rng.uniform(-1.0, 1.0, 3)
        v *= rot * rng.uniform(0.2, 1.0) / max(np.linalg.norm(v), 1e-300)
        th = np.linalg.norm(v)
        K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) / th
        dR = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
        out[f, :9] = (dR @ R).reshape(9)
        out[f, 9:] = t + rng.uniform(-trans, trans, 3)
    return out


def quat_xyzw_to_R(q):
    x, y, z, w = (float(v) for v in q)
    n = math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def window_rt(win, W, Wo):
    """T_{pivot<-i} (Wo, 12) of frames pivot+1 .. W from a get_window() result: T_li = T_wb_i T_lb^-1 (Estimator.cc:1448-1449),
    T_{pivot<-i} = T_l,pivot^-1 T_li.  Any pose is a valid input of the hooks; these are the window's own."""
    R_lb = quat_xyzw_to_R(win["q_lb"])
    t_lb = np.asarray(win["t_lb"], dtype=np.float64)

    def lidar_pose(i):
        R = np.asarray(win["Rs"][i]) @ R_lb.T
        return R, np.asarray(win["Ps"][i]) - R @ t_lb

    Rp, tp = lidar_pose(W - Wo)
    out = np.zeros((Wo, 12))
    for f in range(Wo):
        Ri, ti = lidar_pose(W - Wo + 1 + f)
        out[f, :9] = (Rp.T @ Ri).reshape(9)
        out[f, 9:] = Rp.T @ (ti - tp)
    return out


# ------------------------------------------------------------------------------------------------ windows for the hooks
def dataset(kind, pp_lib):
    """(dataset, surf clouds) of the W 15 / Wo 5 HDL-64E window (outdoor) or the W 8 / Wo 4 VLP-16 window (indoor); the clouds come
    from pp_lib's PointProcessor"""
    from lio_amd import pipeline, synth

    W = 15 if kind == "outdoor" else 8
    ds = synth.make_dataset(kind, W + 2, 0.3 if kind == "outdoor" else 0.2)
    clouds = [pipeline.feature_clouds(pp_lib, ds.lidar, f.scan)[0] for f in ds.frames]
    return ds, clouds


def make_window(lib, data, kind, keep=0, stacks=None, seed=3, build=True, **cfg_fields):
    """An estimator of `lib` holding the window of `data` (init_window: ground truth + the usual perturbation) with its local map and
    features built.  keep: keep_features (the newest frame then has rounds x M slots).  stacks: {frame: xyzi} replacing the
    voxel-filtered stacks of optimised frames before the map is built (slot counts of a frame = its stack's size).
    seed: of the perturbation; build: False leaves the map to a batch solve.
    cfg_fields: further lio_est_config fields (resident_moments, stream_sync)."""
    from lio_amd import capi, pipeline

    ds, clouds = data
    W, Wo = (15, 5) if kind == "outdoor" else (8, 4)
    cfg = pipeline.config_outdoor64(lib, W, Wo) if kind == "outdoor" else pipeline.config_indoor(lib, W, Wo)
    cfg.keep_features, cfg.prior_factor = keep, 1
    for k, v in cfg_fields.items():
        setattr(cfg, k, v)
    pipeline.set_extrinsic(cfg, ds)
    est = capi.Estimator(lib, cfg)
    pipeline.init_window(est, lib, ds, clouds, pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=seed)
    for i, xyzi in (stacks or {}).items():
        est.set_surf_stack(i, np.ascontiguousarray(xyzi, dtype=np.float32))
    if build:
        est.build_local_map()
    return est


def shape_stacks(lib, data, kind, counts, far=(), sparse_tail=()):
    """{frame: stack} for the optimised frames of the window: frame pivot+1+f keeps the first counts[f] points of its own
    voxel-filtered stack (the slots of a frame are its stack's points, so counts[f] is its slot count).  far: indices f whose points
    all move 1 km away from the map (every slot invalid).  sparse_tail: indices f whose slots from the last 256-slot boundary on
    are moved away except every 7th (sparse validity in the last chunk).  Only the newest frame (f = Wo - 1) may be moved: the
    others are part of the local map."""
    from lio_amd import pipeline

    ds, clouds = data
    W, Wo = (15, 5) if kind == "outdoor" else (8, 4)
    cfg = pipeline.config_outdoor64(lib, W, Wo) if kind == "outdoor" else pipeline.config_indoor(lib, W, Wo)
    leaf = cfg.surf_filter_size
    out = {}
    for f, n in enumerate(counts):
        i = W - Wo + 1 + f
        full = lib.voxel_grid(clouds[i], leaf)
        assert full.shape[0] >= n, (full.shape[0], n)
        s = np.array(full[:n], dtype=np.float32, copy=True)
        if f in far:
            s[:, :3] += 1000.0
        if f in sparse_tail and n > 256:
            tail = np.arange((n - 1) // 256 * 256, n)
            s[tail[tail % 7 != 0], :3] += 1000.0
        out[i] = s
    return out


def make_passes(Rt, seed, offsets=(0.0, 1.0, 1e3, 1e30, 1e60)):
    """The passes the hooks are driven with: the window's own poses, three perturbed ones (up to 0.05 rad / 0.2 m: rho' really
    changes), the first perturbed one again (its result must be bit-identical to the first time), and the own poses moved by
    offsets[f] m along every axis in frame f (residuals from ~1e-6 m up to 1e60 m: rsqrt_1p's range and LogProduct's rescaling)."""
    rng = np.random.default_rng(seed)
    p1, p2, p3 = (perturbed_rt(Rt, rng) for _ in range(3))
    big = np.array(Rt, dtype=np.float64, copy=True)
    big[:, 9:] += np.asarray(offsets[:big.shape[0]])[:, None]
    return np.stack([Rt, p1, p2, p3, p1, big])
