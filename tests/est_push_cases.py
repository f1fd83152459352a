"""Cases of tests/test_gpu_est_push_batch.py and tests/test_est_push_batch_abi.py (include/lio_est_push_batch.h): small indoor windows built
twice from one seed (twin handles), the crafted clouds of the chain's edges, and what is compared — every quantity as its uint32 / uint64 view,
so that equal means equal bits (a NaN equals itself, -0 differs from +0)."""
import functools

import numpy as np

from lio_amd import capi, pipeline, synth

IDENT = ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0])
SPECS = [  # kind, W, Wo, keep_features, opt_extrinsic, seed (tests/test_gpu_batch.py: SPECS)
    ("indoor", 4, 2, 0, 1, 3),
    ("indoor", 6, 3, 1, 1, 5),
    ("indoor", 5, 2, 0, 0, 7),
]
N_FRAMES = 6 + 10          # the largest window + the steps of the longest test
LEAF = 0.4                 # surf_filter_size of config_indoor


@functools.lru_cache(maxsize=None)
def data():
    """the indoor sequence: (dataset, per frame (surf, corner), per frame a thinned full-resolution sweep)"""
    hip = capi.load_hip()
    ds = synth.make_dataset("indoor", N_FRAMES, 0.2)
    clouds, fulls = [], []
    for f in ds.frames:
        pp = capi.PointProcessor(hip, ds.lidar.lower_deg, ds.lidar.upper_deg, ds.lidar.rings)
        pp.process(f.scan)
        clouds.append((pp.cloud(capi.PointProcessor.LESS_FLAT), pp.cloud(capi.PointProcessor.LESS_SHARP)))
        fulls.append(np.ascontiguousarray(pp.cloud(capi.PointProcessor.RINGS)[::14][:2049]))
    return ds, clouds, fulls


def config(hip, W, Wo, keep=0, optex=1, deskew="cutoff", device_solve=0, surf_leaf=None):
    """deskew: "cutoff" (cutoff_deskew = 1: filtered, not de-skewed), "imu" (enable_deskew = 1, cutoff_deskew = 0: de-skewed by the IMU poses,
    then filtered), "off" (both switches off: the clouds go in as they are)"""
    ds = data()[0]
    cfg = pipeline.config_indoor(hip, W, Wo)
    cfg.keep_features, cfg.prior_factor, cfg.opt_extrinsic, cfg.device_solve = keep, 1, optex, device_solve
    cfg.enable_deskew, cfg.cutoff_deskew = {"cutoff": (1, 1), "imu": (1, 0), "off": (0, 0)}[deskew]
    if surf_leaf is not None:
        cfg.surf_filter_size = surf_leaf
    pipeline.set_extrinsic(cfg, ds)
    return cfg


def window(hip, W, Wo, seed, refresh=False, full=False, **kw):
    """an initialised window (pipeline.init_window); the same arguments give the same window: twins"""
    ds, clouds, _ = data()
    est = capi.Estimator(hip, config(hip, W, Wo, **kw))
    if refresh:
        est.set_map_refresh(True)
        est.map().process(clouds[0][1], clouds[0][0], IDENT)
    if full:
        est.set_full_cloud(True)
    pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01, seed=seed)
    return est


def imu(est, k):
    f = data()[0].frames[k]
    for j in range(f.imu_dt.shape[0]):
        est.process_imu(float(f.imu_dt[j]), f.imu_acc[j], f.imu_gyr[j], float(f.imu_t[j]))


def ident_T():
    return capi.TransformF.make(*IDENT)


def item(k, surf=None, corner=None):
    """frame k of the sequence as EstimatorBatch.push_frames takes it (surf / corner: a cloud in its place)"""
    ds, clouds, _ = data()
    return (ident_T(), clouds[k][0] if surf is None else surf, clouds[k][1] if corner is None else corner, ds.frames[k].t)


def push_single(est, it):
    est.push_frame(it[0], it[1], it[2], it[3])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def rep_key(r):
    return (r.iterations, r.successful_steps, r.termination, r.n_lidar_residuals, r.n_local_map, r.laser_odom_iterations, r.turn_off, r.convergence_flag,
            r.marginalized, r.initial_cost, r.final_cost, tuple(r.cost_trace[:12]))


def observe(est, prior=False, event=False):
    """what the getters answer, as bits"""
    W = est.W
    out = {}
    stacks = [est.get_surf_stack(i) for i in range(W + 1)]
    out["stack_sizes"] = np.array([len(s) for s in stacks], np.uint32)
    for i, s in enumerate(stacks):
        out[f"stack{i}"] = bits(s)
    for key, v in est.get_window().items():
        out["win_" + key] = bits(np.asarray(v))
    st = est.stage()
    out["stage"] = np.array([int(st["inited"]), st["cir_buf_count"], st["extrinsic_stage"]] + ([est.EVENTS.index(st["event"])] if event else []), np.uint32)
    out["stage_R"] = bits(np.concatenate([st["R_WI"].ravel(), st["g_vec"]]))
    for i in range(W + 1):
        pts, state = est.full_stack(i)
        out[f"full{i}"] = bits(pts)
        out[f"full_state{i}"] = np.array([state or 0, len(pts)], np.uint32)
        if state:
            q, p = est.full_transform_es(i)
            out[f"full_tes{i}"] = bits(np.concatenate([np.asarray(q, np.float32), np.asarray(p, np.float32)]))
    h = est.last_map_refresh()
    out["refresh_have"] = np.array([h is not None], np.uint32)
    if h is not None:
        out["refresh_head"] = np.array([h["applied"]] + list(h["cube_center"]), np.int64).view(np.uint64)
        out["refresh_valid"] = bits(h["valid_idx"])
        out["refresh_T"] = bits(np.concatenate([np.asarray(h["T"][0], np.float32), np.asarray(h["T"][1], np.float32)]))
        out["refresh_corner"], out["refresh_surf"] = bits(h["corner"]), bits(h["surf"])
    if prior:
        p = est.prior()
        out["prior_have"] = np.array([p is not None], np.uint32)
        if p is not None:
            for key in ("JtJ", "Jtr", "x0"):
                out["prior_" + key] = bits(p[key])
    return out


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for key in a:
        assert a[key].shape == b[key].shape, f"{what}: {key} {a[key].shape} != {b[key].shape}"
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")


def assert_twins(A, B, what, **kw):
    for w, (a, b) in enumerate(zip(A, B)):
        assert_same(observe(a, **kw), observe(b, **kw), f"{what}, window {w}")


# ---------------------------------------------------------------- crafted clouds
def room(n, seed):
    """n returns of an indoor room: x, y in +-10 m, z in +-2 m, intensity = ring + fraction of the sweep"""
    rng = np.random.default_rng(seed)
    c = np.empty((n, 4), np.float32)
    c[:, 0:2] = rng.uniform(-10.0, 10.0, (n, 2))
    c[:, 2] = rng.uniform(-2.0, 2.0, n)
    c[:, 3] = rng.integers(0, 16, n) + rng.uniform(0.0, 0.099, n)
    return c


BLOCK_EDGES = (0, 1, 255, 256, 257, 8191, 8192, 8193)   # a block of 256 lanes, a sort tile of 2 x 4096 keys


def one_voxel(n=500, seed=11):
    c = room(n, seed)
    c[:, 0:3] = np.random.default_rng(seed).uniform(0.05, 0.35, (n, 3))   # all of it inside cell (0, 0, 0) of a 0.4 m leaf
    return c


def face_lattice(leaf=LEAF):
    """points ON the faces of the voxels (coordinates that are float multiples of the leaf, both signs), every one twice"""
    g = np.arange(-6, 7, dtype=np.float32) * np.float32(leaf)
    x, y, z = np.meshgrid(g, g, g[4:9], indexing="ij")
    c = np.zeros((x.size, 4), np.float32)
    c[:, 0], c[:, 1], c[:, 2] = x.ravel(), y.ravel(), z.ravel()
    c[:, 3] = (np.arange(x.size) % 16).astype(np.float32) + np.float32(0.05)
    return np.ascontiguousarray(np.vstack([c, c[::-1]]))


def non_finite(n=700, seed=13):
    c = room(n, seed)
    c[5, 0] = np.nan; c[17, 1] = np.inf; c[18, 2] = -np.inf; c[300, 0:3] = np.nan; c[n - 1, 2] = np.nan; c[0, 1] = np.inf
    return c


def beyond_the_key(seed=17):
    """a stray return 150 m up: cell 375 of a 0.4 m leaf, outside the chain's 9-bit z key (+-254 cells)"""
    c = room(900, seed)
    c[123, 0:3] = (0.5, 0.5, 150.0)
    return c


SHARED_SWEEP = 257         # points of every sweep of the shared-filter case: two tiles of 256, the second with one point


def beyond_the_abs_range(seed=29):
    """a sweep with one return 500 m out along x: cell 1250 of a 0.4 m leaf, outside the filter's absolute key (|x| cells < 1024)"""
    c = room(SHARED_SWEEP, seed)
    c[100, 0:3] = (500.0, 0.5, 0.5)
    return c


def stray_above(stack):
    """`stack` with a return 300 m up behind it (tests/test_gpu_batch.py: the window beyond the filter's key range, z cells < 255)"""
    return np.ascontiguousarray(np.vstack([stack, np.array([[0.5, 0.5, 300.0, stack[0, 3]]], np.float32)]))


def pcl_overflow(seed=19):
    """returns at +-2e5 m on every axis: (4e5 / 0.4 + 1)^3 voxels pass INT_MAX — PCL's "leaf size is too small": output = input"""
    c = room(400, seed)
    c[7, 0:3] = (2e5, 2e5, 2e5)
    c[8, 0:3] = (-2e5, -2e5, -2e5)
    return c
