"""Inputs of the TransformToEnd tests (tests/test_full_cloud_ref.py, tests/test_gpu_full_cloud_kernels.py).

Clouds: n = 0, 1, 255, 256, 257 (the edges of a 256-lane workgroup) and 2049 (more than one workgroup, not a multiple), ranges 0.5 ..
120 m, rings 0 .. 63.  With time_factor 10 the relative time of a point is rel_time = s / 10; the fractions cover exactly 0, values
that make s exactly 1 in float32, and values just above (s up to 1 + 1e-3, the reference's own tolerance at Estimator.cc:71).
"""
import numpy as np

SIZES = (0, 1, 255, 256, 257, 2049)
TIME_FACTOR = 10.0


def _quat(axis, angle, scale=1.0, negate=False):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    q = np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]]) * scale
    if negate:
        q = -q
    return q.astype(np.float32)


# (name, q_e xyzw float32, t_e float32)
T_ES = [
    ("identity", np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32)),
    # cos(angle / 2) >= 1 - FLT_EPSILON: the slerp's linear branch
    ("below_threshold", _quat([0.3, -0.5, 0.8], 4.0e-4), np.array([0.002, -0.001, 0.0005], np.float32)),
    ("small", _quat([0.1, 0.2, 1.0], 0.01), np.array([0.3, 0.02, -0.01], np.float32)),
    ("large", _quat([-0.4, 0.3, 0.85], 1.0), np.array([3.0, -0.5, 0.2], np.float32)),
    ("negative_w", _quat([0.2, 0.9, -0.3], 0.2, negate=True), np.array([0.6, 0.1, -0.05], np.float32)),
    ("off_unit", _quat([0.5, -0.2, 0.8], 0.3, scale=1.001), np.array([0.9, -0.3, 0.1], np.float32)),
]


def cloud(n, seed=0):
    """n points: direction uniform on the sphere, range 0.5 .. 120 m (both ends present from n >= 2), ring 0 .. 63, fraction as above"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True) if n else 1.0
    r = np.exp(rng.uniform(np.log(0.5), np.log(120.0), size=n))
    ring = rng.integers(0, 64, size=n).astype(np.float32)
    s = rng.uniform(0.0, 1.0, size=n)
    if n >= 1:
        r[0] = 120.0
    if n >= 2:
        r[1] = 0.5
    # the special fractions, spread over the cloud (and over the rings: ring 63 + 0.1 is not the same float as ring 0 + 0.1)
    special = [0.0, 1.0, 1.0 + 9.5e-4, 1.0 + 5e-4, 0.5, 0.0, 1.0]
    for k in range(min(n, 64)):
        s[k] = special[k % len(special)]
    xyzi = np.zeros((n, 4), np.float32)
    xyzi[:, :3] = (d * r[:, None]).astype(np.float32)
    xyzi[:, 3] = ring + (s / TIME_FACTOR).astype(np.float32)
    # "s exactly 1": float32(10 * f) == 1 needs f within 6e-9 of 0.1, and the fraction of ring + f is a multiple of the ring's ulp
    # (1.2e-7 from ring 1 up): only ring 0 has such an intensity, float32(0.1)
    for k in range(min(n, 64)):
        if special[k % len(special)] == 1.0:
            xyzi[k, 3] = np.float32(0.1)
        if special[k % len(special)] == 0.0:
            xyzi[k, 3] = np.trunc(xyzi[k, 3])
    return xyzi


def integer_intensity_cloud(n, seed=1):
    c = cloud(n, seed)
    c[:, 3] = np.trunc(c[:, 3])
    c[:, :3] = np.where(c[:, :3] == 0, np.float32(1.0), c[:, :3])   # (no signed zero: x + 0 is not a bit-exact no-op on -0)
    return c


def all_cases():
    for n in SIZES:
        c = cloud(n)
        for name, q, t in T_ES:
            yield f"n{n}-{name}", c, q, t
