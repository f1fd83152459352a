"""Plain-Python statement of what the reference does with the full-resolution sweep (include/lio_full_cloud.h).

    PointOdometry.cc:261-292   TransformToEnd(full_cloud_), the odometry's form: the slerp's conjugate is NOT normalised, the
                               intensity loses its fraction (point.intensity = int(point.intensity))
    Estimator.cc:62-103        TransformToEnd, the estimator's form: the conjugate IS normalised (:88); the intensity loses its ring
                               (:80) unless keep_intensity (:79)
    PointMapping.cc:303-314    PointAssociateToMap: rot * p + pos, intensity kept
    Estimator.cc:2284-2286, :2293-2295   the lidar pose of a window frame, in double, cast to float
    Estimator.cc:482, :2355-2420         full_stack_: one copy per processed frame, the newest corrected at the end of every solve

(a) to_end64: both forms in float64 from float32 inputs (the branch of the slerp is taken at the float64 epsilon);
(b) to_end32: both forms in float32, operation for operation as csrc/hmath.h states Eigen's slerp (:164-178), conjugate, normalized and
    quaternion * vector (rotate, :117-124);
(c) rigid_map32: rot * p + pos in float32, operation for operation;
(d) lidar_pose: map_refresh_ref.opt_pose0's arithmetic for any window frame;
(e) FullRingModel: the bookkeeping of the estimator's ring.
"""
import numpy as np

from map_refresh_ref import CircularBuffer, opt_pose0

FULL_MAP_FRAME, FULL_SENSOR_RAW, FULL_SENSOR_END = 1, 2, 3

# Worst |to_end32 - to_end64|_inf / (2^-24 * (|p| + |t_es|)) over every cloud x T_es of tests/full_cloud_cases.py, both forms, as
# tests/test_full_cloud_ref.py::test_fp32_restatement_stays_within_k_deskew measures it on the CPU (numpy float32 against float64;
# the run printed 4.018 for the estimator's form and 4.177 for the odometry's), rounded up.  The product's kernels are held to
# GPU_BOUND_FACTOR x this: device acos, sin, sqrt and the division each differ from libm by a few ulps.  Neither number was
# measured on the code under test.
K_DESKEW = 4.18
GPU_BOUND_FACTOR = 4.0


def scale_of(xyzi, t_es):
    """2^-24 * (|p| + |t_es|) per point, float64"""
    p = np.asarray(xyzi, np.float32).astype(np.float64)[:, :3]
    return 2.0 ** -24 * (np.sqrt(np.sum(p * p, axis=1)) + np.linalg.norm(np.asarray(t_es, np.float32).astype(np.float64)))


# ---------------------------------------------------------------- the quaternion pieces, generic in the dtype
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _rotate(q, v):
    """Eigen's quaternion * vector: v + w * (2 u x v) + u x (2 u x v); q is n x 4 (x y z w)"""
    u = q[:, :3]
    uv = _cross(u, v)
    uv = uv + uv
    a = v + uv * q[:, 3:4]
    return a + _cross(u, uv)


def _slerp_from_identity(t, qe, eps):
    """Quaternion::slerp(t, other) from the identity (hmath.h:164-178): d = dot, |d| >= 1 - eps takes the linear branch, d < 0 flips"""
    dt = t.dtype.type
    one = dt(1) - dt(eps)
    d = dt(0) * qe[0] + dt(0) * qe[1] + dt(0) * qe[2] + dt(1) * qe[3]
    ad = np.abs(d)
    if ad >= one:
        s0, s1 = dt(1) - t, t.copy()
    else:
        th = np.arccos(ad)
        st = np.sin(th)
        s0 = np.sin((dt(1) - t) * th) / st
        s1 = np.sin(t * th) / st
    if d < 0:
        s1 = -s1
    # (w, x, y, z) = s0 * identity + s1 * qe
    return np.stack([s0 * dt(0) + s1 * qe[0], s0 * dt(0) + s1 * qe[1], s0 * dt(0) + s1 * qe[2], s0 * dt(1) + s1 * qe[3]], axis=1)


def _to_end(xyzi, q_e, t_e, time_factor, form, keep_intensity, dt, no_deskew=False, plant=None):
    """form 'est' | 'odo'.  plant: None | 'no_conj' | 'no_st' | 'no_norm' | 'strip_in_keep' (the planted errors of the tests)"""
    f32 = np.asarray(xyzi, np.float32).reshape(-1, 4)
    w32 = f32[:, 3]
    ring32 = np.trunc(w32).astype(np.float32)                   # float(int(w)): truncation
    a = f32.astype(dt)
    qe = np.asarray(q_e, np.float32).astype(dt)
    te = np.asarray(t_e, np.float32).astype(dt)
    frac = a[:, 3] - ring32.astype(dt)
    s = dt(time_factor) * frac
    if no_deskew:
        s = np.zeros_like(s)
    p = a[:, :3].copy()
    if plant != "no_st":
        p = p - s[:, None] * te[None, :]
    qs = _slerp_from_identity(s, qe, np.finfo(dt).eps)
    qc = np.concatenate([-qs[:, :3], qs[:, 3:4]], axis=1)
    if plant == "no_conj":
        qc = qs
    if form == "est" and plant != "no_norm":
        n2 = qc[:, 0] * qc[:, 0] + qc[:, 1] * qc[:, 1] + qc[:, 2] * qc[:, 2] + qc[:, 3] * qc[:, 3]
        qc = qc / np.sqrt(n2)[:, None]
    v = _rotate(qc, p)
    v = _rotate(np.broadcast_to(qe, (len(v), 4)), v)
    v = v + te[None, :]
    if form == "odo":
        w = ring32                                              # PointOdometry.cc:277
    elif keep_intensity and plant != "strip_in_keep":
        w = w32                                                 # Estimator.cc:79
    else:
        w = (w32 - ring32).astype(np.float32)                   # Estimator.cc:80 (exact in float32)
    return v, w


def to_end64(xyzi, q_e, t_e, time_factor=10.0, form="est", keep_intensity=False, no_deskew=False, plant=None):
    """-> (xyz float64 n x 3, intensity float32 n)"""
    return _to_end(xyzi, q_e, t_e, time_factor, form, keep_intensity, np.float64, no_deskew, plant)


def to_end32(xyzi, q_e, t_e, time_factor=10.0, form="est", keep_intensity=False, no_deskew=False, plant=None):
    """-> xyzi float32 n x 4"""
    v, w = _to_end(xyzi, q_e, t_e, time_factor, form, keep_intensity, np.float32, no_deskew, plant)
    assert v.dtype == np.float32
    return np.concatenate([v, w[:, None]], axis=1)


def worst_ratio(got_xyz, xyzi, q_e, t_e, **kw):
    """max over the points of |got - to_end64|_inf / scale (0 for an empty cloud)"""
    if len(xyzi) == 0:
        return 0.0
    want, _ = to_end64(xyzi, q_e, t_e, **kw)
    err = np.max(np.abs(np.asarray(got_xyz).astype(np.float64) - want), axis=1)
    return float(np.max(err / scale_of(xyzi, t_e)))


# ---------------------------------------------------------------- (c) PointAssociateToMap
def rigid_map32(xyzi, q, p):
    a = np.asarray(xyzi, np.float32).reshape(-1, 4)
    q = np.asarray(q, np.float32)
    t = np.asarray(p, np.float32)
    v = _rotate(np.broadcast_to(q, (len(a), 4)), a[:, :3]) + t[None, :]
    assert v.dtype == np.float32
    return np.concatenate([v, a[:, 3:4]], axis=1)


# ---------------------------------------------------------------- (d) the lidar pose of window frame i
def lidar_pose(Rs, Ps, q_lb, t_lb, i):
    """:2284-2286 / :2293-2295: rot = Rs[i] * q_lb.conjugate().normalized(), pos = Ps[i] - rot * t_lb in float64, cast once to float32"""
    W = len(Rs) - 1
    return opt_pose0(Rs, Ps, q_lb, t_lb, W, W - i)


# ---------------------------------------------------------------- (e) the ring
class FullRingModel:
    """full_stack_ (Estimator.cc:482): a CircularBuffer of W + 1; SlideWindow does not touch it.  Its newest entry belongs to the window's
    newest frame, so window frame i is entry i - (frames in the window - entries)."""

    def __init__(self, W, Wo):
        self.W, self.Wo = W, Wo
        self.ring = CircularBuffer(W + 1)
        self.n_frames = 0

    def seed_window(self):
        """a window injected through the test hooks: W + 1 frames, the ring as it was"""
        self.n_frames = self.W + 1

    def push(self, cloud, inited, t_es=None):
        """every pushed frame; before initialisation the cloud is the map's registered one (PointMapping.cc:1244-1248)"""
        self.ring.push(dict(cloud=cloud, state=FULL_SENSOR_RAW if inited else FULL_MAP_FRAME, t_es=t_es, corrections=0))
        self.n_frames = min(self.n_frames + 1, self.W + 1)

    def solved(self, correct=lambda cloud, t_es: cloud):
        """:2355-2420 at the end of every completed solve: the newest entry, once.  A map-frame entry is left as it is (on the
        initialising step the reference's call is an exact no-op)."""
        if len(self.ring) == 0:
            return False
        e = self.ring.last()
        if e["state"] != FULL_SENSOR_RAW:
            return False
        e["cloud"], e["state"] = correct(e["cloud"], e["t_es"]), FULL_SENSOR_END
        e["corrections"] += 1
        return True

    def restore(self):
        """lio_est_restore / lio_est_copy_snapshot: snapshots do not carry full clouds"""
        self.ring = CircularBuffer(self.W + 1)

    def entry(self, frame):
        idx = frame - (self.n_frames - len(self.ring))
        if frame < 0 or frame >= self.n_frames or idx < 0 or idx >= len(self.ring):
            return None
        return self.ring[idx]

    def local_full_points(self):
        """:2372-2375: full_stack_[pivot + 1]"""
        return self.entry(self.W - self.Wo + 1)
