"""Plain-Python statement of the optimisation-window buffers that feed the map-database refresh
(reference src/imu_processor/Estimator.cc; line numbers below are that file's).

    :177-183   seven CircularBuffers of opt_window_size + 1 slots; the ones the refresh reads are restated here:
               opt_point_coeff_mask_, opt_cube_centers_, opt_transforms_, opt_valid_idx_, opt_surf_stack_, opt_corner_stack_
    :467-471   every processed frame pushes mask = false, the map's cube centre, transform_in, the map's valid list
    :474-480   before initialisation, or with both de-skew switches off, the frame's stacks are pushed to the WINDOW here ...
    :484-485   ... and the opt slot takes surf_stack_.last() / corner_stack_.last() as they are AT THIS LINE
    :616       a step taken while not initialised (the initialising step included) sets the newest slot's mask
    :689-693   with de-skew on, an initialised step pushes its stacks to the window only here, AFTER :484: the opt slot of that
               step therefore holds the PREVIOUS frame's stacks
    :2282-2286 at the end of every solve slot 0's transform becomes the optimised lidar pose of frame W - Wo (double, cast to float)
    :626,:703  the refresh runs when the ring is full and slot 0 is not masked, with slot 0's five entries
    :1434,:2615 the pivot fusion and SlideWindow edit window clouds IN PLACE; the stacks are shared pointers, so an opt slot
               that holds such a cloud sees the edit.  SlideWindow does not move the ring: only a push does.

Clouds are `Cloud` objects compared by identity, so the aliasing is the model's own and not the product's frame arithmetic.
No numpy-free restriction: poses use numpy in float64.
"""
import numpy as np


class Cloud:
    """A PointCloudPtr's pointee: shared by reference, edited in place."""

    def __init__(self, pts):
        self.pts = pts


class CircularBuffer:
    """include/utils/CircularBuffer.h: push appends, the oldest element goes once the capacity is reached."""

    def __init__(self, capacity):
        self.capacity, self.items = capacity, []

    def push(self, v):
        if len(self.items) == self.capacity:
            self.items.pop(0)
        self.items.append(v)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def first(self):
        return self.items[0]

    def last(self):
        return self.items[-1]


def quat_from_rot(R):
    """Eigen::Quaterniond(Matrix3d) (Quaternion.h, quaternionbase_assign_impl<Other,3,3>) -> (x, y, z, w)"""
    R = np.asarray(R, np.float64)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def rot_from_quat(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def opt_pose0(Rs, Ps, q_lb, t_lb, W, Wo):
    """:2281-2286 in float64, then one cast to float32: (q xyzw, p).
    transform_lb_.cast<double>(); rot_l0(Rs_[W - Wo] * lb.rot.conjugate().normalized()); pos_l0 = Ps_[W - Wo] - rot_l0 * lb.pos"""
    q = np.asarray(q_lb, np.float32).astype(np.float64)
    t = np.asarray(t_lb, np.float32).astype(np.float64)
    c = np.array([-q[0], -q[1], -q[2], q[3]])
    c = c / np.sqrt(np.sum(c * c))
    o = W - Wo
    R = np.asarray(Rs[o], np.float64) @ rot_from_quat(c)
    rot = quat_from_rot(R)
    pos = np.asarray(Ps[o], np.float64) - rot_from_quat(rot) @ t
    return rot.astype(np.float32), pos.astype(np.float32)


class RefreshModel:
    def __init__(self, W, Wo, deskew):
        self.W, self.Wo, self.deskew = W, Wo, bool(deskew)     # deskew: enable_deskew || cutoff_deskew
        self.inited = False
        self.surf_stack, self.corner_stack = CircularBuffer(W + 1), CircularBuffer(W + 1)          # :161-162
        self.mask, self.cen, self.T, self.valid = (CircularBuffer(Wo + 1) for _ in range(4))     # :177-181
        self.opt_surf, self.opt_corner = CircularBuffer(Wo + 1), CircularBuffer(Wo + 1)          # :182-183

    # ---- ProcessLaserOdom
    def push(self, transform_in, cube_center, valid_idx, surf, corner):
        """:467-485 and, for an initialised step with de-skew on, :689-693.  surf / corner: the stacks this frame pushes to the window
        (as they come at :475-478, de-skewed and filtered at :689-692)."""
        self.mask.push(False)                                   # :467
        self.cen.push(list(cube_center))                        # :469
        self.T.push(transform_in)                               # :470
        self.valid.push(list(valid_idx))                        # :471
        early = (not self.inited) or (not self.deskew)          # :474
        if early:
            self.surf_stack.push(Cloud(surf))                   # :475
            self.corner_stack.push(Cloud(corner))               # :478
        self.opt_surf.push(self.surf_stack.last())              # :484
        self.opt_corner.push(self.corner_stack.last())          # :485
        if not early:
            self.surf_stack.push(Cloud(surf))                   # :689
            self.corner_stack.push(Cloud(corner))               # :692

    def end_uninitialised_step(self, initialised=False):
        """:616 — reached by every step that entered the NOT_INITED case, the one that initialises included."""
        self.mask.items[-1] = True
        if initialised:
            self.inited = True                                   # :543

    def seed_window(self, stacks):
        """The test hooks lio_est_set_window / lio_est_set_surf_stack: an initialised window of W + 1 frames.  Window clouds that
        exist are overwritten IN PLACE (*surf_stack_[i] = cloud), older ones that a short run never pushed are created."""
        assert len(stacks) == self.W + 1
        have = len(self.surf_stack)
        old_s, old_c = list(self.surf_stack.items), list(self.corner_stack.items)
        self.surf_stack.items = [Cloud(None) for _ in range(self.W + 1 - have)] + old_s
        self.corner_stack.items = [Cloud(np.zeros((0, 4), np.float32)) for _ in range(self.W + 1 - have)] + old_c
        for c, s in zip(self.surf_stack.items, stacks):
            c.pts = s
        self.inited = True

    # ---- SolveOptimization
    def solved(self, Rs, Ps, q_lb, t_lb):
        """:2282-2286"""
        if len(self.T):
            self.T.items[0] = opt_pose0(Rs, Ps, q_lb, t_lb, self.W, self.Wo)

    def fuse_pivot(self, pts):
        """:1434 — *(surf_stack_[pivot]) = the fused cloud, in place"""
        self.surf_stack[self.W - self.Wo].pts = pts

    # ---- :626, :703-708
    def refresh(self):
        """-> None (ring not full or slot 0 masked) or the arguments of UpdateMapDatabase"""
        if len(self.mask) != self.Wo + 1 or self.mask.first():
            return None
        return self.slot0()

    def slot0(self):
        if not len(self.mask):
            return None
        return dict(corner=self.opt_corner.first().pts, surf=self.opt_surf.first().pts, valid_idx=self.valid.first(), T=self.T.first(),
                    cube_center=self.cen.first())

    # ---- SlideWindow
    def slide(self, pts=None):
        """:2570-2666.  The ring does not move.  Once the local map exists, *(surf_stack_[pivot + 1]) is replaced in place (:2615)."""
        if pts is not None:
            self.surf_stack[self.W - self.Wo + 1].pts = pts
