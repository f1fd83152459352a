"""The cases that hold the pooled cube map (csrc/mapping.hip) to the oracle and to the plain model of tests/cube_map_ref.py, bit for bit,
and the runner that plays one case on a handle of any of the three.

A case is a list of tracks; a track is a fresh handle (`cfg`: overrides of lio_map_default_config) and a list of ops played on it in order:
  update   lio_map_update_map_database(corner, surf, valid, T, cen); valid / cen None: the handle's own list / centre (lio_map_get_cube_state)
  pose     lio_map_set_init_flag(1), lio_map_set_transform_tobe_mapped(q, p), lio_map_process of two empty clouds: the window shift, the FOV
           cube selection and the from-map clouds at a stated pose, nothing else
  process  lio_map_set_init_flag(0), lio_map_process(corner, surf, T_sum): the whole step (only on maps too small to optimise against)
  snap     record the centre, the valid list, the from-map clouds (after a process also the pose and the filtered stacks) and the cubes:
           kind "all" reads all 4851 indices of both classes, kind "near" those the caller's `probes` name (None: all of them)
Every op carries the return code it must give (`rc`).  An op with rc != 0 must leave the handle as it was: the runner reads everything before
and after it and compares.  `only="product"` marks an op that exists for a limit of the product alone (125 valid cubes, the range of the
packed cube keys): the oracle and the model skip it.

Clouds are xyzi with distinct intensities (a running number), so a moved, swapped or lost point shows in the bits."""
import ctypes as C

import numpy as np

import cube_map_ref as ref
from cube_map_ref import F, H, L, N_CUBES, W, to_index

LIO_OK, LIO_ERR_ARG, LIO_ERR_CAPACITY = 0, -1, -4
IDENT = (0.0, 0.0, 0.0, 1.0)
ID = (IDENT, (0.0, 0.0, 0.0))
HALF_X, HALF_Y, HALF_Z = (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0)
EMPTY = np.zeros((0, 4), F)
CEN0 = (10, 10, 5)
CONFIGS = {"default": {}, "equal": dict(corner_filter_size=0.3, surf_filter_size=0.3)}
DEFAULT_LEAVES = (0.2, 0.4)   # lio_map_default_config; tests/test_cube_map_ref.py asserts it


def leaves(cfg):
    return (cfg.get("corner_filter_size", DEFAULT_LEAVES[0]), cfg.get("surf_filter_size", DEFAULT_LEAVES[1]))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


def up(v):
    return np.nextafter(F(v), F(np.inf))


def around(v):
    return [down(v), F(v), up(v)]


def cloud(xyz, first_intensity=1.0):
    """xyz rows -> xyzi fp32 with intensities first, first + 1, ... (exact in fp32)"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), F)
    out[:, :3] = xyz
    out[:, 3] = F(first_intensity) + np.arange(len(xyz), dtype=F)
    return out


def box(rng, n, lo, hi, first_intensity=1.0):
    return cloud(rng.uniform(lo, hi, (n, 3)), first_intensity)


def update(corner, surf, valid=(), T=ID, cen=CEN0, rc=LIO_OK, only=None):
    return dict(op="update", corner=np.asarray(corner, F).reshape(-1, 4), surf=np.asarray(surf, F).reshape(-1, 4),
                valid=None if valid is None else np.asarray(list(valid), np.uint32), T=T, cen=cen, rc=rc, only=only)


def pose(q, p, rc=LIO_OK, only=None):
    return dict(op="pose", q=q, p=p, rc=rc, only=only)


def process(corner, surf, T_sum):
    return dict(op="process", corner=np.asarray(corner, F).reshape(-1, 4), surf=np.asarray(surf, F).reshape(-1, 4), T=T_sum, rc=LIO_OK, only=None)


def snap(kind="near"):
    return dict(op="snap", kind=kind, rc=LIO_OK, only=None)


def track(ops, cfg="default"):
    return dict(cfg=CONFIGS[cfg], ops=ops)


def block(i0, i1, j0, j1, k0, k1):
    """cube indices of [i0, i1] x [j0, j1] x [k0, k1] in ascending index order (NOT the selection loop's order)"""
    return [to_index(i, j, k) for k in range(k0, k1 + 1) for j in range(j0, j1 + 1) for i in range(i0, i1 + 1)]


# ------------------------------------------------------------------------------------------------ the cases
X_FACES = around(-25) + around(25) + [F(-0.0), F(0.0), F(-75), F(-125), F(-475), F(-525), up(-525), down(525), F(525)]
Z_FACES = around(-25) + around(25) + [F(-0.0), F(0.0), F(-75), F(-125), F(-225), F(-275), up(-275), down(275), F(275)]


def faces():
    """Fresh handle (centre 10, 10, 5), identity pose, no valid cube: every cube hands back what was filed under it.  Coordinates on the
    faces of the cubes, one fp32 step to either side, the exact negative multiples (-75 lands in cube cen - 2) and the first and last kept
    and the first dropped cube of every axis.  Every pair of face values of two axes occurs, the third axis cycles through its own."""
    assert X_FACES[-2] == F(524.99994) and Z_FACES[-2] == F(274.99997)
    rows = []
    n = len(X_FACES)
    for a in range(n):
        for b in range(n):
            c = (a + 2 * b) % n
            rows += [(X_FACES[a], X_FACES[b], Z_FACES[c]), (X_FACES[a], X_FACES[c], Z_FACES[b]), (X_FACES[c], X_FACES[a], Z_FACES[b])]
    corner = cloud(rows)
    surf = cloud(rows[::-1], 5000.0)
    # the half-turn about z mirrors x and y: -25 comes in as +25 and the other way round
    return [track([update(corner, surf), snap("near"), update(surf, corner, T=(HALF_Z, (0.0, 0.0, 0.0))), snap("all")])]


def order_sensitive_triple(rng, lo, hi):
    """three points of the box [lo, hi]^3 for which (a + b) + c != (a + c) + b in fp32 on x and on the intensity"""
    while True:
        p = np.zeros((3, 4), F)
        p[:, :3] = rng.uniform(lo, hi, (3, 3))
        p[:, 3] = rng.uniform(1.0, 200.0, 3)
        if all((p[0, c] + p[1, c]) + p[2, c] != (p[0, c] + p[2, c]) + p[1, c] for c in (0, 3)):
            return p


TRIPLE_BOX, CROWD_BOX = (10.02, 10.18), (-11.98, -11.82)   # each inside one voxel of every leaf used (0.2, 0.3, 0.4)


def voxels_parts(cfg_name):
    """the pieces of `voxels` for one class each: (triple, crowd of 300, grid points on and next to the voxel faces)"""
    rng = np.random.default_rng(11)
    out = []
    for cls, leaf in enumerate(leaves(CONFIGS[cfg_name])):
        triple = order_sensitive_triple(rng, *TRIPLE_BOX)
        crowd = box(rng, 300, *CROWD_BOX, first_intensity=1000.0)
        rows = []
        base = [F(3.05), F(-4.05), F(1.05)]
        for d in range(3):
            for m in (-61, -7, -3, -1, 0, 1, 2, 5, 60):
                for v in around(F(m) * F(leaf)):   # a multiple of the leaf in fp32 and its neighbours
                    r = list(base)
                    r[d] = v
                    rows.append(r)
        out.append((triple, crowd, cloud(rows, 2000.0 + 500.0 * cls)))
    return out


def voxels(cfg_name="default"):
    """Valid cubes: the centre cube with the face points, the order-sensitive triple and the voxel of 300; its +x neighbour, whose corner
    class holds ONE point; the next one, whose points all share z (min = max on that axis)."""
    rng = np.random.default_rng(12)
    parts = voxels_parts(cfg_name)
    single = cloud([[40.0, 1.0, 2.0]], 7000.0)
    several = box(rng, 40, (30.0, -5.0, -5.0), (33.0, 5.0, 5.0), 7100.0)
    flat = box(rng, 60, (80.0, -2.0, 3.0), (84.0, 2.0, 3.0), 7200.0)
    assert np.all(flat[:, 2] == F(3.0))
    clouds = [np.concatenate([parts[0][2], parts[0][0], parts[0][1], single, flat]),
              np.concatenate([parts[1][1], parts[1][2], parts[1][0], several, flat[::-1]])]
    valid = [to_index(10, 10, 5), to_index(11, 10, 5), to_index(12, 10, 5)]
    return [track([update(clouds[0], clouds[1], valid), snap("near")], cfg_name)]


def old_then_new(cfg_name="default"):
    """Three updates into the same two valid cubes; the later points fall into voxels that hold a centroid of the earlier ones, so the
    sums run old first and a centroid is averaged again (not idempotent).  Around x = 6 (a voxel face of every leaf used) the first update
    leaves one centroid exactly one fp32 step below the face and one exactly on it."""
    rng = np.random.default_rng(13)
    face = np.array([[down(6.0), 6.1, 6.1], [down(6.0), 6.12, 6.13], [6.0, 6.1, 6.1], [6.0, 6.13, 6.12]], F)
    later = np.array([[up(6.0), 6.11, 6.11], [down(down(6.0)), 6.11, 6.11], [6.05, 6.1, 6.1], [5.95, 6.1, 6.1]], F)
    valid = [to_index(10, 10, 5), to_index(10, 10, 4)]
    ops = []
    for step in range(3):
        c = np.concatenate([box(rng, 400, (-1.0, -1.0, -26.0), (1.0, 1.0, -24.0), 1.0 + 1000 * step), cloud(face if step == 0 else later, 900.0 + 1000 * step)])
        s = np.concatenate([cloud(face if step == 0 else later, 950.0 + 1000 * step), box(rng, 400, (-1.0, -1.0, -26.0), (1.0, 1.0, -24.0), 500.0 + 1000 * step)])
        ops += [update(c, s, valid), snap("near")]
    return [track(ops, cfg_name)]


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
SIZES_VALID = block(9, 11, 10, 11, 5, 5) + block(10, 10, 10, 10, 4, 4)


def _spread(rng, n, first):
    """points over valid cubes, non-valid cubes and (a few) beyond the window"""
    pts = box(rng, n, (-130.0, -130.0, -60.0), (130.0, 130.0, 60.0), first)
    pts[::17, 0] += F(1000.0)
    return pts


def sizes():
    """New points per class in SIZES (block and wave edges of the rank, scatter, bounds and key kernels), into a valid part that is empty and
    into one that holds unfiltered points (filed with an empty valid list first, so n = 0 is a pure re-filter behind a relayout); then all
    new points dropped, all into non-valid cubes, all into valid cubes, and either class empty beside a full one."""
    rng = np.random.default_rng(14)
    tracks = []
    for populated in (False, True):
        for n in SIZES:
            ops = []
            if populated:
                ops.append(update(_spread(rng, 300, 1.0), _spread(rng, 500, 1.0)))
            ops += [update(_spread(rng, n, 10000.0), _spread(rng, n, 20000.0)[::-1], SIZES_VALID), snap("near")]
            tracks.append(track(ops))
    base = [update(_spread(rng, 300, 1.0), _spread(rng, 500, 1.0), SIZES_VALID)]
    far_away = box(rng, 200, (600.0, 600.0, 300.0), (900.0, 900.0, 500.0), 30000.0)
    non_valid = box(rng, 200, (80.0, -120.0, -20.0), (120.0, -80.0, 20.0), 31000.0)
    in_valid = box(rng, 200, (-20.0, -20.0, -20.0), (20.0, 20.0, 20.0), 32000.0)
    for c, s in ((far_away, far_away[::-1]), (non_valid, non_valid[::-1]), (in_valid, in_valid[::-1]), (EMPTY, in_valid), (non_valid, EMPTY)):
        tracks.append(track(base + [update(c, s, SIZES_VALID), snap("near")]))
    return tracks


FULL_BLOCK = block(8, 12, 8, 12, 3, 7)


def full_valid_clouds():
    rng = np.random.default_rng(15)
    parts = [[], []]
    for n, idx in enumerate(FULL_BLOCK):
        i, j, k = ref.from_index(idx)
        centre = np.array([50.0 * (i - 10), 50.0 * (j - 10), 50.0 * (k - 5)])
        for cls in (0, 1):
            m = 600 if (cls == 0 and n == 77) else 2 + (n + cls) % 3
            half = 1.0 if m == 600 else 20.0   # the 600 share voxels
            parts[cls].append(box(rng, m, centre - half, centre + half, 100.0 * n + 50000.0 * cls))
    return np.concatenate(parts[0]), np.concatenate(parts[1])


def full_valid():
    """Exactly 125 distinct valid cubes (the product's capacity), all populated in both classes, one with 600 points; then 126, which the
    product refuses with the handle unchanged; then 125 again: the handle still works."""
    rng = np.random.default_rng(16)
    corner, surf = full_valid_clouds()
    order = rng.permutation(len(FULL_BLOCK))
    valid = [FULL_BLOCK[i] for i in order]
    more = box(rng, 300, (-120.0, -120.0, -120.0), (120.0, 120.0, 120.0), 90000.0)
    return [track([update(corner, surf, valid), snap("near"),
                   update(more, more[::-1], valid + [to_index(13, 10, 5)], rc=LIO_ERR_CAPACITY, only="product"),
                   update(more, more[::-1], valid[::-1]), snap("near")])]


def valid_list():
    """Duplicates; a stale centre (11, 10, 4) that re-bases i = 0 and k = 10 entries outside the window and the others onto populated cubes
    one step away from where their index points; index 4850 (legal) and 4851 (LIO_ERR_ARG on every side, nothing changed)."""
    rng = np.random.default_rng(17)
    base_c, base_s = box(rng, 600, (-170.0, -170.0, -70.0), (170.0, 170.0, 70.0)), box(rng, 900, (-170.0, -170.0, -70.0), (170.0, 170.0, 70.0))
    new_c, new_s = box(rng, 300, (-170.0, -170.0, -70.0), (170.0, 170.0, 70.0), 40000.0), box(rng, 300, (-170.0, -170.0, -70.0), (170.0, 170.0, 70.0), 41000.0)
    some = block(9, 12, 9, 11, 4, 6)
    stale = (11, 10, 4)
    lst = some[::2] + some[:7] + some[::2] + [to_index(0, 10, 5), to_index(0, 0, 0), to_index(10, 10, 10), N_CUBES - 1]
    return [track([update(base_c, base_s), snap("near"),
                   update(new_c, new_s, lst, cen=stale), snap("near"),
                   update(new_s, new_c, lst + [N_CUBES], rc=LIO_ERR_ARG),
                   update(new_s, new_c, [N_CUBES - 1, N_CUBES - 1] + some[1::2]), snap("near")])]


RELAYOUT_A = block(9, 10, 10, 11, 5, 5) + block(10, 10, 10, 10, 6, 6)
RELAYOUT_B = block(11, 12, 9, 9, 4, 5) + block(8, 8, 10, 10, 5, 5)


def relayout_ops(seed=18):
    """Valid sets A, B (disjoint), A u B, A, A (the last one finds the layout in place); new points at every step, so points travel
    rest -> valid -> rest and back.  The stated centre is the fresh handle's: on a used handle the lists re-base like any stale list."""
    rng = np.random.default_rng(seed)
    ops = [update(box(rng, 300, (-130.0, -130.0, -60.0), (130.0, 130.0, 60.0)), box(rng, 400, (-130.0, -130.0, -60.0), (130.0, 130.0, 60.0)))]
    for step, v in enumerate((RELAYOUT_A, RELAYOUT_B, RELAYOUT_A + RELAYOUT_B, RELAYOUT_A, RELAYOUT_A)):
        ops += [update(box(rng, 150, (-130.0, -130.0, -60.0), (130.0, 130.0, 60.0), 1000.0 * (step + 1)),
                       box(rng, 200, (-130.0, -130.0, -60.0), (130.0, 130.0, 60.0), 1000.0 * (step + 1) + 500.0), v), snap("near")]
    ops[-1] = snap("all")
    return ops


def relayout():
    return [track(relayout_ops())]


GENERIC_Q = tuple(float(v) for v in (np.array([0.3, -0.2, 0.5, 0.7], np.float64) / np.linalg.norm([0.3, -0.2, 0.5, 0.7])).astype(F))
# Exactly on the faces 25, -25 and -75, two axes at a time.  All three at once would put the sensor ON a cube corner, where check1 is
# 100 - |pz - pos|^2 = 0 up to rounding: a rounding decision by construction, which the margin rule of the CPU test excludes.
SHIFT_POSES = [(IDENT, (510.4, 23.1, 3.6)),            # 3 cubes on x
               (IDENT, (710.4, -576.9, 153.6)),       # all three axes at once
               (HALF_X, (-282.3, 191.2, -199.6)),     # negative jumps (and the cone looks down)
               (IDENT, (25.0, -25.0, -22.5)), (HALF_Y, (23.9, -25.0, -75.0)), (IDENT, (25.0, 23.8, -75.0)),
               (IDENT, (2010.4, 23.1, 3.6)),          # every populated cube leaves the window ...
               (IDENT, (10.4, 23.1, 3.6)),            # ... and stays empty on the way back
               (GENERIC_Q, (43.7, 73.8, 16.1))]       # the cone cuts the 5 x 5 x 5 block obliquely
# (the offsets inside the cubes were searched for: at a generic offset some far corner lies within 1e-3 of the cone in the measure of
# tests/test_cube_map_ref.py::test_shift_margins, which these poses keep above 1.6e-3)


def shift_ops(seed=19):
    """A map populated out to the window's border, then the window walked through SHIFT_POSES; everything is read after every pose."""
    rng = np.random.default_rng(seed)
    lo, hi = (-520.0, -520.0, -270.0), (520.0, 520.0, 270.0)
    ops = [update(box(rng, 500, lo, hi), box(rng, 700, lo, hi)),
           update(box(rng, 100, (-60.0, -60.0, -60.0), (60.0, 60.0, 60.0), 5000.0), box(rng, 100, (-60.0, -60.0, -60.0), (60.0, 60.0, 60.0), 6000.0),
                  block(9, 11, 9, 11, 4, 6)), snap("all")]
    for q, p in SHIFT_POSES:
        ops += [pose(q, p), snap("all")]
    # the far end of the walk once more with points and an update there, so the way back is not over an empty map
    ops += [pose(IDENT, (-389.6, 23.1, 3.6)), update(box(rng, 200, (-100.0, -100.0, -50.0), (100.0, 100.0, 50.0), 7000.0),
                                                    box(rng, 200, (-100.0, -100.0, -50.0), (100.0, 100.0, 50.0), 8000.0), None, (IDENT, (-389.6, 23.1, 3.6)), None),
            pose(HALF_Z, (10.4, 23.1, 3.6)), snap("all")]
    return ops


def shift():
    return [track(shift_ops())]


def process_small_map():
    """The whole lio_map_process with the init flag clear: association, round trip of the stacks, their VoxelGrids, window, selection, and
    the update with the call's own valid list.  Identity rotations and dyadic translations keep the association exact; the map never holds
    more than 10 corner points, so no side optimises (PointMapping.cc:327-329) and transform_bef_mapped_ stays the identity: the pose
    of call n is the sum of the translations so far.  The last call carries the window away."""
    rng = np.random.default_rng(20)
    ops = []
    for n_c, t in ((4, (0.0, 0.0, 0.0)), (3, (0.5, -0.25, 0.125)), (3, (1.5, 2.0, -0.75)), (0, (0.25, 0.0, 0.0)), (2, (512.0, -64.0, -256.0))):
        ops += [process(box(rng, n_c, (-20.0, -20.0, -5.0), (20.0, 20.0, 5.0), 100.0), box(rng, 150, (-20.0, -20.0, -5.0), (20.0, 20.0, 5.0), 200.0), (IDENT, t)),
                snap("all" if n_c == 2 else "near")]
    return [track(ops)]


def generic_rotation():
    """A non-trivial unit quaternion: the mapped points come back unfiltered (no valid cube), then the same under a valid list.  Oracle
    only: the model's rotation is exact only for half-turns."""
    rng = np.random.default_rng(21)
    T = (GENERIC_Q, (3.3, -2.2, 1.1))
    c, s = box(rng, 500, (-70.0, -70.0, -30.0), (70.0, 70.0, 30.0)), box(rng, 700, (-70.0, -70.0, -30.0), (70.0, 70.0, 30.0))
    return [track([update(c, s, T=T), snap("near")]), track([update(c, s, block(9, 11, 9, 11, 4, 6), T=T), snap("near")])]


def from_map_after_update():
    """laser_cloud_*_from_map_ are those of the last Process until the next Process: read behind direct updates with other valid lists
    and new points, after a Process that did not update the map (init flag set) and after one that did."""
    rng = np.random.default_rng(22)
    lo, hi = (-130.0, -130.0, -60.0), (130.0, 130.0, 60.0)
    a = [update(box(rng, 400, lo, hi), box(rng, 600, lo, hi), block(9, 11, 9, 11, 4, 6)),
         pose(HALF_X, (17.7, -8.8, 0.4)), snap("near"),
         update(box(rng, 200, lo, hi, 3000.0), box(rng, 300, lo, hi, 4000.0), block(8, 9, 9, 10, 5, 5)), snap("near"),
         update(box(rng, 100, lo, hi, 5000.0), box(rng, 100, lo, hi, 6000.0), block(10, 12, 10, 11, 5, 6)), snap("near"),
         pose(IDENT, (60.4, 23.1, 3.6)), snap("near")]
    small = (-20.0, -20.0, -5.0), (20.0, 20.0, 5.0)
    b = [process(box(rng, 4, *small, first_intensity=100.0), box(rng, 150, *small, first_intensity=200.0), (IDENT, (0.0, 0.0, 0.0))),
         process(box(rng, 3, *small, first_intensity=300.0), box(rng, 150, *small, first_intensity=400.0), (IDENT, (0.5, 0.25, 0.0))), snap("near"),
         update(box(rng, 200, lo, hi, 3000.0), box(rng, 300, lo, hi, 4000.0), block(9, 10, 10, 11, 5, 5)), snap("near")]
    return [track(a), track(b)]


def far():
    """The window walked to x = 20 km, and to y = -20 km, in one pose each (400 shifts), an update and a read-back there.  Then 26 km: beyond
    what the product's packed cube keys hold, refused (LIO_ERR_CAPACITY) before anything changes."""
    rng = np.random.default_rng(23)
    tracks = []
    for p, beyond in (((20010.4, 23.1, 3.6), (26010.4, 23.1, 3.6)), ((10.4, -19976.9, 3.6), (10.4, -25976.9, 3.6))):
        c, s = box(rng, 300, (-120.0, -120.0, -60.0), (120.0, 120.0, 60.0)), box(rng, 400, (-120.0, -120.0, -60.0), (120.0, 120.0, 60.0))
        tracks.append(track([pose(IDENT, p), snap("near"), update(c, s, None, (IDENT, p), None), snap("near"), pose(HALF_Z, p), snap("all"),
                             pose(IDENT, beyond, rc=LIO_ERR_CAPACITY, only="product"),
                             update(s, c, None, (IDENT, p), None), snap("near")]))
    return tracks


CASES = {
    "faces": faces, "voxels": voxels, "voxels_equal_leaves": lambda: voxels("equal"), "old_then_new": old_then_new,
    "old_then_new_equal_leaves": lambda: old_then_new("equal"), "sizes": sizes, "full_valid": full_valid, "valid_list": valid_list,
    "relayout": relayout, "shift": shift, "process_small_map": process_small_map, "generic_rotation": generic_rotation,
    "from_map_after_update": from_map_after_update, "far": far,
}
NO_MODEL = ("generic_rotation",)


# ------------------------------------------------------------------------------------------------ handles
class LibMap:
    """A lio_map of a library (product or oracle) behind the calls the runner makes, with the return codes instead of exceptions."""

    def __init__(self, lib, cfg):
        from lio_amd import capi

        self.capi, self.lib = capi, lib
        self.m = capi.PointMapping(lib, **cfg)
        self.cap = 16   # points ever handed in: no cube or cloud can hold more

    def _grow(self, *clouds):
        self.cap += sum(len(c) for c in clouds)

    def update_map_database(self, corner, surf, valid, T, cen):
        self._grow(corner, surf)
        c, s = np.ascontiguousarray(corner, F), np.ascontiguousarray(surf, F)
        v = np.ascontiguousarray(valid, np.uint32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        return int(self.lib.dll.lio_map_update_map_database(self.m.h, fp(c), len(c), fp(s), len(s), v.ctypes.data_as(C.POINTER(C.c_uint32)), len(v),
                                                            C.byref(self.capi.TransformF.make(*T)), (C.c_int * 3)(*[int(x) for x in cen])))

    def process(self, corner, surf, T_sum):
        self._grow(corner, surf)
        c, s = np.ascontiguousarray(corner, F), np.ascontiguousarray(surf, F)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        return int(self.lib.dll.lio_map_process(self.m.h, fp(c), len(c), fp(s), len(s), C.byref(self.capi.TransformF.make(*T_sum)), None, None, None))

    def set_init_flag(self, on):
        self.m.set_init_flag(on)

    def set_transform_tobe_mapped(self, q, p):
        self.m.set_transform_tobe_mapped(q, p)

    def transform_tobe_mapped(self):
        return self.m.transform_tobe_mapped()

    def cube_state(self):
        return self.m.cube_state()

    def cloud(self, which):
        return self.m.cloud(which)

    def cube(self, cls, idx):
        buf = np.empty((self.cap, 4), F)
        n = self.lib.dll.lio_map_get_cube(self.m.h, cls, int(idx), buf.ctypes.data_as(C.POINTER(C.c_float)))
        assert n <= self.cap
        return buf[:n].copy()


def lib_handles(lib):
    return lambda cfg: LibMap(lib, cfg)


def model_handles(cfg):
    return ref.CubeMapModel(*leaves(cfg))


# ------------------------------------------------------------------------------------------------ the runner
def read(h, kind, probe=None, with_stacks=False):
    cen, valid = h.cube_state()
    s = dict(kind=kind, cen=[int(c) for c in cen], valid=np.asarray(valid, np.uint32),
             clouds={w: np.asarray(h.cloud(w), F).reshape(-1, 4) for w in ((0, 1, 2, 3) if with_stacks else (2, 3))})
    if with_stacks:
        q, p = h.transform_tobe_mapped()
        s["pose"] = np.concatenate([np.asarray(q, F), np.asarray(p, F)])
    s["probed"] = None if (kind == "all" or probe is None) else sorted(int(i) for i in probe)
    idxs = range(N_CUBES) if s["probed"] is None else s["probed"]
    s["cubes"] = {}
    for idx in idxs:
        for cls in (0, 1):
            pts = h.cube(cls, idx)
            if len(pts):
                s["cubes"][(cls, idx)] = np.asarray(pts, F).reshape(-1, 4)
    return s


def play(ops, h, side, probes=None, snaps=None):
    """ops on the handle h of `side` ("product", "oracle" or "model"); appends to and returns the list of snapshots.  probes: per snapshot
    (in order) the cube indices a "near" snapshot reads, or None."""
    snaps = [] if snaps is None else snaps
    after_process = False
    for op in ops:
        if op["only"] not in (None, side):
            continue
        if op["op"] == "snap":
            probe = probes[len(snaps)] if probes is not None else None
            snaps.append(read(h, op["kind"], probe, with_stacks=after_process))
            continue
        before = read(h, "all") if op["rc"] != LIO_OK else None
        if op["op"] == "update":
            cen, valid = h.cube_state()
            rc = h.update_map_database(op["corner"], op["surf"], valid if op["valid"] is None else op["valid"], op["T"], cen if op["cen"] is None else op["cen"])
            after_process = False
        elif op["op"] == "pose":
            h.set_init_flag(True)
            h.set_transform_tobe_mapped(op["q"], op["p"])
            rc = h.process(EMPTY, EMPTY, ID)
            after_process = False
        else:
            h.set_init_flag(False)
            rc = h.process(op["corner"], op["surf"], op["T"])
            after_process = True
        assert rc == op["rc"], (side, op["op"], rc, op["rc"])
        if before is not None:
            same(before, read(h, "all"), f"{side}: a refused {op['op']} changed the handle")
    return snaps


def play_case(case, make_handle, side, probes=None):
    snaps = []
    for t in case:
        play(t["ops"], make_handle(t["cfg"]), side, probes, snaps)
    return snaps


def near_probes(snaps):
    """for every snapshot of a side that read everything: its occupied cubes and all their neighbours inside the window"""
    out = []
    for s in snaps:
        idxs = set()
        for _, idx in s["cubes"]:
            i, j, k = ref.from_index(idx)
            idxs.update(to_index(a, b, c) for a in range(max(i - 1, 0), min(i + 2, L)) for b in range(max(j - 1, 0), min(j + 2, W))
                        for c in range(max(k - 1, 0), min(k + 2, H)))
        out.append(idxs)
    return out


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        rows = np.flatnonzero((a.reshape(len(a), -1).view(np.uint32) != b.reshape(len(b), -1).view(np.uint32)).any(axis=1))
        raise AssertionError(f"{what}: {len(rows)} of {len(a)} rows differ in their bits, first row {rows[0]}: {a[rows[0]]!r} != {b[rows[0]]!r}")


def same(a, b, what):
    """two snapshots, bit for bit: the pose first (after a process), valid list in order, clouds in order, every cube either side read, in order"""
    if "pose" in a or "pose" in b:
        same_bits(a["pose"], b["pose"], f"{what}: transform_tobe_mapped")
    assert a["cen"] == b["cen"], (what, a["cen"], b["cen"])
    same_bits(a["valid"], b["valid"], f"{what}: valid list")
    assert a["clouds"].keys() == b["clouds"].keys(), what
    for w in a["clouds"]:
        same_bits(a["clouds"][w], b["clouds"][w], f"{what}: cloud {w}")
    idxs = range(N_CUBES) if (a["probed"] is None and b["probed"] is None) else (b["probed"] if a["probed"] is None else a["probed"])
    for idx in idxs:
        for cls in (0, 1):
            same_bits(a["cubes"].get((cls, idx), EMPTY), b["cubes"].get((cls, idx), EMPTY), f"{what}: class {cls} cube {idx} {ref.from_index(idx)}")


def same_run(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for n, (x, y) in enumerate(zip(a, b)):
        same(x, y, f"{what}, snapshot {n}")
