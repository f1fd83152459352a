"""Inputs of the tests of include/lio_frontend_batch.h.  tests/test_frontend_batch_abi.py asserts without a GPU that every sensor and every
crafted cloud is what its name says; tests/test_gpu_frontend_batch.py (lio_odom_process_batch_from_pp) and
tests/test_gpu_odom_batch_grids.py (the segmented grid build under the host-fed lio_odom_process_batch) then compare with
lio_odom_process alone, bit for bit.

Sensors of the from-pp tests are RAW sweeps (synth.make_sweeps), because the PointProcessor is part of what is tested.  A sensor is a dict:
  name, lidar
  params   scan_period, io_ratio, max_iter, no_deskew of lio_odom_create
  prep     raw sweeps whose feature clouds are stepped through lio_odom_process before the comparison starts
  disable  lio_odom_enable(h, 0) after prep
  steps    the raw sweeps of the comparison, one per step
"""
import functools
import os
import re

import numpy as np

from lio_amd import synth
import odom_batch_cases as obc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0S = obc.T0S
EMPTY_SWEEP = np.zeros((0, 4), np.float32)


def grid_cells_max():
    text = open(os.path.join(ROOT, "include", "lio_frontend_batch.h")).read()
    return int(re.search(r"#define LIO_ODOM_BATCH_GRID_CELLS_MAX (\d+)\b", text).group(1))


# ---------------------------------------------------------------- raw sweeps
@functools.lru_cache(maxsize=None)
def _raw(kind, t0, n):
    sweeps, _, lid = synth.make_sweeps(kind, n, t0=t0)
    return tuple(np.ascontiguousarray(s, np.float32) for s in sweeps), lid


def raw(kind, t0, n):
    """n consecutive sweeps from t0 -> (sweeps, lidar); treat as read-only"""
    return _raw(kind, float(t0), int(n))


def thin_sweep(sweep):
    """a VLP-16 sweep reduced to its two rings around the horizon and a 20 degree sector: too few features for the next sweep to iterate on"""
    el = np.degrees(np.arctan2(sweep[:, 2], np.hypot(sweep[:, 0], sweep[:, 1])))
    az = np.degrees(np.arctan2(sweep[:, 1], sweep[:, 0]))
    return np.ascontiguousarray(sweep[(el > -2) & (el < 2) & (np.abs(az) < 10)])


def _sensor(name, lidar, steps, prep=(), io_ratio=2, max_iter=25, no_deskew=False, disable=False):
    return dict(name=name, lidar=lidar, params=(0.1, io_ratio, max_iter, bool(no_deskew)), prep=list(prep), disable=disable, steps=list(steps))


def moving(j, n_steps, max_iter=25):
    """moving sensor j = 0, 1, 2: its own t0, io_ratio 1 / 2 / 3, the last one without de-skew"""
    sw, lid = raw("indoor", T0S[j], n_steps + 1)
    return _sensor(f"moving{j}", lid, sw[1:n_steps + 1], prep=sw[:1], io_ratio=j + 1, max_iter=max_iter, no_deskew=(j == 2))


def stationary(n_steps):
    sw, lid = raw("indoor", T0S[0], 2)
    return _sensor("stationary", lid, [sw[0]] * n_steps, prep=sw[:1], no_deskew=True)


def first_call(n_steps):
    sw, lid = raw("indoor", T0S[0], n_steps + 1)
    return _sensor("first_call", lid, sw[:n_steps])


def packer(n_steps):
    sw, lid = raw("indoor", T0S[1], n_steps + 1)
    return _sensor("packer", lid, sw[1:n_steps + 1], prep=sw[:1], disable=True)


def thin_previous(n_steps):
    sw, lid = raw("indoor", T0S[2], n_steps + 1)
    return _sensor("thin", lid, sw[1:n_steps + 1], prep=[thin_sweep(sw[0])])


def empty_sweep(n_steps):
    """step 0 is a sweep without a point (iterations with no queries, then nothing to iterate against), the later ones are ordinary"""
    sw, lid = raw("indoor", T0S[1], n_steps + 1)
    return _sensor("empty", lid, [EMPTY_SWEEP] + list(sw[2:n_steps + 1]), prep=sw[:1])


def hdl64(n_steps):
    sw, lid = raw("outdoor", 1.0, n_steps + 1)
    return _sensor("hdl64", lid, sw[1:n_steps + 1], prep=sw[:1])


def mixed(n_steps=2):
    return [moving(0, n_steps), stationary(n_steps), first_call(n_steps), packer(n_steps), thin_previous(n_steps), empty_sweep(n_steps), moving(2, n_steps),
            hdl64(n_steps)]


# ---------------------------------------------------------------- the grids of the batch, restated
CELL = np.float32(5.0) * np.float32(1.0001)   # odometry.hip: 5.0f * 1.0001f


def grid_ncells(cloud):
    """cells of the 5 m grid the odometry builds over a previous cloud: grid_extent (cloud_kernels.h) over the bounds of its finite points,
    in fp32 as the host computes it"""
    xyz = np.asarray(cloud, np.float32)[:, :3]
    xyz = xyz[np.all(np.isfinite(xyz), axis=1)]
    mn, mx = (xyz.min(axis=0), xyz.max(axis=0)) if len(xyz) else (np.zeros(3, np.float32), np.zeros(3, np.float32))
    inv = np.float32(1.0) / CELL
    n = 1
    for d in range(3):
        lo = int(np.floor(np.float32(mn[d] * inv))) - 1
        hi = int(np.floor(np.float32(mx[d] * inv))) + 1
        n *= hi - lo + 1
    return n


def with_outliers(cloud, offsets):
    """`cloud` with one point added per (dx, dy): the cloud's LAST point moved there, its intensity (ring + relative time) kept, so the
    cloud stays in ring order"""
    extra = np.repeat(cloud[-1:], len(offsets), axis=0).copy()
    for row, (dx, dy) in zip(extra, offsets):
        row[0] += np.float32(dx)
        row[1] += np.float32(dy)
    return np.ascontiguousarray(np.concatenate([cloud, extra]), np.float32)


FAR_X = ((-1500.0, 0.0), (1500.0, 0.0))                                    # a long, thin table: many scan chunks, under the limit
FAR_XY = ((-1500.0, 0.0), (1500.0, 0.0), (0.0, -600.0), (0.0, 600.0))    # over the limit: built by the sensor's own KnnGrid
GRID_KINDS = ("plain", "long_x", "over_limit", "corner11")


def grid_sensors(oracle, n_steps=3):
    """four sensors (dicts of odom_batch_cases) from the indoor sweeps, whose PREVIOUS clouds give four kinds of cell table at every step:
    the less-flat cloud of every sweep of long_x / over_limit carries the outliers, the less-sharp cloud of every sweep of corner11 is cut to
    the 11 points an iterating sensor needs at least"""
    out = []
    for j, kind in enumerate(GRID_KINDS):
        sw = obc.sweeps(oracle, T0S[j % 3], n_steps + 1)
        if kind == "long_x":
            sw = [(c[0], c[1], c[2], with_outliers(c[3], FAR_X)) for c in sw]
        elif kind == "over_limit":
            sw = [(c[0], c[1], c[2], with_outliers(c[3], FAR_XY)) for c in sw]
        elif kind == "corner11":
            sw = [(c[0], np.ascontiguousarray(c[1][:11]), c[2], c[3]) for c in sw]
        out.append(dict(name=kind, kind=kind, params=(0.1, 2, 25, False), prep=[sw[0]], disable=False, steps=list(sw[1:n_steps + 1])))
    return out


def grid_side(kind, n_corner_cells, n_surf_cells):
    """what grid_sensors promises of a sensor's two tables"""
    limit = grid_cells_max()
    if kind == "long_x":
        return n_corner_cells < 4096 and 5 * 4096 < n_surf_cells < limit * 3 // 4        # more than five chunks of the scan, well under the limit
    if kind == "over_limit":
        return n_corner_cells < 4096 and n_surf_cells > 2 * limit
    return n_corner_cells < 4096 and n_surf_cells < 4096                                 # one chunk each


# ---------------------------------------------------------------- what a caller can see of a handle (the set of tests/test_gpu_odom_batch.py)
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def state(od, r, full):
    trace, kz = od.iteration_trace()
    return dict(T_es=bits(np.concatenate(r["T_es"])), T_sum=bits(np.concatenate(r["T_sum"])),
                counts=np.array([r["iterations"], r["num_selected"], kz], np.int64), trace=bits(trace), last_corner=bits(od.last_cloud(0)),
                last_surf=bits(od.last_cloud(1)), full_to_end=bits(od.full_to_end(full)))


def same(a, b, what):
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (what, key, a[key].ravel()[:8], b[key].ravel()[:8])
