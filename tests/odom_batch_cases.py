"""Inputs of the batched scan-to-scan odometry tests (include/lio_odom_batch.h): tests/test_odom_batch_abi.py asserts on the CPU oracle
that every sensor kind does what its name says, tests/test_gpu_odom_batch.py then compares lio_odom_process_batch with lio_odom_process
alone, bit for bit.

The material is VLP-16 sweeps of synth.make_sweeps("indoor", ...) through the ORACLE's PointProcessor (ref_odom_cases.feature_clouds),
made once per process.  A sensor is a dict:
  name, kind
  params   scan_period, io_ratio, max_iter, no_deskew of lio_odom_create
  prep     sweeps (four clouds each) stepped ALONE before the comparison starts: they bring the handle into the state the kind needs
  disable  lio_odom_enable(h, 0) after prep
  steps    the sweeps of the comparison, one per step
"""
import functools

import numpy as np

from lio_amd import synth
from ref_odom_cases import feature_clouds
import degenerate_util

T0S = (1.0, 3.0, 5.5)
EMPTY = np.zeros((0, 4), np.float32)


@functools.lru_cache(maxsize=None)
def _sweeps_cached(oracle_path, t0, n):
    from lio_amd import capi

    oracle = capi.LioLib(oracle_path)
    sweeps, _, lid = synth.make_sweeps("indoor", n, t0=t0)
    return tuple(tuple(feature_clouds(oracle, lid, sw)) for sw in sweeps)


def sweeps(oracle, t0=1.0, n=4):
    """n consecutive sweeps from t0 -> ((sharp, less_sharp, flat, less_flat), ...); treat as read-only"""
    return _sweeps_cached(oracle.path, float(t0), int(n))


@functools.lru_cache(maxsize=None)
def _ground_cached(oracle_path):
    from lio_amd import capi

    cl, singular = degenerate_util.odometry_sweeps(capi.LioLib(oracle_path), "ground_one_pole", 3)
    assert singular
    return tuple(tuple(c) for c in cl)


def _sensor(name, kind, steps, prep=(), io_ratio=2, max_iter=25, no_deskew=False, disable=False):
    return dict(name=name, kind=kind, params=(0.1, io_ratio, max_iter, bool(no_deskew)), prep=list(prep), disable=disable, steps=list(steps))


def cut(cl, n_sharp, n_less_sharp, n_flat, n_less_flat):
    return tuple(np.ascontiguousarray(c[:n]) for c, n in zip(cl, (n_sharp, n_less_sharp, n_flat, n_less_flat)))


def moving(oracle, j, n_steps, max_iter=25):
    """moving sensor j = 0, 1, 2: its own t0, io_ratio 1 / 2 / 3, the last one without de-skew"""
    sw = sweeps(oracle, T0S[j], n_steps + 1)
    return _sensor(f"moving{j}", "moving", sw[1:n_steps + 1], prep=sw[:1], io_ratio=j + 1, max_iter=max_iter, no_deskew=(j == 2))


def stationary(oracle, n_steps):
    sw = sweeps(oracle, T0S[0], 2)
    return _sensor("stationary", "stationary", [sw[0]] * n_steps, prep=sw[:1], no_deskew=True)


def first_call(oracle, n_steps, j=0):
    sw = sweeps(oracle, T0S[j], n_steps + 1)
    return _sensor("first_call", "first_call", sw[:n_steps])


def packer(oracle, n_steps):
    sw = sweeps(oracle, T0S[1], n_steps + 1)
    return _sensor("packer", "packer", sw[1:n_steps + 1], prep=sw[:1], disable=True)


def short_previous(oracle, n_steps):
    sw = sweeps(oracle, T0S[2], n_steps + 1)
    c0 = sw[0]
    return _sensor("short_previous", "short_previous", sw[1:n_steps + 1], prep=[(c0[0], np.ascontiguousarray(c0[1][:10]), c0[2], c0[3])])


def minimal(oracle, n_steps):
    sw = [cut(c, 1, 11, 3, 101) for c in sweeps(oracle, T0S[0], n_steps + 1)]
    return _sensor("minimal", "minimal", sw[1:n_steps + 1], prep=sw[:1])


def no_queries(oracle, n_steps):
    sw = sweeps(oracle, T0S[1], n_steps + 1)
    return _sensor("no_queries", "no_queries", [(EMPTY, c[1], EMPTY, c[3]) for c in sw[1:n_steps + 1]], prep=sw[:1])


def degenerate(oracle, n_steps):
    g = _ground_cached(oracle.path)
    assert n_steps <= 2
    return _sensor("degenerate", "degenerate", g[1:n_steps + 1], prep=g[:1])


# Rigid copies of one sweep (rotation about (1, 1, 1) by `angle` rad, translation (d, 0.3 d, 0) m) converge in the MIDDLE of the loop on the
# oracle — after 7, 13 and 21 iterations — so a peek finds converged and unconverged sensors side by side more than once.  (The pairs the
# sensor itself moves through run all 25 iterations, a sweep against itself converges after 1.)
CONVERGING = ((0.0012, 0.012), (0.005, 0.011), (0.001, 0.02))


def _moved(cl, angle, d):
    ax = np.ones(3) / np.sqrt(3.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    out = []
    for c in cl:
        m = c.copy()
        m[:, :3] = (c[:, :3].astype(np.float64) @ R.T + np.array([d, 0.3 * d, 0.0])).astype(np.float32)
        out.append(m)
    return tuple(out)


def converging(oracle, i, n_steps):
    c0 = sweeps(oracle, T0S[0], 2)[0]
    steps = [c0]
    for _ in range(n_steps):
        steps.append(_moved(steps[-1], *CONVERGING[i]))
    return _sensor(f"converging{i}", "converging", steps[1:], prep=steps[:1])


def mixed(oracle, n_steps=2):
    """all eight kinds side by side, the moving one three times, and the three sensors that converge in the middle of the loop"""
    return [converging(oracle, 0, n_steps), converging(oracle, 1, n_steps), converging(oracle, 2, n_steps), moving(oracle, 0, n_steps),
            stationary(oracle, n_steps), first_call(oracle, n_steps), packer(oracle, n_steps), short_previous(oracle, n_steps), minimal(oracle, n_steps),
            no_queries(oracle, n_steps), degenerate(oracle, n_steps), moving(oracle, 1, n_steps), moving(oracle, 2, n_steps)]


PARTITION_NQ = (1, 255, 256, 257, 768, 16400)


def partition_edges(oracle):
    """six sensors from one sweep pair whose query counts sit on the edges of the row partition (256 threads per block, at most 64
    blocks): 1, 255, 256, 257, 768 and >= 16 400 = more than 64 * 256.  Queries are the sharp points followed by the flat points tiled
    as often as it takes; the previous clouds are the sweep's own."""
    sw = sweeps(oracle, T0S[0], 2)
    sharp, less_sharp, flat, less_flat = sw[1]
    out = []
    for nq in PARTITION_NQ:
        ns = min(len(sharp), nq // 3)
        nf = nq - ns
        fl = np.ascontiguousarray(np.tile(flat, (nf // len(flat) + 1, 1))[:nf])
        out.append(_sensor(f"nq{nq}", "partition", [(np.ascontiguousarray(sharp[:ns]), less_sharp, fl, less_flat)], prep=sw[:1]))
    return out


def run_alone(lib, sensor):
    """the sensor through lio_odom_process of `lib` -> per step the dict PointOdometry.process returns"""
    from lio_amd import capi

    od = capi.PointOdometry(lib, *sensor["params"])
    for cl in sensor["prep"]:
        od.process(*cl)
    if sensor["disable"]:
        od.enable(False)
    return [od.process(*cl) for cl in sensor["steps"]]
