"""Inputs of the batched scan-to-map tests (include/lio_map_batch.h): tests/test_map_batch_abi.py asserts on the CPU oracle that every
sensor kind does what its name says, tests/test_gpu_map_batch.py then compares one chain of B sensors (lio_map_process_batch) with B
chains of one (lio_map_process) on twin handles, bit for bit.

The material is mapping_util.drifting_inputs(oracle, "indoor", N_FRAMES): indoor VLP-16 feature clouds with a drifting transform_sum,
extracted once per process.  A sensor is a dict:
  name, kind
  cfg      overrides of lio_map_default_config
  prep     inputs (corner_last, surf_last, T_sum) stepped ALONE before the comparison starts: they bring the handle into the state the kind needs
  init     lio_map_set_init_flag(h, 1) after prep
  full     {step: cloud}: lio_map_set_full_cloud before that step
  steps    the inputs of the comparison, one per step

moving0..2 start at offsets 0, 1, 2 of the one sequence.  On the oracle their iteration counts differ at every one of the first two steps
(10 / 6 / 10, then 7 / 6 / 5) with the drift the sequence has: no scaling of a sensor's drift was needed.

one_block / two_blocks: the row reduction of a sensor has odom_rows_blocks(Mc + Ms) = ceil((Mc + Ms) / 2048) blocks.  The corner cloud of a
sweep alone filters to about 2200 points, so both clouds are cut (the first CUT[kind] raw points of each) to land the filtered stack at
least MARGIN points below / above 2048 on the oracle.
"""
import functools

import numpy as np

from mapping_util import drifting_inputs

N_FRAMES = 8
EMPTY = np.zeros((0, 4), np.float32)
ROW_STEP = 2048                                   # ODOM_ROW_THREADS * 8 (cloud_kernels.hip: odom_rows_blocks)
MARGIN = 100
CUT = {"one_block": (400, 2200), "two_blocks": (700, 4500)}
MOVING_FILTERS = ((0.2, 0.4), (0.25, 0.5), (0.3, 0.35))   # corner_filter_size, surf_filter_size of moving0..2 when they carry their own
SHIFT_M = 400.0


@functools.lru_cache(maxsize=None)
def _frames_cached(oracle_path):
    from lio_amd import capi

    fr = drifting_inputs(capi.LioLib(oracle_path), "indoor", N_FRAMES)
    return tuple((np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.float32),
                  (np.asarray(T[0], np.float64), np.asarray(T[1], np.float64))) for c, s, T, _ in fr)


def frames(oracle):
    """the sequence -> ((corner_last, surf_last, (q_xyzw, p)), ...); treat as read-only"""
    return _frames_cached(oracle.path)


def _sensor(name, kind, steps, prep=(), cfg=None, init=False, full=None):
    return dict(name=name, kind=kind, cfg=dict(cfg or {}), prep=list(prep), init=init, full=dict(full or {}), steps=list(steps))


def moving(oracle, j, n_steps, own_filters=False, **cfg):
    fr = frames(oracle)
    assert j + 1 + n_steps <= N_FRAMES
    if own_filters:
        cfg = dict(cfg, corner_filter_size=MOVING_FILTERS[j][0], surf_filter_size=MOVING_FILTERS[j][1])
    return _sensor(f"moving{j}", "moving", fr[j + 1:j + 1 + n_steps], prep=fr[j:j + 1], cfg=cfg)


def builder(oracle, j, n_steps, extra_prep=0, **cfg):
    """a MapBuilder handle (4-DoF route, every second call optimises); extra_prep = 1 puts it on the other parity of skip_count"""
    fr = frames(oracle)
    p = 1 + extra_prep
    assert j + p + n_steps <= N_FRAMES
    cfg = dict(dict(map_builder=1, enable_4d=1, skip_count=2), **cfg)
    return _sensor(f"builder{j}", "builder", fr[j + p:j + p + n_steps], prep=fr[j:j + p], cfg=cfg)


def still(oracle, j, n_steps):
    """the last sweep of the prep again, with its transform_sum: the association leaves transform_tobe_mapped_ where the step before ended,
    on a map that already holds the sweep, so the loop converges well before the first peek (2 or 3 rounds on the oracle)"""
    fr = frames(oracle)
    return _sensor(f"still{j}", "still", [fr[j + 1]] * n_steps, prep=fr[j:j + 2])


def first_call(oracle, n_steps):
    return _sensor("first_call", "first_call", frames(oracle)[:n_steps])


def small_map(oracle, n_steps):
    """the 8 corner / 60 surf points of test_mapping_first_frame_and_small_maps, twice on a fresh handle as there: the from-map clouds
    are empty, then 8 / 60 points (a third sweep would find 16 / 119 and iterate)"""
    assert n_steps <= 2
    rng = np.random.default_rng(3)
    surf = np.zeros((60, 4), np.float32)
    surf[:, :3] = rng.uniform(-10, 10, (60, 3))
    corner = surf[:8].copy()
    T = (np.array([0, 0, np.sin(0.05), np.cos(0.05)]), np.array([1.0, 2.0, 0.5]))
    return _sensor("small_map", "small_map", [(corner, surf, T)] * n_steps)


def imu_inited(oracle, n_steps):
    fr = frames(oracle)
    return _sensor("imu_inited", "imu_inited", fr[2:2 + n_steps], prep=fr[:2], init=True)


def empty(oracle, n_steps):
    fr = frames(oracle)
    return _sensor("empty", "empty", [(EMPTY, EMPTY, f[2]) for f in fr[2:2 + n_steps]], prep=fr[:2])


def dry(oracle, n_steps):
    fr = frames(oracle)
    return _sensor("dry", "dry", [(np.ascontiguousarray(f[0][:3]), np.ascontiguousarray(f[1][:20]), f[2]) for f in fr[2:2 + n_steps]], prep=fr[:2])


def no_corner(oracle, n_steps):
    fr = frames(oracle)
    return _sensor("no_corner", "no_corner", [(EMPTY, f[1], f[2]) for f in fr[2:2 + n_steps]], prep=fr[:2])


def shifted(oracle, n_steps):
    """transform_sum jumps by SHIFT_M in x from step to step: the association carries the jump into transform_tobe_mapped_, the window
    shifts and both pools are laid out again (test_mapping_window_shift_matches_oracle)"""
    fr = frames(oracle)
    steps = [(f[0], f[1], (f[2][0], f[2][1] + np.array([SHIFT_M * (k + 1), 0.0, 0.0]))) for k, f in enumerate(fr[1:1 + n_steps])]
    return _sensor("shifted", "shifted", steps, prep=fr[:1])


def full_cloud(oracle, n_steps, at=0):
    fr = frames(oracle)
    rng = np.random.default_rng(11)
    cloud = np.zeros((257, 4), np.float32)
    cloud[:, :3] = rng.uniform(-8, 8, (257, 3))
    cloud[:, 3] = rng.uniform(0, 16, 257)
    return _sensor("full_cloud", "full_cloud", fr[2:2 + n_steps], prep=fr[1:2], full={at: cloud})


def blocks(oracle, kind, n_steps):
    fr = frames(oracle)
    nc, ns = CUT[kind]
    cut = [(np.ascontiguousarray(f[0][:nc]), np.ascontiguousarray(f[1][:ns]), f[2]) for f in fr]
    return _sensor(kind, kind, cut[1:1 + n_steps], prep=fr[:1])


def all_kinds(oracle, n_steps=2):
    return [moving(oracle, 0, n_steps), first_call(oracle, n_steps), small_map(oracle, n_steps), moving(oracle, 1, n_steps), imu_inited(oracle, n_steps),
            empty(oracle, n_steps), dry(oracle, n_steps), no_corner(oracle, n_steps), shifted(oracle, n_steps), full_cloud(oracle, n_steps),
            blocks(oracle, "one_block", n_steps), blocks(oracle, "two_blocks", n_steps), moving(oracle, 2, n_steps)]


KINDS = ("moving", "first_call", "small_map", "imu_inited", "empty", "dry", "no_corner", "shifted", "full_cloud", "one_block", "two_blocks")


def make_handle(lib, sensor):
    """a PointMapping of `lib` brought through the sensor's prep"""
    from lio_amd import capi

    m = capi.PointMapping(lib, **sensor["cfg"])
    for inp in sensor["prep"]:
        m.process(*inp)
    if sensor["init"]:
        m.set_init_flag(True)
    return m


def run_alone(lib, sensor, observe=None):
    """the sensor through lio_map_process of `lib` -> per step (the dict PointMapping.process returns, observe(handle) or None)"""
    m = make_handle(lib, sensor)
    out = []
    for k, inp in enumerate(sensor["steps"]):
        if k in sensor["full"] and lib.has_ext:   # (lio_full_cloud.h is the product's; the oracle's pose does not hang on it)
            m.set_full_cloud(sensor["full"][k])
        r = m.process(*inp)
        out.append((r, observe(m) if observe else None))
    return out
