"""lio_odom_process_batch (include/lio_odom_batch.h) against lio_odom_process alone: the same sweeps through fresh handles, every
comparison bit for bit (uint32 views) — T_es, T_sum, iterations, selected rows, the whole iteration trace and kz, both last clouds and
lio_odom_full_to_end of a 257-point cloud, per sensor and step.  No tolerance anywhere.  lio_odom_process is the same launch chain for a
batch of one, so what is pinned here is that a sensor's result does not depend on its place in the table, its offsets or its neighbours;
the single-handle results themselves are what the other tests pin to the reference.  The sensors are those of tests/odom_batch_cases.py, which tests/test_odom_batch_abi.py checks on the oracle."""
import ctypes as C

import numpy as np
import pytest

from lio_amd import capi
import odom_batch_cases as cases

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _full(oracle):
    return np.ascontiguousarray(cases.sweeps(oracle, cases.T0S[0], 2)[1][3][:257])


def _handle(hip, sensor):
    od = capi.PointOdometry(hip, *sensor["params"])
    for cl in sensor["prep"]:
        od.process(*cl)
    if sensor["disable"]:
        od.enable(False)
    return od


def _state(od, r, full):
    """everything a caller can see of a handle after a step"""
    trace, kz = od.iteration_trace()
    return dict(T_es=_bits(np.concatenate(r["T_es"])), T_sum=_bits(np.concatenate(r["T_sum"])),
                counts=np.array([r["iterations"], r["num_selected"], kz], np.int64), trace=_bits(trace), last_corner=_bits(od.last_cloud(0)),
                last_surf=_bits(od.last_cloud(1)), full_to_end=_bits(od.full_to_end(full)))


def _same(a, b, what):
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (what, key, a[key].ravel()[:8], b[key].ravel()[:8])


def _run(hip, sensors, full, batched):
    """every sensor through its steps; step k goes through ONE lio_odom_process_batch where batched[k], else through lio_odom_process
    handle by handle -> [step][sensor] states"""
    ods = [_handle(hip, s) for s in sensors]
    out = []
    for k, as_batch in enumerate(batched):
        if as_batch:
            rs = capi.PointOdometry.process_batch(ods, [s["steps"][k] for s in sensors])
        else:
            rs = [od.process(*s["steps"][k]) for od, s in zip(ods, sensors)]
        out.append([_state(od, r, full) for od, r in zip(ods, rs)])
    return out


def _compare(hip, oracle, sensors, n_steps, batched=None):
    full = _full(oracle)
    alone = _run(hip, sensors, full, [False] * n_steps)
    batch = _run(hip, sensors, full, batched or [True] * n_steps)
    for k in range(n_steps):
        for j, s in enumerate(sensors):
            _same(alone[k][j], batch[k][j], (s["name"], j, "step", k))
    return alone


def test_one_sensor_through_the_batch_entry_equals_alone(hip, oracle):
    alone = _compare(hip, oracle, [cases.moving(oracle, 0, 3)], 3)
    assert [int(st[0]["counts"][0]) for st in alone] == [25, 25, 25]


def test_three_moving_sensors_with_their_own_parameters(hip, oracle):
    sensors = [cases.moving(oracle, j, 3) for j in range(3)]
    assert len({s["params"] for s in sensors}) == 3
    alone = _compare(hip, oracle, sensors, 3)
    assert not np.array_equal(alone[0][0]["T_es"], alone[0][1]["T_es"])


def test_mixed_states_in_one_batch(hip, oracle):
    """the eight kinds side by side (and three sensors that converge in the middle of the loop), two steps: the converged, the idle and the
    iterating sensors must not disturb each other"""
    sensors = cases.mixed(oracle, 2)
    alone = _compare(hip, oracle, sensors, 2)
    its = {s["name"]: [int(alone[k][j]["counts"][0]) for k in range(2)] for j, s in enumerate(sensors)}
    print(its)
    assert its["moving0"] == [25, 25] and its["first_call"][0] == 0 and its["packer"] == [0, 0] and its["short_previous"][0] == 0
    assert its["minimal"] == [25, 25] and its["no_queries"] == [25, 25] and its["stationary"][0] < 5
    kz = {s["name"]: int(alone[0][j]["counts"][2]) for j, s in enumerate(sensors)}
    assert kz["degenerate"] > 0 and kz["moving0"] == 0


def test_partition_edges_side_by_side(hip, oracle):
    """nq = 1, 255, 256, 257, 768 and 16 400 (> 64 x 256: the block cap and the stride act for one sensor while its neighbours have one block)"""
    sensors = cases.partition_edges(oracle)
    alone = _compare(hip, oracle, sensors, 1)
    assert int(alone[0][-1]["counts"][1]) > 64 * 256 // 2


@pytest.mark.parametrize("max_iter", [1, 7])
def test_last_iteration_off_the_multiples_of_five(hip, oracle, max_iter):
    sensors = [cases.moving(oracle, j, 2, max_iter=max_iter) for j in range(3)]
    alone = _compare(hip, oracle, sensors, 2)
    assert [int(st["counts"][0]) for st in alone[0]] == [max_iter] * 3


def test_batched_and_single_steps_interleave_on_the_same_handles(hip, oracle):
    sensors = [cases.moving(oracle, j, 3) for j in range(3)] + [cases.stationary(oracle, 3)]
    _compare(hip, oracle, sensors, 3, batched=[True, False, True])


def test_forty_copies_of_one_sensor_around_a_stationary_one(hip, oracle):
    """the race detector: 40 x the same moving sensor and a stationary one in the middle — all 40 identical to each other and to alone"""
    full = _full(oracle)
    mov, stat = cases.moving(oracle, 0, 1), cases.stationary(oracle, 1)
    want = _run(hip, [mov, stat], full, [False])[0]
    sensors = [mov] * 20 + [stat] + [mov] * 20
    got = _run(hip, sensors, full, [True])[0]
    for j, s in enumerate(sensors):
        _same(want[0] if s is mov else want[1], got[j], (s["name"], j))
    assert int(want[0]["counts"][0]) == 25 and int(want[1]["counts"][0]) < 5


def test_handles_with_different_max_iterations_fall_back_to_the_same_bits(hip, oracle):
    sensors = [cases.moving(oracle, 0, 2), cases.moving(oracle, 1, 2, max_iter=7), cases.moving(oracle, 2, 2, max_iter=1)]
    alone = _compare(hip, oracle, sensors, 2)
    assert [int(st["counts"][0]) for st in alone[1]] == [25, 7, 1]


def test_refused_arguments_change_nothing(hip, oracle):
    full = _full(oracle)
    sensors = [cases.moving(oracle, j, 1) for j in range(2)]
    want = _run(hip, sensors, full, [False])[0]
    ods = [_handle(hip, s) for s in sensors]
    cl = [[np.ascontiguousarray(c, np.float32) for c in s["steps"][0]] for s in sensors]

    def call(handles, null_cloud=None):
        n = len(handles)
        H = (C.c_void_p * n)(*[h.h for h in handles])
        args = []
        for w in range(4):
            ptrs = [None if null_cloud == (k, w) else cl[k][w].ctypes.data_as(capi.c_float_p) for k in range(n)]
            args += [(capi.c_float_p * n)(*ptrs), (C.c_size_t * n)(*[len(cl[k][w]) for k in range(n)])]
        return hip.dll.lio_odom_process_batch(H, n, *args, None, None, None, None)

    assert call([ods[0], ods[0]]) == -1                          # LIO_ERR_ARG: the same handle twice
    for where in ((0, 0), (1, 1), (1, 3)):
        assert call(ods, null_cloud=where) == -1, where          # a null cloud with a non-zero count
    rs = capi.PointOdometry.process_batch(ods, [s["steps"][0] for s in sensors])
    for j, (od, r) in enumerate(zip(ods, rs)):
        _same(want[j], _state(od, r, full), ("after refused calls", j))
