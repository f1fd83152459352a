"""The segmented grid build of the batched odometry (one bounds pass, one count, one scan, one place over all previous clouds of a call)
under the host-fed lio_odom_process_batch, against lio_odom_process alone (the same build for a batch of one: the comparison pins the
slices and offsets of the shared tables; the build itself is pinned to the serial search by tests/test_gpu_odom_corr.py), bit for bit.  The four sensors of
frontend_batch_cases.grid_sensors sit side by side in every call: a plain cell table, one that spans many chunks of the scan, one above
LIO_ODOM_BATCH_GRID_CELLS_MAX (built by the sensor's own KnnGrid) and one over an 11-point corner cloud.
tests/test_frontend_batch_abi.py asserts the sides without a GPU; here the previous clouds each step really had are checked again."""
import numpy as np
import pytest

from lio_amd import capi
import frontend_batch_cases as cases

pytestmark = pytest.mark.gpu


def _handles(hip, sensors):
    ods = [capi.PointOdometry(hip, *s["params"]) for s in sensors]
    for od, s in zip(ods, sensors):
        for cl in s["prep"]:
            od.process(*cl)
    return ods


def _check_sides(ods, sensors, k):
    for od, s in zip(ods, sensors):                              # the clouds the NEXT step builds its grids over (after TransformToEnd)
        nc, ns = cases.grid_ncells(od.last_cloud(0)), cases.grid_ncells(od.last_cloud(1))
        assert cases.grid_side(s["kind"], nc, ns), (s["kind"], "before step", k, nc, ns)


def _alone(hip, oracle, sensors, n_steps, full):
    ods = _handles(hip, sensors)
    out = []
    for k in range(n_steps):
        _check_sides(ods, sensors, k)
        out.append([cases.state(od, od.process(*s["steps"][k]), full) for od, s in zip(ods, sensors)])
    return out


def test_four_kinds_of_cell_table_in_one_batch(hip, oracle):
    sensors = cases.grid_sensors(oracle, 1)
    full = np.ascontiguousarray(sensors[0]["steps"][0][3][:257])
    want = _alone(hip, oracle, sensors, 1, full)
    ods = _handles(hip, sensors)
    rs = capi.PointOdometry.process_batch(ods, [s["steps"][0] for s in sensors])
    for j, s in enumerate(sensors):
        cases.same(want[0][j], cases.state(ods[j], rs[j], full), (s["kind"], j))
    assert all(int(st["counts"][0]) == 25 and int(st["counts"][1]) > 300 for st in want[0])   # everybody iterates on real correspondences


def test_the_same_handles_again_and_in_reverse_order(hip, oracle):
    """step 0 and step 1 through the same handles in the same order (the count table has to come back zeroed), step 2 with the sensors
    reversed (another lead handle, every base offset moves)"""
    sensors = cases.grid_sensors(oracle, 3)
    full = np.ascontiguousarray(sensors[0]["steps"][0][3][:257])
    want = _alone(hip, oracle, sensors, 3, full)
    ods = _handles(hip, sensors)
    for k, order in enumerate(([0, 1, 2, 3], [0, 1, 2, 3], [3, 2, 1, 0])):
        _check_sides(ods, sensors, k)
        rs = capi.PointOdometry.process_batch([ods[j] for j in order], [sensors[j]["steps"][k] for j in order])
        for j, r in zip(order, rs):
            cases.same(want[k][j], cases.state(ods[j], r, full), (sensors[j]["kind"], j, "step", k))
