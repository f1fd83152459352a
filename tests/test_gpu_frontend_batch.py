"""lio_odom_process_batch_from_pp (include/lio_frontend_batch.h) against lio_odom_process alone (the same chain, host-fed, for a batch of one).  The raw sweeps of
tests/frontend_batch_cases.py go through the product's PointProcessor ONCE per step; one set of odometry handles is then fed from the
processors on the device, a twin set is fed what lio_pp_get_cloud returns through lio_odom_process, handle by handle.  Every comparison is
bit for bit (uint32 views) over the state tests/test_gpu_odom_batch.py compares: T_es, T_sum, iterations, selected rows, the iteration
trace and kz, both last clouds and lio_odom_full_to_end of a 257-point cloud, per sensor and step.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the product library is loaded: both bring a HIP runtime, torch must come first)

from lio_amd import capi
import frontend_batch_cases as cases

pytestmark = pytest.mark.gpu
ERR_STATE = -2


def _full():
    return np.ascontiguousarray(cases.raw("indoor", cases.T0S[0], 2)[0][1][:257])


def _pp(hip, lid):
    return capi.PointProcessor(hip, lid.lower_deg, lid.upper_deg, lid.rings)


def _clouds(pp):
    return [pp.cloud(w) for w in (1, 2, 3, 4)]


def _snapshot(pp):
    """what the accessors answer: the four clouds (and so their counts) and the indices of the three picked classes"""
    out = [cases.bits(c) for c in _clouds(pp)]
    for w in (1, 2, 3):
        out += list(pp.indices(w))
    return out


def _each_alone(pps, sweeps):
    for pp, x in zip(pps, sweeps):
        pp.process(x)


class Rig:
    """the processors of some sensors and two sets of odometry handles: `fed` for the route under test, `alone` for lio_odom_process.
    proc[j]: the processor sensor j reads (default: its own)."""

    def __init__(self, hip, sensors, proc=None, n_procs=None):
        self.hip, self.sensors, self.full = hip, sensors, _full()
        self.proc = list(proc) if proc is not None else list(range(len(sensors)))
        owner = {}
        for j, p in enumerate(self.proc):                         # the first sensor that names a processor supplies its sweeps
            owner.setdefault(p, j)
        self.owner = [owner[p] for p in range(n_procs or len(owner))]
        self.pps = [_pp(hip, sensors[j]["lidar"]) for j in self.owner]
        self.alone = [capi.PointOdometry(hip, *s["params"]) for s in sensors]
        self.fed = [capi.PointOdometry(hip, *s["params"]) for s in sensors]
        for i in range(max(len(s["prep"]) for s in sensors)):
            for p, j in enumerate(self.owner):
                if len(sensors[j]["prep"]) > i:
                    self.pps[p].process(sensors[j]["prep"][i])
            for j, s in enumerate(sensors):
                if len(s["prep"]) > i:
                    cl = _clouds(self.pps[self.proc[j]])
                    self.alone[j].process(*cl), self.fed[j].process(*cl)
        for j, s in enumerate(sensors):
            if s["disable"]:
                self.alone[j].enable(False), self.fed[j].enable(False)

    def step(self, k, feed=_each_alone, route="pp"):
        """sweep k of every processor through `feed`, then every sensor one step -> per sensor the state of the alone handle (the fed
        handle's has been asserted equal)"""
        feed(self.pps, [self.sensors[j]["steps"][k] for j in self.owner])
        before = [_snapshot(pp) for pp in self.pps]
        cl = [_clouds(pp) for pp in self.pps]
        ra = [od.process(*cl[p]) for od, p in zip(self.alone, self.proc)]
        if route == "pp":
            rf = capi.PointOdometry.process_batch_from_pp(self.fed, [self.pps[p] for p in self.proc])
        elif route == "batch":
            rf = capi.PointOdometry.process_batch(self.fed, [cl[p] for p in self.proc])
        else:
            rf = [od.process(*cl[p]) for od, p in zip(self.fed, self.proc)]
        for p, pp in enumerate(self.pps):                         # the processors are only read
            for x, y in zip(before[p], _snapshot(pp)):
                assert x.shape == y.shape and np.array_equal(x, y), ("processor changed", p, k)
        out = []
        for j, s in enumerate(self.sensors):
            a, f = cases.state(self.alone[j], ra[j], self.full), cases.state(self.fed[j], rf[j], self.full)
            cases.same(a, f, (s["name"], j, "step", k, route))
            out.append(a)
        return out


def test_one_sensor_from_a_processor_with_its_own_storage(hip):
    rig = Rig(hip, [cases.moving(0, 3)])
    its = [int(rig.step(k)[0]["counts"][0]) for k in range(3)]
    assert its == [25, 25, 25]


def test_three_moving_sensors_from_pooled_storage(hip):
    """lio_pp_process_batch twice, lio_pp_process_batch_device once: the handles read their sweep of the shared processor"""
    sensors = [cases.moving(j, 3) for j in range(3)]
    assert len({s["params"] for s in sensors}) == 3
    rig = Rig(hip, sensors)

    def from_device(pps, sweeps):
        dev = [torch.from_numpy(x).cuda() for x in sweeps]
        torch.cuda.synchronize()
        capi.PointProcessor.process_batch_device(pps, [t.data_ptr() for t in dev], [t.shape[0] for t in dev])

    got = [rig.step(0, capi.PointProcessor.process_batch), rig.step(1, from_device), rig.step(2, capi.PointProcessor.process_batch)]
    assert all(int(st["counts"][0]) == 25 for step in got for st in step)
    assert not np.array_equal(got[0][0]["T_es"], got[0][1]["T_es"])


def test_mixed_kinds_and_sensor_types_in_one_call(hip):
    """moving, stationary, first call, packer, thin previous sweep, empty sweep and an HDL-64E in one call, two steps; the VLP-16 processors
    share a pool, the HDL-64E one keeps its own storage"""
    sensors = cases.mixed(2)
    names = [s["name"] for s in sensors]
    rig = Rig(hip, sensors)

    def feed(pps, sweeps):
        vlp = [p for p, s in enumerate(sensors) if s["lidar"].rings == 16]
        capi.PointProcessor.process_batch([pps[p] for p in vlp], [sweeps[p] for p in vlp])
        for p, s in enumerate(sensors):
            if s["lidar"].rings != 16:
                pps[p].process(sweeps[p])

    got = [rig.step(k, feed) for k in range(2)]
    its = {n: [int(got[k][j]["counts"][0]) for k in range(2)] for j, n in enumerate(names)}
    print(its)
    assert its["moving0"] == [25, 25] and its["moving2"] == [25, 25] and its["hdl64"] == [25, 25]
    assert its["first_call"][0] == 0 and its["first_call"][1] == 25 and its["packer"] == [0, 0]
    assert its["thin"] == [0, 25]                                # nothing to iterate against, then an ordinary step
    assert its["empty"] == [25, 0]                               # no queries: the iterations run empty; then no previous sweep
    assert its["stationary"][0] < 5
    assert [int(got[0][names.index("empty")][key].size) for key in ("last_corner", "last_surf")] == [0, 0]


def test_forty_handles_fed_from_one_processor(hip):
    mov, other = cases.moving(0, 1), cases.moving(1, 1)
    sensors = [mov] * 20 + [other] + [mov] * 20
    rig = Rig(hip, sensors, proc=[0] * 20 + [1] + [0] * 20)
    assert len(rig.pps) == 2
    got = rig.step(0, capi.PointProcessor.process_batch)
    for j, s in enumerate(sensors):
        if s is mov:
            cases.same(got[0], got[j], ("copy", j))
    assert int(got[0]["counts"][0]) == 25 and not np.array_equal(got[0]["T_es"], got[20]["T_es"])


def test_the_three_entry_points_interleave_on_the_same_handles(hip):
    rig = Rig(hip, [cases.moving(j, 3) for j in range(3)] + [cases.stationary(3)])
    rig.step(0, capi.PointProcessor.process_batch, route="pp")
    rig.step(1, capi.PointProcessor.process_batch, route="batch")
    rig.step(2, capi.PointProcessor.process_batch, route="alone")


def test_handles_with_different_max_iterations_fall_back_to_the_same_bits(hip):
    rig = Rig(hip, [cases.moving(0, 2), cases.moving(1, 2, max_iter=7), cases.moving(2, 2, max_iter=1)])
    got = [rig.step(k, capi.PointProcessor.process_batch) for k in range(2)]
    assert [int(st["counts"][0]) for st in got[1]] == [25, 7, 1]


def test_refused_processors_change_nothing(hip):
    """a processor that never processed, and one whose pooled sweep a later lio_pp_process_batch of its neighbours overwrote: LIO_ERR_STATE,
    and the next ordinary step of every odometry handle equals its twin's, which saw none of it"""
    sensors = [cases.moving(j, 2) for j in range(3)]
    rig = Rig(hip, sensors)
    rig.step(0, capi.PointProcessor.process_batch)

    def call(ods, pps):
        n = len(ods)
        H, P = (C.c_void_p * n)(*[o.h for o in ods]), (C.c_void_p * n)(*[p.h for p in pps])
        T = (capi.TransformF * n)()
        it = np.full(n, 7, np.int32)
        rc = hip.dll.lio_odom_process_batch_from_pp(H, P, n, T, T, it.ctypes.data_as(capi.c_int32_p), None)
        assert rc != 0 and list(it) == [7] * n                   # outputs untouched
        return rc

    fresh = _pp(hip, sensors[0]["lidar"])
    assert call(rig.fed, [rig.pps[0], fresh, rig.pps[2]]) == ERR_STATE
    assert call(rig.fed[:2], [rig.pps[0], fresh]) == ERR_STATE
    assert call([rig.fed[0], rig.fed[0]], rig.pps[:2]) == -1     # LIO_ERR_ARG: the same odometry handle twice
    stale = [_snapshot(pp) for pp in rig.pps[:2]]
    capi.PointProcessor.process_batch(rig.pps[:2], [sensors[j]["steps"][0] for j in range(2)])   # the same sweeps again, without the third handle
    for p in range(2):
        for x, y in zip(stale[p], _snapshot(rig.pps[p])):
            assert np.array_equal(x, y)
    assert hip.dll.lio_pp_get_cloud(rig.pps[2].h, 1, np.zeros((4096, 4), np.float32).ctypes.data_as(capi.c_float_p)) == ERR_STATE
    assert call(rig.fed, rig.pps) == ERR_STATE
    assert call(rig.fed[2:], rig.pps[2:]) == ERR_STATE
    rig.step(1, capi.PointProcessor.process_batch)
