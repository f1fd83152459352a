"""The device code behind include/lio_full_cloud.h on the GPU: TransformToEnd in its two estimator forms (lio_deskew_to_end), the
odometry's form on the full cloud (lio_odom_full_to_end) and the rigid map of the scan-to-map stage (lio_map_set_full_cloud /
lio_map_process / lio_map_get_full_cloud), against tests/full_cloud_ref.py.

x y z of TransformToEnd are held to 4 x K_DESKEW x 2^-24 x (|p| + |t_es|) per point against the float64 evaluation: K_DESKEW is what
numpy float32 in the same operation order loses (tests/test_full_cloud_ref.py measures it), the factor 4 covers the device's acos, sin,
sqrt and division.  Everything without a transcendental is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from lio_amd import capi, pipeline, synth
import full_cloud_cases as cases
import full_cloud_ref as ref

pytestmark = pytest.mark.gpu

GPU_BOUND = ref.GPU_BOUND_FACTOR * ref.K_DESKEW
IDENT = ([0, 0, 0, 1], [0, 0, 0])


def test_deskew_to_end_both_forms_against_fp64(hip):
    worst = {0: 0.0, 1: 0.0}
    for name, c, q, t in cases.all_cases():
        T = capi.TransformF.make(q, t)
        keep, strip = hip.deskew_to_end(c, T, cases.TIME_FACTOR, True), hip.deskew_to_end(c, T, cases.TIME_FACTOR, False)
        assert keep.shape == strip.shape == c.shape
        for k, got in ((1, keep), (0, strip)):
            r = ref.worst_ratio(got[:, :3], c, q, t, time_factor=cases.TIME_FACTOR, form="est", keep_intensity=bool(k))
            worst[k] = max(worst[k], r)
            assert r <= GPU_BOUND, (name, k, r)
        assert keep[:, :3].tobytes() == strip[:, :3].tobytes(), name          # one device body: the same bits
        assert keep[:, 3].tobytes() == c[:, 3].tobytes(), name                 # keep_intensity: the input's bits
        assert strip[:, 3].tobytes() == (c[:, 3] - np.trunc(c[:, 3])).astype(np.float32).tobytes(), name   # the fraction
    print(f"worst |gpu - fp64| / (2^-24 (|p| + |t|)): keep {worst[1]:.3f}  strip {worst[0]:.3f}  (K_DESKEW {ref.K_DESKEW}, bound {GPU_BOUND:.2f})")


def test_deskew_to_end_identity_is_an_exact_no_op_and_n0_writes_nothing(hip):
    T = capi.TransformF.make(*IDENT)
    for n in cases.SIZES:
        c = cases.integer_intensity_cloud(n)
        assert hip.deskew_to_end(c, T, cases.TIME_FACTOR, True).tobytes() == c.tobytes(), n
        strip = hip.deskew_to_end(c, T, cases.TIME_FACTOR, False)    # the production form strips the ring: x y z untouched, w = 0
        assert strip[:, :3].tobytes() == c[:, :3].tobytes() and not np.any(strip[:, 3]), n
    c = cases.cloud(257)                                         # any intensity: x y z survive the identity
    assert hip.deskew_to_end(c, T, cases.TIME_FACTOR, True).tobytes() == c.tobytes()
    out = np.full((3, 4), 7.0, np.float32)
    fp = C.POINTER(C.c_float)
    assert hip.dll.lio_deskew_to_end(None, 0, C.byref(T), 10.0, 1, out.ctypes.data_as(fp)) == 0
    assert np.all(out == 7.0)
    assert hip.dll.lio_deskew_to_end(None, 0, C.byref(T), 10.0, 0, None) == 0


@pytest.fixture(scope="module")
def odom_step(hip):
    """one real lio_odom_process on a VLP-16 synthetic sweep pair"""
    sweeps, _, lid = synth.make_sweeps("indoor", 2)
    assert lid.rings == 16
    od = capi.PointOdometry(hip, 0.1, 2, 25, False)
    cl = []
    for sw in sweeps:
        pp = capi.PointProcessor(hip, lid.lower_deg, lid.upper_deg, lid.rings)
        pp.process(sw)
        cl.append([pp.cloud(w) for w in (1, 2, 3, 4)])
    full0 = np.concatenate([cl[0][1], cl[0][3]])
    od.process(*cl[0])
    first = od.full_to_end(full0)                                # :302-310: the first call publishes nothing; the cloud passes through
    r = od.process(*cl[1])
    return od, cl, r, (full0, first)


def test_odom_full_to_end_is_the_body_that_carried_the_feature_clouds(hip, odom_step):
    od, cl, r, (full0, first) = odom_step
    assert first.tobytes() == full0.tobytes()
    assert r["iterations"] > 0 and np.linalg.norm(r["T_es"][1]) > 1e-3
    less_sharp, less_flat = cl[1][1], cl[1][3]
    assert len(less_sharp) > 50 and len(less_flat) > 500
    full = np.concatenate([less_sharp, less_flat])
    assert np.any(full[:, 3] != np.trunc(full[:, 3]))
    got = od.full_to_end(full)
    want = np.concatenate([od.last_cloud(0), od.last_cloud(1)])
    assert got.tobytes() == want.tobytes()                       # same body, same transform_es_
    np.testing.assert_array_equal(got[:, 3], np.trunc(full[:, 3]))
    assert not np.array_equal(got[:, :3], full[:, :3])
    # in place, and the empty cloud
    buf = full.copy()
    fp = C.POINTER(C.c_float)
    assert hip.dll.lio_odom_full_to_end(od.h, buf.ctypes.data_as(fp), len(buf), buf.ctypes.data_as(fp)) == 0
    assert buf.tobytes() == want.tobytes()
    assert od.full_to_end(np.zeros((0, 4), np.float32)).shape == (0, 4)
    od.enable(False)                                             # /enable_odom off: a byte copy
    assert od.full_to_end(full).tobytes() == full.tobytes()
    od.enable(True)
    assert od.full_to_end(full).tobytes() == want.tobytes()


def test_map_registers_the_full_cloud_once_per_set(hip):
    ds = synth.make_dataset("indoor", 3, 0.2)
    clouds = [pipeline.feature_clouds(hip, ds.lidar, f.scan) for f in ds.frames]     # (surf, corner)
    m = capi.PointMapping(hip)
    assert len(m.full_cloud()) == 0
    full = cases.cloud(2049)
    # an empty map: no optimisation runs, transform_tobe_mapped_ is the prediction
    m.set_full_cloud(full)
    assert m.full_cloud().tobytes() == full.tobytes()            # as set until a process maps it
    T_in = ([0.0, 0.0, np.sin(0.05), np.cos(0.05)], [0.4, -0.2, 0.1])
    m.process(clouds[0][1], clouds[0][0], T_in)
    q, p = m.transform_tobe_mapped()
    assert np.linalg.norm(p) > 0.1
    got = m.full_cloud()
    assert got.tobytes() == ref.rigid_map32(full, q, p).tobytes()
    assert got[:, 3].tobytes() == full[:, 3].tobytes()
    # a seeded map: the optimisation moves the transform; the cloud is mapped by the transform the process ENDED with
    full2 = cases.cloud(257, seed=3)
    m.set_full_cloud(full2)
    T2 = ([0.0, 0.0, np.sin(0.06), np.cos(0.06)], [0.5, -0.2, 0.1])
    r = m.process(clouds[1][1], clouds[1][0], T2)
    assert r["iterations"] > 0
    q2, p2 = m.transform_tobe_mapped()
    got2 = m.full_cloud()
    assert got2.tobytes() == ref.rigid_map32(full2, q2, p2).tobytes()
    # a second process without a new set leaves the bytes alone
    m.process(clouds[2][1], clouds[2][0], T2)
    assert m.full_cloud().tobytes() == got2.tobytes()
    # with the init flag on nothing touches it
    m.set_full_cloud(full2)
    m.set_init_flag(True)
    m.process(clouds[2][1], clouds[2][0], T2)
    assert m.full_cloud().tobytes() == full2.tobytes()
    m.set_full_cloud(np.zeros((0, 4), np.float32))               # n = 0 clears
    assert len(m.full_cloud()) == 0
