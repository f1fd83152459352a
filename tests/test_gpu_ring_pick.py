"""The PRODUCT's per-ring feature picks (k_ring_pick, k_lf_ring, k_pp_pack of csrc/pointproc.hip, through lio_pp_process_rings) on the
crafted sweeps of tests/ring_pick_cases.py, against the serial numpy statement of the contract (tests/ring_pick_ref.py) and against
the oracle, which equals the reference's own PointProcessor.cc on them (tests/golden/ref_ring_pick.json, tests/test_ring_pick.py).

Exactly equal: ring offsets, ring cloud coordinates, the three (ring, index) lists, the pick clouds' coordinates, curvature, mask, the
less-flat count and coordinates.  Intensities carry a relative time that goes through atan2f: within the 8e-6 that
tests/test_gpu_parity.py allows, with its seam rule and nothing wider.  Then the same sweeps through lio_pp_process_rings_batch (LDS
sized by the batch's longest ring), through one reused handle, the two capacity limits as LIO_ERR_CAPACITY, and a shared batch that fails
in front of its chain, which serves nothing to any of its handles."""
import numpy as np
import pytest

from lio_amd import capi
from ref_pp_cases import CLOUDS, digest
from ring_pick_cases import DEFAULT_BATCH, SMALL_BATCH, case, over_capacity_sweeps
from test_gpu_parity import _assert_rel_time_close
from test_ring_pick import CASES, CLASSES, GOLD, IDS, assert_equals_reference, assert_same_results, make_pp, oracle_results, reference, results

pytestmark = pytest.mark.gpu
_SINGLE = {}


def single(hip, name):
    """the product's results for a case through a fresh handle and lio_pp_process_rings, computed once and shared (read-only)"""
    if name not in _SINGLE:
        _, rings, over, scan, ring = case(name)
        pp = make_pp(hip, rings, over)
        pp.process(scan, ring)
        _SINGLE[name] = results(pp)
    return _SINGLE[name]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_product_picks_equal_the_references(hip, oracle, c):
    name = c[0]
    got = single(hip, name)
    seam = assert_equals_reference(got, reference(name))
    orc = oracle_results(oracle, c)
    assert {k: digest(orc[k]) for k in CLOUDS} == GOLD[name]              # the oracle IS the reference here (CPU twin: test_ring_pick.py)
    for k in CLOUDS:
        assert got[k].shape == orc[k].shape
        np.testing.assert_array_equal(got[k][:, :3], orc[k][:, :3])
        seam += _assert_rel_time_close(got[k], orc[k], orc["start_ori"])
    for k, _ in CLASSES:
        np.testing.assert_array_equal(got[k + "_idx"][0], orc[k + "_idx"][0])
        np.testing.assert_array_equal(got[k + "_idx"][1], orc[k + "_idx"][1])
    np.testing.assert_array_equal(got["curvature"], orc["curvature"])
    np.testing.assert_array_equal(got["mask"], orc["mask"])
    np.testing.assert_allclose(got["ring_intensity"], orc["ring_intensity"], rtol=0, atol=8e-6)
    print(f"{name}: all lists exact; {seam} intensity entries needed the seam rule")


@pytest.mark.parametrize("names", [DEFAULT_BATCH, SMALL_BATCH], ids=["rings_up_to_4080", "longest_ring_522"])
def test_batch_equals_single_sweeps(hip, names):
    """one launch chain over >= 4 sweeps sizes the LDS of both per-ring kernels from the batch's longest ring"""
    cs = [case(n) for n in names]
    assert all(c[1] == cs[0][1] and c[2] == {} for c in cs)              # same sensor, default config: one shared chain
    longest = max(int(np.diff(reference(n)["offsets"]).max()) for n in names)
    assert longest == (4080 if names is DEFAULT_BATCH else 522)
    pps = [make_pp(hip, c[1], c[2]) for c in cs]
    capi.PointProcessor.process_rings_batch(pps, [c[3] for c in cs], [c[4] for c in cs])
    for pp, n in zip(pps, names):
        assert_same_results(results(pp), single(hip, n))


def test_reused_handle_keeps_no_stale_state(hip):
    """descending then ascending sizes through ONE handle: reserved buffers only grow, so a smaller sweep runs in a larger one's storage"""
    names = ["cap_ring4080_ns8", "gaps", "tiny_ns8", "gaps", "cap_ring4080_ns8"]
    _, rings, over, _, _ = case(names[0])
    pp = make_pp(hip, rings, over)
    for n in names:
        _, _, _, scan, ring = case(n)
        pp.process(scan, ring)
        assert_same_results(results(pp), single(hip, n))


def _assert_serves_nothing(pp):
    assert [int(pp.lib.dll.lio_pp_count(pp.h, w)) for w in range(5)] == [0] * 5
    assert not pp.ring_offsets().any()


@pytest.mark.parametrize("over_case,limit_name", over_capacity_sweeps(), ids=[c[0][0] for c in over_capacity_sweeps()])
def test_over_capacity_is_reported_as_capacity(hip, over_case, limit_name):
    """one point more than a ring (4081 at ns = 8: every subregion <= 509) or a subregion (7 x 512 + 11 at ns = 7: one of 513 in a ring
    well under 4080) holds: LIO_ERR_CAPACITY, nothing served, and the exact-limit sweep through the same handle is the reference's"""
    _, rings, over, scan, ring = over_case
    pp = make_pp(hip, rings, over)
    pp.process(*case("gaps")[3:])                                          # results that must not be served afterwards
    rc = hip.dll.lio_pp_process_rings(pp.h, capi._fp(scan), ring.ctypes.data_as(capi.c_uint16_p), len(scan))
    assert rc == -4                                                        # LIO_ERR_CAPACITY
    _assert_serves_nothing(pp)
    _, _, _, scan2, ring2 = case(limit_name)
    pp.process(scan2, ring2)
    got = results(pp)
    assert_equals_reference(got, reference(limit_name))
    assert_same_results(got, single(hip, limit_name))


def test_over_capacity_through_wait_and_batch(hip):
    (ring_case, _), (sub_case, sub_limit) = over_capacity_sweeps()
    # lio_pp_process_async + lio_pp_wait: the elevation overload bins the 4081-point arc into one ring (constant elevation)
    pp = make_pp(hip, ring_case[1], ring_case[2])
    pp.process_async(ring_case[3])
    assert hip.dll.lio_pp_wait(pp.h) == -4
    _assert_serves_nothing(pp)
    assert hip.dll.lio_pp_process(pp.h, capi._fp(ring_case[3]), len(ring_case[3])) == -4
    _assert_serves_nothing(pp)
    # lio_pp_process_rings_batch, one chain of four sweeps with the subregion of 513 points in the third: every handle involved reads 0
    limit = case(sub_limit)
    sweeps = [limit, limit, sub_case, limit]
    pps = [make_pp(hip, sub_case[1], sub_case[2]) for _ in sweeps]
    with pytest.raises(capi.LioError, match="code -4"):
        capi.PointProcessor.process_rings_batch(pps, [c[3] for c in sweeps], [c[4] for c in sweeps])
    for p in pps:
        _assert_serves_nothing(p)
    sweeps[2] = limit
    capi.PointProcessor.process_rings_batch(pps, [c[3] for c in sweeps], [c[4] for c in sweeps])
    for p in pps:
        assert_same_results(results(p), single(hip, sub_limit))


def test_failed_batch_serves_nothing_to_any_handle(hip):
    """a shared batch that fails in front of its chain — the second handle's own lio_pp_process_async sweep ended over the ring capacity, which
    the batch meets when it waits for that sweep — leaves EVERY handle of the call with nothing to serve (include/lio_c.h), the first one
    included, whose place in the shared storage still holds the batch before; the next batch then serves each handle its own sweep"""
    (ring_case, _), _ = over_capacity_sweeps()
    names = ["gaps", "tiny_ns8", "gaps", "tiny_ns8"]
    cs = [case(n) for n in names]
    assert all(c[1] == ring_case[1] and c[2] == ring_case[2] == {} for c in cs)   # one sensor: one shared chain
    pps = [make_pp(hip, c[1], c[2]) for c in cs]
    batch = lambda: capi.PointProcessor.process_rings_batch(pps, [c[3] for c in cs], [c[4] for c in cs])
    batch()
    assert all(int(hip.dll.lio_pp_count(p.h, 0)) > 0 for p in pps)      # served from the shared storage
    pps[1].process_async(ring_case[3])                                   # the 4081-point arc: flagged by the kernel, left unfinished
    with pytest.raises(capi.LioError, match="code -4"):
        batch()
    offs = np.ones(ring_case[1] + 1, np.int32)
    for p in pps:
        assert [int(hip.dll.lio_pp_count(p.h, w)) for w in range(5)] == [0] * 5
        offs[:] = 1
        rc = hip.dll.lio_pp_get_ring_offsets(p.h, offs.ctypes.data_as(capi.c_int32_p))
        assert rc == -2 or (rc == 0 and not offs.any())                   # LIO_ERR_STATE, or all zeros
    batch()
    for p, n in zip(pps, names):
        assert_same_results(results(p), single(hip, n))
