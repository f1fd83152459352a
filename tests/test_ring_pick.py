"""The per-ring feature picks at their edges, on the CPU: the oracle against the digests of the reference's own PointProcessor.cc
(tests/golden/ref_ring_pick.json) and against the serial numpy statement of the contract (tests/ring_pick_ref.py), on the crafted
sweeps of tests/ring_pick_cases.py; the conditions every case family is built for, read from the reference's counters alone; and the
planted errors of the numpy statement, each of which must change the outcome of some case.  tests/test_gpu_ring_pick.py holds the
product to the same references."""
import json
import os

import numpy as np
import pytest

from lio_amd import capi
from ref_pp_cases import CLOUDS, digest
from ring_pick_cases import BOUNDARY, LESS_FLAT_MEMBERS, cases
from ring_pick_ref import PLANTS, sweep_reference
from test_gpu_parity import _assert_rel_time_close

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ref_ring_pick.json")))
ORDER = [capi.PointProcessor.RINGS, capi.PointProcessor.SHARP, capi.PointProcessor.LESS_SHARP, capi.PointProcessor.FLAT, capi.PointProcessor.LESS_FLAT]
CLASSES = [("sharp", capi.PointProcessor.SHARP), ("less_sharp", capi.PointProcessor.LESS_SHARP), ("flat", capi.PointProcessor.FLAT)]
CASES = cases()
IDS = [c[0] for c in CASES]
_REF = {}


def reference(name):
    """the numpy reference of a case, computed once and shared (read-only)"""
    if name not in _REF:
        _, rings, over, scan, ring = next(c for c in CASES if c[0] == name)
        _REF[name] = sweep_reference(scan, ring, rings, over)
    return _REF[name]


def make_pp(lib, rings, over):
    cfg = capi.PPConfig()
    lib.dll.lio_pp_default_config(cfg)
    for k, v in over.items():
        setattr(cfg, k, v)
    return capi.PointProcessor(lib, -15.0, 15.0, rings, cfg)


def results(pp):
    """everything the stage decides, through the accessors"""
    out = dict(offsets=pp.ring_offsets(), start_ori=pp.start_ori())
    for c, w in zip(CLOUDS, ORDER):
        out[c] = pp.cloud(w)
    for c, w in CLASSES:
        out[c + "_idx"] = pp.indices(w)
    out["curvature"], out["mask"] = pp.curvature()
    out["ring_intensity"] = pp.ring_intensity()
    return out


def assert_equals_reference(got, ref):
    """ring offsets, ring cloud coordinates, the three index lists, the pick clouds' coordinates, curvature, mask, the less-flat count
    and coordinates: exactly.  Intensities (ring + rel. time, through atan2f): within 8e-6, with the seam rule of test_gpu_parity.
    -> the number of intensity entries that needed the seam rule"""
    np.testing.assert_array_equal(got["offsets"], ref["offsets"])
    assert got["laser_scans"].shape == ref["ring_cloud"].shape
    np.testing.assert_array_equal(got["laser_scans"][:, :3], ref["ring_cloud"][:, :3])
    seam = _assert_rel_time_close(got["laser_scans"], ref["ring_cloud"], ref["start_ori"])
    for c, _ in CLASSES:
        np.testing.assert_array_equal(got[c + "_idx"][0], ref[c][0], err_msg=c + " ring")
        np.testing.assert_array_equal(got[c + "_idx"][1], ref[c][1], err_msg=c + " index")
        np.testing.assert_array_equal(got[c][:, :3], ref[c + "_cloud"][:, :3], err_msg=c)
        seam += _assert_rel_time_close(got[c], ref[c + "_cloud"], ref["start_ori"])
    np.testing.assert_array_equal(got["curvature"], ref["curvature"])
    np.testing.assert_array_equal(got["mask"], ref["mask"])
    assert got["less_flat"].shape == ref["less_flat"].shape
    np.testing.assert_array_equal(got["less_flat"][:, :3], ref["less_flat"][:, :3])
    seam += _assert_rel_time_close(got["less_flat"], ref["less_flat"], ref["start_ori"])
    return seam


def assert_same_results(a, b):
    """two runs of the same library: bit for bit, intensities included"""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], tuple):
            for x, y in zip(a[k], b[k]):
                np.testing.assert_array_equal(x, y, err_msg=k)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def oracle_results(oracle, case):
    _, rings, over, scan, ring = case
    pp = make_pp(oracle, rings, over)
    pp.process(scan, ring)
    return results(pp)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_the_reference_digests_and_the_numpy_statement(oracle, case):
    got = oracle_results(oracle, case)
    row = {c: digest(got[c]) for c in CLOUDS}
    assert row == GOLD[case[0]], {c: (row[c], GOLD[case[0]][c]) for c in CLOUDS if row[c] != GOLD[case[0]][c]}
    seam = assert_equals_reference(got, reference(case[0]))
    assert seam == 0          # no crafted sweep has a return on the start azimuth besides the first


def test_committed_digests_are_what_the_reference_produces(tmp_path):
    """Build container only: rebuild oracle/_ref from the reference tree and regenerate the digests."""
    import subprocess
    import sys

    root = os.path.dirname(HERE)
    if not os.path.isdir("/root/reference/src/point_processor"):
        pytest.skip("the reference tree is not on this machine")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "oracle"), "_ref/libref_pointproc.so"], check=True)
    gen = os.path.join(HERE, "golden", "make_ref_ring_pick.py")
    out = str(tmp_path / "d.json")
    code = open(gen).read().replace('path = os.path.join(HERE, "ref_ring_pick.json")', f"path = {out!r}").replace("__file__", repr(gen))
    subprocess.run([sys.executable, "-c", code], check=True, capture_output=True)
    assert json.load(open(out)) == GOLD


# ------------------------------------------------------------------------------------------------ what the cases are built for
def _total(name, key):
    return sum(c[key] for c in reference(name)["counters"])


def _zone(name, key):
    return sum(sum(c[key].values()) for c in reference(name)["counters"])


def _three_in_a_row(name):
    for c in reference(name)["counters"]:
        b = set(c["zone_decisive"])
        if any({j, j + 1, j + 2} <= b for j in b):
            return True
    return False


def test_the_whole_set_stays_small():
    assert sum(len(c[3]) for c in CASES) <= 60000
    for _, _, _, scan, _ in CASES:
        assert np.isfinite(scan).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_jump_in_the_last_points_of_a_ring(case):
    """a step above 0.1 m^2 in the last nc + 2 points of a ring would make the reference write past its mask vector (:570)"""
    name, rings, over, _, _ = case
    ref = reference(name)
    nc = over.get("num_curvature_regions", 5)
    for r in range(rings):
        p = ref["ring_cloud"][ref["offsets"][r]:ref["offsets"][r + 1], :3].astype(np.float64)
        if len(p) > 2 * nc + 1:
            assert (np.diff(p[-(nc + 3):], axis=0) ** 2).sum(1).max() < 0.09


@pytest.mark.parametrize("ns,nc", BOUNDARY)
def test_boundary_cases_decide_picks_in_the_zone(ns, nc):
    name = f"boundary_ns{ns}_nc{nc}"
    if ns > 1:
        assert _zone(name, "zone_decisive") > 0 and _zone(name, "zone_picked") > 0
    if ns in (8, 16):
        assert _three_in_a_row(name)
    if ns == 16:
        second_group = [j for c in reference(name)["counters"] for j in c["zone_decisive"] if j >= 8]
        assert second_group and 8 in second_group      # the second group of eight waves, and its first wave over what the first group left


@pytest.mark.parametrize("ns", [8, 16])
def test_tiny_rings_have_the_degenerate_subregions(ns):
    name = f"tiny_ns{ns}"
    ref = reference(name)
    lengths = np.diff(ref["offsets"])
    assert set(range(11, 61)) <= set(lengths.tolist())
    sizes = {s for c in ref["counters"] for s in c["sizes"]}
    assert {0, 1, 2} <= sizes and any(2 < s < 5 for s in sizes)
    assert _total(name, "spans_subregion") > 0
    assert _zone(name, "zone_decisive") >= 100
    assert len(ref["sharp"][0]) > 0 and ref["members"][0] == 0 and any(ref["members"][1:30])   # 2 nc + 1 points: skipped; somewhat longer rings: not


def test_chunk_cases_sit_on_the_64_candidate_chunks():
    sizes = {s for n in ("chunks_63_64", "chunks_65_128_129") for c in reference(n)["counters"] for s in c["sizes"]}
    assert sizes == {63, 64, 65, 128, 129}
    ref = reference("chunks_all_masked")
    assert _total("chunks_all_masked", "no_pick_loops") == 2 and all(len(ref[c][0]) == 0 for c, _ in CLASSES)
    assert {s for c in ref["counters"] for s in c["sizes"]} == {130}
    assert (ref["curvature"] > 0.1).sum() > 64       # candidates above the threshold in more than one chunk, all of them masked


def test_tie_case_has_equal_curvatures():
    assert _total("ties_lattice", "ties") >= 100
    assert _total("ties_lattice", "at_threshold") >= 1
    ref = reference("ties_lattice")
    # equal curvatures ABOVE the threshold on both sides of a 64-candidate chunk border of a descending sort: ring 1's subregions
    off = ref["offsets"]
    c = np.sort(ref["curvature"][off[1] + 5 + 70:off[1] + 5 + 140])[::-1]
    assert c[63] == c[64] and c[64] > 0.140625


def test_gap_case_cuts_reaches_and_takes_both_prepare_branches():
    assert _total("gaps", "cut_forward") > 0 and _total("gaps", "cut_backward") > 0
    assert _total("gaps", "prepare_closer") > 0 and _total("gaps", "prepare_farther") > 0 and _total("gaps", "prepare_parallel") > 0


def test_capacity_edge_cases_are_at_the_limits():
    assert np.diff(reference("cap_ring4080_ns8")["offsets"]).max() == 4080
    for name in ("cap_7x512_ns7", "cap_7x512_nc8"):
        sizes = [s for c in reference(name)["counters"] for s in c["sizes"] if s]
        assert sizes == [512] * 7
    assert {0, 11, 12, 4080} == set(np.diff(reference("cap_ring4080_ns8")["offsets"]).tolist())


@pytest.mark.parametrize("less_sharp,flat", [(40, 24), (64, 0), (1, 63)])
def test_quota_cases_fill_their_quotas(less_sharp, flat):
    ref = reference(f"quota_{less_sharp}_{flat}")
    assert len(ref["less_sharp"][0]) == 4 * less_sharp and len(ref["sharp"][0]) == 4 * less_sharp and len(ref["flat"][0]) == 4 * flat


def test_ring_cases_leave_rings_empty():
    lengths = np.diff(reference("rings_128_sparse")["offsets"])
    assert sorted(np.flatnonzero(lengths).tolist()) == [0, 1, 63, 64, 65, 100, 127]
    ref = reference("rings_128_sparse")
    assert set(ref["sharp"][0].tolist()) == {0, 1, 63, 64, 65, 100, 127} and ref["members"][127] > 0
    assert len(reference("rings_2")["offsets"]) == 3


@pytest.mark.parametrize("name", sorted(LESS_FLAT_MEMBERS))
def test_less_flat_cases_have_the_intended_member_counts(name):
    ref = reference(name)
    assert tuple(m for m in ref["members"] if m) == LESS_FLAT_MEMBERS[name]
    assert (ref["ring_cloud"][:, 0] < 0).any() and (ref["ring_cloud"][:, 1] < 0).any()
    leaf = np.float32(0.2 if name.endswith("02") else 0.05)
    z = ref["ring_cloud"][:, 2]
    assert np.all(z / leaf == np.round(z / leaf))        # every member lies on a voxel face in z


# ------------------------------------------------------------------------------------------------ the planted errors
def _outcome(res):
    return [res[k][j].tobytes() for k in ("sharp", "less_sharp", "flat") for j in (0, 1)] + [res["mask"].tobytes(), res["curvature"].tobytes(),
                                                                                               res["less_flat"][:, :3].tobytes()]


@pytest.mark.parametrize("plant", PLANTS)
def test_every_planted_error_is_noticed(plant):
    noticed = []
    for name, rings, over, scan, ring in CASES:
        if len(scan) > 3000 and name != "gaps":
            continue                                   # (the small cases suffice; keeps this test quick)
        if _outcome(sweep_reference(scan, ring, rings, over, plant=plant)) != _outcome(reference(name)):
            noticed.append(name)
    assert noticed, plant
