"""The plain model of the cube map (tests/cube_map_ref.py) against the CPU oracle, bit for bit, on every case of tests/cube_map_cases.py:
the centre, the valid list in its order, the from-map clouds and every cube of both classes in stored order.  Two independent statements
of PointMapping.cc:808-989 and :1112-1208 that agree to the bit are what makes the product's comparison (tests/test_gpu_cube_map.py)
trustworthy.  Also the conditions the cases rest on.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cube_map_cases as cases
import cube_map_ref as ref
from cube_map_ref import F


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    cache = {}

    def run(name):
        if name not in cache:
            cache[name] = cases.play_case(cases.CASES[name](), cases.lib_handles(oracle), "oracle")
        return cache[name]

    return run


@pytest.mark.parametrize("name", [n for n in cases.CASES if n not in cases.NO_MODEL])
def test_model_equals_oracle(oracle_runs, name):
    model = cases.play_case(cases.CASES[name](), cases.model_handles, "model")
    assert len(model) > 0
    cases.same_run(oracle_runs(name), model, f"{name}: oracle vs model")


def test_default_leaves(oracle):
    from lio_amd import capi

    cfg = capi.MapConfig()
    oracle.dll.lio_map_default_config(C.byref(cfg))
    assert (F(cfg.corner_filter_size), F(cfg.surf_filter_size)) == tuple(F(v) for v in cases.DEFAULT_LEAVES)


def test_cube_coord_quirk():
    """truncation, then the decrement: exact negative multiples land one cube low"""
    assert [ref.cube_coord(v, 10) for v in (-25.0, 24.999998, 25.0, -75.0, -125.0, -25.000002, 0.0, -0.0)] == [10, 10, 11, 8, 7, 9, 10, 10]
    assert ref.cube_coord(-525.0, 10) == -1 and ref.cube_coord(cases.up(-525.0), 10) == 0
    assert ref.cube_coord(cases.down(525.0), 10) == 20 and ref.cube_coord(525.0, 10) == 21


def test_faces_reach_every_edge(oracle_runs):
    """first and last kept cube of every axis are occupied; the dropped coordinates are really in the input"""
    last = oracle_runs("faces")[-1]
    ijk = np.array([ref.from_index(idx) for _, idx in last["cubes"]])
    assert ijk.min(axis=0).tolist() == [0, 0, 0] and ijk.max(axis=0).tolist() == [20, 20, 10]
    total_in = 2 * 2 * len(cases.faces()[0]["ops"][0]["corner"])
    total_kept = sum(len(v) for v in last["cubes"].values())
    assert 0 < total_kept < total_in


@pytest.mark.parametrize("cfg", ["default", "equal"])
def test_voxels_pieces(cfg):
    """the triples are order-sensitive on x and on the intensity, and triple and crowd each fill ONE voxel"""
    for cls, (triple, crowd, _) in enumerate(cases.voxels_parts(cfg)):
        a, b, c = triple
        for col in (0, 3):
            assert (a[col] + b[col]) + c[col] != (a[col] + c[col]) + b[col]
        leaf = cases.leaves(cases.CONFIGS[cfg])[cls]
        assert len(ref.voxel_grid(triple, leaf)) == 1 and len(ref.voxel_grid(crowd, leaf)) == 1 and len(crowd) == 300
        assert ref.voxel_grid(triple, leaf).tobytes() != ref.voxel_grid(triple[[0, 2, 1]], leaf).tobytes()
        assert ref.voxel_grid(crowd, leaf).tobytes() != ref.voxel_grid(crowd[::-1], leaf).tobytes()


def test_old_then_new_centroid_next_to_a_face(oracle_runs):
    """after the first update one centroid lies one fp32 step below x = 6, one on it; later updates change both cubes' voxels"""
    runs = oracle_runs("old_then_new")
    idx = ref.to_index(10, 10, 5)
    for cls in (0, 1):
        xs = runs[0]["cubes"][(cls, idx)][:, 0]
        assert cases.down(6.0) in xs and F(6.0) in xs
        assert runs[1]["cubes"][(cls, idx)].tobytes() != runs[0]["cubes"][(cls, idx)].tobytes()


def test_shift_margins():
    """every FOV decision of the shift and far poses is far from a rounding decision: fp32 (the reference, the oracle, the product) and
    float64 (the model) decide alike"""
    for name in ("shift", "far", "from_map_after_update"):
        for t in cases.CASES[name]():
            m = ref.CubeMapModel()
            cases.play([op for op in t["ops"] if op["op"] != "snap"], m, "model")
            assert m.min_margin > 1e-3, (name, m.min_margin)


def test_shift_moves_and_empties(oracle_runs):
    runs = oracle_runs("shift")
    cens = [tuple(s["cen"]) for s in runs]
    assert cens[0] == (10, 10, 5) and cens[1] == (7, 10, 5)                # 3 cubes on x
    assert all(a != b for a, b in zip(cens[1], cens[2]))                   # all three axes at once
    assert len(runs[0]["cubes"]) > 500 and len(runs[7]["cubes"]) == 0      # every populated cube left the window ...
    assert len(runs[8]["cubes"]) == 0 and cens[8] != cens[7]               # ... and the way back finds it empty
    assert len(runs[0]["valid"]) == 0 and all(len(s["valid"]) > 0 for s in runs[1:])
    assert any(0 < len(s["clouds"][2]) and 0 < len(s["clouds"][3]) for s in runs)
    # the valid list is the selection loop's order (i outermost, k innermost), which is not ascending index order
    assert any(np.any(np.diff(s["valid"].astype(np.int64)) < 0) for s in runs)


def test_full_valid_is_full(oracle_runs):
    first = oracle_runs("full_valid")[0]
    assert len(set(cases.FULL_BLOCK)) == 125
    for idx in cases.FULL_BLOCK:
        assert (0, idx) in first["cubes"] and (1, idx) in first["cubes"], idx
    corner, _ = cases.full_valid_clouds()
    assert max(len(v) for v in first["cubes"].values()) < 600 < len(corner)   # the 600 went through the filter


def test_from_map_outlives_direct_updates(oracle_runs):
    """the oracle's contract: the from-map clouds are those of the last Process until the next Process"""
    a = oracle_runs("from_map_after_update")
    for w in (2, 3):
        assert len(a[0]["clouds"][w]) > 0
        assert a[0]["clouds"][w].tobytes() == a[1]["clouds"][w].tobytes() == a[2]["clouds"][w].tobytes() != a[3]["clouds"][w].tobytes()
        assert a[4]["clouds"][w].tobytes() == a[5]["clouds"][w].tobytes()
    assert len(a[4]["clouds"][2]) > 0


def test_far_is_far(oracle_runs):
    runs = oracle_runs("far")
    assert runs[0]["cen"][0] < -380 and runs[4]["cen"][1] > 400
    assert all(len(s["cubes"]) > 0 for s in (runs[1], runs[2], runs[5], runs[6]))
