"""GPU parity of the scan-to-map stage (csrc/mapping.hip) against oracle/mapping.h through the C-ABI.

fp32 throughout.  The voxel-filtered stacks and the cube map are expected equal to the oracle's to a few ulp of the
coordinates (same operation order; the only divergence enters through transform_tobe_mapped_, whose 6x6 normal
equations the GPU accumulates in double and the oracle in float); poses within 1e-4 m / 1e-4 rad."""
import numpy as np
import pytest

from lio_amd import capi
from mapping_util import drifting_inputs

pytestmark = pytest.mark.gpu

POS_TOL = 1e-4   # m
ROT_TOL = 1e-4   # rad (quaternion component difference ~ half the angle)


def _assert_pose_close(a, b):
    qa, pa = a
    qb, pb = b
    assert np.max(np.abs(pa - pb)) < POS_TOL, (pa, pb)
    assert min(np.max(np.abs(qa - qb)), np.max(np.abs(qa + qb))) < ROT_TOL, (qa, qb)


def _cloud_mismatch(a, b, atol):
    """Number of points of `a` without a partner in `b` within atol (xyz and intensity) plus the size difference.
    VoxelGrid is discontinuous: a map point a few ulp from a voxel face may fall on the other side when the pose that
    placed it differs in the last bits, which moves/merges one or two centroids.  Those are counted, not hidden."""
    from scipy.spatial import cKDTree

    if len(a) == 0 or len(b) == 0:
        return len(a) + len(b)
    d, j = cKDTree(b[:, :3]).query(a[:, :3], k=1)
    bad = (d > atol * 2) | (np.abs(a[:, 3] - b[j, 3]) > max(atol, 1e-3))
    return int(bad.sum()) + abs(len(a) - len(b))


def _compare_cubes(mh, mo, idx_list, atol, strict=True):
    total = bad = 0
    for idx in idx_list:
        for cls in (0, 1):
            a, b = mh.cube(cls, idx), mo.cube(cls, idx)
            if strict:
                assert a.shape == b.shape, (cls, idx, a.shape, b.shape)
                if len(a) and atol == 0:   # a pose both sides share to the bit: the cube map is exact (docs/cube_map.md), order included
                    assert a.tobytes() == b.tobytes(), (cls, idx)
                elif len(a):
                    np.testing.assert_allclose(a, b, rtol=0, atol=atol)
            else:
                bad += _cloud_mismatch(a, b, atol)
            total += len(b)
    assert bad <= max(4, total // 200), (bad, total)   # <= 0.5 % voxel-boundary flips
    return total


@pytest.mark.parametrize("kind,n_frames", [("indoor", 5), ("outdoor", 3)])
def test_mapping_sequence_matches_oracle(hip, oracle, kind, n_frames):
    frames = drifting_inputs(oracle, kind, n_frames)
    mh, mo = capi.PointMapping(hip), capi.PointMapping(oracle)
    for k, (corner, surf, T_sum, _) in enumerate(frames):
        rh, ro = mh.process(corner, surf, T_sum), mo.process(corner, surf, T_sum)
        # stacks: map round trip + VoxelGrid, identical operation order
        for which in (capi.PointMapping.CORNER_STACK_DS, capi.PointMapping.SURF_STACK_DS):
            a, b = mh.cloud(which), mo.cloud(which)
            if k == 0:   # same transform bits on both sides: same voxels, same sums
                assert a.shape == b.shape
                np.testing.assert_allclose(a, b, rtol=0, atol=2e-5)
            else:        # the predicted pose differs in the last bits: allow voxel-face flips, count them
                assert _cloud_mismatch(a, b, 1e-4) <= max(4, len(b) // 200), (k, which, a.shape, b.shape)
        # from-map clouds: same cubes, same order
        for which in (capi.PointMapping.CORNER_FROM_MAP, capi.PointMapping.SURF_FROM_MAP):
            a, b = mh.cloud(which), mo.cloud(which)
            assert _cloud_mismatch(a, b, 5e-4) <= max(4, len(b) // 200), (k, which, a.shape, b.shape)
        assert rh["iterations"] == ro["iterations"], (k, rh, ro)
        assert abs(rh["num_selected"] - ro["num_selected"]) <= max(3, ro["num_selected"] // 500)
        _assert_pose_close(rh["T_aft"], ro["T_aft"])
        _assert_pose_close(mh.transform_tobe_mapped(), mo.transform_tobe_mapped())
        ch, vh = mh.cube_state()
        co, vo = mo.cube_state()
        assert ch == co
        np.testing.assert_array_equal(vh, vo)
    total = _compare_cubes(mh, mo, vo, atol=5e-4, strict=False)
    assert total > 5000
    sh, ph, ch_ = mh.score_point_coeff()
    so, po, co_ = mo.score_point_coeff()
    assert abs(len(sh) - len(so)) <= max(3, len(so) // 500) and len(so) >= 50
    assert np.all(np.diff(sh) <= 0)
    np.testing.assert_allclose(sh[:50], so[:50], atol=2e-3)


def test_mapping_first_frame_and_small_maps(hip, oracle):
    """<= 10 corner or <= 100 surf map points: no optimisation, no TransformUpdate (PointMapping.cc:327-329)."""
    rng = np.random.default_rng(3)
    mh, mo = capi.PointMapping(hip), capi.PointMapping(oracle)
    surf = np.zeros((60, 4), np.float32)
    surf[:, :3] = rng.uniform(-10, 10, (60, 3))
    corner = surf[:8].copy()
    T = ([0, 0, np.sin(0.05), np.cos(0.05)], [1.0, 2.0, 0.5])
    for _ in range(2):
        rh, ro = mh.process(corner, surf, T), mo.process(corner, surf, T)
        assert rh["iterations"] == ro["iterations"] == 0
        _assert_pose_close(rh["T_aft"], ro["T_aft"])
        _assert_pose_close(mh.transform_tobe_mapped(), mo.transform_tobe_mapped())
    _, vo = mo.cube_state()
    _compare_cubes(mh, mo, vo, atol=0)
    # empty inputs are legal
    e = np.zeros((0, 4), np.float32)
    rh, ro = mh.process(e, e, T), mo.process(e, e, T)
    _assert_pose_close(mh.transform_tobe_mapped(), mo.transform_tobe_mapped())
    assert mh.cloud(0).shape == (0, 4) and mh.cloud(1).shape == (0, 4)


def test_mapping_window_shift_matches_oracle(hip, oracle):
    rng = np.random.default_rng(1)
    pts = np.zeros((4000, 4), np.float32)
    pts[:, :3] = rng.uniform(-60, 60, (4000, 3))   # spans several 50 m cubes
    pts[:, 3] = rng.uniform(0, 16, 4000)
    mh, mo = capi.PointMapping(hip), capi.PointMapping(oracle)
    all_idx = np.arange(21 * 21 * 11)
    for x in (0.0, 400.0, 380.0, -420.0, 1000.0):
        T = ([0, 0, 0, 1], [x, 30.0, -10.0])
        mh.process(pts[:500], pts, T), mo.process(pts[:500], pts, T)
        ch, vh = mh.cube_state()
        co, vo = mo.cube_state()
        assert ch == co
        np.testing.assert_array_equal(vh, vo)
        # every cube of the window, not only the valid ones: the shift must drop exactly what the reference drops
        occupied = [i for i in all_idx if len(mo.cube(1, i)) or len(mo.cube(0, i))]
        assert _compare_cubes(mh, mo, occupied, atol=0) > 0
        empty_probe = [i for i in all_idx[::37] if i not in occupied]
        for i in empty_probe:
            assert len(mh.cube(0, i)) == 0 and len(mh.cube(1, i)) == 0


def test_update_map_database_rebases_valid_cubes(hip, oracle):
    """UpdateMapDatabase with a stale cube centre and an arbitrary valid list (Estimator.cc:704-708 passes the pivot
    frame's): indices are re-based on the current centre (PointMapping.cc:1165-1186), duplicates are harmless."""
    frames = drifting_inputs(oracle, "indoor", 2)
    mh, mo = capi.PointMapping(hip), capi.PointMapping(oracle)
    for corner, surf, T_sum, _ in frames:
        mh.process(corner, surf, T_sum), mo.process(corner, surf, T_sum)
    cen, valid = mo.cube_state()
    rng = np.random.default_rng(9)
    new_s = np.zeros((3000, 4), np.float32)
    new_s[:, :3] = rng.uniform(-70, 70, (3000, 3))
    new_c = new_s[:400].copy()
    T = ([0.01, -0.02, 0.3, 0.95], [3.0, -2.0, 0.4])
    stale_cen = [cen[0] + 1, cen[1], cen[2] - 1]
    sub = np.concatenate([valid[::3], valid[:5], np.array([0, 4850], np.uint32)])  # duplicates + cubes far outside
    mh.update_map_database(new_c, new_s, sub, T, stale_cen), mo.update_map_database(new_c, new_s, sub, T, stale_cen)
    all_idx = np.arange(21 * 21 * 11)
    occupied = [i for i in all_idx if len(mo.cube(1, i)) or len(mo.cube(0, i))]
    assert _compare_cubes(mh, mo, occupied, atol=5e-4, strict=False) > 3000
    # and the next scan-to-map step still agrees
    corner, surf, T_sum, _ = frames[-1]
    rh, ro = mh.process(corner, surf, T_sum), mo.process(corner, surf, T_sum)
    assert rh["iterations"] == ro["iterations"]
    _assert_pose_close(rh["T_aft"], ro["T_aft"])


def test_mapping_after_imu_init_is_frozen(hip, oracle):
    """SetInitFlag(true): no odometry increment, no map update (PointMapping.cc:781-783,1021)."""
    frames = drifting_inputs(oracle, "indoor", 3)
    mh, mo = capi.PointMapping(hip), capi.PointMapping(oracle)
    for corner, surf, T_sum, _ in frames[:2]:
        mh.process(corner, surf, T_sum), mo.process(corner, surf, T_sum)
    _, valid = mo.cube_state()
    before = {int(i): mh.cube(1, i) for i in valid}
    mh.set_init_flag(True), mo.set_init_flag(True)
    q, p = mo.transform_tobe_mapped()
    mh.set_transform_tobe_mapped(q, p + np.float32(0.05)), mo.set_transform_tobe_mapped(q, p + np.float32(0.05))
    corner, surf, T_sum, _ = frames[2]
    rh, ro = mh.process(corner, surf, T_sum), mo.process(corner, surf, T_sum)
    assert rh["iterations"] == ro["iterations"] > 0
    _assert_pose_close(rh["T_aft"], ro["T_aft"])
    for i, c in before.items():
        np.testing.assert_array_equal(mh.cube(1, i), c)


@pytest.mark.parametrize("enable_4d", [1, 0])
def test_map_builder_matches_oracle(hip, oracle, enable_4d):
    """MapBuilder::ProcessMap / OptimizeMap (MapBuilder.cc:55-75, 220-558, 624-1014) through lio_map_config.map_builder."""
    frames = drifting_inputs(oracle, "indoor", 5)
    kw = dict(map_builder=1, enable_4d=enable_4d, skip_count=2)
    mh, mo = capi.PointMapping(hip, **kw), capi.PointMapping(oracle, **kw)
    for k, (corner, surf, T_sum, _) in enumerate(frames):
        rh, ro = mh.process(corner, surf, T_sum), mo.process(corner, surf, T_sum)
        assert rh["iterations"] == ro["iterations"], (k, rh, ro)
        _assert_pose_close(rh["T_aft"], ro["T_aft"])
        _assert_pose_close(mh.transform_tobe_mapped(), mo.transform_tobe_mapped())
    _, vo = mo.cube_state()
    assert _compare_cubes(mh, mo, vo, atol=5e-4, strict=False) > 5000
    assert len(mh.score_point_coeff()[0]) == len(mo.score_point_coeff()[0])


def test_mapping_with_stack_points_beyond_the_fast_voxel_key_range(hip, oracle):
    """A surf and a corner point > 409 m from the sensor (0.2 / 0.4 m leaves: the absolute-cell voxel keys hold +-204 / +-409 m)
    make the stack VoxelGrids re-run with PCL's own index — the surf one on the handle's second stream, whose consumers on the
    main stream must be ordered behind the RE-RUN, not behind the pass that raised the overflow (a stale or half-written
    down-sampled stack would change the stack itself and the pose).  Same sequence as the plain test, same bounds."""
    frames = drifting_inputs(oracle, "indoor", 4)
    mh, mo = capi.PointMapping(hip), capi.PointMapping(oracle)
    for k, (corner, surf, T_sum, _) in enumerate(frames):
        far = np.array([[450.0 + k, -3.0, 1.5, 0.0], [-470.0, 12.0 + k, 2.0, 0.0]], np.float32)
        surf = np.vstack([surf, far]).astype(np.float32)
        corner = np.vstack([corner, far[:1] + np.float32([0, 5, 0, 0])]).astype(np.float32)
        rh, ro = mh.process(corner, surf, T_sum), mo.process(corner, surf, T_sum)
        for which in (capi.PointMapping.CORNER_STACK_DS, capi.PointMapping.SURF_STACK_DS):
            a, b = mh.cloud(which), mo.cloud(which)
            assert np.abs(b[:, :3]).max() > 400          # the far points survive the filter on the oracle's side ...
            if k == 0:
                assert a.shape == b.shape
                np.testing.assert_allclose(a, b, rtol=0, atol=5e-5)   # (ulp of a 450 m coordinate: 3e-5)
            else:
                assert _cloud_mismatch(a, b, 1e-4) <= max(4, len(b) // 200), (k, which, a.shape, b.shape)
        assert rh["iterations"] == ro["iterations"], (k, rh, ro)
        _assert_pose_close(rh["T_aft"], ro["T_aft"])
        _assert_pose_close(mh.transform_tobe_mapped(), mo.transform_tobe_mapped())
