"""The correspondence search the scan-to-scan odometry runs (csrc/odometry.hip: k_ob_corr, one wave per query, over the one-sensor table
and the grids lio_odom_process builds — the segmented grid build on every case, KnnGrid::build on `grid_oversize` — through the test hook
lio_odom_correspondences) against the plain references of tests/odom_corr_ref.py on the cases of tests/odom_corr_cases.py: equality with
layer A (the contract in fp32, evaluated on the sel the product reports — no tolerance, no query left out), then layer B (fp64 on the same
sel bits, slots within rounding left out, at most 1 % of a case's queries and none on a lattice), and sel itself within
GPU_BOUND_FACTOR x K_START of the fp64 TransformToStart.  What every case contains, and that these checks notice planted errors, is tested
without a GPU in tests/test_odom_corr.py."""
import numpy as np
import pytest

import odom_corr_cases as cases
import odom_corr_ref as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.NAMES)
def test_search_equals_serial_reference(hip, oracle, name):
    c = cases.get(name, oracle)
    ci, si, sel = c.run(hip)
    a, b, _ = c.refs(sel)
    ratio = c.start_ratio(sel)
    n_out = sum(int((~sure).any(axis=1).sum()) for _, sure in b)
    print(f"{name}: {c.sharp.shape[0]} + {c.flat.shape[0]} queries, |sel - to_start64| / scale {ratio:.3f} (bound {ref.GPU_BOUND_FACTOR * ref.K_START:.2f}), "
          f"layer B leaves out {n_out} (cap {c.cap:.0%})")
    np.testing.assert_array_equal(ci, a[0])
    np.testing.assert_array_equal(si, a[1])
    ref.compare((ci, si), a)
    ref.compare_b((ci, si), b, c.cap)
    if c.lattice:
        assert n_out == 0
    assert ratio <= ref.GPU_BOUND_FACTOR * ref.K_START


def test_identity_cases_see_their_queries(hip, oracle):
    """identity transform and no_deskew: sel is the query bit for bit, so the synthetic cases test the geometry they state"""
    for name in ("chunk_edges", "violation_then_valid", "ties", "gate", "ring_rules", "grid_edges"):
        c = cases.get(name, oracle)
        np.testing.assert_array_equal(c.run(hip)[2], c.queries[:, :3], err_msg=name)


def test_bad_queries_find_nothing_and_disturb_nobody(hip, oracle):
    cases.check_bad_queries(cases.get("bad_queries", oracle), hip)


def test_hook_refuses_bad_arguments(hip):
    cases.check_arguments(hip)


def test_no_queries(hip):
    cases.check_no_queries(hip)
