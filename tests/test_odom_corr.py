"""The scan-to-scan correspondence search's references and checks, without a GPU: the oracle's statement of lio_odom_correspondences
(include/lio_test_hooks.h; the functions its own PointOdometry::Process calls) equals layer A of tests/odom_corr_ref.py on every case of
tests/odom_corr_cases.py, layer A satisfies layer B within the cap, every case contains what it claims, the comparison notices each
planted error, and the oracle's sel lies within K_START of the fp64 TransformToStart.  tests/test_gpu_odom_corr.py holds the product's
k_ob_corr to the same references."""
import numpy as np
import pytest

import odom_corr_cases as cases
import odom_corr_ref as ref


@pytest.fixture(scope="module")
def results(oracle):
    """name -> (case, (corner_idx, surf_idx, sel) of the oracle's hook), each computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            c = cases.get(name, oracle)
            memo[name] = (c, c.run(oracle))
        return memo[name]
    return get


@pytest.mark.parametrize("name", cases.NAMES)
def test_oracle_equals_layer_a_and_layer_b_agrees(results, name):
    c, (ci, si, sel) = results(name)
    assert c.last_corner.shape[0] <= 46000 and c.last_surf.shape[0] <= 46000 and c.sharp.shape[0] + c.flat.shape[0] <= 2100
    a, b, _ = c.refs(sel)
    ref.compare((ci, si), a)
    n, n_out = ref.compare_b(a, b, c.cap)
    found = int((ci[:, 0] >= 0).sum() + (si[:, 0] >= 0).sum())
    print(f"{name}: {c.last_corner.shape[0]} + {c.last_surf.shape[0]} previous points, {n} queries, {found} with a closest, "
          f"{int((ci[:, 1] >= 0).sum())} corner seconds, {int(((si[:, 1] >= 0) & (si[:, 2] >= 0)).sum())} surf triples; layer B leaves out {n_out} (cap {c.cap:.0%})")
    if c.lattice:
        assert n_out == 0


def test_oracle_sel_within_k_start(results):
    """K_START of tests/odom_corr_ref.py is this test's worst ratio, rounded up; the fp32 restatement of the module stays inside it too"""
    worst = {}
    for name in cases.NAMES:
        c, (_, _, sel) = results(name)
        worst[name] = c.start_ratio(sel)
        s32, _ = ref.to_start32(c.queries, c.q, c.p, c.scan_period, c.no_deskew)
        assert c.start_ratio(s32) <= ref.K_START, name
    top = max(worst, key=worst.get)
    print("worst |sel - to_start64| / scale per case: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    print(f"K_START {ref.K_START}: worst {worst[top]:.3f} in {top}")
    assert worst[top] <= ref.K_START
    assert worst[top] > 0.8 * ref.K_START, "K_START is the measured worst ratio rounded up, not a loose bound"


def test_identity_cases_see_their_queries(results):
    """identity transform and no_deskew: sel is the query, bit for bit (the synthetic cases rely on it)"""
    for name in cases.NAMES:
        c, (_, _, sel) = results(name)
        if c.no_deskew and (c.q == np.float32([0, 0, 0, 1])).all() and not c.p.any():
            np.testing.assert_array_equal(sel, c.queries[:, :3], err_msg=name)


def _stat(stats, key):
    return np.concatenate([np.asarray(stats[k][key]) for k in ("corner", "surf") if key in stats[k]])


def test_case_contains_what_it_claims(results):
    # chunk_edges: every count of in-window candidates above and below, closest at both ends, windows that run to both ends
    for name in ("chunk_edges", "chunk_edges_swapped"):
        c, (ci, si, sel) = results(name)
        a, _, st = c.refs(sel)
        np.testing.assert_array_equal(a[0][:, 0], c.want_closest[0])
        np.testing.assert_array_equal(a[1][:, 0], c.want_closest[1])
        for kind, n_prev in (("corner", c.last_corner.shape[0]), ("surf", c.last_surf.shape[0])):
            s = st[kind]
            assert set(cases.CHUNK_COUNTS) <= set(s["n_up"]) and set(cases.CHUNK_COUNTS) <= set(s["n_down"]), (name, kind)
        ends, runs = (st["surf"], st["corner"]) if name.endswith("swapped") else (st["corner"], st["surf"])
        n_ends = (c.last_surf if name.endswith("swapped") else c.last_corner).shape[0]
        assert 0 in ends["closest"] and n_ends - 1 in ends["closest"]
        assert any(e and n >= 257 for e, n in zip(runs["end_up"], runs["n_up"])) and any(e and n >= 257 for e, n in zip(runs["end_down"], runs["n_down"]))
        assert (a[0][:, 1] >= 0).sum() > 50 and ((a[1][:, 1] >= 0) & (a[1][:, 2] >= 0)).sum() > 50
    # violation_then_valid: the first violator at every listed position of both walks; taking what lies behind it changes the answer
    c, (ci, si, sel) = results("violation_then_valid")
    a, _, st = c.refs(sel)
    for kind in ("corner", "surf"):
        assert sorted(st[kind]["viol_up"]) == sorted(cases.VIOLATION_OFFSETS) and sorted(st[kind]["viol_down"]) == sorted(cases.VIOLATION_OFFSETS)
    planted = ref.layer_a(c, sel, plant="behind_violation")
    assert ((planted[0] != a[0]).any(axis=1)).all() and ((planted[1] != a[1]).any(axis=1)).all()
    # ties: a few hundred of each kind of tie
    c, (ci, si, sel) = results("ties")
    _, _, st = c.refs(sel)
    counts = {k: int(_stat(st, k).sum()) for k in ("nn_tie", "tie_one_dir", "tie_two_dir", "tie_lanes", "tie_chunks")}
    print("ties:", counts)
    assert min(counts.values()) >= 300, counts
    # gate: blocks whose deciding distance is exactly 25 find nothing there; 1/64 m inside they do
    c, (ci, si, sel) = results("gate")
    a, _, _ = c.refs(sel)
    np.testing.assert_array_equal(a[0][:, 0], c.want_closest[0])
    np.testing.assert_array_equal(a[1][:, 0], c.want_closest[1])
    le = ref.layer_a(c, sel, plant="gate_le")
    changed = int((le[0] != a[0]).any(axis=1).sum()), int((le[1] != a[1]).any(axis=1).sum())
    assert changed[0] == c.n_blocks_exact and changed[1] == c.n_blocks_exact, (changed, c.n_blocks_exact)
    # ring_rules: A blocks take rings cs +- 2 and never cs +- 3; B blocks give a corner no second and a surf its second from its own ring
    c, (ci, si, sel) = results("ring_rules")
    a, _, _ = c.refs(sel)
    np.testing.assert_array_equal(a[0][:, 0], c.want_closest[0])
    ring = lambda cloud, i: np.where(i >= 0, np.trunc(cloud[np.maximum(i, 0), 3]).astype(int), -99)
    A, B = c.kinds == "A", c.kinds == "B"
    cs = ring(c.last_corner, a[0][:, 0])
    assert (np.abs(ring(c.last_corner, a[0][A, 1]) - cs[A]) == 2).all()
    assert (a[0][B, 1] == -1).all() and B.sum() >= 30
    cs = ring(c.last_surf, a[1][:, 0])
    assert (ring(c.last_surf, a[1][:, 1]) == cs).all() and (np.abs(ring(c.last_surf, a[1][A, 2]) - cs[A]) == 2).all() and (a[1][B, 2] == -1).all()
    assert ((a[1][:, 1] > a[1][:, 0]).sum() >= 10) and ((a[1][:, 1] < a[1][:, 0]).sum() >= 10)        # seconds from above and from below
    assert (np.modf(c.last_corner[:, 3])[0] >= 0.5).sum() > 100
    # grid_edges: queries beyond the cloud's bounds by less and by more than 5 m on every axis, and around +-120 m
    c, (ci, si, sel) = results("grid_edges")
    a, _, _ = c.refs(sel)
    for q, cl, idx in ((c.sharp, c.last_corner, a[0]), (c.flat, c.last_surf, a[1])):
        lo, hi = cl[:, :3].min(axis=0), cl[:, :3].max(axis=0)
        beyond = np.maximum(np.maximum(lo - q[:, :3], q[:, :3] - hi), 0)
        for ax in range(3):
            near, far = (beyond[:, ax] > 0) & (beyond[:, ax] < 5), beyond[:, ax] > 5
            assert near.sum() >= 6 and far.sum() >= 6
            assert (idx[near, 0] >= 0).any() and (idx[far, 0] == -1).all()
        assert np.abs(cl[:, :2]).max() > 120 and cl[:, 0].min() < -115
        face = q[-c.n_faces:, :3] / float(cases.CELL)
        assert (np.abs(face - np.rint(face)).min(axis=1) < 1.01e-3).all() and (idx[-c.n_faces:, 0] >= 0).sum() > 0.9 * c.n_faces
    # grid_oversize: both grids above the segmented build's limit (every other case's below it), and queries that find their closest, second
    # and third points in both clusters
    for name in cases.NAMES:
        c, _ = results(name)
        over = [cases.grid_cells(cl) > cases.GRID_CELLS_MAX for cl in (c.last_corner, c.last_surf) if cl.shape[0]]
        assert all(over) if name == "grid_oversize" else not any(over), (name, over)
    c, (ci, si, sel) = results("grid_oversize")
    assert c.last_corner.shape[0] == 200 and c.last_surf.shape[0] == 200 and cases.grid_cells(c.last_corner) > 200000
    for half in (slice(0, 64), slice(64, 128)):
        assert (ci[half, 1] >= 0).sum() > 32 and ((si[half, 1] >= 0) & (si[half, 2] >= 0)).sum() > 32
    assert (ci[:64][ci[:64, 0] >= 0, 0] < 100).all() and (ci[64:][ci[64:, 0] >= 0, 0] >= 100).all()
    for name, sizes in (("prev_0", (0, 0)), ("prev_1", (1, 2)), ("prev_2", (2, 1)), ("prev_identical", (200, 200))):
        c, (ci, si, sel) = results(name)
        assert (c.last_corner.shape[0], c.last_surf.shape[0]) == sizes
        if name == "prev_0":
            assert (ci == -1).all() and (si == -1).all()
        else:
            assert (ci[:, 0] >= 0).any() and (ci[:, 0] == -1).any()
    c, (ci, si, sel) = results("prev_2")
    assert (ci[:, 1] >= 0).any()
    c, (ci, si, sel) = results("prev_identical")
    assert (ci[ci[:, 0] >= 0, 0] == 0).all() and (si[si[:, 0] >= 0, 1] == 1).all() and (si[si[:, 0] >= 0, 2] == 20).all() and (ci[ci[:, 0] >= 0, 1] == 20).all()
    # deskew: relative times over the whole sweep, a motion of 3 degrees and 0.8 m
    c, _ = results("deskew")
    fr = np.modf(c.queries[:, 3])[0] * 10
    assert fr.min() < 0.02 and fr.max() > 0.98 and abs(np.linalg.norm(c.p) - 0.8) < 0.01 and abs(2 * np.degrees(np.arccos(c.q[3])) - 3) < 0.01
    # the sweeps: windows of thousands of candidates
    for name, lo in (("sweep_vlp16_iter0", 2000), ("sweep_vlp16_iter5", 2000), ("sweep_hdl64_iter0", 2500), ("sweep_hdl64_iter5", 2500)):
        c, (ci, si, sel) = results(name)
        _, _, st = c.refs(sel)
        longest = max(max(st["surf"]["n_up"]), max(st["surf"]["n_down"]))
        print(f"{name}: {c.sharp.shape[0]} + {c.flat.shape[0]} queries, longest surf walk {longest}, longest corner walk "
              f"{max(max(st['corner']['n_up']), max(st['corner']['n_down']))}; q_es {c.q} t_es {c.p}")
        assert longest >= lo
        if "hdl64" in name:
            assert c.sharp.shape[0] <= 512 and c.flat.shape[0] <= 512
        if name.endswith("iter5"):
            assert np.linalg.norm(c.p) > 1e-3


def test_bad_queries_find_nothing_and_disturb_nobody(results, oracle):
    cases.check_bad_queries(results("bad_queries")[0], oracle)


def test_no_queries(oracle):
    cases.check_no_queries(oracle)


# which case shows each planted error (every one changes at least one query there)
_PLANT_CASE = {"runner_up": "deskew", "behind_violation": "violation_then_valid", "updown_tie_flip": "ties", "nn_tie_high": "ties", "gate_le": "gate",
               "round_ring": "ring_rules", "surf_lt": "ring_rules"}


@pytest.mark.parametrize("plant", ref.PLANTS)
def test_compare_notices_planted_errors(results, plant):
    c, (_, _, sel) = results(_PLANT_CASE[plant])
    a, b, _ = c.refs(sel)
    wrong = ref.layer_a(c, sel, plant=plant)
    with pytest.raises(AssertionError):
        ref.compare(wrong, a)
    n_c, n_s = int((wrong[0] != a[0]).any(axis=1).sum()), int((wrong[1] != a[1]).any(axis=1).sum())
    print(f"{plant} on {c.name}: changes {n_c} corner and {n_s} surf queries")
    if plant == "surf_lt":
        assert n_c == 0 and n_s > 0
    if plant in ("runner_up", "behind_violation", "gate_le", "round_ring"):     # errors layer B sees as well (the tie rules it cannot)
        with pytest.raises(AssertionError):
            ref.compare_b(wrong, b, c.cap)


def test_compare_notices_a_single_wrong_entry(results):
    c, (ci, si, sel) = results("deskew")
    a, _, _ = c.refs(sel)
    for k, col in ((0, 1), (1, 2), (1, 0)):
        wrong = [a[0].copy(), a[1].copy()]
        row = int(np.nonzero(wrong[k][:, col] >= 0)[0][-1])
        wrong[k][row, col] += 1
        with pytest.raises(AssertionError):
            ref.compare(tuple(wrong), a)


@pytest.mark.parametrize("which", ["oracle", "hip"])
def test_argument_checks(request, which):
    """refused before anything is written; the product refuses without a device"""
    cases.check_arguments(request.getfixturevalue(which))
