"""The Gauss-Newton rows, folds and step without a GPU: the oracle's statements of lio_gn_rows_map, lio_gn_fold, lio_gn_step and lio_gn_round
(include/lio_test_hooks.h: the functions its own loops call) meet the references of tests/gn_ref.py on every case of tests/gn_cases.py — the
run that sets the two constants —, every case contains what it is there for, the product's own qr_solve (csrc/hmath.h) is held to scipy
on the host, and the comparisons the GPU tests use (tests/test_gpu_gn.py) notice the errors these kernels can make."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import gn_cases
import gn_ref
from lio_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAP_IDS = [f"{n}-form{f}" for n, f in gn_cases.MAP_RUNS]


# ------------------------------------------------------------------------------------------------ rows: the oracle against fp64
def test_oracle_rows_meet_fp64(oracle):
    """every case and form under the comparison the product is held to; C_MAP_ROWS is 4 x the largest error / scale seen here"""
    top = 0.0
    for name, form in gn_cases.MAP_RUNS:
        c = gn_cases.get_map(name)
        ok, rows, part = c.run(oracle, form)
        ref = c.ref(form)
        gn_ref.compare_rows((ok, rows), ref, gn_ref.C_MAP_ROWS, f"{name} form {form}")
        top = max(top, gn_ref.rows_ratio(rows, ref))
        assert part.shape == (1, 28)
        gn_ref.compare_sums(part, ok, rows, f"{name} form {form}")
    print(f"largest row error / scale of the oracle: {top:.4f}; constant {gn_ref.C_MAP_ROWS}")
    assert 0.9 * gn_ref.C_MAP_ROWS <= 4 * top <= gn_ref.C_MAP_ROWS, (top, gn_ref.C_MAP_ROWS)


def test_oracle_rows_hook_checks_its_arguments(oracle):
    gn_cases.check_rows_null_pointers(oracle)
    ok, rows, part = gn_cases.get_map("m0").run(oracle, 0)
    assert ok.shape == (0,) and rows.shape == (0, 7) and part.shape == (1, 28) and not part.any()


@pytest.mark.parametrize("name", gn_cases.MAP_NAMES)
def test_map_cases_hold_what_they_claim(name):
    c = gn_cases.get_map(name)
    want = {n: m for n, m, *_ in gn_cases._MAP}[name]
    assert c.m == want and c.stack.shape == (c.m, 4) and c.coeff.shape == (c.m, 4)
    if c.m:
        d = np.linalg.norm(c.stack[:, :3].astype(np.float64), axis=1)
        assert (np.abs(d / c.range - 1) < 0.03).all()
        wn = np.linalg.norm(c.coeff[:, :3].astype(np.float64), axis=1)
        assert (wn > 0.09).all() and (wn < 1.01).all()
        # the residual is centimetres where its terms are metres: b of form 0 cancels
        ok, rows, scale, _ = c.ref(0)
        if ok.any():
            assert np.median(np.abs(rows[ok, 6])) < 0.1
    v = c.valid
    kind = c.valid_kind
    if kind == "all":
        assert v.all()
    elif kind == "none":
        assert not v.any() and c.m > 256
    elif kind == "every64":
        assert (np.nonzero(v)[0] == np.arange(0, c.m, 64)).all() and c.m > 2048
    elif kind == "wave_out":
        assert not v[64:128].any() and v[:64].all() and v[128:].all()
    else:
        assert 0.4 < v.mean() < 0.8
    # the invalid queries carry coefficients a kernel that ignored `valid` would add
    if (v == 0).any():
        assert np.abs(c.coeff[v == 0, :3]).max() > 0.05


def test_map_sizes_and_block_counts():
    sizes = [gn_cases.get_map(n).m for n in gn_cases.MAP_NAMES]
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 2048, 2049, 16385, 524289):
        assert m in sizes
    assert [gn_cases.rows_blocks(m) for m in (0, 1, 2048, 2049, 16384, 16385, 524288, 524289, 10 ** 7)] == [1, 1, 1, 2, 8, 9, 256, 256, 256]
    poses = {tuple(gn_cases.get_map(n).q) for n in gn_cases.MAP_NAMES}
    assert len(poses) == 2 and (0.0, 0.0, 0.0, 1.0) in poses
    assert {gn_cases.get_map(n).range for n in gn_cases.MAP_NAMES} == {1.0, 50.0, 400.0}
    assert {f for _, f in gn_cases.MAP_RUNS} == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ rows of the scan-to-scan loop
@pytest.mark.parametrize("name", gn_cases.ODOM_NAMES)
def test_oracle_odom_rows_and_sums(oracle, name):
    """the oracle's rows on the stated correspondences: zeros where no row exists, its one partial the sums of its own rows' products"""
    c = gn_cases.get_odom(name)
    ok, rows, part = c.run(oracle)
    assert ok.shape == (c.nq,) and rows.shape == (c.nq, 7) and part.shape == (1, 28)
    assert not rows[ok == 0].view(np.uint32).any()
    gn_ref.compare_sums(part, ok, rows, name)
    gn_ref.compare_rows_bits((ok, rows), c.run(oracle), name)
    if not c.special:
        assert np.isfinite(rows).all()
        if c.nq >= 63:
            assert 0.3 < ok.mean() < 0.999 if c.iter >= 5 else ok.mean() > 0.99      # the weight's cut at 0.1 takes some at iter 5, none at iter 4


def test_oracle_odom_rows_meet_fp64(oracle):
    """every case under the comparison the product is held to, on the sel the oracle reports; C_ODOM_ROWS is 4 x the largest ratio seen here"""
    top, left_all = 0.0, 0
    for name in gn_cases.ODOM_NAMES:
        c = gn_cases.get_odom(name)
        got, ref = c.run(oracle), c.ref(c.sel(oracle))
        n_chk, n_left = gn_ref.compare_odom_rows(got, ref, gn_ref.C_ODOM_ROWS, what=name)
        assert n_chk + n_left == c.nq
        left_all += n_left
        top = max(top, gn_ref.odom_rows_ratio(got, ref, gn_ref.C_ODOM_ROWS))
    print(f"largest scan-to-scan row error / scale of the oracle: {top:.4f}; constant {gn_ref.C_ODOM_ROWS}; {left_all} weights inside the band of 0.1")
    assert 0.9 * gn_ref.C_ODOM_ROWS <= 4 * top <= gn_ref.C_ODOM_ROWS, (top, gn_ref.C_ODOM_ROWS)


@pytest.mark.parametrize("name", gn_cases.ODOM_NAMES)
def test_odom_caps_hold_for_the_reference_alone(oracle, name):
    """the reference's own rows (rounded to fp32) pass its comparison, and the band around 0.1 leaves out at most 1 % of the case"""
    c = gn_cases.get_odom(name)
    ref = c.ref(c.sel(oracle))
    clean = (ref.ok.astype(np.uint8), np.nan_to_num(ref.rows, nan=np.nan).astype(np.float32))
    n_chk, n_left = gn_ref.compare_odom_rows(clean, ref, gn_ref.C_ODOM_ROWS, what=name)
    assert n_chk + n_left == c.nq and n_left <= 0.01 * c.nq
    if c.iter >= 5 and c.nq >= 255:
        assert (ref.has & (ref.s > 0.1)).sum() > 50 and (ref.has & (ref.s < 0.1)).sum() > 10      # both sides of the cut


def test_planted_odom_row_errors(oracle):
    c = gn_cases.get_odom("odo_m16384")
    ref = c.ref(c.sel(oracle))
    ok, rows = ref.ok.astype(np.uint8), ref.rows.astype(np.float32)
    gn_ref.compare_odom_rows((ok, rows), ref, gn_ref.C_ODOM_ROWS)
    for i in (int(np.nonzero(ref.ok[:4000])[0][50]), 4000 + int(np.nonzero(ref.ok[4000:])[0][50])):      # a corner and a surf query
        for col in range(7):                                              # one row's sign flipped in one column
            bad = rows.copy()
            bad[i, col] = -bad[i, col]
            with pytest.raises(AssertionError, match="beyond"):
                gn_ref.compare_odom_rows((ok, bad), ref, gn_ref.C_ODOM_ROWS)
    no = int(np.nonzero(ref.has & ~ref.ok & gn_ref.odom_decided(ref, gn_ref.C_ODOM_ROWS))[0][3])        # a row below the weight's cut added
    ok2 = ok.copy()
    ok2[no] = 1
    with pytest.raises(AssertionError, match="ok differs"):
        gn_ref.compare_odom_rows((ok2, rows), ref, gn_ref.C_ODOM_ROWS)
    early = gn_ref.odom_rows_ref(c.sel(oracle), np.concatenate([c.sharp, c.flat]), 4000, c.last_corner, c.last_surf, c.corner_idx, c.surf_idx, c.q, c.p, 4)
    with pytest.raises(AssertionError, match="ok differs"):              # the weight of the iterations before the fifth
        gn_ref.compare_odom_rows((early.ok.astype(np.uint8), early.rows.astype(np.float32)), ref, gn_ref.C_ODOM_ROWS)


def test_odom_cases_hold_what_they_claim(oracle):
    sizes = [gn_cases.get_odom(n).nq for n in gn_cases.ODOM_NAMES]
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 16384, 16385):
        assert m in sizes
    assert [gn_cases.odo_blocks(m) for m in (0, 1, 256, 257, 16384, 16385, 10 ** 6)] == [1, 1, 1, 2, 64, 64, 64]
    assert gn_cases.get_odom("odo_corner_only").flat.shape[0] == 0 and gn_cases.get_odom("odo_surf_only").sharp.shape[0] == 0
    assert {gn_cases.get_odom(n).iter for n in gn_cases.ODOM_NAMES} == {4, 5}
    assert {tuple(gn_cases.get_odom(n).q) for n in gn_cases.ODOM_NAMES} >= {(0.0, 0.0, 0.0, 1.0)} and len({tuple(gn_cases.get_odom(n).q) for n in gn_cases.ODOM_NAMES}) == 2
    for it in (4, 5):
        c = gn_cases.get_odom(f"odo_specials_iter{it}")
        ci, si = c.corner_idx, c.surf_idx
        assert (ci[:8] == -1).all() and (ci[64:70, 1] == -1).all() and (ci[64:70, 0] >= 0).all()
        assert (si[:8] == -1).all() and (si[64:70, 1] == -1).all() and (si[70:76, 2] == -1).all() and (si[64:80, 0] >= 0).all() and (si[76:80, 1:] == -1).all()
        ok, rows, _ = c.run(oracle)
        ns = c.sharp.shape[0]
        assert not ok[:8].any() and not ok[64:70].any() and not ok[ns:ns + 8].any() and not ok[ns + 64:ns + 80].any()      # a -1 in any slot: no row
        # ld2 == 0 and pd2 == 0 exactly: the query is its closest point / lies on the dyadic plane z = 4
        assert (c.sharp[10:14, :3] == c.last_corner[ci[10:14, 0], :3]).all() and not ok[c.special["ld2_zero"]].any()
        tri = c.last_surf[si[20]]
        assert (tri[:, 2] == 4).all() and (c.flat[20:24, 2] == 4).all() and not ok[c.special["pd2_zero"]].any()
        # a collinear triple: the normal is 0 / 0; NaN != 0 holds, so before iteration 5 (s = 1) the row exists and is not finite; from
        # iteration 5 the weight is NaN, NaN > 0.1 does not hold, and the row does not exist
        t = c.last_surf[si[30]].astype(np.float64)
        assert (np.cross(t[1, :3] - t[0, :3], t[2, :3] - t[0, :3]) == 0).all()
        col = c.special["collinear"]
        if it == 4:
            assert ok[col].all() and np.isnan(rows[col]).any(axis=1).all()
        else:
            assert not ok[col].any()
        rest = np.setdiff1d(np.arange(c.nq), col)
        assert np.isfinite(rows[rest]).all()
    d = gn_cases.get_odom("odo_deskew_iter5")
    assert not d.no_deskew and (d.sharp[:, 3] % 1 > 0).any()


def test_oracle_odom_rows_hook_checks_its_arguments(oracle):
    gn_cases.check_odom_rows_arguments(oracle)


# ------------------------------------------------------------------------------------------------ folds
@pytest.mark.parametrize("wide", [0, 1])
def test_oracle_folds_integers_exactly(oracle, wide):
    for nb in gn_cases.NBLOCKS:
        P = gn_cases.integer_partials(nb)
        gn_ref.compare_fold(oracle.gn_fold(P, wide), P, f"oracle fold, wide {wide}")
        Q = gn_ref.position_coded(nb)
        gn_ref.compare_fold(oracle.gn_fold(Q, wide), Q, f"oracle fold of the position-coded set, wide {wide}")
    gn_cases.check_fold_arguments(oracle)


def test_fold_cases_hold_what_they_claim():
    want = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 223, 224, 225, 255, 256, 257, 606, 1023, 1024, 1025]
    assert gn_cases.NBLOCKS == want
    P = gn_cases.integer_partials(606)
    assert P.shape == (606, 28) and (P == np.rint(P)).all() and 0 <= P.min() and P.max() < 2 ** 20 and P.max() > 2 ** 19
    Q = gn_ref.position_coded(606)
    assert (Q[:, 0] == np.arange(1, 607)).all() and (Q[:, 1:].sum(axis=1) == 1).all() and Q[:, 1:].sum(axis=0).min() >= 22


# ------------------------------------------------------------------------------------------------ step: the oracle against fp64
def test_oracle_step_meets_fp64(oracle):
    """every case under the comparison the product is held to; C_QR is 4 x the largest ratio the oracle shows where X is checked"""
    top, n_checked, n_side, where = 0.0, 0, 0, ""
    for c in gn_cases.step_cases():
        if c.kind == "nan":
            continue
        ref = c.ref()
        out = c.run(oracle)
        ratio = gn_ref.compare_step(c.state_in, out, ref, left_update=c.left_update, what=c.name, check_X=c.check_X)
        if ref.stepped and c.check_X and gn_ref.at_identity(c.state_in):      # where X is read back exactly and held to its bound
            assert np.isfinite(ref.cond) and ref.cond < 2e4
            n_checked += 1
            if ratio > top:
                top, where = ratio, c.name
        elif ref.stepped and c.check_X:
            n_side += 1
    print(f"largest |X - X_ref| / (EPS32 cond |X|) of the oracle over {n_checked} steps at the identity: {top:.4f} ({where}); constant {gn_ref.C_QR}; "
          f"{n_side} steps at a general pose held to the composition")
    assert n_checked >= 40 and n_side >= 8
    assert 0.9 * gn_ref.C_QR <= 4 * top <= gn_ref.C_QR, (top, gn_ref.C_QR)


@pytest.mark.parametrize("name", [n for n in gn_cases.STEP_NAMES if n.startswith("nan")])
def test_oracle_step_on_a_nan_sum(oracle, name):
    c = gn_cases.step_case(name)
    out = c.run(oracle)
    Ti, To = np.asarray(c.state_in["T"]), np.asarray(out["T"])
    assert int(out["iters"]) == c.iter + 1 and int(out["nsel"]) == 500 and (Ti[4:7] != 0).all()
    if name.endswith("one_rhs"):
        # a NaN in A^T b: X is NaN throughout, t resets to 0, the rotation is lost, nothing converges
        assert (To[4:7] == 0).all() and not np.isfinite(To[:4]).any() and int(out["converged"]) == 0
    else:
        # every sum NaN: no column passes the pivot test, the solve is of rank 0 and X = 0 (as Eigen's solve() of a rank-0 factorisation):
        # T stays as it is, and a zero step passes the abort test
        assert (To[:7].view(np.uint32) == Ti[:7].view(np.uint32)).all() and int(out["converged"]) == 1


def test_step_cases_hold_what_they_claim():
    cases = gn_cases.step_cases()
    well = [c for c in cases if c.kind == "well"]
    conds = np.array([c.ref().cond for c in well])
    assert len(well) >= 12 and conds.min() > 50 and conds.max() < 2e4 and (conds < 2e2).any() and (conds > 5e3).any()
    assert {c.family for c in well} == {0, 1} and all(gn_ref.at_identity(c.state_in) for c in well)
    side = [c for c in cases if c.kind == "side"]
    assert len(side) == 6 and {c.left_update for c in side} == {0, 1} and not any(gn_ref.at_identity(c.state_in) for c in side)
    for c in side:                                                        # every system away from the identity is also a case at it
        twin = gn_cases.step_case(c.name.split("_general_")[0])
        assert (twin.sums == c.sums).all() and twin.kind == "well"
        r = c.ref()
        assert np.abs(r.q - r.q_other_side).max() > 1e-3 and np.linalg.norm(r.X[3:]) > 1e-3
    for c in well:
        r = c.ref()
        assert r.kz == 0 and r.eig.min() > 2 * gn_ref.THRESHOLD[0] and r.nsel >= 400
    for c in cases:
        if c.kind != "decision":
            continue
        r = c.ref()
        for k, v in c.expect.items():
            assert getattr(r, k) == v, (c.name, k, getattr(r, k), v)
        thr = gn_ref.ABORT[c.family]
        if c.name.startswith("abort"):
            # 2 % either side, each alone and together; X = x to a few ulp (a diagonal system)
            for val in (r.delta_r, r.delta_t):
                assert val < 1e-9 or abs(abs(val / thr - 1) - 0.02) < 1e-6, (c.name, val)
            assert r.cond < 3
        if c.name.startswith("spectrum"):
            e = r.eig / gn_ref.THRESHOLD[c.family]
            assert (np.abs(e[:r.kz] - 0.99) < 1e-4).all() and abs(e[r.kz] - 1.01) < 1e-4 and c.iter == 0
            A = r.A
            assert np.abs(A - np.diag(np.diag(A))).max() > 0.05 * np.abs(A).max()      # a rotated basis, not a diagonal
            assert (r.X[:r.kz] == 0).all() and (np.abs(r.X_unmasked[:r.kz]) > 1e-3).all() if r.kz else True
        if c.name.startswith("carried"):
            assert c.iter == 3 and (r.eig < gn_ref.THRESHOLD[c.family]).sum() == 2 != r.kz
    names = {c.name for c in cases}
    for f in (0, 1):
        assert {f"spectrum_f{f}_kz{k}" for k in range(4)} <= names
        assert {f"abort_f{f}_r{a}_t{b}" for a in ("lo", "hi") for b in ("lo", "hi")} <= names
    assert {"odom_nsel9", "odom_nsel10", "map_min50_nsel49", "map_min50_nsel50", "map_min0_nsel3"} <= names
    for c in cases:
        if c.kind == "rankdef":
            j = c.expect["zero"]
            A, g = gn_ref.system_of(c.sums)
            assert not A[j].any() and not A[:, j].any() and g[j] == 0 and c.iter > 0 and np.linalg.matrix_rank(A) == 5
            r = c.ref()
            keep = [k for k in range(6) if k != j]
            assert r.rank == 5 and abs(r.cond / np.linalg.cond(A[np.ix_(keep, keep)]) - 1) < 1e-9 and 10 < r.cond < 100
            assert gn_ref.at_identity(c.state_in) and c.check_X and (np.abs(r.X[keep]) > 1e-3).all() and abs(r.X[j]) < 1e-12


def test_oracle_drops_the_zero_pivot_exactly(oracle):
    """an exactly rank-deficient A^T A (a zero row and column): the dropped pivot's component of X is 0, as ColPivHouseholderQR::solve does"""
    n = 0
    for c in gn_cases.step_cases():
        if c.kind != "rankdef":
            continue
        out = c.run(oracle)
        X = gn_ref.read_back_X(c.state_in, out)
        assert X[c.expect["zero"]] == 0 and np.isfinite(X).all(), (c.name, X)
        n += 1
    assert n == 6


def test_oracle_step_hook_checks_its_arguments(oracle):
    gn_cases.check_step_arguments(oracle)


# ------------------------------------------------------------------------------------------------ the product's qr_solve on the host
def _qr_check_binary(tmp_path_factory):
    out = tmp_path_factory.mktemp("qr_check") / "qr_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "lio-mapping_amd", "csrc"),
                    os.path.join(HERE, "host", "qr_check.cc"), "-o", str(out)], check=True)
    return str(out)


def test_product_qr_solve_on_the_host_vs_scipy(tmp_path_factory):
    """csrc/hmath.h qr_solve<float, 6, 6> and <float, 5, 3> (the template the device step and the plane fit instantiate), compiled for the
    host, on the qr53 / qr66 vectors of tests/golden: held to scipy's pivoted QR with the tolerance tests/test_second_source.py uses for
    the oracle's colpiv_qr_solve"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import second_source as ss
    V = np.load(os.path.join(HERE, "golden", "second_source_vectors.npz"))
    exe = _qr_check_binary(tmp_path_factory)
    ranks, full = [], 0
    for tag, (rows, cols) in (("qr53", (5, 3)), ("qr66", (6, 6))):
        for A, b in zip(V[f"{tag}_A"], V[f"{tag}_b"]):
            A32, b32 = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(b, np.float32)
            assert A32.shape == (rows, cols)
            text = " ".join(v.hex() for v in np.r_[A32.ravel(), b32].astype(np.float64))
            res = subprocess.run([exe, str(rows), str(cols)], input=text, capture_output=True, text=True, check=True)
            x = np.array([float.fromhex(t) for t in res.stdout.split()], np.float32)
            assert x.shape == (cols,) and np.isfinite(x).all()
            x2, k = ss.colpiv_qr_solve(A, b)
            ranks.append(k)
            if k < cols:
                continue       # rounding-determined in Eigen itself (tests/test_second_source.py); finite is what can be asked
            full += 1
            scale = max(np.abs(x2).max(), 1e-6)
            cond = np.linalg.cond(A.astype(np.float64))
            assert np.abs(x - x2).max() <= 4e-6 * min(cond, 1e4) * scale + 1e-6, (tag, k, x, x2)
    assert min(ranks) == 2 and max(ranks) == 6 and full >= 4


# ------------------------------------------------------------------------------------------------ planted errors are noticed
def test_planted_fold_errors():
    P = gn_ref.position_coded(606)
    exact = gn_ref.fold_ref(P)
    gn_ref.compare_fold(exact, P)
    with pytest.raises(AssertionError, match="row 417 was dropped"):
        gn_ref.compare_fold(exact - P[417], P)
    with pytest.raises(AssertionError, match="row 605 was added twice"):
        gn_ref.compare_fold(exact + P[605], P)
    R = gn_cases.integer_partials(606)
    with pytest.raises(AssertionError, match="606 rows"):
        gn_ref.compare_fold(gn_ref.fold_ref(R) - R[0], R)


def _clean_rows(c, form):
    ok, rows, _, _ = c.ref(form)
    r32 = rows.astype(np.float32)
    T = gn_ref.terms_of_rows(ok, r32)
    part = np.zeros((1, 28))
    part[0, :27] = [math.fsum(T[:, k]) for k in range(27)]
    part[0, 27] = ok.sum()
    return ok.astype(np.uint8), r32, part


@pytest.mark.parametrize("form", [0, 1, 2])
def test_planted_row_errors(form):
    c = gn_cases.get_map("m16385")
    ref = c.ref(form)
    ok, r32, part = _clean_rows(c, form)
    gn_ref.compare_rows((ok, r32), ref, gn_ref.C_MAP_ROWS)
    gn_ref.compare_sums(part, ok, r32)
    i = int(np.nonzero(ok)[0][100])
    for col in range(7):                                                  # one row's sign flipped in one column
        bad = r32.copy()
        bad[i, col] = -bad[i, col]
        with pytest.raises(AssertionError, match="beyond|not equal in bits"):
            gn_ref.compare_rows((ok, bad), ref, gn_ref.C_MAP_ROWS)
        # the same flip inside the kernel's sums only: the rows are right, the partials are not
        T_bad = gn_ref.terms_of_rows(ok, bad)
        p_bad = part.copy()
        p_bad[0, :27] = [math.fsum(T_bad[:, k]) for k in range(27)]
        with pytest.raises(AssertionError, match="column"):
            gn_ref.compare_sums(p_bad, ok, r32)
    j = int(np.nonzero(~ref[0])[0][7])                                    # a row of an invalid query added
    ok2, rows2 = ok.copy(), r32.copy()
    ok2[j] = 1
    rows2[j] = gn_ref.map_rows_ref(form, c.stack, np.ones(c.m, np.uint8), c.coeff, c.q, c.t)[1][j]
    with pytest.raises(AssertionError, match="ok differs"):
        gn_ref.compare_rows((ok2, rows2), ref, gn_ref.C_MAP_ROWS)
    T2 = gn_ref.terms_of_rows(ok2, rows2)
    p2 = np.zeros((1, 28))
    p2[0, :27] = [math.fsum(T2[:, k]) for k in range(27)]
    p2[0, 27] = ok.sum() + 1
    with pytest.raises(AssertionError, match="count column"):
        gn_ref.compare_sums(p2, ok, r32)
    p2[0, 27] = ok.sum()                                                  # ... added to the sums but not counted
    with pytest.raises(AssertionError, match="column"):
        gn_ref.compare_sums(p2, ok, r32)
    p3 = part.copy()                                                      # one row of 11000 dropped from the sums, the count kept
    p3[0, :27] -= gn_ref.terms_of_rows(ok, r32)[5000]
    with pytest.raises(AssertionError, match="column"):
        gn_ref.compare_sums(p3, ok, r32)


def _state_of(ref, state_in):
    s = np.array(state_in, capi.GN_STATE)
    s["T"][:4], s["T"][4:7], s["T"][7] = ref.q, ref.t, ref.pad
    s["converged"], s["iters"], s["degenerate"], s["kz"], s["nsel"] = ref.converged, ref.iters, ref.degenerate, ref.kz, ref.nsel
    return s


def test_planted_step_errors():
    c = gn_cases.step_case("spectrum_f0_kz2")
    ref = c.ref()
    clean = _state_of(ref, c.state_in)
    gn_ref.compare_step(c.state_in, clean, ref, what=c.name)
    for off in (-1, +1):                                                  # kz off by one
        wrong = gn_ref.step_ref(0, c.sums, c.state_in, 0)
        wrong.kz = ref.kz + off
        X = wrong.X_unmasked.copy()
        X[:wrong.kz] = 0
        wrong.q, wrong.t = gn_ref.qmul(np.asarray(c.state_in["T"], np.float64)[:4], np.r_[X[:3] / 2, 1.0]), X[3:]
        with pytest.raises(AssertionError, match="kz"):
            gn_ref.compare_step(c.state_in, _state_of(wrong, c.state_in), ref, what=c.name)
        bad = _state_of(wrong, c.state_in)
        bad["kz"] = ref.kz                                                # ... the mask off by one under the right kz
        with pytest.raises(AssertionError, match="masked rotation component|x EPS32 x cond"):
            gn_ref.compare_step(c.state_in, bad, ref, what=c.name)
    for name in ("well_cond100_3", "well_cond10000_3"):                   # right vs left update, away from the identity
        right, left = gn_cases.step_case(name + "_general_right"), gn_cases.step_case(name + "_general_left")
        for c, other in ((right, left), (left, right)):
            ref = c.ref()
            gn_ref.compare_step(c.state_in, _state_of(ref, c.state_in), ref, left_update=c.left_update, what=c.name)
            with pytest.raises(AssertionError, match="from the other side"):
                gn_ref.compare_step(c.state_in, _state_of(other.ref(), c.state_in), ref, left_update=c.left_update, what=c.name)
            for t_wrong in (np.asarray(c.state_in["T"], np.float64)[4:7],                        # the translation not updated,
                            ref.t + ref.X[3:],                                                     # updated twice,
                            np.asarray(c.state_in["T"], np.float64)[4:7] + ref.X[[4, 5, 3]]):      # its components permuted
                bad = _state_of(ref, c.state_in)
                bad["T"][4:7] = t_wrong
                with pytest.raises(AssertionError, match=r"from t_in \+ X"):
                    gn_ref.compare_step(c.state_in, bad, ref, left_update=c.left_update, what=c.name)
        c = gn_cases.step_case(name)                                      # at the identity: one component of X three bounds off, and half a bound
        ref = c.ref()
        bound = gn_ref.C_QR * gn_ref.EPS32 * ref.cond * np.linalg.norm(ref.X)
        for k in (1, 4):
            for mult, passes in ((3.0, False), (0.5, True)):
                bad = _state_of(ref, c.state_in)
                X = ref.X.copy()
                X[k] += mult * bound
                bad["T"][:3], bad["T"][4:7] = X[:3] / 2, X[3:]
                if passes:
                    gn_ref.compare_step(c.state_in, bad, ref, what=name)
                else:
                    with pytest.raises(AssertionError, match="x EPS32 x cond"):
                        gn_ref.compare_step(c.state_in, bad, ref, what=name)
    for c in gn_cases.step_cases():                                       # a wrong solve of the rank-5 subsystem behind the dropped pivot
        if c.kind != "rankdef":
            continue
        ref = c.ref()
        gn_ref.compare_step(c.state_in, _state_of(ref, c.state_in), ref, what=c.name)
        keep = [k for k in range(6) if k != c.expect["zero"]]
        for k, factor in ((keep[0], 3.0), (keep[-1], 1.01)):
            bad = _state_of(ref, c.state_in)
            X = ref.X.copy()
            X[k] *= factor
            bad["T"][:3], bad["T"][4:7] = X[:3] / 2, X[3:]
            with pytest.raises(AssertionError, match="x EPS32 x cond"):
                gn_ref.compare_step(c.state_in, bad, ref, what=c.name)
        swapped = _state_of(ref, c.state_in)                             # the surviving components in the pivoted order
        X = ref.X.copy()
        X[keep] = X[keep[1:] + keep[:1]]
        swapped["T"][:3], swapped["T"][4:7] = X[:3] / 2, X[3:]
        with pytest.raises(AssertionError, match="x EPS32 x cond"):
            gn_ref.compare_step(c.state_in, swapped, ref, what=c.name)
    c = gn_cases.step_case("abort_f1_rlo_tlo")                           # the abort test of the other family
    ref = c.ref()
    s = _state_of(ref, c.state_in)
    s["converged"] = 0
    with pytest.raises(AssertionError, match="converged"):
        gn_ref.compare_step(c.state_in, s, ref, what=c.name)
    c = gn_cases.step_case("odom_nsel9")                                  # a step taken below the row gate
    ref = c.ref()
    took = _state_of(gn_ref.step_ref(1, gn_cases.step_case("odom_nsel10").sums, c.state_in, 2), c.state_in)
    took["nsel"], took["T"][7] = 9, 9.0
    with pytest.raises(AssertionError, match="T moved without a step"):
        gn_ref.compare_step(c.state_in, took, ref, what=c.name)


# ------------------------------------------------------------------------------------------------ one round, the oracle's
@pytest.mark.parametrize("m", [1, 65, 1025])
def test_oracle_round_is_rows_then_step(oracle, m):
    """lio_gn_round of the oracle: the count and the sums are those of the rows lio_gn_rows_map forms at lio_calculate_features' answer, and
    the state is the step on those sums (the oracle's loop accumulates them in fp32: held to the fp64 step's decisions and composition)"""
    map_xyzi, stack, (q, t) = gn_cases.round_scene(m)
    T = capi.TransformF.make(q, t)
    part, st = oracle.gn_round(map_xyzi, stack, T, 8)
    valid, coeff, _ = oracle.calculate_features(map_xyzi, stack, T)
    ok, rows, part2 = oracle.gn_rows_map(0, stack, valid, coeff, T)
    assert part.shape == (1, 28) and int(st["nsel"]) == int(valid.sum()) and int(st["iters"]) == 1
    if m >= 65:
        assert valid.mean() > 0.8
    gn_ref.compare_sums(part, ok, rows, f"oracle round, m {m}")
    gn_ref.compare_bits((part,), (part2,), "the round's partial vs the rows hook's")
    if m == 1025:
        s_in = gn_cases.state(q, t)
        ref = gn_ref.step_ref(0, part[0], s_in, 0)
        assert np.abs(ref.eig / gn_ref.THRESHOLD[0] - 1).min() > 0.05      # no eigenvalue near the threshold: kz is not the accumulation's to decide
        for k in ("nsel", "iters", "kz", "degenerate", "converged"):
            assert int(st[k]) == getattr(ref, k), (k, int(st[k]), getattr(ref, k))
        To = np.asarray(st["T"], np.float64)
        assert 100 * np.abs(To[:4] - ref.q).max() < np.linalg.norm(ref.X[:3]) / 2 and 100 * np.abs(To[4:7] - ref.t).max() < np.linalg.norm(ref.X[3:])
