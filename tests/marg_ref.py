"""References and checks for the dense tail of the marginalization (MarginalizationFactor.cc:271-302): what tests/test_marg_tail.py (oracle,
numpy second source) and tests/test_gpu_marg_tail.py (csrc/marg_kernels.hip) hold an implementation's (J, r, s) to.

The reference of a case is the Schur complement itself, S_ref and bs_ref, not a second eigensolver: every check below is a statement
about (J, r, s) and S_ref that holds for ANY correct eigendecomposition, whichever basis it picks inside a cluster and whichever sign it
gives a vector.  The checks' own arithmetic runs in long double (64-bit mantissa on x86: its rounding is 2^-11 of the bounds').

  u = 2^-52,  kept = s > 1e-8,  k = #kept,  V = J[kept] / sqrt(s[kept]) (rows),  P = V^T V,  nS = ||S_ref||_2

  structure      s ascending, k == k_ref, rows of J and entries of r with s <= 1e-8 exactly zero
  orthonormal    max |V V^T - I|                              <= K_o n u
  eigenpairs     max_k ||S_ref v_k - s_k v_k||_2              <= K_r n u nS     (V orthonormal and complete: every kept s_k then lies
                                                                                 within that distance of an eigenvalue of its own)
  completeness   max |P S_ref P - J^T J|                      <= K_r n u nS
                 lambda_max((I - P) S_ref (I - P))            <= 1e-8 + K_r n u nS
  gradient       ||J^T r - P bs_ref||_inf                     <= K_g n u ||bs_ref||_inf g,   g = max(1, sqrt(nS / min kept s))
  cost           |r^T r - bs_ref^T V^T diag(1 / s) V bs_ref|  <= K_g n u g times the latter
"""
import numpy as np

U = 2.0 ** -52
EPS = 1e-8          # the cut of MarginalizationFactor.cc:276-302: eigenvalues <= 1e-8 (absolute) are dropped
LD = np.longdouble


def schur_ref_mp(A, b, m, digits=40):
    """(S_ref, bs_ref) of MarginalizationFactor.cc:275-291 in `digits`-digit arithmetic, rounded to fp64: Amm symmetrised, Amm^+ through
    its eigendecomposition with the > 1e-8 cut, Arm from the lower-left block and Amr from the upper-right one, and the lower triangle
    of S mirrored (SelfAdjointEigenSolver reads that one, :293)."""
    import mpmath as mp

    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    n = A.shape[0] - m
    with mp.workdps(digits):
        M = mp.matrix(A.tolist())
        bv = mp.matrix(b.tolist())
        Amm = mp.matrix(m, m)
        for i in range(m):
            for j in range(m):
                Amm[i, j] = (M[i, j] + M[j, i]) / 2
        w, Q = mp.eigsy(Amm)
        pinv = mp.matrix(m, m)
        for k in range(m):
            if w[k] > mp.mpf(EPS):
                qk = Q[:, k]
                pinv += qk * qk.T / w[k]
        T = M[m:, :m] * pinv
        S = M[m:, m:] - T * M[:m, m:]
        bs = bv[m:] - T * bv[:m]
        S_ref = np.zeros((n, n))
        for i in range(n):
            for j in range(i + 1):
                S_ref[i, j] = S_ref[j, i] = float(S[i, j])
        bs_ref = np.array([float(bs[i]) for i in range(n)])
    return S_ref, bs_ref


def self_conditions(A, m, S_ref):
    """What a case asserts about itself from the reference alone, before any output is looked at: its spectra keep clear of the cut by
    far more than any implementation's rounding (u nS <= 1e-12 on every case), so the kept count k_ref is a property of the case.
    Returns k_ref."""
    w = np.linalg.eigvalsh(S_ref)
    assert not np.any((w > 1e-10) & (w < 1e-6)), w[(w > 1e-10) & (w < 1e-6)]
    Amm = 0.5 * (A[:m, :m] + A[:m, :m].T)
    wm = np.linalg.eigvalsh(Amm)
    assert not np.any((wm > 1e-11) & (wm < 1e-5)), wm[(wm > 1e-11) & (wm < 1e-5)]
    return int((w > EPS).sum())


def _ratio(num, den):
    num = float(num)
    return 0.0 if num <= 0.0 else (num / den if den > 0.0 else np.inf)


def structure(J, r, s, k_ref):
    """the exact part of the contract (include/lio_c.h: lio_marginalize_schur)"""
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(r)) and np.all(np.isfinite(s))
    assert np.all(np.diff(s) >= 0), s
    kept = s > EPS
    assert int(kept.sum()) == k_ref, (int(kept.sum()), k_ref, s)
    assert not J[~kept].any() and not r[~kept].any()


def ratios(S_ref, bs_ref, J, r, s):
    """every bounded quantity divided by its bound without the K: {'o': ..., 'r': ..., 'g': ...} (the larger of each group)"""
    n = s.shape[0]
    S, bs = S_ref.astype(LD), bs_ref.astype(LD)
    nS = float(np.linalg.norm(S_ref, 2))
    kept = s > EPS
    sk = s[kept].astype(LD)
    V = J[kept].astype(LD) / np.sqrt(sk)[:, None]
    Jl, rl = J.astype(LD), r.astype(LD)
    k = V.shape[0]
    out = {}
    out["o"] = _ratio(np.abs(V @ V.T - np.eye(k, dtype=LD)).max() if k else 0.0, n * U)
    res = V @ S - sk[:, None] * V                                  # row k: (S v_k - s_k v_k)^T, S symmetric
    out["r_pairs"] = _ratio(np.sqrt((res * res).sum(axis=1)).max() if k else 0.0, n * U * nS)
    P = V.T @ V
    out["r_span"] = _ratio(np.abs(P @ S @ P - Jl.T @ Jl).max(), n * U * nS)
    Q = np.eye(n, dtype=LD) - P
    rest = (Q @ S @ Q).astype(np.float64)
    out["r_rest"] = _ratio(np.linalg.eigvalsh(0.5 * (rest + rest.T)).max() - EPS, n * U * nS)
    out["r"] = max(out["r_pairs"], out["r_span"], out["r_rest"])
    g = max(1.0, float(np.sqrt(nS / float(sk.min())))) if k else 1.0
    out["g_grad"] = _ratio(np.abs(Jl.T @ rl - P @ bs).max(), n * U * float(np.abs(bs_ref).max()) * g)
    c = V @ bs
    cost_ref = (c * c / sk).sum() if k else LD(0)
    out["g_cost"] = _ratio(abs(rl @ rl - cost_ref), n * U * g * float(cost_ref))
    out["g"] = max(out["g_grad"], out["g_cost"])
    return out


def check(case, J, r, s, K_o, K_r, K_g, log=None):
    structure(J, r, s, case.k_ref)
    q = ratios(case.S_ref, case.bs_ref, J, r, s)
    if log is not None:
        log(f"{case.name:28s} n {case.n:2d} m {case.m:2d} k {case.k_ref:2d}  orth {q['o']:7.3f}  pairs {q['r_pairs']:7.3f}  span {q['r_span']:7.3f}  "
            f"rest {q['r_rest']:7.3f}  grad {q['g_grad']:7.3f}  cost {q['g_cost']:7.3f}")
    assert q["o"] <= K_o, ("orthonormality", q)
    assert q["r_pairs"] <= K_r, ("eigenpairs", q)
    assert q["r_span"] <= K_r and q["r_rest"] <= K_r, ("completeness", q)
    assert q["g_grad"] <= K_g, ("gradient", q)
    assert q["g_cost"] <= K_g, ("cost", q)
    return q


def check_exact(case, J, r, s, tie_order=True):
    """diagonal / isolated parameter / zero: what has to come out bit for bit (case.exact says which).  tie_order: equal eigenvalues of
    the diagonal case come in ascending original index (off: in any order, each index once)"""
    kind = case.exact
    n = case.n
    if kind == "zero":
        assert not J.any() and not r.any() and not s.any()
    elif kind == "diagonal":
        d = np.diag(case.S_ref)
        order = np.argsort(d, kind="stable")                       # equal values in ascending original index
        assert np.array_equal(s, d[order]), (s, d[order])
        if not tie_order:                                           # the order the implementation chose inside each run of equal values
            order = np.array([int(np.argmax(J[k] != 0)) if J[k].any() else order[k] for k in range(n)])
            assert np.array_equal(np.sort(order), np.arange(n)) and np.array_equal(s, d[order])
        want = np.zeros((n, n))
        want[np.arange(n), order] = np.where(d[order] > EPS, np.sqrt(d[order]), 0.0)
        assert np.array_equal(J, want), np.argwhere(J != want)[:8]
    elif kind == "isolated":
        for j, val in case.isolated:
            rows = np.flatnonzero(s == val)
            assert rows.shape[0] == 1, (j, val, s)
            want = np.zeros(n)
            want[j] = np.sqrt(val) if val > EPS else 0.0
            assert np.array_equal(J[rows[0]], want), (j, val, J[rows[0]])
    else:
        raise AssertionError(kind)
