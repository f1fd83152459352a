"""The cases the dense tail of the marginalization is pinned on (tests/test_marg_tail.py on the CPU: the oracle and the numpy second source;
tests/test_gpu_marg_tail.py: csrc/marg_kernels.hip through lio_marginalize_schur).  Every case is seeded and is (A, b, m) plus its reference
(S_ref, bs_ref) and what it knows about itself (k_ref, `exact`); the checks are in tests/marg_ref.py.

Pure eigensolver cases: A = [[1, 0], [0, S]] with m = 1, so T = Arm Amm^+ = 0 and the Schur complement an implementation decomposes is S
bit for bit — S_ref = S and bs_ref = b[1:] need no arithmetic.  Schur cases: A = Jm^T Jm from a Gaussian Jm with 4 (m + n) rows and
b = Jm^T e; S_ref and bs_ref are the 40-digit values of tests/golden/marg_tail_refs.npz (tests/golden/make_marg_tail_refs.py).

The constants of the bounds.  Each is 4 x the worst ratio (quantity / bound without K, tests/marg_ref.py: ratios) that the project's two
CPU sources reach over ALL cases, and at least 8; the device is held to them, it did not set them.  Measured by tests/test_marg_tail.py
(which prints the table per case with -s):

                         oracle (cyclic Jacobi)             second source (LAPACK dsyevd)      4 x max    K
  K_o  orthonormality     5.247  clusters_n72                0.655  schur_m15_n15               20.99     21
  K_r  eigenpairs         3.159  clusters_n72                0.302  toeplitz_n3
       P S P - J^T J      1.281  schur_m15_n1                0.491  toeplitz_n3
       rest above cut     0.000                              0.000                              12.63     13
  K_g  gradient           0.100  schur_m15_n16               0.266  toeplitz_n2
       cost               0.161  toeplitz_n2                 0.515  toeplitz_n2                  2.06      8
  K_g at n = 1
       gradient           9.022  schur_m15_n1               15.690  schur_m15_n1
       cost              18.045  schur_m15_n1               31.379  schur_m15_n1               125.52    126

(n = 1 has a K_g of its own: the bound's n u is one ulp there and the fifteen products of bs = br - T bm alone round by more.  Measured
over all cases as one group it would be 126 everywhere, sixteen times looser than the sources need at n >= 2.)
"""
import functools
import os

import numpy as np

import marg_ref

K_O, K_R, K_G, K_G_N1 = 21.0, 13.0, 8.0, 126.0


def k_g(n):
    return K_G_N1 if n == 1 else K_G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marg_tail_refs.npz")


class Case:
    def __init__(self, name, A, b, m, S_ref=None, bs_ref=None, exact=None):
        self.name, self.m, self.exact = name, int(m), exact
        self.A = np.ascontiguousarray(A, np.float64)
        self.b = np.ascontiguousarray(b, np.float64)
        self.n = self.A.shape[0] - self.m
        self.schur = S_ref is None                                   # a case whose reference is the high-precision fixture
        self._ref = None if S_ref is None else (np.ascontiguousarray(S_ref, np.float64), np.ascontiguousarray(bs_ref, np.float64))

    def _load(self):
        if self._ref is None:
            with np.load(FIXTURE) as f:
                self._ref = (f[self.name + "_S"], f[self.name + "_bs"])
            assert self._ref[0].shape == (self.n, self.n) and self._ref[1].shape == (self.n,)
        return self._ref

    @property
    def S_ref(self):
        return self._load()[0]

    @property
    def bs_ref(self):
        return self._load()[1]

    @functools.cached_property
    def k_ref(self):
        return marg_ref.self_conditions(self.A, self.m, self.S_ref)


# ------------------------------------------------------------------------------------------------ pure eigensolver cases
def _pure(name, S, seed, exact=None):
    n = S.shape[0]
    assert np.array_equal(S, S.T)
    A = np.zeros((n + 1, n + 1))
    A[0, 0] = 1.0
    A[1:, 1:] = S
    b = np.random.default_rng(seed).normal(size=n + 1)
    return Case(name, A, b, 1, S, b[1:], exact)


def _sym(M):
    """a product Q D Q^T rounded: exactly symmetric (its lower triangle mirrored)"""
    return np.tril(M) + np.tril(M, -1).T


def _orth(rng, n):
    return np.linalg.qr(rng.normal(size=(n, n)))[0]


def _gram(rng, n):
    G = rng.normal(size=(4 * n, n))
    return G.T @ G


def _diagonal():
    """no reflector at any row, every eigenvalue deflates at once: the values repeat (ties by index) and are unsorted; one is below the cut"""
    rng = np.random.default_rng(101)
    d = rng.choice(np.array([0.25, 1.0, 3.0, 7.5, 1e3, 2.0 ** -40, 0.0, 2.0 ** -3, 6.0]), size=80)
    return _pure("diagonal_n80", np.diag(d), 101, exact="diagonal")


def _isolated():
    """one parameter that nothing couples to inside a dense block: row 11 asks for no reflector, and QL deflates it between two blocks"""
    rng = np.random.default_rng(102)
    S = _sym(_gram(rng, 30))
    S[11, :] = 0.0
    S[:, 11] = 0.0
    S[11, 11] = 3.5
    c = _pure("isolated_parameter_n30", S, 102, exact="isolated")
    c.isolated = ((11, 3.5),)
    return c


def _isolated_many():
    """the same at an odd n with several such parameters at once: on either side of element 64, the last one, and one below the cut"""
    rng = np.random.default_rng(104)
    S = _sym(_gram(rng, 79))
    iso = ((3, 3.5), (63, 0.75), (64, 1e3), (70, 2.0 ** -40), (78, 12.0))
    for j, v in iso:
        S[j, :] = 0.0
        S[:, j] = 0.0
        S[j, j] = v
    c = _pure("isolated_parameters_n79", S, 104, exact="isolated")
    c.isolated = iso
    return c


def _zero():
    return _pure("zero_n17", np.zeros((17, 17)), 103, exact="zero")


def _toeplitz(n):
    """already tridiagonal, 2 I - E - E^T: eigenvalues 2 - 2 cos(k pi / (n + 1)); n = 63 / 64 / 65 is where lane k's second element and the
    second ballot word begin"""
    S = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    return _pure(f"toeplitz_n{n}", S, 110 + n)


def _blocks(n1, n2):
    """two dense blocks nothing couples: the sub-diagonal is exactly zero at n1, on either side of element 64"""
    rng = np.random.default_rng(120 + n1)
    S = np.zeros((n1 + n2, n1 + n2))
    S[:n1, :n1] = _sym(_gram(rng, n1))
    S[n1:, n1:] = _sym(_gram(rng, n2))
    return _pure(f"blocks_{n1}_{n2}", S, 120 + n1)


def _clusters():
    rng = np.random.default_rng(130)
    Q = _orth(rng, 72)
    w = np.r_[np.full(18, 1.0), np.full(36, 5.0), np.full(18, 100.0)]
    return _pure("clusters_n72", _sym((Q * w) @ Q.T), 130)


def _wilkinson():
    """W21+: diagonal |10 .. 0 .. 10|, sub-diagonal 1 — pairs of eigenvalues that agree to 1e-14 relative"""
    S = np.diag(np.abs(np.arange(-10, 11)).astype(np.float64)) + np.eye(21, k=1) + np.eye(21, k=-1)
    return _pure("wilkinson_w21", S, 131)


def _indefinite():
    rng = np.random.default_rng(132)
    Q = _orth(rng, 33)
    return _pure("indefinite_n33", _sym((Q * np.linspace(-3, 3, 33)) @ Q.T), 132)


def _cut():
    """eigenvalues on both sides of the absolute 1e-8 cut, nS = 1"""
    rng = np.random.default_rng(133)
    Q = _orth(rng, 40)
    w = np.r_[np.full(10, 1.0), np.full(10, 1e-3), np.full(10, 1e-5), np.full(5, 1e-11), np.zeros(5)]
    return _pure("cut_both_sides_n40", _sym((Q * w) @ Q.T), 133)


# ------------------------------------------------------------------------------------------------ Schur cases
def _grid(x):
    """multiples of 2^-10: the sums of products below are then exact in fp64, so (A, b) are the same bits under any BLAS and the
    committed references belong to them"""
    return np.round(x * 1024.0) / 1024.0


def _schur(name, m, n, null=0, asym=False):
    seed = 1000 * m + 10 * n + null + (5 if asym else 0)
    rng = np.random.default_rng(seed)
    N = m + n
    Jm = _grid(rng.normal(size=(4 * N, N)))
    if null:   # a lidar-degenerate dropped pose: the last `null` columns of the dropped block are combinations of its others
        Jm[:, m - null:m] = Jm[:, :m - null] @ (rng.integers(-4, 5, size=(m - null, null)) / 4.0)
    A = Jm.T @ Jm
    if asym:   # MarginalizationFactor.cc:275, :286-293 — Amm symmetrised, Arm / Amr from their own blocks, the lower triangle of S read
        A = A + 0.5 * np.triu(rng.normal(size=(N, N)), 1)
    b = Jm.T @ _grid(rng.normal(size=4 * N))
    return Case(name, A, b, m)


_MAKERS = dict(diagonal_n80=_diagonal, isolated_parameter_n30=_isolated, isolated_parameters_n79=_isolated_many, zero_n17=_zero)
for _n in (2, 3, 63, 64, 65, 80):
    _MAKERS[f"toeplitz_n{_n}"] = functools.partial(_toeplitz, _n)
for _a, _b in ((63, 17), (64, 16), (65, 15)):
    _MAKERS[f"blocks_{_a}_{_b}"] = functools.partial(_blocks, _a, _b)
_MAKERS.update(clusters_n72=_clusters, wilkinson_w21=_wilkinson, indefinite_n33=_indefinite, cut_both_sides_n40=_cut)
for _m in (1, 2, 7, 14, 15):
    _MAKERS[f"schur_m{_m}_n20"] = functools.partial(_schur, f"schur_m{_m}_n20", _m, 20)
for _n in (1, 15, 16, 17, 33, 79):
    _MAKERS[f"schur_m15_n{_n}"] = functools.partial(_schur, f"schur_m15_n{_n}", 15, _n)
_MAKERS["schur_rank_deficient_m15_n20"] = functools.partial(_schur, "schur_rank_deficient_m15_n20", 15, 20, null=2)
_MAKERS["schur_rank_deficient_m6_n33"] = functools.partial(_schur, "schur_rank_deficient_m6_n33", 6, 33, null=1)
_MAKERS["schur_asymmetric_m9_n18"] = functools.partial(_schur, "schur_asymmetric_m9_n18", 9, 18, asym=True)
NAMES = tuple(_MAKERS)
SCHUR_NAMES = tuple(k for k in NAMES if k.startswith("schur_"))
EXACT_NAMES = ("diagonal_n80", "isolated_parameter_n30", "isolated_parameters_n79", "zero_n17")


@functools.lru_cache(maxsize=None)
def get(name):
    c = _MAKERS[name]()
    assert c.name == name, (c.name, name)
    return c
