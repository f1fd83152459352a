"""The dense tail of the marginalization on the device (csrc/marg_kernels.hip: marg_schur_body — the Householder + implicit-QL eigensolver
tridiag_ql_lds and the zero-padded fp64-MFMA Schur complement) on the cases of tests/marg_cases.py, held to the checks of tests/marg_ref.py
with the constants the CPU sources set (tests/test_marg_tail.py); and the tail only the batched kernel k_bw_marg_schur has, J^T J and J^T r
of the new prior formed from LDS, against the factors it was formed from.  Each case is one launch of one workgroup."""
import numpy as np
import pytest

import marg_cases
import marg_ref
from lio_amd import pipeline

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.mark.parametrize("name", marg_cases.NAMES)
def test_device_tail_meets_the_bounds(hip, name):
    c = marg_cases.get(name)
    k_ref = c.k_ref                                                  # the case's own conditions, before the product is asked
    J, r, s = hip.marginalize_schur(c.A, c.b, c.m)
    assert k_ref == c.k_ref
    marg_ref.check(c, J, r, s, marg_cases.K_O, marg_cases.K_R, marg_cases.k_g(c.n), log=print)


@pytest.mark.parametrize("name", marg_cases.EXACT_NAMES)
def test_device_tail_on_the_exact_cases(hip, name):
    """no reflector and immediate deflation leave the input's own numbers: sorted diagonal with ties by index, unit vectors, exact zeros.
    A parameter that nothing couples to keeps them from the middle of a dense block too, on either side of element 64 and several at
    once: marg_schur_body moves such parameters to the front before the reduction (left in place, index i is the sub-diagonal position
    of row i + 1 and that row's reflector mixes it in: before that, 3.5 came back
    rounded and its row of J carried entries of 1e-17 .. 5e-16 beside sqrt(3.5))."""
    c = marg_cases.get(name)
    marg_ref.check_exact(c, *hip.marginalize_schur(c.A, c.b, c.m))


def test_batched_tail_forms_the_prior_from_its_factors(hip):
    """device_solve = 1: k_bw_marg_schur leaves lin_jac / lin_res in LDS (over S and T of marg_schur_body's carve-up) and sums
    JtJ = lin_jac^T lin_jac and Jtr = lin_jac^T lin_res from there, ascending k.  n fp64 terms: each entry is within (n + 1) u of the
    sum of its terms' magnitudes, which Cauchy-Schwarz bounds by max diag(JtJ), respectively sqrt(max diag(JtJ)) |lin_res|; 2 n u is
    asserted.  m = 15, n = 15 + 6 Wo = 27 (a window without the IMU factor, m = 6, is not taken by the device path: estimator.hip
    keeps it on the host, so there is nothing of this kernel to check on it)."""
    from window_util import make_pair
    W, Wo = 4, 2
    ds, clouds, (est,) = make_pair((hip,), "indoor", W, Wo, W + 3, 0.2, cfg_fields={"device_solve": 1})
    est.solve()
    est.slide()
    n = 15 + 6 * Wo
    for k in (W + 1, W + 2):
        rep = pipeline.feed_frame(est, ds, k, clouds[k][0], clouds[k][1])
        assert rep.marginalized == 1
        p, f = est.prior(), est.prior_factor()
        assert p["n"] == f["n"] == n
        J, r = f["lin_jac"].astype(LD), f["lin_res"].astype(LD)
        JtJ = (J.T @ J).astype(np.float64)
        top = float(np.abs(np.diag(JtJ)).max())
        assert top > 0 and np.any(f["lin_res"])
        e_jtj = float(np.abs(p["JtJ"].astype(LD) - J.T @ J).max())
        e_jtr = float(np.abs(p["Jtr"].astype(LD) - J.T @ r).max())
        b_jtj = 2 * n * marg_ref.U * top
        b_jtr = 2 * n * marg_ref.U * np.sqrt(top) * float(np.linalg.norm(f["lin_res"]))
        G = (J @ J.T).astype(np.float64)
        off = float(np.abs(G - np.diag(np.diag(G))).max())
        b_off = marg_cases.K_O * n * marg_ref.U * float(np.diag(G).max())
        print(f"[marg tail] frame {k}: |JtJ - J^T J| {e_jtj:.3e} (bound {b_jtj:.3e})  |Jtr - J^T r| {e_jtr:.3e} (bound {b_jtr:.3e})  "
              f"off-diagonal of J J^T {off:.3e} (bound {b_off:.3e})")
        assert e_jtj <= b_jtj
        assert e_jtr <= b_jtr
        assert off <= b_off
        assert np.all(np.diff(np.diag(G)) >= -marg_cases.K_O * n * marg_ref.U * np.diag(G)[1:])     # the rows' s_k ascend (|row k|^2 = s_k |v_k|^2)
