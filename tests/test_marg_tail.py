"""The dense tail of the marginalization on the CPU: every case of tests/marg_cases.py through the oracle (cyclic Jacobi) and through the numpy
second source (LAPACK), held to the checks of tests/marg_ref.py.  This proves the cases, their self-conditions and the bounds with the
references alone; tests/test_gpu_marg_tail.py then holds csrc/marg_kernels.hip to the same.  Run with -s for the table of measured ratios
that the constants K_o, K_r, K_g of tests/marg_cases.py come from."""
import os
import sys

import numpy as np
import pytest

import marg_cases
import marg_ref

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import second_source as ss  # noqa: E402


def _run(source, oracle, c):
    return oracle.marginalize_schur(c.A, c.b, c.m) if source == "oracle" else ss.marginalize_schur(c.A, c.b, c.m)


@pytest.mark.parametrize("name", marg_cases.NAMES)
def test_case_conditions_hold_on_the_reference_alone(name):
    c = marg_cases.get(name)
    assert c.A.shape == (c.m + c.n, c.m + c.n) and c.S_ref.shape == (c.n, c.n)
    assert np.array_equal(c.S_ref, c.S_ref.T)
    assert 0 <= c.k_ref <= c.n                                       # (k_ref runs the self-conditions)
    if not c.schur:                                                  # pure cases: S sits in A untouched behind a decoupled unit block
        assert c.m == 1 and c.A[0, 0] == 1.0 and not c.A[0, 1:].any() and not c.A[1:, 0].any()
        assert np.array_equal(c.A[1:, 1:], c.S_ref) and np.array_equal(c.b[1:], c.bs_ref)


@pytest.mark.parametrize("source", ["oracle", "numpy"])
@pytest.mark.parametrize("name", marg_cases.NAMES)
def test_cpu_sources_meet_the_bounds(oracle, source, name):
    c = marg_cases.get(name)
    J, r, s = _run(source, oracle, c)
    marg_ref.check(c, J, r, s, marg_cases.K_O, marg_cases.K_R, marg_cases.k_g(c.n))


@pytest.mark.parametrize("source", ["oracle", "numpy"])
@pytest.mark.parametrize("name", marg_cases.EXACT_NAMES)
def test_cpu_sources_on_the_exact_cases(oracle, source, name):
    """The oracle gives all of it bit for bit (a Jacobi sweep leaves a zero off-diagonal entry alone).  LAPACK's divide and conquer gives
    the zero matrix and the diagonal one exactly but orders equal eigenvalues as its merge left them, and it returns the isolated 3.5
    with an error of 24 ulp: for it the tie order is not asserted, and the isolated case is held to the bounds only."""
    c = marg_cases.get(name)
    if source == "numpy" and c.exact == "isolated":
        return
    marg_ref.check_exact(c, *_run(source, oracle, c), tie_order=source == "oracle")


def test_measured_ratio_table(oracle):
    """the worst ratio per source and quantity over all cases, and the constants they give: 4 x the larger, at least 8 (the table in
    the docstring of tests/marg_cases.py is this output where the constants were set; another LAPACK build moves its ratios a little)."""
    keys = ("o", "r_pairs", "r_span", "r_rest", "g_grad", "g_cost", "g_grad_n1", "g_cost_n1")
    worst = {src: dict.fromkeys(keys, 0.0) for src in ("oracle", "numpy")}
    where = {src: dict.fromkeys(keys, "-") for src in ("oracle", "numpy")}
    for name in marg_cases.NAMES:
        c = marg_cases.get(name)
        for src in worst:
            J, r, s = _run(src, oracle, c)
            marg_ref.structure(J, r, s, c.k_ref)
            q = marg_ref.ratios(c.S_ref, c.bs_ref, J, r, s)
            for k in ("g_grad", "g_cost"):                            # n = 1 has a K_g of its own (tests/marg_cases.py)
                q[k + "_n1"] = q[k] if c.n == 1 else 0.0
                q[k] = 0.0 if c.n == 1 else q[k]
            for k in keys:
                if q[k] > worst[src][k]:
                    worst[src][k], where[src][k] = q[k], name
    print()
    for k in keys:
        print(f"  {k:9s} oracle {worst['oracle'][k]:7.3f} ({where['oracle'][k]:28s})  numpy {worst['numpy'][k]:7.3f} ({where['numpy'][k]})")
    groups = (("K_O", ("o",), marg_cases.K_O), ("K_R", ("r_pairs", "r_span", "r_rest"), marg_cases.K_R), ("K_G", ("g_grad", "g_cost"), marg_cases.K_G),
              ("K_G_N1", ("g_grad_n1", "g_cost_n1"), marg_cases.K_G_N1))
    for K, group, have in groups:
        top = max(worst[src][k] for src in worst for k in group)
        print(f"  {K} = max(8, 4 x worst) = {max(8.0, 4.0 * top):.2f}; tests/marg_cases.py has {have}")
        assert have >= 8.0 and have >= top


def test_fixture_regenerates():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_marg_tail_refs

    out = make_marg_tail_refs.generate()
    with np.load(marg_cases.FIXTURE) as f:
        assert sorted(f.files) == sorted(out)
        for k, v in out.items():
            assert np.array_equal(f[k], v), k
