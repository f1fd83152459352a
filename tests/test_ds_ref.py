"""The references of tests/ds_ref.py checked on the CPU before anything runs on a GPU (docs/device_solve_pins.md):

* the IMU block against the oracle's ImuFactor (lio_factor_imu) on the oracle's own pre-integrations — a formula check, bounded by the
  conditioning of cov^-1 that both sides whiten with in their own way; a flipped sign and a zeroed Jacobian block are caught;
* the product's own statements (csrc/solve_step.h: the aux row, the relative poses, the first linearisation with max_iterations = 0)
  replayed by the one-thread executor of tests/host/aux_row_check.hip against the references, in the unit the GPU tests use and at a
  quarter of their margin — built with the address and undefined-behaviour sanitizers;
* the first dogleg step of tests/golden/second_source.py: CeresDogleg on the reference's normal equations is valid for every case."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ds_cases
import ds_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

# 8 x the largest ratio |ref - oracle| / (cond(cov) eps64 max|block|) seen over the cases below (docs/device_solve_pins.md)
C_FORMULA = 8 * 6.3e-7


@pytest.fixture(scope="module")
def cases(oracle):
    return ds_cases.standard_cases(oracle)


def _oracle_block(case, i):
    x = case["x"]
    res, js = case["pim_handles"][i].factor(x["pose"][i], x["sb"][i], x["pose"][i + 1], x["sb"][i + 1])
    J = np.concatenate([js[0][:, :6], js[1], js[2][:, :6], js[3]], axis=1)
    return J.T @ J, J.T @ res, 0.5 * res @ res


def _formula_ratio(case, i, wrong=None):
    pm = case["pim"][i]
    x = case["x"]
    out, _ = R.imu_block(pm, x["pose"][i], x["sb"][i], x["pose"][i + 1], x["sb"][i + 1], wrong)
    H, g, cost = _oracle_block(case, i)
    cond = np.linalg.cond(pm["cov"])
    big = np.abs(H).max()
    dH = np.abs(np.asarray(out[:900], np.float64).reshape(30, 30) - H).max() / (cond * R.EPS64 * big)
    dg = np.abs(np.asarray(out[900:930], np.float64) - g).max() / (cond * R.EPS64 * max(np.abs(g).max(), 1e-300))
    dc = abs(float(out[930]) - cost) / (cond * R.EPS64 * max(cost, 1e-300))
    return cond, dH, dg, dc


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_imu_block_matches_the_oracle_factor(cases):
    worst = 0.0
    for c in cases:
        for i in range(c["Wo"]):
            cond, dH, dg, dc = _formula_ratio(c, i)
            worst = max(worst, dH, dg, dc)
            assert 1e6 < cond < 1e16, cond
    print(f"IMU block vs oracle: largest |ref - oracle| / (cond(cov) eps64 max) = {worst:.3e}  (bound {C_FORMULA:.3e})")
    assert worst <= C_FORMULA


@pytest.mark.parametrize("wrong", ["sign", "zero_block"])
def test_a_wrong_imu_formula_is_caught(cases, wrong):
    c = cases[1]
    for i in range(c["Wo"]):
        _, dH, dg, dc = _formula_ratio(c, i, wrong)
        assert max(dH, dg) > 100 * C_FORMULA, (wrong, i, dH, dg)


@pytest.fixture(scope="module")
def replay(cases, tmp_path_factory):
    """the product's statements through the one-thread executor, under the address and undefined-behaviour sanitizers"""
    tmp = tmp_path_factory.mktemp("aux_row")
    exe, fin, fout = str(tmp / "aux_row_check"), str(tmp / "in.txt"), str(tmp / "out.txt")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mavx2", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "lio-mapping_amd", "csrc"), os.path.join(ROOT, "tests", "host", "aux_row_check.hip"), "-o", exe], check=True)
    ds_cases.write_cases(fin, cases)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return ds_cases.read_results(fout, cases)


def _lin_of(case):
    lin = dict(case)
    lin["cand"] = case["x"]
    return lin


def test_replayed_aux_row_meets_the_reference(cases, replay, oracle):
    worst = {}
    for k, (c, got) in enumerate(zip(cases, replay)):
        lin = _lin_of(c)
        meta, inp = R.meta_of(lin), R.inputs_of(lin, "cand")
        ref, unit = R.with_unit(lambda q: R.aux_row(meta, q, oracle), inp, seed=k)
        names = ["imu_out", "lmap", "cand_Rt"] + (["prior_out"] if c["have_prior"] else []) + (["exprior_out"] if c["use_ex_prior"] else [])
        for name in names:
            g = got[name]
            if name == "lmap":
                assert np.all(g[:, 247] == 0)
                g = g[:, :247]
            if name == "exprior_out":
                g = g[:43]
            r = R.ratio(g, ref[name], unit[name])
            worst[name] = max(worst.get(name, 0.0), r)
        assert np.all(got["imu_out"][:, 931] == 1.0)
    print("one-thread replay, largest |Q - R| / u per array:", {k: round(v, 3) for k, v in worst.items()})
    for name, r in worst.items():
        assert r <= R.CPU_MARGIN, (name, r)


def test_replayed_first_linearisation_meets_the_reference(cases, replay, oracle):
    worst = {}
    for k, (c, got) in enumerate(zip(cases, replay)):
        lin = _lin_of(c)
        meta, inp = R.meta_of(lin), R.inputs_of(lin, "x", S=c["S"])
        ref, unit = R.with_unit(lambda q: R.assemble(meta, q, oracle), inp, seed=100 + k)
        assert (got["it"], got["termination"], got["done"], got["need_host"]) == (0, 0, 1, 0)
        for name, g in (("scale", got["scale"]), ("H", got["Hcur"]), ("g", got["g"]), ("costs", got["costs0"])):
            worst[name] = max(worst.get(name, 0.0), R.ratio(g, ref[name], unit[name]))
        # entries no factor touches are exactly zero
        zero = np.asarray(unit["H"] == 0)
        assert zero.any() and np.all(got["Hcur"][zero] == 0)
    print("one-thread replay of the first linearisation, largest |Q - R| / u per array:", {k: round(v, 3) for k, v in worst.items()})
    for name, r in worst.items():
        assert r <= R.CPU_MARGIN, (name, r)


def test_a_misplaced_block_is_far_outside_the_margin(cases, replay, oracle):
    """what the margin is for: one IMU block one frame off, or a stale value in one entry, misses by orders of magnitude"""
    c, got = cases[4], replay[4]
    lin = _lin_of(c)
    meta, inp = R.meta_of(lin), R.inputs_of(lin, "x", S=c["S"])
    ref, unit = R.with_unit(lambda q: R.assemble(meta, q, oracle), inp, seed=7)
    H = got["Hcur"].copy()
    H[15:45, 15:45], H[30:60, 30:60] = got["Hcur"][30:60, 30:60], got["Hcur"][15:45, 15:45]
    assert R.ratio(H, ref["H"], unit["H"]) > 1e6
    H = got["Hcur"].copy()
    H[3, 20] = got["Hcur"][3, 21]
    assert R.ratio(H, ref["H"], unit["H"]) > 1e3


def test_first_dogleg_step_of_the_reference_is_valid(cases, oracle):
    """the candidate step the GPU test compares with exists for every case (no draw has to be skipped)"""
    from second_source import CeresDogleg

    for c in cases:
        lin = _lin_of(c)
        meta, inp = R.meta_of(lin), R.inputs_of(lin, "x", S=c["S"])
        ref, _ = R.assemble(meta, inp, oracle)
        dl = CeresDogleg(np.asarray(ref["H_unscaled"], np.float64), np.asarray(ref["g_unscaled"], np.float64), float(ref["costs"].sum()))
        step, model = dl.compute_step()
        assert step is not None and model > 0
