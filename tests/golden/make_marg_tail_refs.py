"""Generates tests/golden/marg_tail_refs.npz: the Schur complement S_ref and reduced gradient bs_ref of every Schur case of
tests/marg_cases.py in 40-digit arithmetic (mpmath), rounded to fp64 — tests/marg_ref.py: schur_ref_mp.

  python tests/golden/make_marg_tail_refs.py

<case>_S    n x n, symmetric (the lower triangle of MarginalizationFactor.cc:291's S, mirrored)
<case>_bs   n

The pure eigensolver cases need no entry: their S_ref is their input.  Needs mpmath; the tests that read the file do not."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import marg_cases  # noqa: E402
import marg_ref  # noqa: E402


def generate():
    out = {}
    for name in marg_cases.SCHUR_NAMES:
        c = marg_cases.get(name)
        out[name + "_S"], out[name + "_bs"] = marg_ref.schur_ref_mp(c.A, c.b, c.m)
    return out


def main():
    out = generate()
    np.savez_compressed(marg_cases.FIXTURE, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(marg_cases.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
