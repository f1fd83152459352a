"""csrc/knn_merge.h on the host — the merge of two five-entry K-NN lists by a fixed network, and the four-candidate form the walk's trips
use — held to std::sort over every order pattern of its inputs (tests/host/knn_merge_check.cc); and that the maps of
tests/knn_merge_cases.py put the winners where their names say, so that tests/test_gpu_knn_merge.py has to compare results only.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import knn_merge_cases as cases
import knn_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def check_binary(tmp_path_factory):
    out = tmp_path_factory.mktemp("knn_merge_check") / "knn_merge_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "lio-mapping_amd", "csrc"),
                    os.path.join(HERE, "host", "knn_merge_check.cc"), "-o", str(out)], check=True)
    return str(out)


def test_merges_equal_std_sort_on_every_order_pattern(check_binary):
    res = subprocess.run([check_binary], capture_output=True, text=True)
    print(res.stdout, res.stderr)
    assert res.returncode == 0, res.stderr
    m = re.match(r"knn_merge5: (\d+) cases, knn_merge4: (\d+) cases, 0 differ", res.stdout)
    # three key maps x the dealings of na + nb ranks over two lists, na, nb in 0..5: sum of C(na + nb, na) = 923
    assert m and int(m.group(1)) == 3 * 923 and int(m.group(2)) > 24 * 3 * 252, res.stdout


def test_the_check_notices_a_short_network_and_an_unsorted_four(check_binary):
    res = subprocess.run([check_binary, "planted"], capture_output=True, text=True, check=True)
    m = re.match(r"planted: .* noticed in (\d+) cases, .* in (\d+)", res.stdout)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, res.stdout


# ------------------------------------------------------------------------------------------------ the steering maps
def _winner_positions(c, i):
    """flat positions of query i's five reference neighbours, which must be single points of their cells; total candidates"""
    rows, first, single = cases.flat_positions(c, i)
    top = c.ref[0][i, :5]
    assert (top >= 0).all()
    at = {int(r): k for k, r in enumerate(rows)}
    ks = [at[int(r)] for r in top]
    assert all(single[k] for k in ks), "a winner shares its cell: its position is not fixed"
    return np.array([first[k] for k in ks]), len(rows)


@pytest.mark.parametrize("name", ["five_on_one_sublane", "four_on_one_sublane_of_eight", "one_winner_per_sublane", "winners_in_last_trip"])
def test_steered_winners_are_the_five_nearest_and_sit_where_stated(name):
    c = cases.get(name)
    assert c.query.shape[0] == cases.NQ > 256 // 4
    for i in range(cases.NQ):
        assert set(c.ref[0][i, :5].tolist()) == set(c.winners[i].tolist())
        pos, total = _winner_positions(c, i)
        if name == "five_on_one_sublane":
            assert len(set(pos % 8)) == 1 and len(set(pos % 4)) == 1 and total > 32
        elif name == "four_on_one_sublane_of_eight":
            assert np.bincount(pos % 8).max() == 4
        elif name == "one_winner_per_sublane":
            assert len(set(pos % 8)) == 5 and len(set(pos % 4)) == 4
        else:
            for lanes in cases.LANES:
                assert (pos // (4 * lanes) == (total - 1) // (4 * lanes)).all() and total > 4 * lanes


def test_lattice_has_exact_ties_at_the_fifth_rank_decided_by_the_index():
    c = cases.get("lattice_ties")
    idx, sqd = c.ref[0], c.ref[1]
    assert knn_ref.rank56_ties((idx, sqd)) == cases.NQ            # every query: the sixth candidate is as far as the fifth
    assert (idx[:, 4] < idx[:, 5]).all()
    assert {float(v) for v in sqd[:, 4]} == {0.5625, 1.125}
    for i in range(cases.NQ):
        _, _, single = cases.flat_positions(c, i)
        assert single.all()
    # indices run against the flat order often enough: the tie is not decided by who comes first in the walk
    rows, first, _ = cases.flat_positions(c, 0)
    assert (np.diff(rows) < 0).any()


def test_sparse_blocks_and_trip_boundaries_hold_the_stated_totals():
    c = cases.get("sparse_blocks")
    found = (c.ref[0][:, :5] >= 0).sum(axis=1)
    assert found.tolist() == [min(t, 5) for t in c.totals]
    assert {0, 1, 4, 5}.issubset(set(found.tolist())) and 6 in c.totals
    for w in range(0, cases.NQ, 8):                               # a wave at eight lanes per query: eight consecutive queries
        assert 0 in c.totals[w:w + 8] and 26 in c.totals[w:w + 8]
    c = cases.get("trip_boundaries")
    assert set(c.totals) == {15, 16, 17, 31, 32, 33}
    for i in range(cases.NQ):
        assert len(cases.flat_positions(c, i)[0]) == c.totals[i]
