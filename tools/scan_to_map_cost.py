"""The scan-to-map loop of this tree against another build of the product (docs/scan_to_map.md): same bits, same speed.

Both libraries are loaded into one process and get the same bytes.  A GPU is required; the inputs are the ones of the test suite
(tests/mapping_util.py, tests/kf_util.py, tests/gn_cases.py), so the CPU oracle library has to be built too.

    python tools/scan_to_map_cost.py --parent-lib PATH [--this-lib PATH] [--steps 24] [--skip-bits] [--skip-speed] [--out FILE.json]

--this-lib PATH takes another build in this tree's place: with the other build and a byte copy of it under another name the speed lines
are an A/A run, whose gap between the two medians is what a gap between this tree and the other build is held against.

bits   every 32-bit word of the outputs compared as uint32 (a NaN equals a NaN of the same bits):
         lio_map_process over the sequences of test_mapping_sequence_matches_oracle (indoor 5, outdoor 3 sweeps) and of
         test_map_builder_matches_oracle (both enable_4d): T_aft, transform_tobe_mapped, iterations, num_selected, kz, the four clouds and the
         three arrays of score_point_coeff() after every sweep;
         lio_kf_batch_refine on the inputs of test_batch_matches_oracle_vlp16 (both modes) and test_batch_edge_cases;
         lio_gn_rows_map on every map case of gn_cases, all three forms.
speed  alternating, the order swapped every pair, 3 warm-up steps, equal bits asserted at every step, median (min - max):
         lio_map_process per sweep, indoor and outdoor, on the drifting sequence bench.py: mapping_ms_per_scan steps through (walked to and fro);
         device_ms of lio_kf_batch_refine at 4 VLP-16 keyframes (8 lanes per query) and at 64 HDL-64E keyframes (one lane per query).
       Criterion: this tree's median is not above the other build's slowest step of the same run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lio-mapping_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP = 3


def _words(*arrays):
    """the arguments as one uint32 vector (integers and bytes widened: equal values give equal words)"""
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        if a.dtype == np.float64:
            out.append(a.reshape(-1).view(np.uint32))
        elif a.dtype == np.float32:
            out.append(a.reshape(-1).view(np.uint32))
        else:
            out.append(a.reshape(-1).astype(np.int64).astype(np.uint32))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def _map_outputs(mp, r):
    from lio_amd import capi

    q, p = r["T_aft"]
    q2, p2 = mp.transform_tobe_mapped()
    clouds = [mp.cloud(w) for w in (capi.PointMapping.CORNER_STACK_DS, capi.PointMapping.SURF_STACK_DS, capi.PointMapping.CORNER_FROM_MAP,
                                    capi.PointMapping.SURF_FROM_MAP)]
    return _words(q, p, q2, p2, np.array([r["iterations"], r["num_selected"], r["kz"], r["degenerate"]]), *clouds, *mp.score_point_coeff())


def _refine_outputs(r):
    return _words(r["p"], r["q"], r["iterations"], r["rows"])


def _equal(name, a, b, table):
    same = a.shape == b.shape and bool(np.array_equal(a, b))
    table.append(dict(what=name, words=int(a.size), equal=same))
    print(json.dumps(table[-1]), flush=True)
    return same


def bits(hip, parent, oracle):
    from lio_amd import capi
    import gn_cases
    from kf_util import keyframe_inputs, load
    from mapping_util import drifting_inputs

    table = []
    runs = [("lio_map_process indoor 5", "indoor", 5, {}), ("lio_map_process outdoor 3", "outdoor", 3, {}),
            ("lio_map_process map_builder enable_4d=1", "indoor", 5, dict(map_builder=1, enable_4d=1, skip_count=2)),
            ("lio_map_process map_builder enable_4d=0", "indoor", 5, dict(map_builder=1, enable_4d=0, skip_count=2)),
            ("lio_map_process map_builder enable_4d=1 skip_count=1", "indoor", 4, dict(map_builder=1, enable_4d=1, skip_count=1))]
    for name, kind, n, kw in runs:
        frames = drifting_inputs(oracle, kind, n)
        a, b = capi.PointMapping(hip, **kw), capi.PointMapping(parent, **kw)
        wa, wb = [], []
        for corner, surf, T_sum, _ in frames:
            wa.append(_map_outputs(a, a.process(corner, surf, T_sum)))
            wb.append(_map_outputs(b, b.process(corner, surf, T_sum)))
        _equal(name, np.concatenate(wa), np.concatenate(wb), table)
    maps, kfs = keyframe_inputs(oracle, "indoor", 4, 4)
    for four_dof in (0, 1):
        ra, rb = [load(capi.KeyframeBatch(lib, map_builder=four_dof, enable_4d=four_dof), maps, kfs).refine() for lib in (hip, parent)]
        _equal(f"lio_kf_batch_refine vlp16 four_dof={four_dof}", _refine_outputs(ra), _refine_outputs(rb), table)
    maps, kfs = keyframe_inputs(oracle, "indoor", 2, 1)
    res = []
    for lib in (hip, parent):   # the batch of tests/test_gpu_kf_batch.py::test_batch_edge_cases
        b = capi.KeyframeBatch(lib)
        tiny, ok = b.add_map(maps[0][0][:10], maps[0][1][:100]), b.add_map(*maps[0])
        _, cs, ss, T0, _ = kfs[0]
        b.add_keyframe(tiny, cs, ss, T0)
        b.add_keyframe(ok, np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), T0)
        b.add_keyframe(ok, cs, ss, T0)
        b.add_keyframe(ok, cs[:3], ss[:20], T0)
        res.append(_refine_outputs(b.refine()))
    _equal("lio_kf_batch_refine edge cases", res[0], res[1], table)
    wa, wb = [], []
    for name, form in gn_cases.MAP_RUNS:
        c = gn_cases.get_map(name)
        wa.append(_words(*c.run(hip, form)))
        wb.append(_words(*c.run(parent, form)))
    _equal(f"lio_gn_rows_map {len(gn_cases.MAP_RUNS)} runs", np.concatenate(wa), np.concatenate(wb), table)
    return table


def _ms(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def _stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def _line(name, here, there, extra=None):
    row = dict(what=name, steps_measured=len(here), this_tree_ms=_stats(here), parent_ms=_stats(there),
               holds=bool(np.median(here) <= np.max(there)), **(extra or {}))
    print(json.dumps(row), flush=True)
    return row


def speed_map(hip, parent, kind, frames, steps):
    from lio_amd import capi

    a, b = capi.PointMapping(hip), capi.PointMapping(parent)
    n = len(frames)
    walk = list(range(n)) + list(range(n - 2, 0, -1))   # to and fro: every step is a real motion against a map that holds the place
    t_a, t_b, its = [], [], []
    for k in range(WARMUP + steps):
        corner, surf, T_sum, _ = frames[walk[k % len(walk)]]
        if k % 2:
            (ra, ta), (rb, tb) = _ms(lambda: a.process(corner, surf, T_sum)), _ms(lambda: b.process(corner, surf, T_sum))
        else:
            (rb, tb), (ra, ta) = _ms(lambda: b.process(corner, surf, T_sum)), _ms(lambda: a.process(corner, surf, T_sum))
        assert np.array_equal(_words(*ra["T_aft"], [ra["iterations"], ra["num_selected"]]), _words(*rb["T_aft"], [rb["iterations"], rb["num_selected"]]))
        if k >= WARMUP:
            t_a.append(ta), t_b.append(tb), its.append(ra["iterations"])
    return _line(f"lio_map_process {kind}", t_a, t_b, dict(iterations_median=int(np.median(its))))


def speed_refine(hip, parent, name, maps, kfs, steps):
    from lio_amd import capi
    from kf_util import load

    a, b = load(capi.KeyframeBatch(hip), maps, kfs), load(capi.KeyframeBatch(parent), maps, kfs)
    t_a, t_b = [], []
    for k in range(WARMUP + steps):
        ra, rb = (a.refine(), b.refine()) if k % 2 else (b.refine(), a.refine())[::-1]
        assert np.array_equal(_refine_outputs(ra), _refine_outputs(rb))
        if k >= WARMUP:
            t_a.append(ra["device_ms"]), t_b.append(rb["device_ms"])
    return _line(name, t_a, t_b, dict(keyframes=len(kfs), queries=int(sum(len(k[1]) + len(k[2]) for k in kfs))))


def speed(hip, parent, oracle, steps):
    from kf_util import keyframe_inputs
    from mapping_util import drifting_inputs

    rows = []
    for kind in ("indoor", "outdoor"):
        rows.append(speed_map(hip, parent, kind, drifting_inputs(oracle, kind, 6), steps))
    maps, kfs = keyframe_inputs(oracle, "indoor", 3, 2)
    rows.append(speed_refine(hip, parent, "lio_kf_batch_refine device_ms, 4 VLP-16 keyframes", maps, kfs, steps))
    maps, kfs = keyframe_inputs(oracle, "outdoor", 3, 32, dpos=0.15, drot=0.01)
    rows.append(speed_refine(hip, parent, "lio_kf_batch_refine device_ms, 64 HDL-64E keyframes", maps, kfs, steps))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--this-lib", default=None)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--skip-bits", action="store_true")
    ap.add_argument("--skip-speed", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 24, "at least 24 timed steps"
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi
    from odom_batch_cost import load_parent

    hip, parent = load_parent(args.this_lib) if args.this_lib else capi.load_hip(), load_parent(args.parent_lib)
    oracle = capi.LioLib(os.path.join(ROOT, "oracle", "liblio_oracle.so"))
    out = {}
    if not args.skip_bits:
        out["bits"] = bits(hip, parent, oracle)
    if not args.skip_speed:
        out["speed"] = speed(hip, parent, oracle, args.steps)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    assert all(r["equal"] for r in out.get("bits", [])), "bits differ from the other build"


if __name__ == "__main__":
    main()
