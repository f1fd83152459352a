"""What lio_map_process_batch buys over a loop of lio_map_process (docs/map_batch.md).

B copies of one sensor step through the same sweeps twice: one set of handles by a loop of lio_map_process, one set by ONE
lio_map_process_batch, alternating step by step with the order swapped every step.  The sweeps are the drifting sequences
bench.py: mapping_ms_per_scan steps through (tests/mapping_util.py: indoor VLP-16, outdoor HDL-64E), walked to and fro, so every step is a
real motion against a map that holds the place.  Both calls end synchronised, so the host clock around them is the latency the caller pays.
Equal bits (pose, iterations, selected rows, the four clouds, the score list) are asserted at every timed step.  Medians with min - max
over the steps after the warm-up; a GPU is required, and the CPU oracle library (it extracts the features).

    python tools/map_batch_cost.py [--steps 12] [--batches 1,8,64] [--kinds indoor,outdoor] [--out FILE.json]

--parent-lib PATH additionally times this tree against another build of the product (the parent commit's liblio_hip.so) in the same
process, alternating, the order swapped every pair, equal bits asserted at every step: lio_map_process ALONE (24 steps), the same with a
full cloud of FULL_POINTS points set before every step (the registration the call waits for; the set itself is not timed), and
lio_map_process_batch at the sizes of --parent-batches.  Criterion (docs/scan_to_map.md): this tree's median is not above the other
build's slowest step.
--this-lib PATH takes another build in this tree's place: with the parent's library and a byte copy of it under another name the same
lines are an A/A run, whose gap between the two medians is what a gap between this tree and the parent is held against.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARMUP = 3   # the first steps grow the buffers and load the code objects
N_FRAMES = 6
FULL_POINTS = 2049   # the full clouds of tests/test_gpu_full_cloud_estimator.py


def _ms(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def _stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def _walk(n):
    return list(range(n)) + list(range(n - 2, 0, -1))   # to and fro


def _words(m, r):
    """what a handle answers after a step, as one uint32 vector"""
    parts = [np.asarray(x, np.float32).ravel() for x in (*r["T_aft"], *m.transform_tobe_mapped())]
    parts += [m.cloud(w).ravel() for w in range(4)] + [a.ravel() for a in m.score_point_coeff()]
    ints = np.array([r["iterations"], r["num_selected"], r["kz"], r["degenerate"]], np.uint32)
    return np.concatenate([np.concatenate(parts).view(np.uint32), ints])


def measure_batch(hip, kind, frames, B, steps):
    from lio_amd import capi

    loop, batch = [capi.PointMapping(hip) for _ in range(B)], [capi.PointMapping(hip) for _ in range(B)]
    walk = _walk(len(frames))
    t_loop, t_batch, its = [], [], []
    for k in range(WARMUP + steps):
        corner, surf, T_sum, _ = frames[walk[k % len(walk)]]
        inp = (corner, surf, T_sum)

        def run_loop():
            return [m.process(*inp) for m in loop]

        def run_batch():
            return capi.PointMapping.process_batch(batch, [inp] * B)

        if k % 2:
            (ra, a), (rb, b) = _ms(run_loop), _ms(run_batch)
        else:
            (rb, b), (ra, a) = _ms(run_batch), _ms(run_loop)
        for j in sorted({0, B // 2, B - 1}):   # the batch's contract, at the size that is timed (every getter of every handle: tests/test_gpu_map_batch.py)
            assert np.array_equal(_words(loop[j], ra[j]), _words(batch[j], rb[j])), (kind, B, k, j)
        for x, y in zip(ra, rb):
            assert x["iterations"] == y["iterations"] and x["num_selected"] == y["num_selected"]
            assert all(np.array_equal(np.asarray(p, np.float32).view(np.uint32), np.asarray(q, np.float32).view(np.uint32)) for p, q in zip(x["T_aft"], y["T_aft"]))
        if k >= WARMUP:
            t_loop.append(a), t_batch.append(b), its.append(ra[0]["iterations"])
    med_l, med_b = float(np.median(t_loop)), float(np.median(t_batch))
    return dict(what="batch", kind=kind, B=B, steps_measured=steps, queries=int(len(loop[0].cloud(0)) + len(loop[0].cloud(1))),
                iterations_median=int(np.median(its)), loop_ms=_stats(t_loop), batch_ms=_stats(t_batch), loop_per_sensor_us=round(med_l / B * 1e3, 2),
                batch_per_sensor_us=round(med_b / B * 1e3, 2), ratio=round(med_l / med_b, 3),
                holds=bool(med_b <= np.max(t_loop)) if B == 1 else bool(med_b < np.min(t_loop)))


def measure_parent(hip, parent, kind, frames, steps, full_points=0):
    from lio_amd import capi

    here, there = capi.PointMapping(hip), capi.PointMapping(parent)
    walk = _walk(len(frames))
    t_here, t_there, its = [], [], []
    rng = np.random.default_rng(7)
    for k in range(WARMUP + steps):
        corner, surf, T_sum, _ = frames[walk[k % len(walk)]]
        if full_points:
            full = np.zeros((full_points, 4), np.float32)
            full[:, :3] = rng.uniform(-8, 8, (full_points, 3))
            here.set_full_cloud(full), there.set_full_cloud(full)
        if k % 2:
            (ra, a), (rb, b) = _ms(lambda: here.process(corner, surf, T_sum)), _ms(lambda: there.process(corner, surf, T_sum))
        else:
            (rb, b), (ra, a) = _ms(lambda: there.process(corner, surf, T_sum)), _ms(lambda: here.process(corner, surf, T_sum))
        assert np.array_equal(_words(here, ra), _words(there, rb)), (kind, k)   # same results as the parent
        if full_points:
            assert here.full_cloud().tobytes() == there.full_cloud().tobytes(), (kind, k)
        if k >= WARMUP:
            t_here.append(a), t_there.append(b), its.append(ra["iterations"])
    return dict(what="single_vs_parent", kind=kind, full_points=full_points, steps_measured=steps, iterations_median=int(np.median(its)),
                this_tree_ms=_stats(t_here), parent_ms=_stats(t_there), holds=bool(np.median(t_here) <= np.max(t_there)))


def measure_batch_parent(hip, parent, kind, frames, B, steps):
    """one lio_map_process_batch of B copies in this tree against the same call of the other build"""
    from lio_amd import capi

    here, there = [capi.PointMapping(hip) for _ in range(B)], [capi.PointMapping(parent) for _ in range(B)]
    walk = _walk(len(frames))
    t_here, t_there, its = [], [], []
    for k in range(WARMUP + steps):
        corner, surf, T_sum, _ = frames[walk[k % len(walk)]]
        inputs = [(corner, surf, T_sum)] * B
        if k % 2:
            (ra, a), (rb, b) = _ms(lambda: capi.PointMapping.process_batch(here, inputs)), _ms(lambda: capi.PointMapping.process_batch(there, inputs))
        else:
            (rb, b), (ra, a) = _ms(lambda: capi.PointMapping.process_batch(there, inputs)), _ms(lambda: capi.PointMapping.process_batch(here, inputs))
        for j in sorted({0, B // 2, B - 1}):
            assert np.array_equal(_words(here[j], ra[j]), _words(there[j], rb[j])), (kind, B, k, j)
        if k >= WARMUP:
            t_here.append(a), t_there.append(b), its.append(ra[0]["iterations"])
    return dict(what="batch_vs_parent", kind=kind, B=B, steps_measured=steps, iterations_median=int(np.median(its)), this_tree_ms=_stats(t_here),
                parent_ms=_stats(t_there), holds=bool(np.median(t_here) <= np.max(t_there)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--kinds", default="indoor,outdoor")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-batches", default="8,64")
    ap.add_argument("--this-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 8, "medians over at least 8 steps"
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi
    from mapping_util import drifting_inputs
    from odom_batch_cost import load_parent

    hip = load_parent(args.this_lib) if args.this_lib else capi.load_hip()
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    oracle = capi.LioLib(os.path.join(ROOT, "oracle", "liblio_oracle.so"))
    results = []
    for kind in args.kinds.split(","):
        frames = drifting_inputs(oracle, kind, N_FRAMES)
        for B in [int(b) for b in args.batches.split(",") if b]:
            results.append(measure_batch(hip, kind, frames, B, args.steps))
            print(json.dumps(results[-1]), flush=True)
        if parent is not None:
            for full_points in (0, FULL_POINTS):
                results.append(measure_parent(hip, parent, kind, frames, max(args.steps, 24), full_points))
                print(json.dumps(results[-1]), flush=True)
            for B in [int(b) for b in args.parent_batches.split(",") if b]:
                results.append(measure_batch_parent(hip, parent, kind, frames, B, args.steps))
                print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
