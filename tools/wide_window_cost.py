"""What the device trust-region loop buys for windows of seven optimised frames (indoor 12 / 7, docs/wide_window.md).

B copies of one 12 / 7 window (lio_est_copy_snapshot of a window that has run a few steps and holds a prior) in up to three batches:
  limit7   this tree, lio_est_set_device_solve_limit(h, 7) on every member: the device loop solves the B windows together
  limit6   this tree, the limit left at its default: every window is solved by the single-window path, one after the other
  parent   another build of the product (--parent-lib: the parent commit's liblio_hip.so), which has no such call
Per step every batch runs ONE lio_est_batch_solve_restored(1) (restore + solve), the batches alternating, the order rotated every step;
the call ends synchronised, so the host clock around it is what the caller pays.  Solves per second = B / median, with min - max over
the steps after the warm-up.  limit6 and parent must give the same bits (asserted at every step on windows 0, B / 2, B - 1) and limit7
must agree with them as the device and host loops do (1e-4 m).  A last pass times the limit7 batch's three kernels of an iteration
with events (lio_est_batch_set_option time_kernels): the step kernel's average time per launch at n_pad = 128.  Needs a GPU.

    python tools/wide_window_cost.py [--steps 16] [--batches 8,64] [--parent-lib PATH] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lio-mapping_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARMUP = 3   # the first steps grow the buffers and load the code objects
W, WO, DT = 12, 7, 0.2
EXTRA = 3    # steps the window runs before its snapshot (a prior exists, convergence_flag_ is set)


def _stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def _config(lib, ds):
    from lio_amd import pipeline

    cfg = pipeline.config_indoor(lib, W, WO)
    cfg.cutoff_deskew, cfg.keep_features, cfg.prior_factor = 1, 0, 1
    pipeline.set_extrinsic(cfg, ds)
    return cfg


def source_window(lib, ds, clouds):
    """a 12 / 7 window that has run EXTRA steps on the default path, one more frame pushed, snapshotted: the next solve is the one timed"""
    from lio_amd import capi, pipeline

    est = capi.Estimator(lib, _config(lib, ds))
    pipeline.init_window(est, lib, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01)
    est.solve()
    est.slide()
    for k in range(W + 1, W + 1 + EXTRA):
        pipeline.feed_frame(est, ds, k, clouds[k][0], clouds[k][1])
    k = W + 1 + EXTRA
    f = ds.frames[k]
    est.process_imu_batch(f.imu_dt, f.imu_acc, f.imu_gyr, f.imu_t)
    est.push_frame(capi.TransformF.make([0, 0, 0, 1], [0, 0, 0]), clouds[k][0], clouds[k][1], f.t)
    est.sync()
    est.snapshot()
    return est


class Arm:
    def __init__(self, name, lib, ds, src, B, limit):
        from lio_amd import capi

        self.name, self.lib, self.B = name, lib, B
        self.ests = []
        for _ in range(B):
            e = capi.Estimator(lib, _config(lib, ds))
            e.copy_snapshot_of(src)
            e.restore()
            if limit is not None:
                e.set_device_solve_limit(limit)
            self.ests.append(e)
        self.batch = capi.EstimatorBatch(lib, self.ests)
        self.reps = (capi.SolveReport * B)()
        self.t, self.n_device = [], []

    def step(self):
        t0 = time.perf_counter()
        if self.lib.dll.lio_est_batch_solve_restored(self.batch.h, 1, self.reps) != 0:
            raise RuntimeError(f"{self.name}: lio_est_batch_solve_restored failed")
        return (time.perf_counter() - t0) * 1e3

    def words(self, j):
        w = self.ests[j].get_window()
        r = self.reps[j]
        parts = [np.ascontiguousarray(w[k], np.float64).ravel().view(np.uint32) for k in ("Ps", "Rs", "Vs", "Bas", "Bgs")]
        parts.append(np.array([r.iterations, r.successful_steps, r.termination, r.n_lidar_residuals, r.n_local_map], np.uint32))
        parts.append(np.array([r.initial_cost, r.final_cost]).view(np.uint32))
        return np.concatenate(parts)


def measure(arms, B, steps):
    probe = sorted({0, B // 2, B - 1})
    for s in range(WARMUP + steps):
        order = arms[s % len(arms):] + arms[:s % len(arms)]
        for a in order:
            ms = a.step()
            if s >= WARMUP:
                a.t.append(ms)
                a.n_device.append(int(a.batch.clock()["n_device"]))
        by = {a.name: a for a in arms}
        if "parent" in by:
            for j in probe:
                assert np.array_equal(by["limit6"].words(j), by["parent"].words(j)), ("limit 6 differs from the parent build", B, s, j)
        for j in probe:
            dp = float(np.max(np.abs(by["limit7"].ests[j].get_window()["Ps"] - by["limit6"].ests[j].get_window()["Ps"])))
            assert dp < 1e-4, (B, s, j, dp)
            assert by["limit7"].reps[j].iterations == by["limit6"].reps[j].iterations
    out = dict(what="wide_window", W=W, Wo=WO, B=B, steps_measured=steps)
    for a in arms:
        med = float(np.median(a.t))
        out[a.name] = dict(ms=_stats(a.t), runs=[round(v, 4) for v in a.t], solves_per_s=round(B / med * 1e3, 1),
                           solves_per_s_range=[round(B / max(a.t) * 1e3, 1), round(B / min(a.t) * 1e3, 1)], n_device=sorted(set(a.n_device)))
    base = "parent" if any(a.name == "parent" for a in arms) else "limit6"
    by = {a.name: a for a in arms}
    out["baseline"] = base
    out["speedup_limit7"] = round(float(np.median(by[base].t)) / float(np.median(by["limit7"].t)), 3)
    out["limit7_beats_baseline_beyond_spread"] = bool(np.max(by["limit7"].t) < np.min(by[base].t))
    if base == "parent":
        out["limit6_vs_parent"] = round(float(np.median(by["limit6"].t)) / float(np.median(by["parent"].t)), 3)
    # the kernels of an iteration, bracketed by events (a measurement run of its own: the events serialise the loop groups' launches)
    a = by["limit7"]
    a.batch.set_option("time_kernels", 1)
    acc = dict(aux_ms=0.0, moments_ms=0.0, step_ms=0.0, step_launches=0.0)
    for _ in range(4):
        a.step()
        clk = a.batch.clock()
        for k in acc:
            acc[k] += clk[k]
    a.batch.set_option("time_kernels", 0)
    out["limit7_kernels"] = dict(step_us_per_launch=round(acc["step_ms"] / max(acc["step_launches"], 1) * 1e3, 2), step_launches_per_solve=acc["step_launches"] / 4,
                                 aux_ms_per_solve=round(acc["aux_ms"] / 4, 4), moments_ms_per_solve=round(acc["moments_ms"] / 4, 4),
                                 step_ms_per_solve=round(acc["step_ms"] / 4, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 8, "medians over at least 8 steps"
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi, pipeline, synth

    hip = capi.load_hip()
    parent = None
    if args.parent_lib:
        from odom_batch_cost import load_parent

        parent = load_parent(args.parent_lib)
    ds = synth.make_dataset("indoor", W + 2 + EXTRA, DT)
    clouds = [pipeline.feature_clouds(hip, ds.lidar, f.scan) for f in ds.frames]
    src = source_window(hip, ds, clouds)
    src_parent = source_window(parent, ds, clouds) if parent else None
    results = []
    for B in [int(b) for b in args.batches.split(",") if b]:
        arms = [Arm("limit7", hip, ds, src, B, 7), Arm("limit6", hip, ds, src, B, None)]
        if parent:
            arms.append(Arm("parent", parent, ds, src_parent, B, None))
        results.append(measure(arms, B, args.steps))
        print(json.dumps(results[-1]), flush=True)
        for a in arms:
            a.batch.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
