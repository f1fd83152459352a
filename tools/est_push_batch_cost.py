"""What lio_est_batch_push_frames / _slide_windows / _process_laser_odom buy over the per-handle calls around a batched solve
(docs/est_push_batch.md).

B copies of one window (lio_est_copy_snapshot of a window that has run a few steps and stands right behind a slide) in two batches.  Per step
every window is restored and given the IMU samples of the next frame (untimed: the IMU side is per handle on both routes); then
  host    B x lio_est_push_frame, lio_est_batch_solve, B x lio_est_slide_window — straight calls of the compiled library with arguments
          built beforehand, in one loop
  device  ONE lio_est_batch_process_laser_odom
alternate, the order swapped every step.  Both end synchronised, so the host clock around them is what the caller pays.  Equal bits (the
pushed stack, the stack behind the slide, the window, the report of windows 0, B / 2 and B - 1) are asserted at every step.  The same again
without the solve (push + slide alone).  Medians with min - max over the steps after the warm-up.  Needs a GPU.

    python tools/est_push_batch_cost.py [--steps 16] [--batches 1,8,64,512] [--kinds indoor,outdoor] [--out FILE.json]

Criteria (orderings against the host route of the same run): at B = 64 and 512 the new call's median is below the host route's fastest step;
at B = 1 it is not above the host route's slowest step.
--parent-lib PATH times B x lio_est_push_frame + B x lio_est_slide_window ALONE, this tree against another build of the product (the parent
commit's liblio_hip.so), in one process: this tree's median not above the other build's slowest step.  Where that build has the batched calls
too, they are timed the same way (push + slide alone, and the composite), every run listed.
--only-device runs the new call alone (a kernel trace of it without the host route's launches in it).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lio-mapping_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARMUP = 3   # the first steps grow the buffers and load the code objects
WINDOWS = {"indoor": (10, 6, 0.2), "outdoor": (15, 5, 0.3)}   # W, Wo, frame spacing: the largest window the device loop takes; the headline
EXTRA = 3    # steps the window runs before its snapshot (a prior exists, the local map has been built)


def _stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def _config(lib, ds, kind, W, Wo):
    from lio_amd import pipeline

    cfg = pipeline.config_outdoor64(lib, W, Wo) if kind == "outdoor" else pipeline.config_indoor(lib, W, Wo)
    if kind != "outdoor":
        cfg.cutoff_deskew, cfg.keep_features, cfg.prior_factor = 1, 0, 1
    pipeline.set_extrinsic(cfg, ds)
    return cfg


def source_window(lib, ds, clouds, kind, W, Wo):
    """a window that has run EXTRA steps, right behind a slide, snapshotted; the next frame is ds.frames[W + 1 + EXTRA]"""
    from lio_amd import capi, pipeline

    est = capi.Estimator(lib, _config(lib, ds, kind, W, Wo))
    pipeline.init_window(est, lib, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01)
    est.solve()
    est.slide()
    for k in range(W + 1, W + 1 + EXTRA):
        pipeline.feed_frame(est, ds, k, clouds[k][0], clouds[k][1])
    est.sync()
    est.snapshot()
    return est


def clones(lib, ds, kind, W, Wo, src, B):
    from lio_amd import capi

    out = []
    for _ in range(B):
        e = capi.Estimator(lib, _config(lib, ds, kind, W, Wo))
        e.copy_snapshot_of(src)
        e.restore()
        out.append(e)
    return out


class Stepper:
    """a set of B windows and the prepared arguments of the per-handle calls"""

    def __init__(self, lib, ests, frame, surf, corner, batch=True):
        from lio_amd import capi

        self.lib, self.ests, self.f = lib, ests, frame
        self.batch = capi.EstimatorBatch(lib, ests) if batch else None
        self.surf, self.corner = np.ascontiguousarray(surf, np.float32), np.ascontiguousarray(corner, np.float32)
        self.T = capi.TransformF.make([0, 0, 0, 1], [0, 0, 0])
        self.items = [(self.T, self.surf, self.corner, frame.t)] * len(ests)
        self.frames, self._keep = capi.EstimatorBatch.frames(self.items)
        self.reps = (capi.SolveReport * len(ests))()
        self.handles = [e.h for e in ests]
        self.sp, self.cp = self.surf.ctypes.data_as(capi.c_float_p), self.corner.ctypes.data_as(capi.c_float_p)

    def prepare(self):
        f = self.f
        for e in self.ests:
            e.restore()
            e.process_imu_batch(f.imu_dt, f.imu_acc, f.imu_gyr, f.imu_t)

    def per_handle(self, solve):
        dll, Tr, sp, ns, cp, nc, t = self.lib.dll, C.byref(self.T), self.sp, self.surf.shape[0], self.cp, self.corner.shape[0], self.f.t
        push, slide = dll.lio_est_push_frame, dll.lio_est_slide_window
        t0 = time.perf_counter()
        for h in self.handles:
            if push(h, Tr, sp, ns, cp, nc, t) != 0:
                raise RuntimeError("lio_est_push_frame failed")
        if solve and dll.lio_est_batch_solve(self.batch.h, self.reps) != 0:
            raise RuntimeError("lio_est_batch_solve failed")
        for h in self.handles:
            if slide(h) != 0:
                raise RuntimeError("lio_est_slide_window failed")
        if not solve:
            self.ests[-1].get_surf_stack(0)   # the per-handle slide does not wait: one small read-back ends the step synchronised, as the new call's push does
        return (time.perf_counter() - t0) * 1e3

    def batched(self, solve):
        dll = self.lib.dll
        t0 = time.perf_counter()
        if solve:
            if dll.lio_est_batch_process_laser_odom(self.batch.h, self.frames, self.reps) != 0:
                raise RuntimeError("lio_est_batch_process_laser_odom failed")
        else:
            if dll.lio_est_batch_push_frames(self.batch.h, self.frames) != 0 or dll.lio_est_batch_slide_windows(self.batch.h) != 0:
                raise RuntimeError("lio_est_batch_push_frames / _slide_windows failed")
            self.ests[-1].get_surf_stack(0)
        return (time.perf_counter() - t0) * 1e3

    def words(self, j, solve):
        e = self.ests[j]
        W = e.W
        parts = [e.get_surf_stack(W).ravel().view(np.uint32), e.get_surf_stack(W - e.cfg.opt_window_size + 1).ravel().view(np.uint32)]
        w = e.get_window()
        parts += [np.ascontiguousarray(w[k], np.float64).ravel().view(np.uint32) for k in ("Ps", "Rs", "Vs", "Bas", "Bgs")]
        if solve:
            r = self.reps[j]
            parts.append(np.array([r.iterations, r.successful_steps, r.termination, r.n_lidar_residuals, r.n_local_map], np.uint32))
            parts.append(np.array([r.initial_cost, r.final_cost]).view(np.uint32))
        return np.concatenate(parts)


def measure(hip, kind, ds, clouds, src, B, steps, only_device=False):
    W, Wo, _ = WINDOWS[kind]
    k = W + 1 + EXTRA
    host = None if only_device else Stepper(hip, clones(hip, ds, kind, W, Wo, src, B), ds.frames[k], clouds[k][0], clouds[k][1])
    dev = Stepper(hip, clones(hip, ds, kind, W, Wo, src, B), ds.frames[k], clouds[k][0], clouds[k][1])
    out = dict(what="device_only" if only_device else "host_vs_device", kind=kind, W=W, Wo=Wo, B=B, steps_measured=steps, n_surf=int(len(clouds[k][0])))
    for solve in (True, False):
        t_host, t_dev = [], []
        for s in range(WARMUP + steps):
            dev.prepare()
            if only_device:
                b = dev.batched(solve)
            else:
                host.prepare()
                if s % 2:
                    a, b = host.per_handle(solve), dev.batched(solve)
                else:
                    b, a = dev.batched(solve), host.per_handle(solve)
                for j in sorted({0, B // 2, B - 1}):   # the calls' contract at the size that is timed (every getter: tests/test_gpu_est_push_batch.py)
                    assert np.array_equal(host.words(j, solve), dev.words(j, solve)), (kind, B, s, j, solve)
            if s >= WARMUP:
                t_dev.append(b)
                if not only_device:
                    t_host.append(a)
        key = "step" if solve else "push_slide"
        out[key] = dict(device_ms=_stats(t_dev), device_per_window_us=round(float(np.median(t_dev)) / B * 1e3, 2))
        if not only_device:
            med_h, med_d = float(np.median(t_host)), float(np.median(t_dev))
            out[key].update(host_ms=_stats(t_host), host_per_window_us=round(med_h / B * 1e3, 2), ratio=round(med_h / med_d, 3),
                            holds=bool(med_d <= np.max(t_host)) if B == 1 else bool(med_d < np.min(t_host)))
    out["push_stats"] = dev.batch.push_stats()
    for st in (host, dev):
        if st is not None:
            st.batch.close()
    return out


def measure_parent(hip, parent, kind, ds, clouds, B, steps):
    """B x lio_est_push_frame + B x lio_est_slide_window alone: this tree against another build, alternating in one process"""
    W, Wo, _ = WINDOWS[kind]
    k = W + 1 + EXTRA
    sets = []
    for lib in (hip, parent):
        src = source_window(lib, ds, clouds, kind, W, Wo)
        sets.append(Stepper(lib, clones(lib, ds, kind, W, Wo, src, B), ds.frames[k], clouds[k][0], clouds[k][1], batch=False))
    mine, theirs = sets
    t_mine, t_theirs = [], []
    for s in range(WARMUP + steps):
        mine.prepare(), theirs.prepare()
        if s % 2:
            a, b = mine.per_handle(False), theirs.per_handle(False)
        else:
            b, a = theirs.per_handle(False), mine.per_handle(False)
        for j in sorted({0, B - 1}):
            assert np.array_equal(mine.words(j, False), theirs.words(j, False)), (kind, B, s, j)
        if s >= WARMUP:
            t_mine.append(a), t_theirs.append(b)
    return dict(what="per_handle_calls_vs_parent_build", kind=kind, B=B, steps_measured=steps, this_ms=_stats(t_mine), parent_ms=_stats(t_theirs),
                holds=bool(np.median(t_mine) <= np.max(t_theirs)))


def measure_parent_batched(hip, parent, kind, ds, clouds, B, steps):
    """the batched calls themselves — lio_est_batch_push_frames + _slide_windows alone, and lio_est_batch_process_laser_odom — this tree against
    another build that has them, alternating in one process; equal bits asserted at every step"""
    W, Wo, _ = WINDOWS[kind]
    k = W + 1 + EXTRA
    sets = []
    for lib in (hip, parent):
        src = source_window(lib, ds, clouds, kind, W, Wo)
        sets.append(Stepper(lib, clones(lib, ds, kind, W, Wo, src, B), ds.frames[k], clouds[k][0], clouds[k][1]))
    mine, theirs = sets
    out = dict(what="batched_calls_vs_parent_build", kind=kind, B=B, steps_measured=steps)
    for solve in (True, False):
        t_mine, t_theirs = [], []
        for s in range(WARMUP + steps):
            mine.prepare(), theirs.prepare()
            if s % 2:
                a, b = mine.batched(solve), theirs.batched(solve)
            else:
                b, a = theirs.batched(solve), mine.batched(solve)
            for j in sorted({0, B // 2, B - 1}):
                assert np.array_equal(mine.words(j, solve), theirs.words(j, solve)), (kind, B, s, j, solve)
            if s >= WARMUP:
                t_mine.append(a), t_theirs.append(b)
        out["step" if solve else "push_slide"] = dict(this_ms=_stats(t_mine), parent_ms=_stats(t_theirs), this_runs=[round(v, 4) for v in t_mine],
                                                      parent_runs=[round(v, 4) for v in t_theirs], holds=bool(np.median(t_mine) <= np.max(t_theirs)))
    out["push_stats"] = mine.batch.push_stats()
    for st in sets:
        st.batch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--batches", default="1,8,64,512")
    ap.add_argument("--kinds", default="indoor,outdoor")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-batches", default="1,64")
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 16, "medians over at least 16 steps"
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi, pipeline, synth

    hip = capi.load_hip()
    results = []
    for kind in args.kinds.split(","):
        W, Wo, dt = WINDOWS[kind]
        ds = synth.make_dataset(kind, W + 2 + EXTRA, dt)
        clouds = [pipeline.feature_clouds(hip, ds.lidar, f.scan) for f in ds.frames]
        src = source_window(hip, ds, clouds, kind, W, Wo)
        for B in [int(b) for b in args.batches.split(",") if b]:
            results.append(measure(hip, kind, ds, clouds, src, B, args.steps, args.only_device))
            print(json.dumps(results[-1]), flush=True)
        if args.parent_lib:
            from odom_batch_cost import load_parent

            parent = load_parent(args.parent_lib)
            for B in [int(b) for b in args.parent_batches.split(",") if b]:
                results.append(measure_parent(hip, parent, kind, ds, clouds, B, args.steps))
                print(json.dumps(results[-1]), flush=True)
                if hasattr(parent.dll, "lio_est_batch_push_frames"):
                    results.append(measure_parent_batched(hip, parent, kind, ds, clouds, B, args.steps))
                    print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
