"""What lio_est_batch_process_compact_from_odom buys over the host route between the odometry and the estimator's windows
(docs/est_from_odom.md).

B copies of one initialised window (tools/est_push_batch_cost.py: source_window / clones) in two batches, and B sensors — a PointProcessor
and a PointOdometry each, the odometry in packer mode (lio_odom_enable(h, 0): the clouds are kept as they come).  The front end of a step
runs once and is not timed: lio_pp_process_batch on the next frame's sweep, then lio_odom_process_batch_from_pp.  Every window is restored
and given the frame's IMU samples (untimed), then twin sets of windows take the step, alternating with the order swapped every step:
  host    the route include/lio_est_from_odom.h states as the contract, straight calls of the compiled library into buffers made beforehand:
          per window lio_odom_get_last_cloud twice and, with the full cloud on, lio_pp_get_cloud(RINGS), lio_odom_full_to_end and
          lio_map_set_full_cloud; then ONE lio_est_batch_process_laser_odom with host pointers (the batched solve on both sides: the
          per-handle lio_est_process_compact would add B single-window solves to the host route's side)
  device  ONE lio_est_batch_process_compact_from_odom
Both end synchronised, so the host clock around them is what the caller pays.  Equal bits (the pushed stack, the stack behind the slide, the
window, the report and, with the full cloud on, the newest full-ring entry, of windows 0, B / 2 and B - 1) are asserted at every step.
Medians with min - max over the steps after the warm-up, and the bytes of cloud data that cross PCIe per window and step on each route,
computed from the counts.  Needs a GPU.

    python tools/est_from_odom_cost.py [--steps 16] [--batches 1,8,64] [--kinds indoor,outdoor] [--full 1,0] [--out FILE.json]

Criteria (orderings): at B = 8 and 64 the new call's median is below the host route's fastest step; at B = 1 it is not above the host
route's slowest step.
--parent-lib PATH times the host-fed lio_est_batch_process_laser_odom (and push + slide alone) of this tree against another build of the
product (the parent commit's liblio_hip.so) in one process (tools/est_push_batch_cost.py: measure_parent_batched): this tree's median not
above the other build's slowest step.
--only-device runs the new call alone (a kernel trace of it without the host route's launches and copies in it).
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

from est_push_batch_cost import EXTRA, WARMUP, WINDOWS, _stats, clones, measure_parent_batched, source_window   # noqa: E402

RINGS = 0
POINT = 16   # bytes of one xyzi point


class Fleet:
    """B windows in a batch, and the buffers and arguments of both routes made beforehand"""

    def __init__(self, lib, ests, frame, full, cap):
        from lio_amd import capi

        self.lib, self.ests, self.f, self.full = lib, ests, frame, full
        B = len(ests)
        for e in ests:
            e.set_full_cloud(full)
        self.maps = [e.map() for e in ests]                      # (created before the first step on both sides)
        self.batch = capi.EstimatorBatch(lib, ests)
        self.reps = (capi.SolveReport * B)()
        self.T = (capi.TransformF * B)()
        self.stamps = (C.c_double * B)(*([frame.t] * B))
        self.frames = (capi.EstFrame * B)()
        self.buf = [[np.zeros((cap, 4), np.float32) for _ in range(4)] for _ in range(B)]   # corner, surf, ring cloud, full cloud at the sweep's end
        self.ptr = [[b.ctypes.data_as(capi.c_float_p) for b in four] for four in self.buf]
        ident = capi.TransformF.make([0, 0, 0, 1], [0, 0, 0])    # transform_aft_mapped_ of a map that has not stepped: what the composite hands on
        for w in range(B):
            self.frames[w].transform_in = ident
            self.frames[w].stamp = frame.t
            self.frames[w].corner_xyzi, self.frames[w].surf_xyzi = self.ptr[w][0], self.ptr[w][1]

    def prepare(self):
        f = self.f
        for e in self.ests:
            e.restore()
            e.process_imu_batch(f.imu_dt, f.imu_acc, f.imu_gyr, f.imu_t)

    def host(self, ods, pps):
        dll, fr = self.lib.dll, self.frames
        t0 = time.perf_counter()
        for w, (od, pp) in enumerate(zip(ods, pps)):
            p = self.ptr[w]
            fr[w].n_corner = dll.lio_odom_get_last_cloud(od.h, 0, p[0])
            fr[w].n_surf = dll.lio_odom_get_last_cloud(od.h, 1, p[1])
            if self.full:
                n = dll.lio_pp_count(pp.h, RINGS)
                if dll.lio_pp_get_cloud(pp.h, RINGS, p[2]) < 0 or dll.lio_odom_full_to_end(od.h, p[2], n, p[3]) != 0 \
                        or dll.lio_map_set_full_cloud(self.maps[w].h, p[3], n) != 0:
                    raise RuntimeError("the full cloud's host route failed")
        if dll.lio_est_batch_process_laser_odom(self.batch.h, fr, self.reps) != 0:
            raise RuntimeError("lio_est_batch_process_laser_odom failed")
        return (time.perf_counter() - t0) * 1e3

    def device(self, O, P):
        t0 = time.perf_counter()
        if self.lib.dll.lio_est_batch_process_compact_from_odom(self.batch.h, O, P, self.stamps, self.T, self.reps) != 0:
            raise RuntimeError("lio_est_batch_process_compact_from_odom failed")
        return (time.perf_counter() - t0) * 1e3

    def words(self, j):
        e = self.ests[j]
        W = e.W
        parts = [e.get_surf_stack(W).ravel().view(np.uint32), e.get_surf_stack(W - e.cfg.opt_window_size + 1).ravel().view(np.uint32)]
        w = e.get_window()
        parts += [np.ascontiguousarray(w[k], np.float64).ravel().view(np.uint32) for k in ("Ps", "Rs", "Vs", "Bas", "Bgs")]
        r = self.reps[j]
        parts.append(np.array([r.iterations, r.successful_steps, r.termination, r.n_lidar_residuals, r.n_local_map], np.uint32))
        parts.append(np.array([r.initial_cost, r.final_cost]).view(np.uint32))
        if self.full:
            parts.append(e.full_stack(W)[0].ravel().view(np.uint32))
            parts.append(self.maps[j].full_cloud().ravel().view(np.uint32))
        return np.concatenate(parts)


def measure(hip, kind, ds, clouds, src, B, steps, full, only_device=False):
    from lio_amd import capi

    W, Wo, _ = WINDOWS[kind]
    k = W + 1 + EXTRA
    frame, lid = ds.frames[k], ds.lidar
    scan = np.ascontiguousarray(frame.scan, np.float32)
    pps = [capi.PointProcessor(hip, lid.lower_deg, lid.upper_deg, lid.rings) for _ in range(B)]
    ods = [capi.PointOdometry(hip) for _ in range(B)]
    for od in ods:
        od.enable(False)                                         # packer mode
    O = (C.c_void_p * B)(*[o.h for o in ods])
    P = (C.c_void_p * B)(*[p.h for p in pps]) if full else None
    host = None if only_device else Fleet(hip, clones(hip, ds, kind, W, Wo, src, B), frame, full, len(scan))
    dev = Fleet(hip, clones(hip, ds, kind, W, Wo, src, B), frame, full, len(scan))
    t_host, t_dev = [], []
    for s in range(WARMUP + steps):
        if B > 1:
            capi.PointProcessor.process_batch(pps, [scan] * B)
        else:
            pps[0].process(scan)
        capi.PointOdometry.process_batch_from_pp(ods, pps)
        dev.prepare()
        if only_device:
            b = dev.device(O, P)
        else:
            host.prepare()
            if s % 2:
                a, b = host.host(ods, pps), dev.device(O, P)
            else:
                b, a = dev.device(O, P), host.host(ods, pps)
            for j in sorted({0, B // 2, B - 1}):   # the call's contract at the size that is timed (every getter: tests/test_gpu_est_from_odom.py)
                assert np.array_equal(host.words(j), dev.words(j)), (kind, B, s, j, full)
        if s >= WARMUP:
            t_dev.append(b)
            if not only_device:
                t_host.append(a)
    nc, ns = len(ods[0].last_cloud(0)), len(ods[0].last_cloud(1))
    nf = len(pps[0].cloud(RINGS)) if full else 0
    refresh = 0   # (the map refresh is off in these windows: the corner sweep crosses once, down)
    # down: both clouds, and with the full cloud the ring cloud and lio_odom_full_to_end's result; up: the surf sweep (the corner one only with the
    # refresh on), lio_odom_full_to_end's input and the full cloud
    host_bytes = (nc + ns + 2 * nf) * POINT + (ns + refresh * nc + 2 * nf) * POINT
    out = dict(what="device_only" if only_device else "host_vs_device", kind=kind, W=W, Wo=Wo, B=B, full_cloud=bool(full), steps_measured=steps,
               counts=dict(n_corner=nc, n_surf=ns, n_full=nf), device_ms=_stats(t_dev), device_per_window_us=round(float(np.median(t_dev)) / B * 1e3, 2),
               push_stats=dev.batch.push_stats(), from_odom_stats=dev.batch.from_odom_stats())
    if not only_device:
        med_h, med_d = float(np.median(t_host)), float(np.median(t_dev))
        out.update(host_ms=_stats(t_host), host_per_window_us=round(med_h / B * 1e3, 2), ratio=round(med_h / med_d, 3),
                   pcie_bytes_per_window_step=dict(host=host_bytes, device=0),
                   holds=bool(med_d <= np.max(t_host)) if B == 1 else bool(med_d < np.min(t_host)))
    for st in (host, dev):
        if st is not None:
            st.batch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--kinds", default="indoor,outdoor")
    ap.add_argument("--full", default="1,0")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-batches", default="1,8,64")
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 16, "medians over at least 16 steps"
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi, pipeline, synth

    hip = capi.load_hip()
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)

    for kind in args.kinds.split(","):
        W, Wo, dt = WINDOWS[kind]
        ds = synth.make_dataset(kind, W + 2 + EXTRA, dt)
        clouds = [pipeline.feature_clouds(hip, ds.lidar, f.scan) for f in ds.frames]
        src = source_window(hip, ds, clouds, kind, W, Wo)
        for full in [int(v) for v in args.full.split(",") if v]:
            for B in [int(b) for b in args.batches.split(",") if b]:
                emit(measure(hip, kind, ds, clouds, src, B, args.steps, full, args.only_device))
        if args.parent_lib:
            from odom_batch_cost import load_parent

            parent = load_parent(args.parent_lib)
            for B in [int(b) for b in args.parent_batches.split(",") if b]:
                emit(measure_parent_batched(hip, parent, kind, ds, clouds, B, args.steps))


if __name__ == "__main__":
    main()
