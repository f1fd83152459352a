"""What lio_map_process_batch_from_odom buys over the host route between the odometry and the scan-to-map step (docs/map_from_odom.md).

B sensors (a PointProcessor and a PointOdometry each) step through the same raw sweeps: synth.make_sweeps of the indoor VLP-16 and the
outdoor HDL-64E world, the worlds of tools/map_batch_cost.py, walked to and fro.  The front end of a step runs once and is not timed:
lio_pp_process_batch, then lio_odom_process_batch_from_pp.  Twin sets of map handles then take the step, alternating with the order swapped
every step:
  host   the route include/lio_map_from_odom.h states as the contract, full cloud on: per sensor lio_odom_get_last_cloud twice,
         lio_pp_get_cloud(RINGS), lio_odom_full_to_end and lio_map_set_full_cloud, then ONE lio_map_process_batch
  device ONE lio_map_process_batch_from_odom
Both end synchronised, so the host clock around them is the latency the caller pays.  Equal bits (pose, iterations, selected rows, the four
clouds, the score list, the full cloud) are asserted at every step.  Medians with min - max over the steps after the warm-up, and the
bytes of cloud data copied over PCIe per sensor and step on each route, computed from the counts.  Needs a GPU.

    python tools/map_from_odom_cost.py [--steps 16] [--batches 1,8,64] [--kinds indoor,outdoor] [--out FILE.json]

Criteria (orderings, as in docs/map_batch.md): at B >= 8 the device route's median is below the host route's fastest step; at B = 1 it is not
above the host route's slowest step.
--parent-lib PATH additionally times lio_map_process_batch ALONE, host-fed, of this tree against another build of the product (the parent
commit's liblio_hip.so) through tools/map_batch_cost.py: measure_batch_parent — equal bits at every step, this tree's median not above
the other build's slowest step.
--only-device runs the device route alone (a kernel trace of the call without the host route's copies in it).
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
N_SWEEPS = 6
T0 = {"indoor": 1.0, "outdoor": 1.0}
RINGS = 0
POINT = 16   # bytes of one xyzi point


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
    parts += [m.cloud(w).ravel() for w in range(4)] + [a.ravel() for a in m.score_point_coeff()] + [m.full_cloud().ravel()]
    ints = np.array([r["iterations"], r["num_selected"], r["kz"], r["degenerate"]], np.uint32)
    return np.concatenate([np.concatenate(parts).view(np.uint32), ints])


def measure(hip, kind, sweeps, lidar, B, steps, only_device=False):
    from lio_amd import capi

    pps = [capi.PointProcessor(hip, lidar.lower_deg, lidar.upper_deg, lidar.rings) for _ in range(B)]
    ods = [capi.PointOdometry(hip) for _ in range(B)]
    host, dev = [capi.PointMapping(hip) for _ in range(B)], [capi.PointMapping(hip) for _ in range(B)]
    walk = _walk(len(sweeps))
    last = [None]

    def front_end(k):
        x = sweeps[walk[k % len(walk)]]
        if B > 1:
            capi.PointProcessor.process_batch(pps, [x] * B)
        else:
            pps[0].process(x)
        last[0] = capi.PointOdometry.process_batch_from_pp(ods, pps)

    def run_host():
        inputs = []
        for m, od, pp, r in zip(host, ods, pps, last[0]):
            corner, surf = od.last_cloud(0), od.last_cloud(1)
            m.set_full_cloud(od.full_to_end(pp.cloud(RINGS)))
            inputs.append((corner, surf, r["T_sum"]))
        return capi.PointMapping.process_batch(host, inputs)

    def run_device():
        return capi.PointMapping.process_batch_from_odom(dev, ods, pps)

    t_host, t_dev, its, pcie = [], [], [], []
    for k in range(WARMUP + steps):
        front_end(k)
        if only_device:
            rb, b = _ms(run_device)
            if k >= WARMUP:
                t_dev.append(b), its.append(rb[0]["iterations"])
            continue
        if k % 2:
            (ra, a), (rb, b) = _ms(run_host), _ms(run_device)
        else:
            (rb, b), (ra, a) = _ms(run_device), _ms(run_host)
        for j in sorted({0, B // 2, B - 1}):   # the call's contract, at the size that is timed (every getter of every handle: tests/test_gpu_map_from_odom.py)
            assert np.array_equal(_words(host[j], ra[j]), _words(dev[j], rb[j])), (kind, B, k, j)
        if k >= WARMUP:
            t_host.append(a), t_dev.append(b), its.append(ra[0]["iterations"])
            nc, ns, nf = len(ods[0].last_cloud(0)), len(ods[0].last_cloud(1)), len(pps[0].cloud(RINGS))
            # down: both stack clouds, the ring cloud, lio_odom_full_to_end's result; up: lio_odom_full_to_end's input, the full cloud, both stack clouds
            pcie.append(dict(host_d2h=(nc + ns + 2 * nf) * POINT, host_h2d=(nc + ns + 2 * nf) * POINT, device_d2h=0, device_h2d=0, n_corner=nc, n_surf=ns, n_full=nf))
    out = dict(what="device_only" if only_device else "host_vs_device", kind=kind, B=B, steps_measured=steps, iterations_median=int(np.median(its)),
               device_ms=_stats(t_dev), device_per_sensor_us=round(float(np.median(t_dev)) / B * 1e3, 2))
    if only_device:
        return out
    med_h, med_d = float(np.median(t_host)), float(np.median(t_dev))
    mid = pcie[len(pcie) // 2]
    out.update(host_ms=_stats(t_host), host_per_sensor_us=round(med_h / B * 1e3, 2), ratio=round(med_h / med_d, 3),
               pcie_bytes_per_sensor_step=dict(host=mid["host_d2h"] + mid["host_h2d"], device=0), counts=dict(n_corner=mid["n_corner"], n_surf=mid["n_surf"], n_full=mid["n_full"]),
               holds=bool(med_d <= np.max(t_host)) if B == 1 else bool(med_d < np.min(t_host)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--kinds", default="indoor,outdoor")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-batches", default="1,8,64")
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.steps >= 16, "medians over at least 16 steps"
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi, synth

    hip = capi.load_hip()
    results = []
    for kind in args.kinds.split(","):
        sweeps, _, lidar = synth.make_sweeps(kind, N_SWEEPS, t0=T0[kind])
        sweeps = [np.ascontiguousarray(s, np.float32) for s in sweeps]
        for B in [int(b) for b in args.batches.split(",") if b]:
            results.append(measure(hip, kind, sweeps, lidar, B, args.steps, args.only_device))
            print(json.dumps(results[-1]), flush=True)
    if args.parent_lib:
        from map_batch_cost import N_FRAMES, measure_batch_parent
        from mapping_util import drifting_inputs
        from odom_batch_cost import load_parent

        parent = load_parent(args.parent_lib)
        oracle = capi.LioLib(os.path.join(ROOT, "oracle", "liblio_oracle.so"))
        for kind in args.kinds.split(","):
            frames = drifting_inputs(oracle, kind, N_FRAMES)
            for B in [int(b) for b in args.parent_batches.split(",") if b]:
                results.append(measure_batch_parent(hip, parent, kind, frames, B, args.steps))
                print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
