"""Device time of one voxel filter (VoxelGridDev::run through lio_bench_voxel_grid) at the sizes the product filters (docs/voxel_sort.md).

    python tools/voxel_filter_cost.py [--lib PATH] [--reps 200] [--rounds 5] [--no-bench-map] [--out FILE.json]

--lib PATH measures another build of the product in this tree's place; run the tool once per build, alternating, to compare two builds.

sizes   2 k (a scan-to-map stack), 43 k (the sensor-frame stack Estimator::PushFrame filters), 177 k (the HDL-64E window's local map,
        Estimator::BuildLocalMap) and 260 k points
clouds  random: planes + clutter over 40 m x 40 m, the clouds of tests/test_gpu_parity.py (_random_cloud), 20 non-finite rows
        bench:  the surf stacks of bench.py's HDL-64E window that BuildLocalMap concatenates (pivot to newest but one, about 177 k points); smaller
                sizes take every k-th point, 260 k adds a shifted copy of the first points
time    HIP events around `reps` back-to-back filters of the resident cloud, host waits included; median (min - max) over `rounds` rounds
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lio-mapping_amd"))
sys.path.insert(0, ROOT)

SIZES = (2000, 43000, 177000, 260000)
LEAF = 0.4


def random_cloud(n):
    rng = np.random.default_rng(n)
    pts = np.zeros((n, 4), dtype=np.float32)
    pts[:, 0] = rng.uniform(-20.0, 20.0, n)
    pts[:, 1] = rng.uniform(-20.0, 20.0, n)
    pts[:, 2] = np.where(rng.random(n) < 0.7, rng.normal(0, 0.02, n), rng.uniform(0, 5, n))
    pts[:, 3] = rng.uniform(0, 64, n)
    pts[rng.integers(0, n, 20), 0] = np.nan
    return pts


def bench_local_map(hip):
    """the points bench.py's flagship solve filters: the surf stacks of its window"""
    import bench

    W, Wo = 15, 5
    ds = bench.make_dataset("outdoor", W)
    clouds, _ = bench.feature_clouds(hip, ds)
    est = bench.make_estimator(hip, ds, clouds, "outdoor", W, Wo)
    return np.concatenate([est.get_surf_stack(i) for i in range(W - Wo, W)], axis=0)


def resized(cloud, n):
    if n <= len(cloud):
        return np.ascontiguousarray(cloud[:: len(cloud) // n][:n])
    extra = cloud[: n - len(cloud)].copy()
    extra[:, :3] += np.float32(0.13)
    return np.concatenate([cloud, extra], axis=0)


def measure(hip, pts, reps, rounds):
    ms, n_out = zip(*[hip.bench_voxel_grid(pts, LEAF, reps=reps) for _ in range(rounds)])
    return dict(points_in=int(len(pts)), points_out=int(n_out[0]), ms_per_filter=dict(median=round(float(np.median(ms)), 5), min=round(float(np.min(ms)), 5),
                                                                                      max=round(float(np.max(ms)), 5)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-bench-map", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi

    hip = capi.LioLib(args.lib) if args.lib else capi.load_hip()
    rows = []
    kinds = [("random", None)] if args.no_bench_map else [("random", None), ("bench", bench_local_map(hip))]
    for kind, base in kinds:
        for n in SIZES:
            pts = random_cloud(n) if base is None else resized(base, n)
            row = dict(cloud=kind, **measure(hip, pts, args.reps, args.rounds))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(lib=hip.path, leaf=LEAF, reps=args.reps, rounds=args.rounds, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
