"""What the map refresh and the surround map cost (docs/map_refresh.md).

Two estimators on the same frames, alternating step by step: one with lio_est_set_map_refresh off (the default path), one with it on.
Every timed call ends in a device synchronise (push_frame waits for its VoxelGrid's count, refresh_map and lio_map_get_surround
for their stream), so the host clock around it is the call's latency as the caller pays it; `solve` is the report's ms_total.
Medians over the steps after the ring has filled; a GPU is required.

    python tools/map_refresh_cost.py [--steps 8] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lio-mapping_amd"))

IDENT = ([0, 0, 0, 1], [0, 0, 0])


def _ms(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def measure(hip, kind, W, Wo, steps):
    from lio_amd import capi, pipeline, synth

    n_frames = W + 1 + Wo + 1 + steps
    ds = synth.make_dataset(kind, n_frames, 0.3 if kind == "outdoor" else 0.2)
    pp = capi.PointProcessor(hip, ds.lidar.lower_deg, ds.lidar.upper_deg, ds.lidar.rings)
    clouds = []
    for f in ds.frames:
        pp.process(f.scan)
        clouds.append((pp.cloud(4), pp.cloud(2)))
    ests = {}
    for name in ("off", "on"):
        cfg = pipeline.config_outdoor64(hip, W, Wo) if kind == "outdoor" else pipeline.config_indoor(hip, W, Wo)
        if kind != "outdoor":
            cfg.cutoff_deskew, cfg.keep_features, cfg.prior_factor = 1, 0, 1
        pipeline.set_extrinsic(cfg, ds)
        est = capi.Estimator(hip, cfg)
        if name == "on":
            est.set_map_refresh(True)
            est.map().process(clouds[0][1], clouds[0][0], IDENT)     # the scan-to-map stage's first sweep: centre, valid list, surround list
        pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01)
        ests[name] = est
    T = capi.TransformF.make(*IDENT)
    rows = []
    for k in range(W + 1, n_frames):
        row = {}
        for name in (("off", "on") if k % 2 else ("on", "off")):
            est, f = ests[name], ds.frames[k]
            for j in range(f.imu_dt.shape[0]):
                est.process_imu(float(f.imu_dt[j]), f.imu_acc[j], f.imu_gyr[j], float(f.imu_t[j]))
            _, row[name + "_push"] = _ms(lambda: est.push_frame(T, clouds[k][0], clouds[k][1], f.t))
            rep = est.solve()
            row[name + "_solve"] = rep.ms_total
            if name == "on":
                r, row["refresh"] = _ms(est.refresh_map)
                row["applied"] = r
                h = est.last_map_refresh()
                row["n_corner"], row["n_surf"] = len(h["corner"]), len(h["surf"])
            _, row[name + "_slide"] = _ms(est.slide)
            if name == "on":
                m = est.map()
                n, row["surround_count"] = _ms(lambda: hip.dll.lio_map_get_surround(m.h, 0.6, None))
                out, row["surround_copy"] = _ms(lambda: m.surround(0.6))     # count call + copy call
                row["n_surround"] = int(n)
        rows.append(row)
    full = [r for r in rows if r["applied"] == 1][1:]   # the first applied refresh lays the pool out and grows buffers
    med = lambda key: float(np.median([r[key] for r in full]))
    keys = ("off_push", "on_push", "off_solve", "on_solve", "refresh", "off_slide", "on_slide", "surround_count", "surround_copy")
    res = {k: round(med(k), 4) for k in keys}
    res.update(kind=kind, W=W, Wo=Wo, steps_measured=len(full), n_corner=int(med("n_corner")), n_surf=int(med("n_surf")), n_surround=int(med("n_surround")),
               spread={k: [round(float(np.min([r[k] for r in full])), 4), round(float(np.max([r[k] for r in full])), 4)] for k in keys})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before the product library, as in __graft_entry__.py)

    assert torch.cuda.is_available(), "needs a GPU"
    from lio_amd import capi

    hip = capi.load_hip()
    results = [measure(hip, "indoor", 4, 2, args.steps), measure(hip, "outdoor", 15, 5, args.steps)]
    for r in results:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
