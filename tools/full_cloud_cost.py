"""What carrying the full-resolution sweep costs (docs/full_cloud.md).

Two estimators on the same frames, alternating step by step: one with lio_est_set_full_cloud off (the default path), one with it on.
The full cloud of a step is the sweep's ring-ordered cloud (LIO_PP_RINGS: 29 k points for the VLP-16, 130 k for the HDL-64E).  Every timed
call ends in a device synchronise or a host wait, so the host clock around it is the call's latency as the caller pays it; `solve` is
the report's ms_total and contains the correction's launch (the kernel itself runs behind the solve, on the estimator's stream).
Medians over the steps after the first; a GPU is required.

    python tools/full_cloud_cost.py [--steps 8] [--out FILE.json]
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

    n_frames = W + 1 + 1 + steps
    ds = synth.make_dataset(kind, n_frames, 0.3 if kind == "outdoor" else 0.2)
    pp = capi.PointProcessor(hip, ds.lidar.lower_deg, ds.lidar.upper_deg, ds.lidar.rings)
    clouds = []
    for f in ds.frames:
        pp.process(f.scan)
        clouds.append((pp.cloud(4), pp.cloud(2), pp.cloud(0)))
    ests = {}
    for name in ("off", "on"):
        cfg = pipeline.config_outdoor64(hip, W, Wo) if kind == "outdoor" else pipeline.config_indoor(hip, W, Wo)
        if kind != "outdoor":
            cfg.keep_features, cfg.prior_factor = 0, 1
        cfg.enable_deskew, cfg.cutoff_deskew = 1, 0          # a real transform_es_: the correction has its full arithmetic to do
        pipeline.set_extrinsic(cfg, ds)
        est = capi.Estimator(hip, cfg)
        if name == "on":
            est.set_full_cloud(True)
        pipeline.init_window(est, hip, ds, [c[0] for c in clouds], pos_sigma=0.01, rot_sigma=0.001, vel_sigma=0.01)
        ests[name] = est
    T = capi.TransformF.make(*IDENT)
    pivot1 = W - Wo + 1
    rows = []
    for k in range(W + 1, n_frames):
        row = {}
        for name in (("off", "on") if k % 2 else ("on", "off")):
            est, f = ests[name], ds.frames[k]
            for j in range(f.imu_dt.shape[0]):
                est.process_imu(float(f.imu_dt[j]), f.imu_acc[j], f.imu_gyr[j], float(f.imu_t[j]))
            if name == "on":
                m = est.map()
                _, row["set"] = _ms(lambda: m.set_full_cloud(clouds[k][2]))
            _, row[name + "_push"] = _ms(lambda: est.push_frame(T, clouds[k][0], clouds[k][1], f.t))
            rep = est.solve()
            row[name + "_solve"] = rep.ms_total
            if name == "on":
                out = np.zeros((max(len(c[2]) for c in clouds), 4), np.float32)   # any ring entry fits: the sweeps differ in size
                fp = out.ctypes.data_as(capi.c_float_p)
                n, row["get_stack"] = _ms(lambda: hip.dll.lio_est_get_full_stack(est.h, W, fp, None))
                row["n_full"] = int(n)
                row["registered"] = float("nan")
                if est.full_stack(pivot1)[1] == capi.FULL_SENSOR_END:
                    n_out = capi.C.c_size_t(0)
                    assert hip.dll.lio_est_get_registered_full(est.h, pivot1, None, capi.C.byref(n_out), None) == 0 and n_out.value <= len(out)
                    rc, row["registered"] = _ms(lambda: hip.dll.lio_est_get_registered_full(est.h, pivot1, None, capi.C.byref(n_out), fp))
                    assert rc == 0
            est.slide()
        rows.append(row)
    rows = rows[1:]   # the first step grows the buffers
    med = lambda key: float(np.nanmedian([r[key] for r in rows]))
    keys = ("off_push", "on_push", "off_solve", "on_solve", "set", "get_stack", "registered")
    res = {k: round(med(k), 4) for k in keys}
    res.update(kind=kind, W=W, Wo=Wo, steps_measured=len(rows), n_full=int(med("n_full")), mbytes=round(med("n_full") * 16 / 1e6, 3),
               spread={k: [round(float(np.nanmin([r[k] for r in rows])), 4), round(float(np.nanmax([r[k] for r in rows])), 4)] for k in keys})
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
