"""Times the radar Doppler path (mh_radar_*) on the GPU and the same arithmetic on the CPU; prints one JSON line.

  sync_500        one synchronous mh_radar_factor_linearize of a factor with 500 targets (host wall clock, median)
  batch_64x1000   one mh_radar_factor_linearize_batch of 64 factors x 1 000 targets (host wall clock, median; kernel time from
                  HIP events with mh_set_profiling on, in a separate pass)
  frontend_5000   one mh_radar_prepare_input of a 5 000-point mmWave cloud (host wall clock incl. the upload, median)
  *_c_call_ms     the same calls through ctypes with prebuilt arguments and no result conversion: the library's own time
                  (the plain figures above include the Python binding's dict building)
  cpu_*           the same arithmetic on one CPU core in numpy: the restatement in tests/radar_ref.py for the factor
                  (vectorised per factor, so it stands for a vectorised loop, not for the reference's per-target Eigen loop),
                  and the front end's gates vectorised in float32 (numpy's arctan2)

Run from the repository root: python tools/radar_time.py [--repeats N].  Under rocprofv3 --kernel-trace --stats each batch
call shows as ONE radar_linearize_kernel dispatch.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mimosa_amd import capi, synth_radar  # noqa: E402
import radar_ref  # noqa: E402


def med_ms(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = capi.Context(0)
    out = {"tool": "radar_time", "repeats": a.repeats}

    st = synth_radar.random_state(rng)
    t500 = synth_radar.random_targets(rng, 500)
    f = capi.RadarFactor(ctx, t500, st["R_B_S"], st["t_B_S"], st["omega"], 0.1)
    out["sync_500_ms"] = med_ms(lambda: f.linearize(st["R_W_B"], st["v_W"], st["bias_gyro"]), a.repeats)
    out["cpu_sync_500_ms"] = med_ms(lambda: radar_ref.linearize(t500, st["R_B_S"], st["t_B_S"], st["omega"], 0.1, st["R_W_B"], st["v_W"],
                                                                st["bias_gyro"]), max(20, a.repeats // 4))

    facs, states, tgs = [], [], []
    for _ in range(64):
        s = synth_radar.random_state(rng)
        tg = synth_radar.random_targets(rng, 1000)
        facs.append(capi.RadarFactor(ctx, tg, s["R_B_S"], s["t_B_S"], s["omega"], 0.1))
        states.append(s)
        tgs.append(tg)
    Rs = np.array([s["R_W_B"] for s in states])
    vs = np.array([s["v_W"] for s in states])
    bs = np.array([s["bias_gyro"] for s in states])
    out["batch_64x1000_ms"] = med_ms(lambda: capi.radar_linearize_batch(facs, Rs, vs, bs), a.repeats)
    ctx.set_profiling(1)
    k = [capi.radar_linearize_batch(facs, Rs, vs, bs)[0]["gpu_ms"] for _ in range(a.repeats)]
    out["batch_64x1000_kernel_ms"] = round(float(np.median(k)), 4)
    k1 = [f.linearize(st["R_W_B"], st["v_W"], st["bias_gyro"])["gpu_ms"] for _ in range(a.repeats)]
    out["sync_500_kernel_ms"] = round(float(np.median(k1)), 4)
    ctx.set_profiling(0)
    out["sequential_64x1000_ms"] = med_ms(lambda: [g.linearize(s["R_W_B"], s["v_W"], s["bias_gyro"]) for g, s in zip(facs, states)],
                                          max(10, a.repeats // 10))

    def cpu_window():
        for tg, s in zip(tgs, states):
            radar_ref.linearize(tg, s["R_B_S"], s["t_B_S"], s["omega"], 0.1, s["R_W_B"], s["v_W"], s["bias_gyro"])

    out["cpu_batch_64x1000_ms"] = med_ms(cpu_window, max(5, a.repeats // 20), warmup=1)

    L = ctx.L
    hs = (C.c_void_p * 64)(*[g.h for g in facs])
    Rf, vf, bf = (np.ascontiguousarray(x, np.float64).ravel() for x in (Rs, vs, bs))
    res = (capi.RadarResult * 64)()
    out["batch_64x1000_c_call_ms"] = med_ms(lambda: L.mh_radar_factor_linearize_batch(hs, 64, capi._p(Rf), capi._p(vf), capi._p(bf), res),
                                            a.repeats)
    R1, v1, b1 = (np.ascontiguousarray(st[k], np.float64).ravel() for k in ("R_W_B", "v_W", "bias_gyro"))
    r1 = capi.RadarResult()
    out["sync_500_c_call_ms"] = med_ms(lambda: L.mh_radar_factor_linearize(f.h, capi._p(R1), capi._p(v1), capi._p(b1), C.byref(r1)),
                                       a.repeats)

    sc = synth_radar.make_scene(n_static=4950, n_dynamic=39, seed=1)
    raw, lay = synth_radar.pack(sc["points"], "mmwave")
    cfg = capi.make_radar_config(**sc["cfg"])
    scan = capi.RadarScan(ctx)
    L = synth_radar.capi_layout(lay)
    out["frontend_points"] = len(sc["labels"])
    out["frontend_5000_ms"] = med_ms(lambda: scan.prepare_input(raw, L, cfg), a.repeats)
    n = len(sc["labels"])

    def cpu_front():
        x, y, z, i, v = radar_ref.decode(raw, n, "mmwave", lay["point_step"], lay)
        c = sc["cfg"]
        with np.errstate(invalid="ignore"):
            r = np.sqrt((x * x + y * y) + z * z)
            az = np.arctan2(y, x)
            el = np.arctan2(z, np.sqrt(x * x + y * y))
            keep = ~(np.isnan(x) | np.isnan(y) | np.isnan(z) | np.isnan(i) | np.isnan(v)) & ~(i < np.float32(c["filter_min_db"]))
            keep &= ~((r < np.float32(c["range_min"])) | (r > np.float32(c["range_max"])))
            keep &= ~(np.abs(az) > radar_ref.deg2rad_f(c["threshold_azimuth_deg"]))
            keep &= ~(np.abs(el) > radar_ref.deg2rad_f(c["threshold_elevation_deg"]))
        k = np.nonzero(keep)[0]
        return np.stack([x[k], y[k], z[k], r[k], az[k], el[k], v[k], i[k]], 1).astype(np.float64)

    out["cpu_frontend_5000_ms"] = med_ms(cpu_front, max(20, a.repeats // 4))
    out["frontend_valid"] = scan.prepare_input(raw, L, cfg)["n_points_valid"]
    for g in facs:
        g.destroy()
    f.destroy()
    scan.destroy()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
