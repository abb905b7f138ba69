"""Times the photometric window batch (mh_photo_factor_linearize_batch) against separate calls; prints one JSON line.

  W = 1, 5, 16, 64 factors of 60 features each (clones of one factor on the 128 x 1024 synthetic frames of synth_photo):
  batch_W_ms         one blocking mh_photo_factor_linearize_batch of the W factors (host wall clock, median)
  singles_W_ms       W blocking mh_photo_factor_linearize calls one after the other (host wall clock, median)
  batch_W_kernel_ms  the batch launch's kernel time (HIP events, mh_set_profiling on, separate pass; median)
  single_ms / single_kernel_ms   one blocking single call and its kernel time
  replay_*           the native replay (host/mimosa_hip/replay.hpp, pipelined) over --replay-scans scans of 128 x 1024, with
                     and without photo_window: scans per second (best of --replay-repeats runs inside the driver)

All calls go through ctypes with prebuilt arguments and no result conversion (the library's own time).  Run from the
repository root: python tools/photo_batch_time.py [--repeats N] [--replay-scans N | 0].  Under rocprofv3 --kernel-trace
--stats each batch call shows as ONE photo_linearize_batch_kernel dispatch.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimosa_amd import capi, replay, synth_photo as sp  # noqa: E402

WINDOWS = (1, 5, 16, 64)


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
    ap.add_argument("--replay-scans", type=int, default=10)
    ap.add_argument("--replay-repeats", type=int, default=2)
    a = ap.parse_args()
    out = {"tool": "photo_batch_time", "repeats": a.repeats}
    cfg = sp.photo_config()
    fr = [sp.make_frame(cfg, k) for k in range(2)]
    ctx = capi.Context(0)
    g = capi.Photo(ctx, cfg)
    g.preprocess(fr[0]["raw"], fr[0]["deskewed"], fr[0]["unique_ns"], fr[0]["T_Le_Lt"])
    g.detect(60, fr[0]["R_W_Be"], fr[0]["t_W_Be"], sp.BIAS_DIRECTIONS)
    g.preprocess(fr[1]["raw"], fr[1]["deskewed"], fr[1]["unique_ns"], fr[1]["T_Le_Lt"])
    src = g.make_factor()
    out["features_per_factor"] = src.n
    facs = [src.clone() for _ in range(max(WINDOWS))]
    R, t = np.ascontiguousarray(fr[1]["R_W_Be"], np.float64), np.ascontiguousarray(fr[1]["t_W_Be"], np.float64)
    out["valid_features"] = int(src.linearize(R, t)["status_hist"][8])
    L = ctx.L
    r1 = capi.PhotoResult()
    pR, pt = capi._p(R.ravel()), capi._p(t)
    out["single_ms"] = med_ms(lambda: L.mh_photo_factor_linearize(src.h, pR, pt, None, None, C.byref(r1)), a.repeats)
    for W in WINDOWS:
        hs = (C.c_void_p * W)(*[f.h for f in facs[:W]])
        Rs = np.ascontiguousarray(np.tile(R, (W, 1, 1)))
        ts = np.ascontiguousarray(np.tile(t, (W, 1)))
        res = (capi.PhotoResult * W)()
        out[f"batch_{W}_ms"] = med_ms(lambda: L.mh_photo_factor_linearize_batch(hs, W, capi._p(Rs), capi._p(ts), None, None, res), a.repeats)
        one = [f.h for f in facs[:W]]

        def singles():
            for h in one:
                L.mh_photo_factor_linearize(h, pR, pt, None, None, C.byref(r1))

        out[f"singles_{W}_ms"] = med_ms(singles, max(20, a.repeats // max(1, W // 4)))
    ctx.set_profiling(1)
    k = []
    for _ in range(a.repeats):
        L.mh_photo_factor_linearize(src.h, pR, pt, None, None, C.byref(r1))
        k.append(r1.gpu_ms)
    out["single_kernel_ms"] = round(float(np.median(k)), 4)
    for W in WINDOWS:
        hs = (C.c_void_p * W)(*[f.h for f in facs[:W]])
        Rs = np.ascontiguousarray(np.tile(R, (W, 1, 1)))
        ts = np.ascontiguousarray(np.tile(t, (W, 1)))
        res = (capi.PhotoResult * W)()
        k = []
        for _ in range(a.repeats):
            L.mh_photo_factor_linearize_batch(hs, W, capi._p(Rs), capi._p(ts), None, None, res)
            k.append(res[0].gpu_ms)
        out[f"batch_{W}_kernel_ms"] = round(float(np.median(k)), 4)
    ctx.set_profiling(0)
    for f in facs:
        f.destroy()
    src.destroy()
    g.destroy()
    ctx.close()
    if a.replay_scans:
        cfg_r = replay.ReplayConfig(n_scans=a.replay_scans)
        scans = replay.make_scans(cfg_r)
        out["replay_scans"] = a.replay_scans
        with tempfile.TemporaryDirectory() as d:
            for on in (False, True):
                c = replay.ReplayConfig(n_scans=a.replay_scans, photo_window=on)
                r = replay.run_native(c, scans, d, repeats=a.replay_repeats)
                key = "replay_photo_window" if on else "replay"
                out[key + "_scans_per_s"] = round(float(r["scans_per_s"]), 2)
                out[key + "_photo_valid_min"] = int(min(r["photo_valid"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
