"""Times mh_scan_deskew_imu (per-timestamp poses on the device) against the sequence it replaces; prints one JSON line.

Per case (1024 distinct timestamps = a 128 x 1024 Ouster grid; 131 072 = one per point; 12 and 40 IMU segments), medians over
--repeats calls after a warm-up, each call followed by mh_synchronize so that both sides pay for all of their device work:

  parent_get_unique_ns_ms   mh_scan_get_unique_ns (from the pinned block up to 4096 timestamps, a stream wait + copy beyond)
  parent_host_poses_ms      the per-timestamp extrapolation on the host, numpy-vectorised (replay.propagate: it stands for a
                            vectorised loop, not for the C++ mirror's scalar loop, which the replay pairs below time in place)
  parent_deskew_ms          mh_scan_deskew with the float table (pinned copy, copy kernel, K1), wall / HIP events
  device_deskew_imu_ms      mh_scan_deskew_imu (segment block, copy kernel, pose kernel, K1), wall / HIP events
  photo_scan_ms / photo_scan_resident_ms   mh_photo_preprocess_scan (96 KB table for 1024 groups) / _resident, 1024 case only

--replay-pairs N: native replay scans/s with and without device_poses, N alternating pairs of fresh processes, and from the same
runs the C++ mirror's host time per scan in the IMU stage and in the deskew call (the parent's host extrapolation as the C++
loop runs it, at 1024 timestamps).
Under rocprofv3 --kernel-trace --stats (a run of its own, no counters) the pose kernel shows as deskew_pose_kernel.
Run from the repository root: python tools/deskew_imu_time.py [--repeats 200] [--replay-pairs 5]
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

from mimosa_amd import capi, replay, synth, synth_photo  # noqa: E402


def med(fn, repeats, warmup=10):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def imu_case(n_seg, header_ts=100.0, span=0.1):
    rng = np.random.default_rng(n_seg)
    ts = header_ts - 0.001 + np.arange(n_seg + 1) * ((span + 0.002) / n_seg)
    gyro, acc = rng.normal(0, 0.2, (n_seg + 1, 3)), rng.normal(0, 0.5, (n_seg + 1, 3)) + np.array([0, 0, 9.81])
    return ts, gyro, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--replay-pairs", type=int, default=0)
    a = ap.parse_args()
    ctx = capi.Context(0)
    L = ctx.L
    out = {"tool": "deskew_imu_time", "repeats": a.repeats, "cases": {}}
    n = 128 * 1024
    rng = np.random.default_rng(0)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz = d * rng.uniform(2.0, 40.0, n)[:, None]
    raw = np.zeros(n, dtype=synth.OUSTER_DTYPE)
    raw["x"], raw["y"], raw["z"], raw["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 50.0
    raw["ring"] = (np.arange(n) // 1024).astype(np.uint16)
    icfg = capi.make_input_config(range_min=0.0, range_max=1000.0)
    R0, p0, v0 = synth.so3_exp(np.array([0.02, -0.01, 0.4])), np.array([3.0, -2.0, 1.0]), np.array([1.5, 0.2, -0.1])
    for n_ts in (1024, n):
        raw["t"] = np.tile(np.arange(1024, dtype=np.uint32) * 97_656, 128) if n_ts == 1024 else np.sort(rng.choice(99_900_000, n, replace=False)).astype(np.uint32)
        sc = capi.Scan(ctx)
        sc.prepare_input(raw, icfg)
        for n_seg in (12, 40):
            imu = imu_case(n_seg)
            seg, (R_end, p_end, _) = replay.imu_segments(R0, p0, v0, imu)
            g = np.ascontiguousarray(replay.GRAVITY, np.float64)
            Rl, tl = np.ascontiguousarray(R_end.T), np.ascontiguousarray(-R_end.T @ p_end)
            Rb, tb = np.eye(3), np.zeros(3)
            uns = np.empty(n_ts, np.uint32)
            m = C.c_size_t()
            r = {}

            def get_uns():
                ctx.check(L.mh_scan_get_unique_ns(sc.h, capi._p(uns), n_ts, C.byref(m)))

            r["parent_get_unique_ns_ms"] = med(get_uns, a.repeats)

            def host_poses():
                T, (Rp, pp, _) = replay.propagate(R0, p0, v0, imu, 100.0, uns)
                o = np.empty_like(T)
                o[:, :9] = (Rp.T @ T[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
                o[:, 9:] = (T[:, 9:] - pp) @ Rp
                return o

            r["parent_host_poses_ms"] = med(host_poses, max(20, a.repeats // 4))
            T32 = np.ascontiguousarray(host_poses(), np.float32)

            def parent():
                ctx.check(L.mh_scan_deskew(sc.h, capi._p(T32), n_ts))
                ctx.check(L.mh_synchronize(ctx.h))

            def device():
                ctx.check(L.mh_scan_deskew_imu(sc.h, capi._p(seg), len(seg), 100.0, capi._p(g), capi._p(Rl), capi._p(tl), capi._p(Rb), capi._p(tb)))
                ctx.check(L.mh_synchronize(ctx.h))

            def events(fn):
                ms, t = C.c_float(), []
                for _ in range(a.repeats):
                    ctx.check(L.mh_timer_begin(ctx.h))
                    fn()
                    ctx.check(L.mh_timer_end(ctx.h, C.byref(ms)))
                    t.append(ms.value)
                return round(float(np.median(t)), 4)

            r["parent_deskew_ms"], r["device_deskew_imu_ms"] = med(parent, a.repeats), med(device, a.repeats)
            r["parent_deskew_events_ms"], r["device_deskew_imu_events_ms"] = events(parent), events(device)
            out["cases"][f"{n_ts}ts_{n_seg}seg"] = r
        sc.destroy()

    # the photometric frame: 128 x 1024 scene, 1024 groups
    pcfg = synth_photo.photo_config()
    f = synth_photo.make_frame(pcfg, 1)
    full = np.zeros(pcfg["rows"] * pcfg["cols"], dtype=synth.OUSTER_DTYPE)
    full["x"] = np.nan
    for k in ("x", "y", "z", "intensity", "t"):
        full[k][f["raw"]["idx"]] = f["raw"][k]
    full["ring"] = (np.arange(len(full)) // pcfg["cols"]).astype(np.uint16)
    sc, ph = capi.Scan(ctx), capi.Photo(ctx, pcfg)
    ctx.check(L.mh_scan_keep_raw(sc.h, 1))
    imu = imu_case(12, header_ts=0.0)
    vel = f["R_W_L"] @ np.array([1.2, 0.2, 0.0])
    seg, (R_end, p_end, _) = replay.imu_segments(f["R_W_L"] @ synth.so3_exp(np.array([0.0, 0.0, -0.35 * 0.101])), f["t_W_L"] - vel * 0.101, vel, (imu[0], np.tile([0.0, 0.0, 0.35], (13, 1)),
                                                                                           np.tile(f["R_W_L"].T @ -replay.GRAVITY, (13, 1))))

    def frame(resident):
        sc.prepare_input(full, icfg)
        sc.deskew_imu(seg, 0.0, replay.GRAVITY, (R_end.T, -R_end.T @ p_end), (np.eye(3), np.zeros(3)))
        T = None if resident else sc.deskew_poses()
        t0 = time.perf_counter()
        ph.preprocess_scan_resident(sc) if resident else ph.preprocess_scan(sc, T)
        return (time.perf_counter() - t0) * 1e3

    for name, res in (("photo_scan_ms", False), ("photo_scan_resident_ms", True)):
        t = [frame(res) for _ in range(a.repeats // 4 + 5)][5:]
        out[name] = round(float(np.median(t)), 4)
    ph.destroy()
    sc.destroy()
    ctx.close()

    if a.replay_pairs:
        import dataclasses
        cfg = replay.ReplayConfig(n_scans=20, rows=128)
        scans = replay.make_scans(cfg)
        on, off = [], []
        with tempfile.TemporaryDirectory() as tmp:
            for _ in range(a.replay_pairs):
                off.append(replay.run_native(cfg, scans, tmp, repeats=2))
                on.append(replay.run_native(dataclasses.replace(cfg, device_poses=True), scans, tmp, repeats=2))
        out["replay_scans_per_s_off"], out["replay_scans_per_s_on"] = [r["scans_per_s"] for r in off], [r["scans_per_s"] for r in on]
        # the C++ mirror's own host time per scan (main thread, 1024 timestamps): the IMU stage (off: propagate() over every
        # timestamp + the T_Le_Lt table; on: the sample-to-sample half alone) and the deskew call
        for name, rs in (("off", off), ("on", on)):
            out[f"replay_host_imu_ms_per_scan_{name}"] = [round(r["stage_s"]["imu"] / cfg.n_scans * 1e3, 5) for r in rs]
            out[f"replay_host_deskew_call_ms_per_scan_{name}"] = [round(r["detail_s"]["deskew"] / cfg.n_scans * 1e3, 5) for r in rs]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
