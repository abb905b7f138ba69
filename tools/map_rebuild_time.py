"""Times mh_map_rebuild_from_keyframes on the GPU against the route a caller had before it: mh_map_create plus one
mh_map_insert_device per keyframe, fed from the same keyframe store.  Every figure is a median host wall clock over --repeats
repeats after warm-up, in ms.

Sizes:   64 keyframes of 8 016 points, 512 keyframes of 8 016 points, 512 keyframes of 32 064 points
Scene:   a sensor walking down a 240 x 16 x 5 m hall, 0.4 m per keyframe; each cloud is a ray cast of the hall from the keyframe's
         true pose, so the map is the consistent one a rebuild produces
Cycles:  lru_clear_cycle 10 (the reference's value: a chunk is at most 10 keyframes) and 2^31 - 1 (never purges: chunks are cut by the
         point budget alone, the default 4 Mi)
Sides:   rebuild   mh_map_rebuild_from_keyframes
         twin      mh_map_create + one mh_map_insert_device per keyframe
Both sides end with the same mh_map_get_stats (checked), and the maps are released outside the timed region.

The sides alternate in fresh child processes, --rounds rounds, each child under a time limit; a failed child ends the run.
Writes profiles/map_rebuild_time.json (or --out) and, unless --no-trace, profiles/map_rebuild_kernel_stats.txt: two
rocprofv3 --kernel-trace --stats runs of their own (no counters) — `small`: one rebuild and one twin loop per cycle at 64 keyframes;
`long`: one rebuild of 512 keyframes of 8 016 points in ONE chunk (the never-purging cycle), the longest segments phase C meets here.
--trace-only writes the second file alone.

  timeout -k 10 1100 python tools/map_rebuild_time.py

  python tools/map_rebuild_time.py [--repeats N] [--rounds R] [--out PATH] [--no-trace]
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((64, 8016), (512, 8016), (512, 32064))   # keyframes, points per keyframe (48 rows x 167 / 668 columns)
CYCLES = (10, 2 ** 31 - 1)
SIDES = ("rebuild", "twin")
WARMUP = 1
HALL = np.array([240.0, 16.0, 5.0])


def keyframes(K: int, n: int):
    """K clouds of n points in the sensor frame (f32) and the poses they were cast from (R K x 3 x 3, t K x 3, f32)"""
    rows = 48
    cols = n // rows
    assert rows * cols == n
    alt = np.linspace(-0.6, 0.6, rows)
    az = np.arange(cols) * (2.0 * np.pi / cols)
    a, z = np.meshgrid(alt, az, indexing="ij")
    d_s = np.stack([np.cos(a) * np.cos(z), np.cos(a) * np.sin(z), np.sin(a)], axis=-1).reshape(-1, 3)
    clouds, Rs, ts = [], [], []
    for k in range(K):
        yaw = 0.3 * np.sin(0.05 * k)
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        t = np.array([6.0 + 0.4 * k, 8.0 + 2.0 * np.sin(0.03 * k), 1.5])
        d = d_s @ R.T
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d > 0, (HALL - t) / d, np.where(d < 0, (0.0 - t) / d, np.inf)).min(axis=1)
        clouds.append((np.minimum(r, 60.0)[:, None] * d_s).astype(np.float32))
        Rs.append(R)
        ts.append(t)
    return clouds, np.asarray(Rs, np.float32), np.asarray(ts, np.float32)


def setup(K: int, n: int):
    from mimosa_amd import capi
    ctx = capi.Context(0)
    clouds, Rs, ts = keyframes(K, n)
    st = capi.KeyframeStore(ctx, capacity_keyframes=K, capacity_points=K * n)
    for k, c in enumerate(clouds):
        st.add(c, tag=k)
    return ctx, st, Rs, ts


def twin(ctx, st, Rs, ts, cycle):
    from mimosa_amd import capi
    tw = capi.VoxelMap(ctx, lru_clear_cycle=cycle)
    for k in range(st.size()):
        d, m = st.device_points(k)
        ctx.check(ctx.L.mh_map_insert_device(tw.h, d, m, 4, capi._p(Rs[k]), capi._p(ts[k])))
    return tw


def comparable(stats: dict) -> dict:
    return {k: v for k, v in stats.items() if k != "device_bytes"}


def one(K: int, n: int, cycle: int, side: str, repeats: int) -> dict:
    ctx, st, Rs, ts = setup(K, n)
    ref = twin(ctx, st, Rs, ts, cycle)
    want = comparable(ref.stats())
    ref.release()
    out = {"keyframes": K, "points_per_keyframe": n, "lru_clear_cycle": cycle, "side": side, "repeats": repeats, "n_points": want["n_points"],
           "n_voxels": want["n_voxels"]}
    t_ms = []
    for i in range(repeats + WARMUP):
        ctx.synchronize()
        a = time.perf_counter()
        if side == "rebuild":
            gm, res = st.rebuild_map((Rs, ts), lru_clear_cycle=cycle)
            out["chunks"], out["purges"] = res["chunks"], res["purges"]
        else:
            gm = twin(ctx, st, Rs, ts, cycle)
        b = time.perf_counter()
        if comparable(gm.stats()) != want:
            sys.exit("map_rebuild_time: the sides disagree: %r against %r" % (gm.stats(), want))
        gm.release()
        if i >= WARMUP:
            t_ms.append((b - a) * 1e3)
    out["ms"] = round(float(np.median(t_ms)), 3)
    st.destroy()
    ctx.close()
    return out


TRACES = {"small": "%d keyframes of %d points into the store, then per lru_clear_cycle in %r one mh_map_rebuild_from_keyframes and one twin loop"
                   % (SIZES[0][0], SIZES[0][1], list(CYCLES)),
          "long": "%d keyframes of %d points into the store, then one mh_map_rebuild_from_keyframes with lru_clear_cycle %d: one chunk" % (SIZES[1][0], SIZES[1][1], CYCLES[1])}


def traced(which: str) -> None:
    K, n = SIZES[0] if which == "small" else SIZES[1]
    ctx, st, Rs, ts = setup(K, n)
    for cycle in (CYCLES if which == "small" else CYCLES[1:]):
        gm, _ = st.rebuild_map((Rs, ts), lru_clear_cycle=cycle)
        gm.release()
        if which == "small":
            twin(ctx, st, Rs, ts, cycle).release()
    st.destroy()
    ctx.close()


def child(args, timeout=280) -> dict:
    print("map_rebuild_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(path: str) -> None:
    with open(path, "w") as f:
        for which in TRACES:
            kernel_stats_of(f, which)


def kernel_stats_of(f, which: str) -> None:
    """one rocprofv3 --kernel-trace --stats run of `--traced which` in a fresh process; the per-kernel table of its rocpd database"""
    import sqlite3
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="map_rebuild_trace_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "rebuild", "--", sys.executable, os.path.abspath(__file__), "--traced", which]
        print("map_rebuild_time:", " ".join(cmd), file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(r.returncode or 1)
        dbs = sorted(glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True))
        if not dbs:
            sys.exit("map_rebuild_time: no rocpd database under " + tmp)
        rows = sqlite3.connect(dbs[-1]).execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                                                "order by sum(end - start) desc").fetchall()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    f.write("kernel-trace summary of: python tools/map_rebuild_time.py --traced %s (rocprofv3 --kernel-trace --stats; durations in ns):\n%s\n"
            % (which, TRACES[which]))
    f.write("%-100s %8s %10s %10s %10s\n" % ("kernel", "calls", "avg", "min", "max"))
    for name, calls, avg, lo, hi in rows:
        f.write("%-100s %8d %10.0f %10d %10d\n" % (name[:100], calls, avg, lo, hi))
    f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_rebuild_time.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "map_rebuild_kernel_stats.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--one", action="store_true", help="run one size, cycle and side in this process and print its JSON")
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--points", type=int, default=8016)
    ap.add_argument("--cycle", type=int, default=10)
    ap.add_argument("--side", default="rebuild", choices=SIDES)
    ap.add_argument("--trace-only", action="store_true", help="write the kernel-trace file alone")
    ap.add_argument("--traced", default="", choices=("",) + tuple(TRACES), help="the workload of a kernel trace, in this process")
    a = ap.parse_args()
    if a.traced:
        traced(a.traced)
        return
    if a.trace_only:
        kernel_stats(a.stats_out)
        return
    if a.one:
        print(json.dumps(one(a.keyframes, a.points, a.cycle, a.side, a.repeats)))
        return
    out = {"tool": "map_rebuild_time", "cases": []}
    for K, n in SIZES:
        for cycle in CYCLES:
            runs = {s: [] for s in SIDES}
            for _ in range(a.rounds):
                for side in SIDES:  # alternating fresh processes
                    runs[side].append(child(["--one", "--keyframes", str(K), "--points", str(n), "--cycle", str(cycle), "--side", side, "--repeats", str(a.repeats)]))
            first = runs["rebuild"][0]
            row = {"keyframes": K, "points_per_keyframe": n, "lru_clear_cycle": cycle, "repeats": a.repeats, "rounds": a.rounds, "chunks": first["chunks"],
                   "purges": first["purges"], "n_points": first["n_points"], "n_voxels": first["n_voxels"]}
            for side in SIDES:
                vals = [q["ms"] for q in runs[side]]
                row[side + "_ms"] = round(float(np.median(vals)), 3)
                row[side + "_ms_runs"] = vals
            row["twin_over_rebuild"] = round(row["twin_ms"] / row["rebuild_ms"], 2)
            out["cases"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not a.no_trace:
        kernel_stats(a.stats_out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
