"""Times mh_icp_window_optimise_lin on the GPU against mh_icp_window_optimise: W = 5 factors of 24 576 and of 1 024 points, the
replay's 6 iterations, its between sigmas, the tight prior and a damping of 1e-9 (the set-up of tools/icp_window_time.py and
tools/icp_window_relin_time.py).  Four sides, every figure the median host wall clock of one whole optimisation over --repeats
repeats after warm-up, per iteration in us:

  plain   mh_icp_window_optimise (the yardstick, of the same library)
  lin0    mh_icp_window_optimise_lin without a linear factor (the other step kernel and the added phase alone)
  lin1    ... with one linear factor, on the newest pose (a photometric factor)
  lin5    ... with one on every pose (photo_window)

The linear factors: SPD, eigenvalues 1e2 .. 1e4, linearized 5 mrad / 5 mm from the start pose of their variable.  Every repeat
starts from the same warm association state (clones of a factor linearized once).  The sides alternate in fresh child
processes, --pairs rounds per size, each child under a time limit; a failed child ends the run.  The spread of `plain` over its
rounds is what a difference has to exceed to count.

--replay-pairs P > 0 adds a native replay pair with the photometric factor on (10 scans of 64 x 512): device_window +
window_photo_linear against the host loop, P alternating pairs, scans per second of each run.

Writes profiles/icp_window_lin_time.json (or --out) and prints it.

  python tools/icp_window_lin_time.py [--repeats N] [--pairs P] [--replay-pairs P] [--out PATH]
  the step kernel's time, from a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o lin -- python tools/icp_window_lin_time.py --one 24576 --side lin5 --repeats 20
    python tools/icp_window_lin_time.py --kernel-stats OUT/lin_results.db > profiles/icp_window_lin_kernel_stats.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from icp_window_time import ITERS, W, expmap  # noqa: E402

SIDES = {"plain": None, "lin0": 0, "lin1": 1, "lin5": W}


def linear_factors(capi, n_lin, poses0):
    rng = np.random.default_rng(11)
    at = [W - 1] if n_lin == 1 else list(range(n_lin))
    out = []
    for i in at:
        R, t = poses0[i]
        ax, dt = rng.standard_normal(3), rng.standard_normal(3)
        L = (R @ expmap(ax / np.linalg.norm(ax) * 5e-3), t + R @ (dt / np.linalg.norm(dt) * 5e-3))
        Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
        H = (Q * np.logspace(2, 4, 6)) @ Q.T
        out.append(dict(pose=i, at=L, H=(H + H.T) / 2, b=np.zeros(6), f=0.0))
    return capi.make_window_linear(out)


def one(n_pts: int, side: str, repeats: int) -> dict:
    from mimosa_amd import capi, synth

    ctx = capi.Context(0)
    gm = capi.VoxelMap(ctx)
    gm.insert(synth.make_room(synth.BASE_SEED, 0, 0))
    scan, _ = synth.make_scan(64)
    pts = np.ascontiguousarray(scan[:: max(1, len(scan) // n_pts)][:n_pts])
    assert len(pts) == n_pts
    base = capi.ICPFactor(ctx, gm, pts, capi.make_reg_config(**synth.enwide_config()))
    base.set_components(False)
    Rq, tq = synth.query_pose()
    rng = np.random.default_rng(3)
    poses0 = [(Rq @ expmap(rng.standard_normal(3) * 0.003), tq + rng.standard_normal(3) * 0.02) for _ in range(W)]
    g = np.array([0.0, 0.0, -1.0])
    base.linearize(Rq, tq, g)
    L = ctx.L
    cfg = capi.make_window_config(iters=ITERS)
    R0 = np.ascontiguousarray(np.array([p[0].ravel() for p in poses0]))
    t0 = np.ascontiguousarray(np.array([p[1] for p in poses0]))
    hz = np.array([0] + [1] * (W - 1), np.int32)
    ZR = np.ascontiguousarray(np.tile(np.eye(3).ravel(), (W, 1)))
    Zt = np.zeros((W, 3))
    out_res = capi.WindowResult()
    trace = np.zeros((ITERS, W, 12))
    n_lin = SIDES[side]
    lin = linear_factors(capi, n_lin, poses0) if n_lin is not None else None

    def call(h):
        if lin is None:
            rc = L.mh_icp_window_optimise(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), C.byref(out_res),
                                          capi._p(trace))
        else:
            rc = L.mh_icp_window_optimise_lin(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), None, lin, n_lin,
                                              C.byref(out_res), capi._p(trace), None)
        assert rc == 0 and out_res.iters == ITERS

    t = []
    for i in range(repeats + 5):
        fs = [base.clone() for _ in range(W)]
        h = (C.c_void_p * W)(*[f.h for f in fs])
        a = time.perf_counter()
        call(h)
        b = time.perf_counter()
        for f in fs:
            f.destroy()
        if i >= 5:
            t.append((b - a) * 1e6 / ITERS)
    out = {"points": n_pts, "factors": W, "iters": ITERS, "repeats": repeats, "side": side, "us_per_iter": round(float(np.median(t)), 3)}
    base.destroy()
    gm.release()
    ctx.close()
    return out


def replay_one(on: bool) -> dict:
    from mimosa_amd import replay
    cfg = replay.ReplayConfig(n_scans=10, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2, keyframe_rot_thresh_deg=5.0, photometric=True,
                              device_window=on, window_photo_linear=on)
    scans = replay.make_scans(cfg)
    with tempfile.TemporaryDirectory() as d:
        r = replay.run_native(cfg, scans, d, repeats=2)
    return {"side": "device_window+window_photo_linear" if on else "host_loop", "scans_per_s": round(float(r["scans_per_s"]), 3)}


def kernel_stats(db_path: str) -> None:
    """the per-kernel table of a rocprofv3 kernel trace (the `kernels` view of its rocpd database: name, start, end in ns)"""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                      "order by sum(end - start) desc").fetchall()
    print("kernel-trace summary of: python tools/icp_window_lin_time.py --one 24576 --side lin5 --repeats 20 (rocprofv3 --kernel-trace; durations in ns)")
    print("%-100s %8s %10s %10s %10s" % ("kernel", "calls", "avg", "min", "max"))
    for name, calls, avg, lo, hi in rows:
        print("%-100s %8d %10.0f %10d %10d" % (name[:100], calls, avg, lo, hi))


def child(args, timeout=240) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--replay-pairs", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_window_lin_time.json"))
    ap.add_argument("--one", type=int, default=0, help="run one size and one side in this process and print its JSON")
    ap.add_argument("--side", default="lin5", choices=list(SIDES))
    ap.add_argument("--replay-one", default="", choices=["", "on", "off"], help="run one native replay in this process and print its JSON")
    ap.add_argument("--kernel-stats", default="", help="reduce this rocprofv3 database to the per-kernel table and print it")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
        return
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    if a.replay_one:
        print(json.dumps(replay_one(a.replay_one == "on")))
        return
    out = {"tool": "icp_window_lin_time", "sizes": []}
    for n in (24576, 1024):
        runs = {s: [] for s in SIDES}
        for _ in range(a.pairs):
            for side in SIDES:  # alternating fresh processes
                runs[side].append(child(["--one", str(n), "--side", side, "--repeats", str(a.repeats)]))
        row = {"points": n, "factors": W, "iters": ITERS, "repeats": a.repeats, "pairs": a.pairs}
        for side in SIDES:
            vals = [q["us_per_iter"] for q in runs[side]]
            row[side + "_us_per_iter"] = round(float(np.median(vals)), 3)
            row[side + "_us_per_iter_runs"] = vals
        row["plain_spread_us"] = round(max(row["plain_us_per_iter_runs"]) - min(row["plain_us_per_iter_runs"]), 3)
        for side in ("lin0", "lin1", "lin5"):
            row[side + "_minus_plain_us"] = round(row[side + "_us_per_iter"] - row["plain_us_per_iter"], 3)
        out["sizes"].append(row)
    if a.replay_pairs:
        runs = {"off": [], "on": []}
        for _ in range(a.replay_pairs):
            for side in ("off", "on"):
                runs[side].append(child(["--replay-one", side], timeout=400)["scans_per_s"])
        out["native_replay_photometric"] = {"scans": 10, "rows": 64, "cols": 512, "pairs": a.replay_pairs, "host_loop_scans_per_s_runs": runs["off"],
                                            "device_window_photo_linear_scans_per_s_runs": runs["on"],
                                            "host_loop_scans_per_s": round(float(np.median(runs["off"])), 3),
                                            "device_window_photo_linear_scans_per_s": round(float(np.median(runs["on"])), 3)}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
