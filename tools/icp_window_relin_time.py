"""Times mh_icp_window_optimise_relin on the GPU against mh_icp_window_optimise: W = 5 factors of 24 576 and of 1 024 points, the
replay's 6 iterations, its between sigmas, the tight prior and a damping of 1e-9 (the set-up of tools/icp_window_time.py, whose
scene this tool builds through its `one`-style helpers).  Three sides, every figure the median host wall clock of one whole
optimisation over --repeats repeats after warm-up, per iteration in us:

  plain        mh_icp_window_optimise
  relin_zero   mh_icp_window_optimise_relin at thresholds 0 (every factor every iteration: the added phases alone)
  relin_ref    ... at the reference's thresholds, 1.75e-2 rad and 5e-3 m; with the mean number of factors evaluated per iteration

Every repeat starts from the same warm association state (clones of a factor linearized once).  The sides alternate in fresh
child processes, --pairs rounds per size, each child under a time limit; a failed child ends the run.  The spread of `plain`
over its rounds is what `relin_zero` has to stay within to count as level.

Writes profiles/icp_window_relin_time.json and prints it.

  python tools/icp_window_relin_time.py [--repeats N] [--pairs P]
  the step kernel's time, from a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o relin -- python tools/icp_window_relin_time.py --one 24576 --side relin_ref --repeats 20
    python tools/icp_window_relin_time.py --kernel-stats OUT/relin_results.db > profiles/icp_window_relin_kernel_stats.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from icp_window_time import ITERS, W, expmap  # noqa: E402

SIDES = {"plain": None, "relin_zero": (0.0, 0.0), "relin_ref": (1.75e-2, 5.0e-3)}


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
    masks = np.zeros(ITERS, np.uint32)
    relin = SIDES[side]
    rl = capi.WindowRelin(*relin) if relin is not None else None

    def call(h):
        if rl is None:
            rc = L.mh_icp_window_optimise(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), C.byref(out_res),
                                          capi._p(trace))
        else:
            rc = L.mh_icp_window_optimise_relin(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), C.byref(rl),
                                                C.byref(out_res), capi._p(trace), capi._p(masks))
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
    if rl is not None:
        out["evaluated_masks"] = [int(m) for m in masks]
        out["mean_factors_evaluated_per_iter"] = round(float(np.mean([bin(int(m)).count("1") for m in masks])), 3)
    base.destroy()
    gm.release()
    ctx.close()
    return out


def kernel_stats(db_path: str) -> None:
    """the per-kernel table of a rocprofv3 kernel trace (the `kernels` view of its rocpd database: name, start, end in ns)"""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                      "order by sum(end - start) desc").fetchall()
    print("kernel-trace summary of: python tools/icp_window_relin_time.py --one 24576 --side relin_ref --repeats 20 (rocprofv3 --kernel-trace; durations in ns)")
    print("%-100s %8s %10s %10s %10s" % ("kernel", "calls", "avg", "min", "max"))
    for name, calls, avg, lo, hi in rows:
        print("%-100s %8d %10.0f %10d %10d" % (name[:100], calls, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--one", type=int, default=0, help="run one size and one side in this process and print its JSON")
    ap.add_argument("--side", default="relin_ref", choices=list(SIDES))
    ap.add_argument("--kernel-stats", default="", help="reduce this rocprofv3 database to the per-kernel table and print it")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
        return
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "icp_window_relin_time", "relin_ref": list(SIDES["relin_ref"]), "sizes": []}
    for n in (24576, 1024):
        runs = {s: [] for s in SIDES}
        for _ in range(a.pairs):
            for side in SIDES:  # alternating fresh processes
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--side", side, "--repeats", str(a.repeats)],
                                   capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-2000:])
                    sys.exit(r.returncode or 1)
                runs[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = {"points": n, "factors": W, "iters": ITERS, "repeats": a.repeats, "pairs": a.pairs}
        for side in SIDES:
            vals = [q["us_per_iter"] for q in runs[side]]
            row[side + "_us_per_iter"] = round(float(np.median(vals)), 3)
            row[side + "_us_per_iter_runs"] = vals
        row["plain_spread_us"] = round(max(row["plain_us_per_iter_runs"]) - min(row["plain_us_per_iter_runs"]), 3)
        row["relin_zero_minus_plain_us"] = round(row["relin_zero_us_per_iter"] - row["plain_us_per_iter"], 3)
        row["relin_ref_over_plain"] = round(row["relin_ref_us_per_iter"] / row["plain_us_per_iter"], 4)
        row["relin_ref_evaluated_masks"] = runs["relin_ref"][0]["evaluated_masks"]
        row["relin_ref_mean_factors_evaluated_per_iter"] = runs["relin_ref"][0]["mean_factors_evaluated_per_iter"]
        out["sizes"].append(row)
    path = os.path.join(ROOT, "profiles", "icp_window_relin_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
