"""Times mh_pose_graph_optimise on a WIDE graph (mh_pose_graph_create_wide) on the GPU, by the protocol of tools/pose_graph_time.py:
every figure is a median host wall clock, in ms, of ONE optimise call of --iters iterations with convergence off (eps = 0),
after warm-up; the sides alternate in fresh child processes, --rounds rounds, one GPU process at a time, each child under a time
limit; a failed child ends the run.

Sizes: 512 and 4 096 poses with 32, 128 and 512 far edges.  The 32-edge graphs are those of tools/pose_graph_time.py; the others
take their loops from tests/pose_graph_wide_cases.wide_loops.  Sides: "wide" (a graph created wide for exactly the case's far
edges), "plain" (mh_pose_graph_create; 32 far edges only: the non-regression comparison, whose bar is the spread between the
plain side's own rounds), "scipy" (the restatement with the system assembled sparse and solved by scipy.sparse.linalg.spsolve:
its whole iteration and the time inside spsolve alone).  At every size the wide side also records the distance of its final
poses to the sparse restatement's.

Kernel times come from rocprofv3 --kernel-trace --stats runs of their own (a fresh process each: one call of --iters iterations on
a wide graph of 4 096 poses, per far-edge count), with no counter collection in them; --no-trace leaves them out.  Writes
profiles/pose_graph_wide_time.json and profiles/pose_graph_wide_kernel_stats.txt (or --out / --stats-out) and prints the JSON.  On
a shared machine run it as one step under its own limit:

  timeout -k 10 1100 python tools/pose_graph_wide_time.py
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = ((512, 32), (512, 128), (512, 512), (4096, 32), (4096, 128), (4096, 512))
SIDES = ("wide", "plain", "scipy")
WARMUP = 2


def graph(n: int, n_far: int) -> dict:
    import pose_graph_cases as cases
    import pose_graph_time as plain_tool
    import pose_graph_wide_cases as wide_cases
    if n_far <= 32:
        return plain_tool.graph(n, n_far)
    return cases.circuit(n, 1000 + n + n_far, loops=wide_cases.wide_loops(n, n_far, 2000 + n + n_far))


def as_dicts(edges):
    return [{"a": a, "b": b, "Z": (ZR, Zt), "info": Om} for a, b, ZR, Zt, Om in edges]


def device_graph(ctx, c, n_far, side):
    from mimosa_amd import capi
    pg = capi.PoseGraph(ctx, len(c["R"]), len(c["edges"]), max_far=n_far if side == "wide" else None)
    pg.set_poses(c["R"], c["t"])
    pg.set_fixed(c["fixed"])
    pg.set_edges(as_dicts(c["edges"]))
    return pg


def one(n: int, n_far: int, side: str, iters: int, repeats: int) -> dict:
    import pose_graph_time as plain_tool
    c = graph(n, n_far)
    path = os.path.join(tempfile.gettempdir(), "pose_graph_wide_time_%d_%d.npy" % (n, n_far))
    if side == "scipy":
        ms, solve_ms = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            R, t, in_solve = plain_tool.sparse_optimise(c, iters)
            ms.append((time.perf_counter() - t0) * 1e3)
            solve_ms.append(in_solve * 1e3)
        np.save(path, np.concatenate([R.reshape(-1, 9), t], axis=1))
        return {"ms": float(np.median(ms)), "spsolve_ms": float(np.median(solve_ms))}
    import pose_graph_ref as ref
    from mimosa_amd import capi
    ctx = capi.Context(0)
    pg = device_graph(ctx, c, n_far, side)
    cfg = capi.make_pose_graph_config(iters=iters, check_every=0, damping=0.0, eps_rot=0.0, eps_trans=0.0)
    ms = []
    for k in range(WARMUP + repeats):
        pg.set_poses(c["R"], c["t"])
        t0 = time.perf_counter()
        got = pg.optimise(cfg)
        if k >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert got["iters"] == iters and all(q["flags"] == 0 for q in got["trace"]) and got["n_far"] == n_far
    out = {"ms": float(np.median(ms)), "f_first": got["f_first"], "f_last": got["f_last"], "last_step_trans": got["trace"][-1]["step_trans"]}
    if os.path.exists(path):  # the host side of this round left its result: how far apart the two are
        P = np.load(path)
        out["to_scipy_m"], out["to_scipy_rad"] = ref.pose_error(got["R"], got["t"], P[:, :9], P[:, 9:])
    pg.destroy()
    ctx.close()
    return out


def traced(n_far: int, iters: int) -> None:
    from mimosa_amd import capi
    c = graph(4096, n_far)
    ctx = capi.Context(0)
    pg = device_graph(ctx, c, n_far, "wide")
    pg.optimise(capi.make_pose_graph_config(iters=iters, eps_rot=0.0, eps_trans=0.0))
    pg.destroy()
    ctx.close()


def child(args, timeout=280) -> dict:
    print("pose_graph_wide_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(f, n_far: int, iters: int) -> None:
    """one rocprofv3 --kernel-trace --stats run of `--traced` in a fresh process; the per-kernel table of its rocpd database"""
    import sqlite3
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="pose_graph_wide_trace_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "pgo", "--", sys.executable, os.path.abspath(__file__), "--traced", "--far", str(n_far),
               "--iters", str(iters)]
        print("pose_graph_wide_time:", " ".join(cmd), file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(r.returncode or 1)
        dbs = sorted(glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True))
        if not dbs:
            sys.exit("pose_graph_wide_time: no rocpd database under " + tmp)
        rows = sqlite3.connect(dbs[-1]).execute("select name, count(*), sum(end - start), avg(end - start), min(end - start), max(end - start) from kernels "
                                                "group by name order by sum(end - start) desc").fetchall()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    f.write("\nkernel-trace summary of: python tools/pose_graph_wide_time.py --traced --far %d --iters %d (rocprofv3 --kernel-trace --stats; durations in ns):\n"
            "one mh_pose_graph_optimise call on a wide graph of 4 096 poses and %d far edges\n" % (n_far, iters, n_far))
    f.write("%-90s %8s %12s %10s %10s %10s\n" % ("kernel", "calls", "total", "avg", "min", "max"))
    for name, calls, total, avg, lo, hi in rows:
        f.write("%-90s %8d %12d %10.0f %10d %10d\n" % (name[:90], calls, total, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_wide_time.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "pose_graph_wide_kernel_stats.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--one", action="store_true", help="run one size and side in this process and print its JSON")
    ap.add_argument("--poses", type=int, default=0)
    ap.add_argument("--far", type=int, default=0)
    ap.add_argument("--side", default="wide", choices=SIDES)
    ap.add_argument("--traced", action="store_true", help="the workload of a kernel trace, in this process")
    a = ap.parse_args()
    if a.traced:
        traced(a.far, a.iters)
        return
    if a.one:
        print(json.dumps(one(a.poses, a.far, a.side, a.iters, a.repeats)))
        return
    out = {"tool": "pose_graph_wide_time", "iters": a.iters, "cases": []}
    for n, n_far in SIZES:
        sides = [s for s in ("scipy", "plain", "wide") if s != "plain" or n_far <= 32]   # the host side first: the device sides measure their distance to it
        runs = {s: [] for s in sides}
        for _ in range(a.rounds):
            for side in sides:
                runs[side].append(child(["--one", "--poses", str(n), "--far", str(n_far), "--side", side, "--iters", str(a.iters), "--repeats",
                                         str(a.host_repeats if side == "scipy" else a.repeats)]))
        row = {"poses": n, "far_edges": n_far, "edges": n - 1 + n_far, "repeats": a.repeats, "scipy_repeats": a.host_repeats, "rounds": a.rounds}
        for side in sides:
            vals = [q["ms"] for q in runs[side]]
            row[side + "_ms"] = round(float(np.median(vals)), 3)
            row[side + "_ms_runs"] = [round(v, 3) for v in vals]
        row["wide_ms_per_iteration"] = round(row["wide_ms"] / a.iters, 3)
        row["spsolve_alone_ms"] = round(float(np.median([q["spsolve_ms"] for q in runs["scipy"]])), 3)
        row["scipy_over_wide"] = round(row["scipy_ms"] / row["wide_ms"], 2)
        row["spsolve_alone_over_wide"] = round(row["spsolve_alone_ms"] / row["wide_ms"], 2)
        if "plain" in runs:
            vals = row["plain_ms_runs"]
            row["plain_spread"] = round((max(vals) - min(vals)) / row["plain_ms"], 5)      # the bar: what two runs of the plain graph differ by
            row["wide_over_plain"] = round(row["wide_ms"] / row["plain_ms"], 5)
            row["wide_within_plain_spread"] = bool(row["wide_ms"] <= row["plain_ms"] * (1.0 + row["plain_spread"]))
        last = runs["wide"][-1]
        row.update({k: last[k] for k in ("f_first", "f_last", "last_step_trans", "to_scipy_m", "to_scipy_rad") if k in last})
        out["cases"].append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # after every size: a run that is cut short leaves what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
    if not a.no_trace:
        with open(a.stats_out, "w") as f:
            f.write("per-kernel times of a wide pose graph, 4 096 poses (tools/pose_graph_wide_time.py)\n")
            for n_far in (32, 128, 512):
                kernel_stats(f, n_far, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
