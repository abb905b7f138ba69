"""Times mh_pose_graph_covariances on the GPU: `cov` alone and `cov` with 64 pairs, against ONE iteration of
mh_pose_graph_optimise on the same graph (the natural unit: the call is an iteration's assembly and factorisation plus the
recursion, the correction and the pairs' columns) and against the restatement's route on the host, a sparse LU of A
(scipy.sparse.linalg.splu) and 64 columns of A^-1 from it.  cov needs 6 n columns; the host figure for that is SCALED from the
64 measured ones (`host_cov_scaled_ms`), not measured.  Every figure is a median host wall clock in ms after warm-up.

Sizes: 512 poses with 2 far edges, 4 096 with 2, 4 096 with 32 (the graphs of tools/pose_graph_time.py).  The sides alternate in
fresh child processes, --rounds rounds, one GPU process at a time, each child under a time limit; a failed child ends the run.
Kernel times come from one rocprofv3 --kernel-trace --stats run of its own (a fresh process: two calls with 64 pairs at 4 096
poses and 32 far edges).  Writes profiles/pose_graph_cov_time.json and profiles/pose_graph_cov_kernel_stats.txt and prints the
JSON.  On a shared machine run it as one step under its own limit:

  timeout -k 10 1100 python tools/pose_graph_cov_time.py

  python tools/pose_graph_cov_time.py [--repeats N] [--rounds R] [--out PATH] [--stats-out PATH] [--no-trace]
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

import pose_graph_time as base  # noqa: E402  (the graphs)

SIDES = ("device", "host")
WARMUP = 2
HOST_COLUMNS = 64


def pairs_of(n: int):
    return [(1 + (k * (n - 3)) // 64, min(n - 1, 2 + (k * (n - 3)) // 64 + (k % 8) * (n // 16))) for k in range(64)]


def device_graph(c):
    from mimosa_amd import capi
    ctx = capi.Context(0)
    pg = capi.PoseGraph(ctx, len(c["R"]), len(c["edges"]))
    pg.set_poses(c["R"], c["t"])
    pg.set_fixed(c["fixed"])
    pg.set_edges(base.as_dicts(c["edges"]))
    return ctx, pg


def one(n: int, n_far: int, side: str, repeats: int) -> dict:
    c = base.graph(n, n_far)
    if side == "host":
        import pose_graph_cov_ref as cref
        import scipy.sparse.linalg as spl
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            A = cref.sparse_system(dict(c, priors=[], edge_loss=None))
            t1 = time.perf_counter()
            lu = spl.splu(A)
            E = np.zeros((6 * n, HOST_COLUMNS))
            E[6 * (n // 2) + np.arange(HOST_COLUMNS), np.arange(HOST_COLUMNS)] = 1.0
            lu.solve(E)
            ms.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        return {"assemble_ms": float(np.median([m[0] for m in ms])), "ms": float(np.median([m[1] for m in ms]))}
    from mimosa_amd import capi
    ctx, pg = device_graph(c)
    pairs = pairs_of(n)
    cfg = capi.make_pose_graph_config(iters=1, check_every=0, damping=0.0, eps_rot=0.0, eps_trans=0.0)
    out = {}
    for name, call in (("cov", lambda: pg.covariances(0.0)), ("cov_pairs64", lambda: pg.covariances(0.0, pairs)), ("iteration", lambda: pg.optimise(cfg))):
        ms = []
        for k in range(WARMUP + repeats):
            pg.set_poses(c["R"], c["t"])
            t0 = time.perf_counter()
            got = call()
            if k >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
        if name != "iteration":
            assert got[2]["flags"] == 0 and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        out[name + "_ms"] = float(np.median(ms))
    pg.destroy()
    ctx.close()
    return out


def traced() -> None:
    c = base.graph(4096, 32)
    ctx, pg = device_graph(c)
    for _ in range(2):
        pg.covariances(0.0, pairs_of(4096))
    pg.destroy()
    ctx.close()


def child(args, timeout=280) -> dict:
    print("pose_graph_cov_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(path: str) -> None:
    """one rocprofv3 --kernel-trace --stats run of `--traced` in a fresh process; the per-kernel table of its rocpd database"""
    import sqlite3
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="pose_graph_cov_trace_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "pgo", "--", sys.executable, os.path.abspath(__file__), "--traced"]
        print("pose_graph_cov_time:", " ".join(cmd), file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(r.returncode or 1)
        dbs = sorted(glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True))
        if not dbs:
            sys.exit("pose_graph_cov_time: no rocpd database under " + tmp)
        rows = sqlite3.connect(dbs[-1]).execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                                                "order by sum(end - start) desc").fetchall()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(path, "w") as f:
        f.write("kernel-trace summary of: python tools/pose_graph_cov_time.py --traced (rocprofv3 --kernel-trace --stats; durations in ns):\n"
                "two mh_pose_graph_covariances calls with 64 pairs at 4 096 poses, 4 127 edges, 32 far edges\n")
        f.write("%-100s %8s %10s %10s %10s\n" % ("kernel", "calls", "avg", "min", "max"))
        for name, calls, avg, lo, hi in rows:
            f.write("%-100s %8d %10.0f %10d %10d\n" % (name[:100], calls, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_cov_time.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "pose_graph_cov_kernel_stats.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--one", action="store_true", help="run one size and side in this process and print its JSON")
    ap.add_argument("--poses", type=int, default=0)
    ap.add_argument("--far", type=int, default=0)
    ap.add_argument("--side", default="device", choices=SIDES)
    ap.add_argument("--traced", action="store_true", help="the workload of the kernel trace, in this process")
    a = ap.parse_args()
    if a.traced:
        traced()
        return
    if a.one:
        print(json.dumps(one(a.poses, a.far, a.side, a.repeats)))
        return
    out = {"tool": "pose_graph_cov_time", "cases": []}
    for n, n_far in base.SIZES:
        runs = {s: [] for s in SIDES}
        for _ in range(a.rounds):
            for side in ("host", "device"):
                runs[side].append(child(["--one", "--poses", str(n), "--far", str(n_far), "--side", side, "--repeats", str(a.repeats if side == "device" else 1)]))
        row = {"poses": n, "far_edges": n_far, "repeats": a.repeats, "rounds": a.rounds}
        for key in ("cov_ms", "cov_pairs64_ms", "iteration_ms"):
            vals = [q[key] for q in runs["device"]]
            row[key] = round(float(np.median(vals)), 3)
            row[key + "_runs"] = [round(v, 3) for v in vals]
        row["cov_over_iteration"] = round(row["cov_ms"] / row["iteration_ms"], 2)
        row["cov_pairs64_over_iteration"] = round(row["cov_pairs64_ms"] / row["iteration_ms"], 2)
        row["host_lu_and_64_columns_ms"] = round(float(np.median([q["ms"] for q in runs["host"]])), 3)
        row["host_cov_scaled_ms"] = round(row["host_lu_and_64_columns_ms"] * 6 * n / HOST_COLUMNS, 1)  # scaled, not measured
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
