"""Times mh_pose_graph_optimise on the GPU against the numpy restatement (tests/pose_graph_ref.py) with the system assembled sparse
and solved by scipy.sparse.linalg.spsolve on the host.  Every figure is a median host wall clock, in ms, of ONE optimise call of
--iters iterations with convergence off (eps = 0), after warm-up.

Sizes: 512 poses with 2 far edges, 4 096 poses with 2 far edges, 4 096 poses with 32 far edges: seeded circuits as in
tests/pose_graph_cases.py (odometry chain, loops, dense information matrices, pose 0 fixed, start = integrated odometry).  The
host side reports its whole iteration and, separately, the time inside spsolve alone: the rest of it is the per-edge Python
loop of the restatement, which a C++ host would not pay.

The sides alternate in fresh child processes, --rounds rounds, one GPU process at a time, each child under a time limit; a failed
child ends the run.  Kernel times come from one rocprofv3 --kernel-trace --stats run of its own (a fresh process: two calls of
--iters iterations at 4 096 poses and 32 far edges), with no counter collection in it; --no-trace leaves it out.  Writes
profiles/pose_graph_time.json and profiles/pose_graph_kernel_stats.txt (or --out / --stats-out) and prints the JSON.  On a
shared machine run it as one step under its own limit:

  timeout -k 10 1100 python tools/pose_graph_time.py

  python tools/pose_graph_time.py [--iters K] [--repeats N] [--host-repeats N] [--rounds R] [--out PATH] [--stats-out PATH] [--no-trace]
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

SIZES = ((512, 2), (4096, 2), (4096, 32))
SIDES = ("device", "scipy")
WARMUP = 2


def graph(n: int, n_far: int) -> dict:
    import pose_graph_cases as cases
    if n_far == 2:
        loops = [(0, n - 1), (n // 4, 3 * n // 4)]
    else:
        loops = [(0, n - 1)] + [(k * (n // 2) // n_far, n - 1 - k * (n // 2) // n_far) for k in range(1, n_far)]
    assert len(loops) == n_far and all(b - a >= 2 for a, b in loops)
    return cases.circuit(n, 1000 + n + n_far, loops=loops)


def sparse_optimise(c: dict, iters: int):
    """ref.optimise with the system assembled in 6 x 6 blocks into a sparse matrix: (poses, seconds inside spsolve)"""
    import pose_graph_ref as ref
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    R, t, fixed = [x.copy() for x in c["R"]], [x.copy() for x in c["t"]], c["fixed"]
    n, in_solve = len(R), 0.0
    for _ in range(iters):
        rows, cols, vals, g = [], [], [], np.zeros(6 * n)

        def add(i, j, B):
            rr, cc = np.meshgrid(np.arange(6 * i, 6 * i + 6), np.arange(6 * j, 6 * j + 6), indexing="ij")
            rows.append(rr.ravel()), cols.append(cc.ravel()), vals.append(B.ravel())

        for a, b, ZR, Zt, Om in c["edges"]:
            r, Ja = ref.edge_terms(R[a], t[a], R[b], t[b], ZR, Zt)
            if not fixed[a]:
                add(a, a, Ja.T @ Om @ Ja)
                g[6 * a:6 * a + 6] += Ja.T @ Om @ r
            if not fixed[b]:
                add(b, b, Om)
                g[6 * b:6 * b + 6] += Om @ r
            if not fixed[a] and not fixed[b]:
                add(b, a, Om @ Ja)
                add(a, b, (Om @ Ja).T)
        for i in np.flatnonzero(fixed):
            add(int(i), int(i), np.eye(6))
        A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n))
        t0 = time.perf_counter()
        xi = spsolve(A, -g).reshape(-1, 6)
        in_solve += time.perf_counter() - t0
        for i in range(n):
            if not fixed[i]:
                t[i] = t[i] + R[i] @ xi[i, 3:]
                R[i] = R[i] @ ref.so3_exp(xi[i, :3])
    return np.array(R), np.array(t), in_solve


def as_dicts(edges):
    return [{"a": a, "b": b, "Z": (ZR, Zt), "info": Om} for a, b, ZR, Zt, Om in edges]


def one(n: int, n_far: int, side: str, iters: int, repeats: int) -> dict:
    c = graph(n, n_far)
    if side == "scipy":
        ms, solve_ms = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            R, t, in_solve = sparse_optimise(c, iters)
            ms.append((time.perf_counter() - t0) * 1e3)
            solve_ms.append(in_solve * 1e3)
        np.save(os.path.join(tempfile.gettempdir(), "pose_graph_time_%d_%d.npy" % (n, n_far)), np.concatenate([R.reshape(-1, 9), t], axis=1))
        return {"ms": float(np.median(ms)), "spsolve_ms": float(np.median(solve_ms))}
    import pose_graph_ref as ref
    from mimosa_amd import capi
    ctx = capi.Context(0)
    pg = capi.PoseGraph(ctx, n, len(c["edges"]))
    pg.set_poses(c["R"], c["t"])
    pg.set_fixed(c["fixed"])
    pg.set_edges(as_dicts(c["edges"]))
    cfg = capi.make_pose_graph_config(iters=iters, check_every=0, damping=0.0, eps_rot=0.0, eps_trans=0.0)
    ms = []
    for k in range(WARMUP + repeats):
        pg.set_poses(c["R"], c["t"])
        t0 = time.perf_counter()
        got = pg.optimise(cfg)
        if k >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert got["iters"] == iters and all(q["flags"] == 0 for q in got["trace"])
    out = {"ms": float(np.median(ms)), "f_first": got["f_first"], "f_last": got["f_last"], "last_step_trans": got["trace"][-1]["step_trans"]}
    path = os.path.join(tempfile.gettempdir(), "pose_graph_time_%d_%d.npy" % (n, n_far))
    if os.path.exists(path):  # the host side of an earlier round left its result: how far apart the two are
        P = np.load(path)
        out["to_scipy_m"], out["to_scipy_rad"] = ref.pose_error(got["R"], got["t"], P[:, :9], P[:, 9:])
    pg.destroy()
    ctx.close()
    return out


def traced(iters: int) -> None:
    from mimosa_amd import capi
    c = graph(4096, 32)
    ctx = capi.Context(0)
    pg = capi.PoseGraph(ctx, 4096, len(c["edges"]))
    pg.set_poses(c["R"], c["t"])
    pg.set_fixed(c["fixed"])
    pg.set_edges(as_dicts(c["edges"]))
    for _ in range(2):
        pg.set_poses(c["R"], c["t"])
        pg.optimise(capi.make_pose_graph_config(iters=iters, eps_rot=0.0, eps_trans=0.0))
    pg.destroy()
    ctx.close()


def child(args, timeout=280) -> dict:
    print("pose_graph_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(path: str, iters: int) -> None:
    """one rocprofv3 --kernel-trace --stats run of `--traced` in a fresh process; the per-kernel table of its rocpd database"""
    import sqlite3
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="pose_graph_trace_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "pgo", "--", sys.executable, os.path.abspath(__file__), "--traced", "--iters", str(iters)]
        print("pose_graph_time:", " ".join(cmd), file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(r.returncode or 1)
        dbs = sorted(glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True))
        if not dbs:
            sys.exit("pose_graph_time: no rocpd database under " + tmp)
        rows = sqlite3.connect(dbs[-1]).execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                                                "order by sum(end - start) desc").fetchall()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(path, "w") as f:
        f.write("kernel-trace summary of: python tools/pose_graph_time.py --traced --iters %d (rocprofv3 --kernel-trace --stats; durations in ns):\n"
                "two mh_pose_graph_optimise calls at 4 096 poses, 4 127 edges, 32 far edges\n" % iters)
        f.write("%-100s %8s %10s %10s %10s\n" % ("kernel", "calls", "avg", "min", "max"))
        for name, calls, avg, lo, hi in rows:
            f.write("%-100s %8d %10.0f %10d %10d\n" % (name[:100], calls, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_time.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "pose_graph_kernel_stats.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--one", action="store_true", help="run one size and side in this process and print its JSON")
    ap.add_argument("--poses", type=int, default=0)
    ap.add_argument("--far", type=int, default=0)
    ap.add_argument("--side", default="device", choices=SIDES)
    ap.add_argument("--traced", action="store_true", help="the workload of the kernel trace, in this process")
    a = ap.parse_args()
    if a.traced:
        traced(a.iters)
        return
    if a.one:
        print(json.dumps(one(a.poses, a.far, a.side, a.iters, a.repeats)))
        return
    out = {"tool": "pose_graph_time", "iters": a.iters, "cases": []}
    for n, n_far in SIZES:
        runs = {s: [] for s in SIDES}
        for _ in range(a.rounds):
            for side in ("scipy", "device"):  # alternating fresh processes; the host side first: the device side measures its distance to it
                runs[side].append(child(["--one", "--poses", str(n), "--far", str(n_far), "--side", side, "--iters", str(a.iters), "--repeats",
                                         str(a.repeats if side == "device" else a.host_repeats)]))
        row = {"poses": n, "far_edges": n_far, "edges": n - 1 + n_far, "repeats": a.repeats, "scipy_repeats": a.host_repeats, "rounds": a.rounds}
        for side in SIDES:
            vals = [q["ms"] for q in runs[side]]
            row[side + "_ms"] = round(float(np.median(vals)), 3)
            row[side + "_ms_runs"] = [round(v, 3) for v in vals]
        row["spsolve_alone_ms"] = round(float(np.median([q["spsolve_ms"] for q in runs["scipy"]])), 3)
        row["scipy_over_device"] = round(row["scipy_ms"] / row["device_ms"], 2)
        row["spsolve_alone_over_device"] = round(row["spsolve_alone_ms"] / row["device_ms"], 2)
        last = runs["device"][-1]
        row.update({k: last[k] for k in ("f_first", "f_last", "last_step_trans", "to_scipy_m", "to_scipy_rad") if k in last})
        out["cases"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not a.no_trace:
        kernel_stats(a.stats_out, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
