"""Times place recognition on the GPU against the vectorised numpy restatement (tests/place_ref.py) doing the same work.  Every figure
is a median host wall clock over --repeats repeats after warm-up, in us.

Cases:
  add     mh_place_db_add_from_scan (describe + norms on the device, then mh_synchronize: the call itself does not wait) on the full
          cloud of a 32 x 256 scan (8 192 points) and of a 128 x 1024 scan (131 072 points), against place_ref.describe + norms
          of the same cloud
  query   mh_place_db_query with top_k = 4 on databases of 256 / 4 096 / 16 384 seeded sparse descriptors, against
          place_ref.distances + rank (--host-repeats repeats at 256, one above: it takes seconds there)

The sides alternate in fresh child processes, --rounds rounds, each child under a time limit; a failed child ends the run.  Kernel
times come from one rocprofv3 --kernel-trace --stats run of its own (a fresh process: ten adds of each size, twenty queries at 4 096),
with no counter collection in it; --no-trace leaves it out.  Writes profiles/place_time.json and profiles/place_kernel_stats.txt
(or --out / --stats-out) and prints the JSON.  On a shared machine run it as one step under its own limit:

  timeout -k 10 1100 python tools/place_time.py

  python tools/place_time.py [--repeats N] [--host-repeats N] [--rounds R] [--out PATH] [--stats-out PATH] [--no-trace]
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

ADD_SIZES = (8192, 131072)
QUERY_SIZES = (256, 4096, 16384)
SIDES = ("device", "numpy")
WARMUP = 5
TOP_K = 4
CFG = dict(r_min=0.5, r_max=40.0, z_min=-2.0, z_max=30.0, min_overlap=30)


def sparse_descriptors(m: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.1, 6.0, (m, 20, 60)).astype(np.float32)
    d *= rng.random((m, 20, 60)) < 0.25                  # a quarter of the cells occupied
    d *= (rng.random((m, 1, 60)) < 0.8)                  # a fifth of the columns empty
    return d.reshape(m, 1200)


def scan_for(ctx, n_points: int):
    from mimosa_amd import capi, synth
    if n_points == 8192:
        raw, _ = synth.make_raw_scan(32, n_cols=256, dropouts=False)
    else:
        raw, _ = synth.make_raw_scan(128, dropouts=False)
    assert len(raw) == n_points
    sc = capi.Scan(ctx)
    sc.prepare_input(raw, capi.make_input_config())
    return sc


def one_add(n_points: int, side: str, repeats: int) -> dict:
    import place_ref as ref
    from mimosa_amd import capi
    ctx = capi.Context(0)
    sc = scan_for(ctx, n_points)
    rec = sc.points(capi.Scan.FULL)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    db = capi.PlaceDatabase(ctx, **dict(CFG, capacity=repeats + WARMUP + 1))
    want = ref.describe(xyz, np.eye(3), CFG)
    out = {"case": "add", "n_points": int(len(xyz)), "side": side, "repeats": repeats, "occupied_cells": int((want > 0).sum())}
    t_us = []
    for i in range(repeats + WARMUP):
        if side == "device":
            ctx.synchronize()
            a = time.perf_counter()
            db.add_from_scan(sc, capi.Scan.FULL, tag=i)
            ctx.synchronize()
            b = time.perf_counter()
        else:
            a = time.perf_counter()
            d = ref.describe(xyz, np.eye(3), CFG)
            ref.norms(d)
            b = time.perf_counter()
        if i >= WARMUP:
            t_us.append((b - a) * 1e6)
    if side == "device" and not np.array_equal(db.get(db.size() - 1)[0].view(np.uint32), want.view(np.uint32)):
        sys.exit("place_time: the device's descriptor is not the restatement's")
    out["us"] = round(float(np.median(t_us)), 3)
    db.destroy()
    sc.destroy()
    ctx.close()
    return out


def one_query(m: int, side: str, repeats: int) -> dict:
    import place_ref as ref
    from mimosa_amd import capi
    E = sparse_descriptors(m, 100 + m)
    q = sparse_descriptors(1, 7)[0]
    out = {"case": "query", "entries": m, "side": side, "repeats": repeats, "top_k": TOP_K}
    ctx = capi.Context(0)
    db = capi.PlaceDatabase(ctx, **dict(CFG, capacity=m))
    for i in range(m):
        db.add(E[i], i)
    hits, all_ = db.query(q, top_k=TOP_K, want_all=True)
    t_us = []
    if side == "device":
        for i in range(repeats + WARMUP):
            a = time.perf_counter()
            h2, _ = db.query(q, top_k=TOP_K)
            b = time.perf_counter()
            if i >= WARMUP:
                t_us.append((b - a) * 1e6)
        if not np.array_equal(h2, hits):
            sys.exit("place_time: a repeat answered differently")
    else:
        for i in range(repeats):
            a = time.perf_counter()
            D, shift, _ = ref.distances(q, E, CFG["min_overlap"])
            want = ref.rank(D, TOP_K)
            b = time.perf_counter()
            t_us.append((b - a) * 1e6)
        err = float(np.abs(all_["dist"] - D).max())
        if err > 1e-12 or hits["index"].tolist() != want.tolist():
            sys.exit("place_time: the sides disagree: %g, %r against %r" % (err, hits["index"].tolist(), want.tolist()))
        out["largest_D_difference"] = err
    out["us"] = round(float(np.median(t_us)), 3)
    out["hits"] = hits["index"].tolist()
    db.destroy()
    ctx.close()
    return out


def traced() -> None:
    """what the kernel trace records: one process, adds of both sizes and queries at 4 096 entries"""
    from mimosa_amd import capi
    ctx = capi.Context(0)
    db = capi.PlaceDatabase(ctx, **dict(CFG, capacity=4096))
    for n in ADD_SIZES:
        sc = scan_for(ctx, n)
        for i in range(10):
            db.add_from_scan(sc, capi.Scan.FULL, tag=i)
        ctx.synchronize()
        sc.destroy()
    E = sparse_descriptors(4096 - db.size(), 100)
    for i in range(len(E)):
        db.add(E[i], i)
    q = sparse_descriptors(1, 7)[0]
    for _ in range(20):
        db.query(q, top_k=TOP_K)
    db.destroy()
    ctx.close()


def child(args, timeout=280) -> dict:
    print("place_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(path: str) -> None:
    """one rocprofv3 --kernel-trace --stats run of `--traced` in a fresh process; the per-kernel table of its rocpd database"""
    import sqlite3
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="place_trace_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "place", "--", sys.executable, os.path.abspath(__file__), "--traced"]
        print("place_time:", " ".join(cmd), file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(r.returncode or 1)
        dbs = sorted(glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True))
        if not dbs:
            sys.exit("place_time: no rocpd database under " + tmp)
        rows = sqlite3.connect(dbs[-1]).execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                                                "order by sum(end - start) desc").fetchall()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(path, "w") as f:
        f.write("kernel-trace summary of: python tools/place_time.py --traced (rocprofv3 --kernel-trace --stats; durations in ns): 10 adds from a\n"
                "8 192-point and 10 from a 131 072-point scan, 4 076 host adds, 20 queries of 4 096 entries with top_k = 4\n")
        f.write("%-100s %8s %10s %10s %10s\n" % ("kernel", "calls", "avg", "min", "max"))
        for name, calls, avg, lo, hi in rows:
            f.write("%-100s %8d %10.0f %10d %10d\n" % (name[:100], calls, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_time.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "place_kernel_stats.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--one", default="", choices=("", "add", "query"), help="run one case, size and side in this process and print its JSON")
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--side", default="device", choices=SIDES)
    ap.add_argument("--traced", action="store_true", help="the workload of the kernel trace, in this process")
    a = ap.parse_args()
    if a.traced:
        traced()
        return
    if a.one:
        print(json.dumps((one_add if a.one == "add" else one_query)(a.size, a.side, a.repeats)))
        return
    out = {"tool": "place_time", "config": CFG, "top_k": TOP_K, "add": [], "query": []}
    for case, sizes in (("add", ADD_SIZES), ("query", QUERY_SIZES)):
        for n in sizes:
            runs = {s: [] for s in SIDES}
            host_repeats = a.repeats if case == "add" else (a.host_repeats if n <= 256 else 1)
            for _ in range(a.rounds):
                for side in SIDES:  # alternating fresh processes
                    runs[side].append(child(["--one", case, "--size", str(n), "--side", side, "--repeats", str(a.repeats if side == "device" else host_repeats)]))
            row = {("n_points" if case == "add" else "entries"): n, "repeats": a.repeats, "numpy_repeats": host_repeats, "rounds": a.rounds}
            for side in SIDES:
                vals = [q["us"] for q in runs[side]]
                row[side + "_us"] = round(float(np.median(vals)), 3)
                row[side + "_us_runs"] = vals
            row["numpy_over_device"] = round(row["numpy_us"] / row["device_us"], 2)
            if case == "query":
                row["largest_D_difference"] = max(q["largest_D_difference"] for q in runs["numpy"])
            out[case].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not a.no_trace:
        kernel_stats(a.stats_out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
