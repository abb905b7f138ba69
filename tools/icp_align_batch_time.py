"""Times mh_icp_align_batch on the GPU against what a caller had before it: B mh_icp_align calls one after another on the same
clones.  B in {1, 4, 8} x {1 024, 24 576} points, 10 iterations with convergence switched off (eps = 0), every figure the median
host wall clock of one whole call (batch) or of the B calls (sequential) over --repeats repeats after warm-up, in us; each
(B, points, side) runs in a fresh child process, the sides alternating, --rounds times.

  batch   mh_icp_align_batch, everything queued at once (through ctypes with prebuilt arguments)
  seq     B x mh_icp_align in a loop on the same clones

and mh_icp_relocalise_batch against mh_icp_relocalise at the relocalisation row's configuration (729 poses, coarse stride 4,
top_k = 4, the 1 024-point cloud of synth.small_world()):

  reloc_batch   mh_icp_relocalise_batch end to end, on four clones made once
  reloc         mh_icp_relocalise end to end

Every repeat starts from the same warm association state (clones of one factor linearized once; the relocalise calls reset their
factors themselves).  Writes profiles/icp_align_batch_time.json (or --out) and prints it.  On a shared machine run it as one step
under its own limit:

  timeout -k 10 900 python tools/icp_align_batch_time.py
  rocprofv3 --kernel-trace --stats -d profiles/align_batch_trace -o t -- python tools/icp_align_batch_time.py --one 4 --points 1024 --side batch --repeats 20
  python tools/icp_align_batch_time.py --reduce profiles/align_batch_trace > profiles/icp_align_batch_kernel_stats.txt

  python tools/icp_align_batch_time.py [--repeats N] [--rounds R] [--out PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS = 10
BATCHES = (1, 4, 8)
POINTS = (1024, 24576)
SIDES = ("batch", "seq")
RELOC_SIDES = ("reloc_batch", "reloc")


def one_align(B: int, n_pts: int, side: str, repeats: int) -> dict:
    from mimosa_amd import capi, synth

    ctx = capi.Context(0)
    gm = capi.VoxelMap(ctx)
    gm.insert(synth.make_room(synth.BASE_SEED, 0, 0))
    scan, _ = synth.make_scan(64)
    pts = np.ascontiguousarray(scan[:: max(1, len(scan) // n_pts)][:n_pts])
    base = capi.ICPFactor(ctx, gm, pts, capi.make_reg_config(**synth.enwide_config()))
    base.set_components(False)
    R0, t0 = synth.query_pose()
    g = np.array([0.0, 0.0, -1.0])
    base.linearize(R0, t0, g)
    L = ctx.L
    cfg = capi.make_align_config(max_iters=ITERS, eps_rot=0.0, eps_trans=0.0, damping=1e-9, check_every=0)
    # member i starts a few centimetres from the query pose, each elsewhere
    R = np.ascontiguousarray(np.tile(R0.reshape(9), (B, 1)))
    t = np.ascontiguousarray(np.stack([t0 + 0.02 * np.array([np.cos(i), np.sin(i), 0.0]) for i in range(B)]))
    outs = (capi.AlignResult * B)()
    t_us = []
    for i in range(repeats + 5):
        fs = [base.clone() for _ in range(B)]
        handles = (C.c_void_p * B)(*[f.h for f in fs])
        a = time.perf_counter()
        if side == "batch":
            rc = L.mh_icp_align_batch(handles, B, capi._p(R), capi._p(t), capi._p(g), C.byref(cfg), outs)
        else:
            rc = 0
            for m in range(B):
                rc |= L.mh_icp_align(fs[m].h, capi._p(R[m]), capi._p(t[m]), capi._p(g), C.byref(cfg), C.byref(outs[m]))
        b = time.perf_counter()
        assert rc == 0 and all(outs[m].iters == ITERS for m in range(B))
        for f in fs:
            f.destroy()
        if i >= 5:
            t_us.append((b - a) * 1e6)
    base.destroy()
    gm.release()
    ctx.close()
    return {"B": B, "points": n_pts, "side": side, "iters": ITERS, "repeats": repeats, "us": round(float(np.median(t_us)), 3)}


def one_reloc(side: str, repeats: int) -> dict:
    from mimosa_amd import capi, synth

    ctx = capi.Context(0)
    m, pts, aux = synth.small_world()
    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    f = capi.ICPFactor(ctx, gm, pts, capi.make_reg_config(**synth.enwide_config()))
    f.set_components(False)
    Rg, tg = aux["R_W_L"], aux["t_W_L"]
    R0, t0 = synth.rot_z(np.deg2rad(20.0)) @ Rg, tg + np.array([1.2, -0.9, 0.0])
    Rs, ts = capi.pose_grid(R0, t0, 2.0, 0.5, np.deg2rad(30.0), np.deg2rad(7.5))
    acfg = capi.make_align_config(max_iters=30, eps_rot=1e-9, eps_trans=1e-9, damping=1e-9)
    cfg = capi.make_reloc_config(gate=1.0, stride=4, top_k=4, align=acfg, final_gate=0.1)
    t_us = []
    for i in range(repeats + 5):
        a = time.perf_counter()
        r = f.relocalise(Rs, ts, cfg, batch=(side == "reloc_batch"))  # (the clones are made in the first warm-up repeat)
        b = time.perf_counter()
        if i >= 5:
            t_us.append((b - a) * 1e6)
    out = {"side": side, "points": len(pts), "n_poses": len(Rs), "repeats": repeats, "us": round(float(np.median(t_us)), 3),
           "winner_m_from_truth": float(np.linalg.norm(r["t"] - tg)), "align_iters": [c["iters"] for c in r["cand"]]}
    f.destroy()
    gm.release()
    ctx.close()
    return out


def child(args, timeout=240) -> dict:
    import subprocess
    print("icp_align_batch_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def reduce_trace(path: str):
    """the per-kernel table of a rocprofv3 --kernel-trace run (its rocpd database: the `kernels` view, start / end in ns)"""
    import sqlite3
    dbs = sorted(glob.glob(os.path.join(path, "**", "*.db"), recursive=True)) if os.path.isdir(path) else [path]
    if not dbs:
        sys.exit("no rocpd database under " + path)
    db = sqlite3.connect(dbs[-1])
    rows = db.execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                      "order by sum(end - start) desc").fetchall()
    print("kernel-trace summary of: python tools/icp_align_batch_time.py --one 4 --points 1024 --side batch --repeats 20 "
          "(rocprofv3 --kernel-trace --stats; durations in ns)")
    print("%-100s %8s %10s %10s %10s" % ("kernel", "calls", "avg", "min", "max"))
    for name, calls, avg, lo, hi in rows:
        print("%-100s %8d %10.0f %10d %10d" % (name[:100], calls, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_align_batch_time.json"))
    ap.add_argument("--one", type=int, default=0, help="run one batch size and one side in this process and print its JSON (B; ignored by the reloc sides)")
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--side", default="batch", choices=SIDES + RELOC_SIDES)
    ap.add_argument("--reduce", default="", help="print the per-kernel table of a rocprofv3 kernel trace (directory or database)")
    a = ap.parse_args()
    if a.reduce:
        reduce_trace(a.reduce)
        return
    if a.one:
        print(json.dumps(one_reloc(a.side, a.repeats) if a.side in RELOC_SIDES else one_align(a.one, a.points, a.side, a.repeats)))
        return
    out = {"tool": "icp_align_batch_time", "iters": ITERS, "sizes": [], "relocalise": {}}
    for n in POINTS:
        for B in BATCHES:
            runs = {s: [] for s in SIDES}
            for _ in range(a.rounds):
                for side in SIDES:  # alternating fresh processes
                    runs[side].append(child(["--one", str(B), "--points", str(n), "--side", side, "--repeats", str(a.repeats)]))
            row = {"B": B, "points": n, "repeats": a.repeats, "rounds": a.rounds}
            for side in SIDES:
                vals = [q["us"] for q in runs[side]]
                row[side + "_us"] = round(float(np.median(vals)), 3)
                row[side + "_us_runs"] = vals
            row["batch_us_per_iter"] = round(row["batch_us"] / ITERS, 3)
            row["batch_over_seq"] = round(row["batch_us"] / row["seq_us"], 4)
            out["sizes"].append(row)
    runs = {s: [] for s in RELOC_SIDES}
    for _ in range(a.rounds):
        for side in RELOC_SIDES:
            runs[side].append(child(["--one", "1", "--side", side, "--repeats", str(a.repeats)]))
    rel = {"n_poses": runs["reloc"][0]["n_poses"], "points": runs["reloc"][0]["points"], "repeats": a.repeats, "rounds": a.rounds,
           "align_iters": runs["reloc"][0]["align_iters"], "align_iters_batch": runs["reloc_batch"][0]["align_iters"]}
    for side in RELOC_SIDES:
        vals = [q["us"] for q in runs[side]]
        rel[side + "_us"] = round(float(np.median(vals)), 3)
        rel[side + "_us_runs"] = vals
    rel["reloc_batch_over_reloc"] = round(rel["reloc_batch_us"] / rel["reloc_us"], 4)
    out["relocalise"] = rel
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
