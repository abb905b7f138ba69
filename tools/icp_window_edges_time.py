"""Times mh_icp_window_optimise_edges on the GPU against mh_icp_window_optimise_lin with n_lin = 0: W = 5 factors of 24 576 and of
1 024 points, the replay's 6 iterations, its between sigmas, the tight prior and a damping of 1e-9 (the set-up and the
protocol of tools/icp_window_lin_time.py).  Four sides, every figure the median host wall clock of one whole optimisation over
--repeats repeats after warm-up, per iteration in us:

  lin     mh_icp_window_optimise_lin, n_lin = 0 (the yardstick, of the same library)
  edges0  mh_icp_window_optimise_edges without an edge (dispatches to the yardstick's step kernel: the entry point alone)
  edges2  ... with two edges of span 2, (0, 2) and (2, 4): the odometry manager's factor at every second scan
  edges8  ... with eight edges: every pair of span 2 and 3, one of span 4, two on one pair

The edges: the start poses' own relative pose, dense SPD information matrices with eigenvalues 1e2 .. 1e6.  Every repeat starts
from the same warm association state (clones of a factor linearized once).  The sides alternate in fresh child processes,
--pairs rounds per size, each child under a time limit; a failed child ends the run.  The spread of `lin` over its rounds is
what a difference has to exceed to count.

Writes profiles/icp_window_edges_time.json (or --out) and prints it.

  python tools/icp_window_edges_time.py [--repeats N] [--pairs P] [--out PATH]
  the step kernel's time, from a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o edges -- python tools/icp_window_edges_time.py --one 24576 --side edges8 --repeats 20
    python tools/icp_window_lin_time.py --kernel-stats OUT/edges_results.db > profiles/icp_window_edges_kernel_stats.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from icp_window_time import ITERS, W, expmap  # noqa: E402

PAIRS = {"lin": None, "edges0": [], "edges2": [(0, 2), (2, 4)], "edges8": [(0, 2), (1, 3), (2, 4), (0, 3), (1, 4), (0, 4), (2, 4), (1, 3)]}


def edges(capi, pairs, poses0):
    rng = np.random.default_rng(13)
    out = []
    for a, b in pairs:
        (Ra, ta), (Rb, tb) = poses0[a], poses0[b]
        Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
        Om = (Q * np.logspace(2, 6, 6)) @ Q.T
        out.append(dict(a=a, b=b, Z=(Ra.T @ Rb, Ra.T @ (tb - ta)), info=(Om + Om.T) / 2))
    return capi.make_window_edge(out)


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
    pairs = PAIRS[side]
    ed = edges(capi, pairs, poses0) if pairs is not None else None

    def call(h):
        if ed is None:
            rc = L.mh_icp_window_optimise_lin(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), None, None, 0,
                                              C.byref(out_res), capi._p(trace), None)
        else:
            rc = L.mh_icp_window_optimise_edges(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), None, None, 0, ed,
                                                len(pairs), C.byref(out_res), capi._p(trace), None)
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


def child(args, timeout=240) -> dict:
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_window_edges_time.json"))
    ap.add_argument("--one", type=int, default=0, help="run one size and one side in this process and print its JSON")
    ap.add_argument("--side", default="edges8", choices=list(PAIRS))
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "icp_window_edges_time", "sizes": []}
    for n in (24576, 1024):
        runs = {s: [] for s in PAIRS}
        for _ in range(a.pairs):
            for side in PAIRS:  # alternating fresh processes
                runs[side].append(child(["--one", str(n), "--side", side, "--repeats", str(a.repeats)]))
        row = {"points": n, "factors": W, "iters": ITERS, "repeats": a.repeats, "pairs": a.pairs}
        for side in PAIRS:
            vals = [q["us_per_iter"] for q in runs[side]]
            row[side + "_us_per_iter"] = round(float(np.median(vals)), 3)
            row[side + "_us_per_iter_runs"] = vals
        row["lin_spread_us"] = round(max(row["lin_us_per_iter_runs"]) - min(row["lin_us_per_iter_runs"]), 3)
        for side in ("edges0", "edges2", "edges8"):
            row[side + "_minus_lin_us"] = round(row[side + "_us_per_iter"] - row["lin_us_per_iter"], 3)
        out["sizes"].append(row)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
