"""Times the blocking mh_icp_window_marginalise on the GPU against one synchronous mh_icp_linearize (components off) of the same
oldest factor in the same library — the call's floor: it runs that factor's K3 and adds one one-wave kernel behind it.  W = 5
factors of 24 576 and of 1 024 points, the replay's between sigmas on every consecutive pair, the loose prior and a damping of
1e-9 (the set-up of tools/icp_window_edges_time.py).  Every figure is the median host wall clock of one call over --repeats
repeats after warm-up, in us:

  linearize  mh_icp_linearize of the oldest factor at its pose (the yardstick)
  marginal   mh_icp_window_marginalise with the has_Z tie alone
  marginal8  ... with 8 linear factors on pose 0 and 8 edges on (0, 1)

Every repeat starts from the same warm association state (clones of a factor linearized once).  The sides alternate in fresh
child processes, --pairs rounds per size, each child under a time limit; a failed child ends the run.  The spread of `linearize`
over its rounds is what a difference has to exceed to count.

Writes profiles/icp_window_marginal_time.json (or --out) and prints it.

  python tools/icp_window_marginal_time.py [--repeats N] [--pairs P] [--out PATH]
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

from icp_window_time import W, expmap  # noqa: E402

SIDES = {"linearize": None, "marginal": 0, "marginal8": 8}


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
    cfg = capi.make_window_config(iters=1, prior_sigma_rot=0.017453292519943295, prior_sigma_trans=0.1)
    R0 = np.ascontiguousarray(np.array([p[0].ravel() for p in poses0]))
    t0 = np.ascontiguousarray(np.array([p[1] for p in poses0]))
    hz = np.array([0] + [1] * (W - 1), np.int32)
    ZR = np.ascontiguousarray(np.tile(np.eye(3).ravel(), (W, 1)))
    Zt = np.zeros((W, 3))
    n_terms = SIDES[side] or 0
    lin, ed = [], []
    for _ in range(n_terms):
        Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
        Om = (Q * np.logspace(2, 5, 6)) @ Q.T
        (Ra, ta), (Rb, tb) = poses0[0], poses0[1]
        ed.append(dict(a=0, b=1, Z=(Ra.T @ Rb, Ra.T @ (tb - ta)), info=(Om + Om.T) / 2))
        lin.append(dict(pose=0, at=(Ra @ expmap(rng.standard_normal(3) * 0.01), ta + rng.standard_normal(3) * 0.01), H=(Om + Om.T) / 2, b=np.zeros(6), f=1.0))
    lin_arr, ed_arr = capi.make_window_linear(lin), capi.make_window_edge(ed)
    out_m, out_r = capi.WindowMarginal(), capi.IcpResult()

    def call(h):
        if SIDES[side] is None:
            rc = L.mh_icp_linearize(h[0], capi._p(R0[0]), capi._p(t0[0]), None, None, capi._p(g), C.byref(out_r))
            assert rc == 0
        else:
            rc = L.mh_icp_window_marginalise(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), lin_arr, n_terms, ed_arr,
                                             n_terms, C.byref(out_m))
            assert rc == 0 and out_m.valid == 1

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
            t.append((b - a) * 1e6)
    out = {"points": n_pts, "factors": W, "repeats": repeats, "side": side, "us": round(float(np.median(t)), 3)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_window_marginal_time.json"))
    ap.add_argument("--one", type=int, default=0, help="run one size and one side in this process and print its JSON")
    ap.add_argument("--side", default="marginal", choices=list(SIDES))
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "icp_window_marginal_time", "sizes": []}
    for n in (24576, 1024):
        runs = {s: [] for s in SIDES}
        for _ in range(a.pairs):
            for side in SIDES:  # alternating fresh processes
                runs[side].append(child(["--one", str(n), "--side", side, "--repeats", str(a.repeats)]))
        row = {"points": n, "factors": W, "repeats": a.repeats, "pairs": a.pairs}
        for side in SIDES:
            vals = [q["us"] for q in runs[side]]
            row[side + "_us"] = round(float(np.median(vals)), 3)
            row[side + "_us_runs"] = vals
        row["linearize_spread_us"] = round(max(row["linearize_us_runs"]) - min(row["linearize_us_runs"]), 3)
        for side in ("marginal", "marginal8"):
            row[side + "_minus_linearize_us"] = round(row[side + "_us"] - row["linearize_us"], 3)
        out["sizes"].append(row)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
