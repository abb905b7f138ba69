"""Times the joint-factor calls of the fixed-lag window chain on the GPU, each against its yardstick in the same library.  W = 5
factors of 24 576 and of 1 024 points, the replay's between sigmas on every consecutive pair, the loose prior and a damping of
1e-9 (the set-up of tools/icp_window_edges_time.py).  Every figure is the median host wall clock of one blocking call over
--repeats repeats after warm-up, in us; the consumer's are divided by its 6 iterations.

Consumer (us per iteration of the whole call):
  edges2     mh_icp_window_optimise_edges with 2 edges of span 2 (the yardstick)
  joint2     mh_icp_window_optimise_joint with the same 2 edges and a joint factor on poses {0, 2}
  joint4     ... on poses {0, 1, 2, 3}
Producer (us per call):
  linearize  mh_icp_linearize of the oldest factor at its pose (the floor)
  marginal   mh_icp_window_marginalise with the has_Z tie alone
  jmarginal1 mh_icp_window_marginalise_joint with the has_Z tie alone (separator {1})
  jmarginal4 ... with edges (0, 2), (0, 3), (0, 4) (separator {1, 2, 3, 4})

Every repeat starts from the same warm association state (clones of a factor linearized once).  The sides alternate in fresh
child processes, --pairs rounds per size, each child under a time limit; a failed child ends the run.  The spread of a yardstick
over its rounds is what a difference has to exceed to count.

Writes profiles/icp_window_joint_time.json (or --out) and prints it.

The step kernel's own time is not a host wall clock: it comes from a kernel trace in a run of its own (no counters, nothing
else traced), one child of this tool as the program behind `--`, under a time limit:

  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profiles/icp_window_joint_trace -- \
      python tools/icp_window_joint_time.py --one 24576 --side joint4 --repeats 25

and is read from the `icp_window_joint_step_kernel` rows of the trace it writes (summarised in profiles/icp_window_joint_kernel_stats.txt) (25 + 5 calls of 6 iterations: 180
launches); `--side edges2` gives `icp_window_edge_step_kernel` beside it.

  python tools/icp_window_joint_time.py [--repeats N] [--pairs P] [--out PATH]
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

SIDES = ["edges2", "joint2", "joint4", "linearize", "marginal", "jmarginal1", "jmarginal4"]
ITERS = 6


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
    consumer = side in ("edges2", "joint2", "joint4")
    cfg = capi.make_window_config(iters=ITERS if consumer else 1, prior_sigma_rot=0.017453292519943295, prior_sigma_trans=0.1)
    R0 = np.ascontiguousarray(np.array([p[0].ravel() for p in poses0]))
    t0 = np.ascontiguousarray(np.array([p[1] for p in poses0]))
    hz = np.array([0] + [1] * (W - 1), np.int32)
    ZR = np.ascontiguousarray(np.tile(np.eye(3).ravel(), (W, 1)))
    Zt = np.zeros((W, 3))

    def info(n):
        Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        Om = (Q * np.logspace(2, 5, n)) @ Q.T
        return (Om + Om.T) / 2

    def edge(a, b):
        (Ra, ta), (Rb, tb) = poses0[a], poses0[b]
        return dict(a=a, b=b, Z=(Ra.T @ Rb, Ra.T @ (tb - ta)), info=info(6))

    pairs = {"edges2": [(0, 2), (2, 4)], "joint2": [(0, 2), (2, 4)], "joint4": [(0, 2), (2, 4)], "jmarginal4": [(0, 2), (0, 3), (0, 4)]}.get(side, [])
    ed = [edge(a, b) for a, b in pairs]
    members = {"joint2": [0, 2], "joint4": [0, 1, 2, 3]}.get(side)
    joint = None
    if members is not None:
        at = [(poses0[i][0] @ expmap(rng.standard_normal(3) * 0.01), poses0[i][1] + rng.standard_normal(3) * 0.01) for i in members]
        joint = capi.make_window_joint(dict(poses=members, at=at, H=info(6 * len(members)), b=np.zeros(6 * len(members)), f=1.0))
    lin_arr, ed_arr = capi.make_window_linear([]), capi.make_window_edge(ed)
    out_m, out_j, out_r, out_w = capi.WindowMarginal(), capi.WindowJointMarginal(), capi.IcpResult(), capi.WindowResult()
    head = lambda h: (h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg))  # noqa: E731

    def call(h):
        if side == "linearize":
            rc = L.mh_icp_linearize(h[0], capi._p(R0[0]), capi._p(t0[0]), None, None, capi._p(g), C.byref(out_r))
            assert rc == 0
        elif side == "marginal":
            rc = L.mh_icp_window_marginalise(*head(h), lin_arr, 0, ed_arr, 0, C.byref(out_m))
            assert rc == 0 and out_m.valid == 1
        elif side in ("jmarginal1", "jmarginal4"):
            rc = L.mh_icp_window_marginalise_joint(*head(h), lin_arr, 0, ed_arr, len(ed), None, C.byref(out_j))
            assert rc == 0 and out_j.valid == 1 and out_j.prior.n_poses == (1 if side == "jmarginal1" else 4)
        elif side == "edges2":
            rc = L.mh_icp_window_optimise_edges(*head(h), None, lin_arr, 0, ed_arr, len(ed), C.byref(out_w), None, None)
            assert rc == 0 and out_w.iters == ITERS
        else:
            rc = L.mh_icp_window_optimise_joint(*head(h), None, lin_arr, 0, ed_arr, len(ed), C.byref(out_w), None, None, C.byref(joint))
            assert rc == 0 and out_w.iters == ITERS

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
            t.append((b - a) * 1e6 / (ITERS if consumer else 1))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_window_joint_time.json"))
    ap.add_argument("--one", type=int, default=0, help="run one size and one side in this process and print its JSON")
    ap.add_argument("--side", default="joint2", choices=SIDES)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "icp_window_joint_time", "sizes": []}
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
        for yard in ("edges2", "linearize"):
            row[yard + "_spread_us"] = round(max(row[yard + "_us_runs"]) - min(row[yard + "_us_runs"]), 3)
        for side in ("joint2", "joint4"):
            row[side + "_minus_edges2_us"] = round(row[side + "_us"] - row["edges2_us"], 3)
        for side in ("jmarginal1", "jmarginal4"):
            row[side + "_minus_marginal_us"] = round(row[side + "_us"] - row["marginal_us"], 3)
            row[side + "_minus_linearize_us"] = round(row[side + "_us"] - row["linearize_us"], 3)
        out["sizes"].append(row)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
