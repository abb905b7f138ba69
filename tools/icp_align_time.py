"""Times scan-to-map alignment on the GPU: mh_icp_align (the Gauss-Newton loop as one chain of launches) against the loop a
caller writes around mh_icp_linearize.  For 24 576 and 131 072 points, 10 iterations with convergence switched off (eps = 0),
every figure the median host wall clock of one whole alignment over --repeats repeats after warm-up, per iteration in us:

  align_ce0 / _ce1 / _ce4   mh_icp_align with check_every 0, 1, 4 (through ctypes with prebuilt arguments)
  host_loop                 10 x (mh_icp_linearize with components off + a numpy 6 x 6 solve + retraction)
  host_loop_floor           the same loop with the solve and the retraction left out (every call at the start pose of its
                            iteration of a recorded trajectory): the floor of the host-driven loop

Every repeat starts from the same warm association state (a clone of one factor linearized once).  Each size runs in a child
process of its own under a time limit; a failed child ends the run.  Writes profiles/icp_align_time.json and prints it.

  python tools/icp_align_time.py [--repeats N]
  rocprofv3 --kernel-trace --stats -- python tools/icp_align_time.py --one 24576 --repeats 20    (the step kernel's time)
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

ITERS = 10


def expmap(w):
    th2 = float(w @ w)
    th = np.sqrt(th2)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    A, B = (1.0 - th2 / 6.0, 0.5 - th2 / 24.0) if th < 1e-10 else (np.sin(th) / th, (1.0 - np.cos(th)) / th2)
    return np.eye(3) + A * K + B * (K @ K)


def one(n_pts: int, repeats: int) -> dict:
    from mimosa_amd import capi, synth

    ctx = capi.Context(0)
    gm = capi.VoxelMap(ctx)
    gm.insert(synth.make_room(synth.BASE_SEED, 0, 0))
    scan, _ = synth.make_scan(128 if n_pts > 65536 else 64)
    pts = np.ascontiguousarray(scan[:: max(1, len(scan) // n_pts)][:n_pts])
    base = capi.ICPFactor(ctx, gm, pts, capi.make_reg_config(**synth.enwide_config()))
    base.set_components(False)
    R0, t0 = synth.query_pose()
    g = np.array([0.0, 0.0, -1.0])
    base.linearize(R0, t0, g)
    L = ctx.L
    out_res = capi.AlignResult()
    res = capi.IcpResult()
    R0c, t0c = np.ascontiguousarray(R0.ravel()), np.ascontiguousarray(t0)

    def timed(fn, prep):
        t = []
        for i in range(repeats + 5):
            f = prep()
            a = time.perf_counter()
            fn(f)
            b = time.perf_counter()
            f.destroy()
            if i >= 5:
                t.append((b - a) * 1e6 / ITERS)
        return round(float(np.median(t)), 3)

    def clone():
        return base.clone()

    out = {"points": n_pts, "iters": ITERS, "repeats": repeats}
    for ce in (0, 1, 4):
        cfg = capi.make_align_config(max_iters=ITERS, eps_rot=0.0, eps_trans=0.0, damping=1e-9, check_every=ce)
        out[f"align_ce{ce}_us_per_iter"] = timed(
            lambda f: L.mh_icp_align(f.h, capi._p(R0c), capi._p(t0c), capi._p(g), C.byref(cfg), C.byref(out_res)), clone)
        assert out_res.iters == ITERS
    traj = [(np.array(out_res.trace[i].R).reshape(3, 3).copy(), np.array(out_res.trace[i].t).copy()) for i in range(ITERS)]
    poses = [(R0c, t0c)] + [(np.ascontiguousarray(R.ravel()), np.ascontiguousarray(t)) for R, t in traj[:-1]]

    def host_loop(f):
        R, t = R0.copy(), t0.copy()
        for _ in range(ITERS):
            Rc, tc = np.ascontiguousarray(R.ravel()), t
            L.mh_icp_linearize(f.h, capi._p(Rc), capi._p(tc), None, None, capi._p(g), C.byref(res))
            H = np.array(res.H_ss).reshape(6, 6)
            H[np.diag_indices(6)] += 1e-9
            xi = np.linalg.solve(H, -np.array(res.b_s))
            R, t = R @ expmap(xi[:3]), t + R @ xi[3:]

    def host_floor(f):
        for Rc, tc in poses:
            L.mh_icp_linearize(f.h, capi._p(Rc), capi._p(tc), None, None, capi._p(g), C.byref(res))

    out["host_loop_us_per_iter"] = timed(host_loop, clone)
    out["host_loop_floor_us_per_iter"] = timed(host_floor, clone)
    out["align_ce0_over_floor"] = round(out["align_ce0_us_per_iter"] / out["host_loop_floor_us_per_iter"], 4)
    out["align_ce0_over_host_loop"] = round(out["align_ce0_us_per_iter"] / out["host_loop_us_per_iter"], 4)
    base.destroy()
    gm.release()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--one", type=int, default=0, help="run one size in this process and print its JSON")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.repeats)))
        return
    out = {"tool": "icp_align_time", "sizes": []}
    for n in (24576, 131072):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--repeats", str(a.repeats)], capture_output=True, text=True,
                           timeout=240)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(r.returncode or 1)
        out["sizes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    path = os.path.join(ROOT, "profiles", "icp_align_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
