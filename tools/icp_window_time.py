"""Times the fixed-lag window loop on the GPU: mh_icp_window_optimise (the smoother's Gauss-Newton iterations as one chain of
launches) against the host-driven loop around mh_icp_linearize_batch.  W = 5 factors of 24 576 and of 1 024 points, the
replay's 6 iterations, its between sigmas, the tight prior and a damping of 1e-9; every figure the median host wall clock of
one whole optimisation over --repeats repeats after warm-up, per iteration in us:

  window                the chain queued at once (through ctypes with prebuilt arguments)
  host_loop             6 x (mh_icp_linearize_batch with components off + numpy assembly, solve and retraction)
  host_loop_floor       the same loop with the assembly, the solve and the retraction left out (every call at the poses of its
                        iteration of a recorded trajectory): the floor of the host-driven loop

Every repeat starts from the same warm association state (clones of factors linearized once).  The two sides alternate in
fresh child processes (--pairs of them per size), each under a time limit; a failed child ends the run; the figures reported
are the medians over the children.

  replay                the native replay (FixedLagReplay, 20 scans of 64 x 512 without the photometric factor, the second of two
                        passes timed) with and without device_window: --replay-pairs alternating pairs, every run a fresh
                        process; scans/s and the optimise stage's ms per scan, medians

Writes profiles/icp_window_time.json and prints it.

  python tools/icp_window_time.py [--repeats N] [--pairs P] [--replay-pairs Q]
  the step kernel's time, from a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o window -- python tools/icp_window_time.py --one 24576 --side window --repeats 20
    python tools/icp_window_time.py --kernel-stats OUT/window_results.db > profiles/icp_window_kernel_stats.txt
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

ITERS, W = 6, 5


def expmap(w):
    th2 = float(w @ w)
    th = np.sqrt(th2)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    A, B = (1.0 - th2 / 6.0, 0.5 - th2 / 24.0) if th < 1e-10 else (np.sin(th) / th, (1.0 - np.cos(th)) / th2)
    return np.eye(3) + A * K + B * (K @ K)


def so3log(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    th = np.arccos(c)
    s = 0.5 if th < 1e-9 else th / (2.0 * np.sin(th))
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * s


def adjoint(R, t):
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    return A


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
    Wb, prior = np.diag(np.array(cfg.between_info)), np.diag(np.array(cfg.prior_info))
    R0 = np.ascontiguousarray(np.array([p[0].ravel() for p in poses0]))
    t0 = np.ascontiguousarray(np.array([p[1] for p in poses0]))
    hz = np.array([0] + [1] * (W - 1), np.int32)
    ZR = np.ascontiguousarray(np.tile(np.eye(3).ravel(), (W, 1)))
    Zt = np.zeros((W, 3))
    gW = np.ascontiguousarray(np.tile(g, (W, 1)))
    out_res = capi.WindowResult()
    res = (capi.IcpResult * W)()
    trace = np.zeros((ITERS, W, 12))

    def clones():
        return [base.clone() for _ in range(W)]

    def handles(fs):
        return (C.c_void_p * W)(*[f.h for f in fs])

    def timed(fn):
        t = []
        for i in range(repeats + 5):
            fs = clones()
            h = handles(fs)
            a = time.perf_counter()
            fn(h)
            b = time.perf_counter()
            for f in fs:
                f.destroy()
            if i >= 5:
                t.append((b - a) * 1e6 / ITERS)
        return round(float(np.median(t)), 3)

    def window(h):
        rc = L.mh_icp_window_optimise(h, W, capi._p(R0), capi._p(t0), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(g), C.byref(cfg), C.byref(out_res),
                                      capi._p(trace))
        assert rc == 0 and out_res.iters == ITERS

    def host_loop(h):
        R, t = R0.reshape(W, 3, 3).copy(), t0.copy()
        for _ in range(ITERS):
            Rc = np.ascontiguousarray(R.reshape(W, 9))
            rc = L.mh_icp_linearize_batch(h, W, capi._p(Rc), capi._p(t), None, None, capi._p(gW), res)
            assert rc == 0
            A, gr = np.zeros((6 * W, 6 * W)), np.zeros(6 * W)
            for i in range(W):
                A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += np.array(res[i].H_ss).reshape(6, 6)
                gr[6 * i:6 * i + 6] += np.array(res[i].b_s)
            for i in range(1, W):
                abR, abt = R[i - 1].T @ R[i], R[i - 1].T @ (t[i] - t[i - 1])
                r = np.concatenate([so3log(abR), abt])
                Ja = -adjoint(abR.T, -abR.T @ abt)
                a, b = slice(6 * (i - 1), 6 * i), slice(6 * i, 6 * i + 6)
                A[a, a] += Ja.T @ Wb @ Ja
                A[a, b] += Ja.T @ Wb
                A[b, a] += Wb @ Ja
                A[b, b] += Wb
                gr[a] += Ja.T @ Wb @ r
                gr[b] += Wb @ r
            A[:6, :6] += prior
            xi = np.linalg.solve(A + 1e-9 * np.eye(6 * W), -gr).reshape(W, 6)
            for i in range(W):
                R[i], t[i] = R[i] @ expmap(xi[i, :3]), t[i] + R[i] @ xi[i, 3:]

    out = {"points": n_pts, "factors": W, "iters": ITERS, "repeats": repeats, "side": side}
    if side == "window":
        out["window_us_per_iter"] = timed(window)
    else:
        fs = clones()
        window(handles(fs))  # the trajectory the floor replays
        for f in fs:
            f.destroy()
        traj = [(R0, t0)] + [(np.ascontiguousarray(trace[i, :, :9]), np.ascontiguousarray(trace[i, :, 9:])) for i in range(ITERS - 1)]

        def host_floor(h):
            for Rc, tc in traj:
                rc = L.mh_icp_linearize_batch(h, W, capi._p(Rc), capi._p(tc), None, None, capi._p(gW), res)
                assert rc == 0

        out["host_loop_us_per_iter"] = timed(host_loop)
        out["host_loop_floor_us_per_iter"] = timed(host_floor)
    base.destroy()
    gm.release()
    ctx.close()
    return out


def replay_pairs(pairs: int) -> dict:
    """the native replay with and without device_window, alternating, every run a fresh process (the driver)"""
    import dataclasses
    import tempfile
    from mimosa_amd import replay

    cfg = replay.ReplayConfig(n_scans=20, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2, keyframe_rot_thresh_deg=5.0,
                              photometric=False)
    sides = {"off": cfg, "on": dataclasses.replace(cfg, device_window=True)}
    scans = replay.make_scans(cfg)
    runs = {k: {"scans_per_s": [], "optimise_ms_per_scan": []} for k in sides}
    with tempfile.TemporaryDirectory() as d:
        for _ in range(pairs):
            for key, c in sides.items():
                r = replay.run_native(c, scans, d, repeats=2, timeout=200)
                runs[key]["scans_per_s"].append(round(r["scans_per_s"], 2))
                runs[key]["optimise_ms_per_scan"].append(round(r["stage_s"]["optimise"] / cfg.n_scans * 1e3, 4))
    out = {"scans": cfg.n_scans, "rows": cfg.rows, "cols": cfg.cols, "window": cfg.window, "update_iters": cfg.update_iters, "pairs": pairs}
    for key in sides:
        out[f"scans_per_s_{key}"] = round(float(np.median(runs[key]["scans_per_s"])), 2)
        out[f"optimise_ms_per_scan_{key}"] = round(float(np.median(runs[key]["optimise_ms_per_scan"])), 4)
        out[f"runs_{key}"] = runs[key]
    out["scans_per_s_on_over_off"] = round(out["scans_per_s_on"] / out["scans_per_s_off"], 4)
    out["optimise_on_over_off"] = round(out["optimise_ms_per_scan_on"] / out["optimise_ms_per_scan_off"], 4)
    return out


def kernel_stats(db_path: str) -> None:
    """the per-kernel table of a rocprofv3 kernel trace (the `kernels` view of its rocpd database: name, start, end in ns)"""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name "
                      "order by sum(end - start) desc").fetchall()
    print("kernel-trace summary of: python tools/icp_window_time.py --one 24576 --side window --repeats 20 (rocprofv3 --kernel-trace; durations in ns)")
    print("%-100s %8s %10s %10s %10s" % ("kernel", "calls", "avg", "min", "max"))
    for name, calls, avg, lo, hi in rows:
        print("%-100s %8d %10.0f %10d %10d" % (name[:100], calls, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--one", type=int, default=0, help="run one size and one side in this process and print its JSON")
    ap.add_argument("--side", default="window", choices=["window", "host"])
    ap.add_argument("--replay-pairs", type=int, default=5)
    ap.add_argument("--kernel-stats", default="", help="reduce this rocprofv3 database to the per-kernel table and print it")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
        return
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "icp_window_time", "sizes": []}
    for n in (24576, 1024):
        runs = {"window": [], "host": []}
        for _ in range(a.pairs):
            for side in ("window", "host"):  # alternating fresh processes
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--side", side, "--repeats", str(a.repeats)],
                                   capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-2000:])
                    sys.exit(r.returncode or 1)
                runs[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
        row = {"points": n, "factors": W, "iters": ITERS, "repeats": a.repeats, "pairs": a.pairs}
        for side, key in (("window", "window_us_per_iter"), ("host", "host_loop_us_per_iter"), ("host", "host_loop_floor_us_per_iter")):
            vals = [q[key] for q in runs[side]]
            row[key] = round(float(np.median(vals)), 3)
            row[key + "_runs"] = vals
        row["window_over_host_loop"] = round(row["window_us_per_iter"] / row["host_loop_us_per_iter"], 4)
        row["window_over_floor"] = round(row["window_us_per_iter"] / row["host_loop_floor_us_per_iter"], 4)
        out["sizes"].append(row)
    out["replay"] = replay_pairs(a.replay_pairs)
    path = os.path.join(ROOT, "profiles", "icp_window_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
