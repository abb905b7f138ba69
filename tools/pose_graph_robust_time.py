"""Times what priors and losses cost mh_pose_graph_optimise on the GPU.  Every figure is a median host wall clock, in ms, of ONE
optimise call of --iters iterations with convergence off (eps = 0), after warm-up, on the sizes of tools/pose_graph_time.py
(512 poses with 2 far edges, 4 096 poses with 2 and with 32 far edges).

Three sides, alternating in fresh child processes, --rounds rounds of --repeats calls each, one GPU process at a time, each
child under a time limit; a failed child ends the run:
  parent   the plain call (no prior, no loss) with the PARENT commit's library, --parent-lib (default
           mimosa_amd/lib/variants/pgo_parent.so).  tools/variant.sh rebuilds icp_kernels.hip alone, so the parent's
           library is built from a checkout of the parent:
             git worktree add ../parent HEAD~1 && (cd ../parent && python -m mimosa_amd.build) &&
             mkdir -p mimosa_amd/lib/variants && cp ../parent/mimosa_amd/lib/libmimosa_hip.so mimosa_amd/lib/variants/pgo_parent.so
           Without that file the side is left out and the JSON says so.
  plain    the plain call with this commit's library                                             -> (a) plain / parent
  robust   Cauchy (k = 3) on every far edge and 8 priors spread over the circuit, this commit     -> (b) robust / plain
The parent's spread is its largest round median over its smallest.  Writes profiles/pose_graph_robust_time.json (or --out) and
prints the JSON.  On a shared machine run it as one step under its own limit:

  timeout -k 10 900 python tools/pose_graph_robust_time.py

  python tools/pose_graph_robust_time.py [--iters K] [--repeats N] [--rounds R] [--parent-lib PATH] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIDES = ("parent", "plain", "robust")
WARMUP = 2
N_PRIORS = 8
CAUCHY_K = 3.0


def one(n: int, n_far: int, side: str, iters: int, repeats: int, lib: str) -> dict:
    """one side in this process, through ctypes on `lib` itself: the parent's library lacks the new symbols, so capi.load(), which
    binds every export, cannot load it; all three sides go the same way"""
    import ctypes as C

    import pose_graph_time as base
    from mimosa_amd import capi
    c = base.graph(n, n_far)
    L = C.CDLL(lib)
    vp, sz = C.c_void_p, C.c_size_t
    L.mh_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.mh_shutdown.argtypes = [vp]
    L.mh_shutdown.restype = None
    L.mh_pose_graph_create.argtypes = [vp, sz, sz, C.POINTER(vp)]
    L.mh_pose_graph_destroy.argtypes = [vp]
    L.mh_pose_graph_destroy.restype = None
    L.mh_pose_graph_set_poses.argtypes = [vp, vp, vp, sz]
    L.mh_pose_graph_set_fixed.argtypes = [vp, vp]
    L.mh_pose_graph_set_edges.argtypes = [vp, C.POINTER(capi.WindowEdge), sz]
    L.mh_pose_graph_optimise.argtypes = [vp, C.POINTER(capi.PoseGraphConfig), C.POINTER(capi.PoseGraphResult), vp]

    def ok(rc):
        if rc != 0:
            raise RuntimeError("pose_graph_robust_time: the library returned %d" % rc)

    ctx, pg = vp(), vp()
    ok(L.mh_init(0, C.byref(ctx)))
    ok(L.mh_pose_graph_create(ctx, n, len(c["edges"]), C.byref(pg)))
    R, t = np.ascontiguousarray(c["R"], np.float64).reshape(-1, 9), np.ascontiguousarray(c["t"], np.float64)
    fixed = np.ascontiguousarray(c["fixed"], np.uint8)
    ok(L.mh_pose_graph_set_poses(pg, capi._p(R), capi._p(t), n))
    ok(L.mh_pose_graph_set_fixed(pg, capi._p(fixed)))
    ok(L.mh_pose_graph_set_edges(pg, capi.make_window_edge(base.as_dicts(c["edges"])), len(c["edges"])))
    if side == "robust":
        L.mh_pose_graph_set_priors.argtypes = [vp, C.POINTER(capi.PosePrior), sz]
        L.mh_pose_graph_set_loss.argtypes = [vp, C.POINTER(capi.PoseGraphLoss), C.POINTER(capi.PoseGraphLoss)]
        info = np.diag([1.0 / 4e-3 ** 2] * 3 + [1.0 / 2e-2 ** 2] * 3)
        at = [int(i) for i in np.linspace(1, n - 1, N_PRIORS)]
        ok(L.mh_pose_graph_set_priors(pg, capi.make_pose_prior([{"pose": i, "Z": (c["truth_R"][i], c["truth_t"][i]), "info": info} for i in at]), N_PRIORS))
        ok(L.mh_pose_graph_set_loss(pg, capi.make_pose_graph_loss([((2, CAUCHY_K) if b - a >= 2 else (0, 0.0)) for a, b, *_ in c["edges"]]), None))
    cfg, res = capi.make_pose_graph_config(iters=iters, check_every=0, damping=0.0, eps_rot=0.0, eps_trans=0.0), capi.PoseGraphResult()
    ms = []
    for k in range(WARMUP + repeats):
        ok(L.mh_pose_graph_set_poses(pg, capi._p(R), capi._p(t), n))
        t0 = time.perf_counter()
        ok(L.mh_pose_graph_optimise(pg, C.byref(cfg), C.byref(res), None))
        if k >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    assert res.iters == iters and all(res.trace[i].flags == 0 for i in range(iters))
    out = {"ms": float(np.median(ms)), "f_first": float(res.f_first), "f_last": float(res.f_last)}
    L.mh_pose_graph_destroy(pg)
    L.mh_shutdown(ctx)
    return out


def child(args, timeout=280) -> dict:
    print("pose_graph_robust_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    import pose_graph_time as base
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "mimosa_amd", "lib", "variants", "pgo_parent.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_robust_time.json"))
    ap.add_argument("--one", action="store_true", help="run one size and side in this process and print its JSON")
    ap.add_argument("--poses", type=int, default=0)
    ap.add_argument("--far", type=int, default=0)
    ap.add_argument("--side", default="plain", choices=SIDES)
    a = ap.parse_args()
    if a.one:
        from mimosa_amd import build
        print(json.dumps(one(a.poses, a.far, a.side, a.iters, a.repeats, os.path.abspath(a.parent_lib) if a.side == "parent" else build.LIB)))
        return
    have_parent = os.path.exists(a.parent_lib)
    sides = [s for s in SIDES if s != "parent" or have_parent]
    out = {"tool": "pose_graph_robust_time", "iters": a.iters, "repeats": a.repeats, "rounds": a.rounds, "priors": N_PRIORS, "cauchy_k": CAUCHY_K,
           "parent_measured": have_parent, "cases": []}
    for n, n_far in base.SIZES:
        runs = {s: [] for s in sides}
        for _ in range(a.rounds):
            for side in sides:
                runs[side].append(child(["--one", "--poses", str(n), "--far", str(n_far), "--side", side, "--iters", str(a.iters), "--repeats", str(a.repeats),
                                         "--parent-lib", a.parent_lib]))
        row = {"poses": n, "far_edges": n_far, "edges": n - 1 + n_far}
        for side in sides:
            vals = [q["ms"] for q in runs[side]]
            row[side + "_ms"] = round(float(np.median(vals)), 3)
            row[side + "_ms_runs"] = [round(v, 3) for v in vals]
        if have_parent:
            row["parent_spread"] = round(max(row["parent_ms_runs"]) / min(row["parent_ms_runs"]), 4)
            row["plain_over_parent"] = round(row["plain_ms"] / row["parent_ms"], 4)
            row["plain_same_bits_as_parent"] = all(p["f_last"] == q["f_last"] and p["f_first"] == q["f_first"] for p, q in zip(runs["parent"], runs["plain"]))
        row["robust_over_plain"] = round(row["robust_ms"] / row["plain_ms"], 4)
        out["cases"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
