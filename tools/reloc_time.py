"""Times the relocalisation calls on the GPU against the only route the library offered before them.  Scene: synth.small_world()
(a ~5 k point map, a 16 x 64 scan = 1 024 points), candidate poses drawn with a fixed seed over the room (xy within +-3 m of the
truth, any yaw).  Every figure is a median host wall clock over --repeats repeats after warm-up, in us.

Sides, per n_poses in 256 / 4 096 / 65 536:
  score      mh_icp_score_poses, stride 1, gate 1 m, top_k = 8, scores = NULL (the winners alone come back)
  knn        the yardstick: the same queries through mh_map_knn(k = 1) — the transform of the cloud by every pose in numpy, the
             queries uploaded and n x 56 bytes downloaded per pose, inliers and sums reduced in numpy, a numpy sort for the
             winners.  256 poses per mh_map_knn call (262 144 queries).  Above 4 096 poses it is timed on a sample of 1 024 poses
             and scaled by n_poses / 1 024; the record says so (knn_sampled_poses).  Its repeats are capped at 5: one repeat at
             4 096 poses is seconds.
Relocalise (729 poses: the grid of tests/test_gpu_reloc.py, coarse stride 4, top_k = 4, final gate 0.1 m):
  reloc      mh_icp_relocalise end to end
  reloc_score / reloc_align / reloc_rescore   the same three stages as separate calls from here (mh_icp_score_poses, a reset and an
             mh_icp_align per candidate, mh_icp_score_poses on the aligned poses): where its time goes

The sides alternate in fresh child processes, --rounds rounds, each child under a time limit; a failed child ends the run.
Writes profiles/reloc_time.json (or --out) and prints it.  On a shared machine run it as one step under its own limit:

  timeout -k 10 1100 python tools/reloc_time.py

The score kernel's own time is not a host wall clock: it comes from a kernel trace in a run of its own (no counters, nothing
else traced), one child of this tool as the program behind `--`, under a time limit, reduced by --reduce:

  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profiles/reloc_trace -o reloc -- \\
      python tools/reloc_time.py --one 4096 --side score --repeats 25 && \\
  python tools/reloc_time.py --reduce profiles/reloc_trace > profiles/reloc_kernel_stats.txt

  python tools/reloc_time.py [--repeats N] [--rounds R] [--out PATH]
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (256, 4096, 65536)
SIDES = ("score", "knn")
RELOC_SIDES = ("reloc", "reloc_score", "reloc_align", "reloc_rescore")
KNN_CHUNK, KNN_SAMPLE, KNN_REPEATS = 256, 1024, 5
GATE = 1.0


def transform(R, t, xyz):
    """q [n_poses, m, 3], every product and sum on its own (the expression of mh_icp_score_poses)"""
    x, y, z = (xyz[:, a].astype(np.float64)[None, :] for a in range(3))
    q = np.empty((len(R), xyz.shape[0], 3))
    for a in range(3):
        q[:, :, a] = ((R[:, a, 0, None] * x + R[:, a, 1, None] * y) + R[:, a, 2, None] * z) + t[:, a, None]
    return q


def one(n_poses: int, side: str, repeats: int) -> dict:
    from mimosa_amd import capi, synth

    ctx = capi.Context(0)
    m, pts, aux = synth.small_world()
    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    f = capi.ICPFactor(ctx, gm, pts, capi.make_reg_config(**synth.enwide_config()))
    f.set_components(False)
    xyz = synth.points_xyz(pts)
    Rg, tg = aux["R_W_L"], aux["t_W_L"]
    out = {"points": len(pts), "side": side}
    t_us = []
    if side in SIDES:
        rng = np.random.default_rng(17)
        yaw = rng.uniform(-np.pi, np.pi, n_poses)
        R = np.stack([synth.rot_z(a) @ Rg for a in yaw])
        t = tg + np.concatenate([rng.uniform(-3.0, 3.0, (n_poses, 2)), np.zeros((n_poses, 1))], axis=1)
        R[0], t[0] = Rg, tg
        out["n_poses"] = n_poses
        if side == "score":
            for i in range(repeats + 5):
                a = time.perf_counter()
                _, best = f.score_poses(R, t, GATE, stride=1, top_k=8, want_scores=False)
                b = time.perf_counter()
                if i >= 5:
                    t_us.append((b - a) * 1e6)
            out["best"] = [int(v) for v in best]
            out["repeats"] = repeats
        else:
            n_timed = n_poses if n_poses <= 4096 else KNN_SAMPLE
            reps = min(repeats, KNN_REPEATS)
            for i in range(reps + 1):
                a = time.perf_counter()
                n_in, s_sq = np.zeros(n_timed, np.int64), np.zeros(n_timed)
                for c0 in range(0, n_timed, KNN_CHUNK):
                    q = transform(R[c0:c0 + KNN_CHUNK], t[c0:c0 + KNN_CHUNK], xyz)
                    _, sq, found = gm.knn(q.reshape(-1, 3), 1)
                    d2 = sq[:, 0].reshape(q.shape[0], -1)
                    inl = (found.reshape(q.shape[0], -1) > 0) & (d2 <= GATE * GATE)
                    n_in[c0:c0 + KNN_CHUNK] = inl.sum(axis=1)
                    s_sq[c0:c0 + KNN_CHUNK] = np.where(inl, d2, 0.0).sum(axis=1)
                best = np.lexsort((np.arange(n_timed), s_sq, -n_in))[:8]
                b = time.perf_counter()
                if i >= 1:
                    t_us.append((b - a) * 1e6 * (n_poses / n_timed))
            out["best_of_timed"] = [int(v) for v in best]
            out["repeats"] = reps
            out["knn_sampled_poses"] = n_timed if n_timed != n_poses else 0
    else:
        R0, t0 = synth.rot_z(np.deg2rad(20.0)) @ Rg, tg + np.array([1.2, -0.9, 0.0])
        Rs, ts = capi.pose_grid(R0, t0, 2.0, 0.5, np.deg2rad(30.0), np.deg2rad(7.5))
        acfg = capi.make_align_config(max_iters=30, eps_rot=1e-9, eps_trans=1e-9, damping=1e-9)
        cfg = capi.make_reloc_config(gate=GATE, stride=4, top_k=4, align=acfg, final_gate=0.1)
        out["n_poses"] = len(Rs)
        _, best = f.score_poses(Rs, ts, GATE, stride=4, top_k=4, want_scores=False)
        aligned = []
        for i in range(repeats + 5):
            a = time.perf_counter()
            if side == "reloc":
                r = f.relocalise(Rs, ts, cfg)
            elif side == "reloc_score":
                _, best = f.score_poses(Rs, ts, GATE, stride=4, top_k=4, want_scores=False)
            elif side == "reloc_align":
                aligned = []
                for c in best:
                    f.reset()
                    aligned.append(f.align(Rs[c], ts[c], acfg))
                f.reset()
            else:
                if not aligned:
                    for c in best:
                        f.reset()
                        aligned.append(f.align(Rs[c], ts[c], acfg))
                    f.reset()
                    a = time.perf_counter()
                f.score_poses(np.stack([q["R"] for q in aligned]), np.stack([q["t"] for q in aligned]), 0.1, stride=1, top_k=len(aligned))
            b = time.perf_counter()
            if i >= 5:
                t_us.append((b - a) * 1e6)
        if side == "reloc":
            out["winner_m_from_truth"] = float(np.linalg.norm(r["t"] - tg))
            out["align_iters"] = [c["iters"] for c in r["cand"]]
        out["repeats"] = repeats
    out["us"] = round(float(np.median(t_us)), 3)
    f.destroy()
    gm.release()
    ctx.close()
    return out


def child(args, timeout=280) -> dict:
    import subprocess
    print("reloc_time:", " ".join(args), file=sys.stderr, flush=True)
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
    print("kernel-trace summary of: python tools/reloc_time.py --one 4096 --side score --repeats 25 (rocprofv3 --kernel-trace --stats; durations in ns)")
    print("%-100s %8s %10s %10s %10s" % ("kernel", "calls", "avg", "min", "max"))
    for name, calls, avg, lo, hi in rows:
        print("%-100s %8d %10.0f %10d %10d" % (name[:100], calls, avg, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_time.json"))
    ap.add_argument("--one", type=int, default=0, help="run one size and one side in this process and print its JSON (n_poses; ignored by the reloc sides)")
    ap.add_argument("--side", default="score", choices=SIDES + RELOC_SIDES)
    ap.add_argument("--reduce", default="", help="print the per-kernel table of a rocprofv3 kernel trace (directory or database)")
    a = ap.parse_args()
    if a.reduce:
        reduce_trace(a.reduce)
        return
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "reloc_time", "points": 1024, "gate": GATE, "sizes": [], "relocalise": {}}
    for n in SIZES:
        runs = {s: [] for s in SIDES}
        for _ in range(a.rounds):
            for side in SIDES:  # alternating fresh processes
                runs[side].append(child(["--one", str(n), "--side", side, "--repeats", str(a.repeats)]))
        row = {"n_poses": n, "repeats": a.repeats, "rounds": a.rounds, "knn_repeats": runs["knn"][0]["repeats"],
               "knn_sampled_poses": runs["knn"][0]["knn_sampled_poses"]}
        for side in SIDES:
            vals = [q["us"] for q in runs[side]]
            row[side + "_us"] = round(float(np.median(vals)), 3)
            row[side + "_us_runs"] = vals
        row["knn_over_score"] = round(row["knn_us"] / row["score_us"], 2)
        row["score_not_slower"] = bool(row["score_us"] <= row["knn_us"])
        out["sizes"].append(row)
    runs = {s: [] for s in RELOC_SIDES}
    for _ in range(a.rounds):
        for side in RELOC_SIDES:
            runs[side].append(child(["--one", "1", "--side", side, "--repeats", str(a.repeats)]))
    rel = {"n_poses": runs["reloc"][0]["n_poses"], "repeats": a.repeats, "rounds": a.rounds, "winner_m_from_truth": runs["reloc"][0]["winner_m_from_truth"],
           "align_iters": runs["reloc"][0]["align_iters"]}
    for side in RELOC_SIDES:
        vals = [q["us"] for q in runs[side]]
        rel[side + "_us"] = round(float(np.median(vals)), 3)
        rel[side + "_us_runs"] = vals
    out["relocalise"] = rel
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
