"""Times map carving on the GPU against the only route to the same map the library offered before it.  Every figure is a median host
wall clock over --repeats repeats after warm-up, in us.

Cases:
  small   a 64 x 512 scan (its full deskewed cloud, lidar frame) on the map of one 12 x 10 x 3 m room plus 2 000 points of clutter
  large   a 128 x 1024 scan (131 072 points) on the 2 x 5-room map (~5 M stored points) plus 20 000 points of clutter in its room
Sides:
  preview      mh_map_carve_from_scan with apply = 0
  apply        mh_map_carve_from_scan with apply = 1, on a copy made (and released) outside the timed region
  host_route   mh_map_get_cloud, the numpy restatement of the rule (tests/map_carve_ref.py), mh_map_create and one mh_map_insert of
               the survivors: the same map without the feature (--host-repeats repeats, no warm-up: it takes seconds at the large size)
  insert       mh_map_insert_from_scan alone on such a copy: what a keyframe update costs without the carve, for scale

N = 64, ring 1, margin 0.3 m.  The sides alternate in fresh child processes, --rounds rounds, each child under a time limit; a failed
child ends the run.  Writes profiles/map_carve_time.json (or --out) and prints it.  On a shared machine run it as one step under
its own limit:

  timeout -k 10 1100 python tools/map_carve_time.py

  python tools/map_carve_time.py [--repeats N] [--host-repeats N] [--rounds R] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ("small", "large")
SIDES = ("preview", "apply", "host_route", "insert")
WARMUP = 5
CFG = dict(grid=64, ring=1, range_min=0.5, range_max=60.0, margin_abs=0.3, margin_rel=0.0)


def one(case: str, side: str, repeats: int) -> dict:
    import map_carve_ref as ref
    from mimosa_amd import capi, synth

    ctx = capi.Context(0)
    gm = capi.VoxelMap(ctx)
    rng = np.random.default_rng(5)
    if case == "small":
        room = (12.0, 10.0, 3.0)
        gm.insert(synth.make_room(synth.BASE_SEED, 0, 0, room=np.asarray(room)))
        raw, aux = synth.make_raw_scan(64, n_cols=512, room=room, sensor_local=np.array([2.3, 2.6, 1.2]))
        n_clutter = 2000
    else:
        room = tuple(synth.ROOM)
        for _, _, xyz in synth.make_map_rooms(2, 5):
            gm.insert(xyz)
        raw, aux = synth.make_raw_scan(128)
        n_clutter = 20000
    gm.insert((synth.room_origin(0, 0) + rng.uniform(0.05, 0.95, (n_clutter, 3)) * np.asarray(room)).astype(np.float32))
    sc = capi.Scan(ctx)
    sc.prepare_input(raw, capi.make_input_config())
    sc.deskew(aux["Rt12"][np.searchsorted(aux["unique_ns"], sc.unique_ns())])
    sc.preprocess_geometric(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    R, t = aux["R_W_L"], aux["t_W_L"]
    origin = np.zeros(3)
    before = gm.stats()
    want = gm.carve_from_scan(sc, capi.Scan.FULL, origin, R, t, dict(CFG, apply=False))
    out = {"case": case, "side": side, "repeats": repeats, "map_points": before["n_points"], "map_voxels": before["n_voxels"], "counters": want}
    obs = None
    if side == "host_route":
        rec = sc.points(capi.Scan.FULL)
        obs = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    warm = 0 if side == "host_route" else WARMUP
    t_us = []
    for i in range(repeats + warm):
        if side == "preview":
            a = time.perf_counter()
            got = gm.carve_from_scan(sc, capi.Scan.FULL, origin, R, t, dict(CFG, apply=False))
            b = time.perf_counter()
            left = before["n_points"] - got["n_removed"]
        elif side == "host_route":
            a = time.perf_counter()
            cloud = gm.get_cloud()
            _, removed = ref.carve(cloud, ref.voxel_counts(cloud, 0.5), obs, origin, R, t, CFG)
            twin = capi.VoxelMap(ctx)
            twin.insert(cloud[~removed])
            b = time.perf_counter()
            left = twin.stats()["n_points"]
            twin.release()
        else:
            twin = gm.copy()
            ctx.check(ctx.L.mh_synchronize(ctx.h))
            a = time.perf_counter()
            if side == "apply":
                got = twin.carve_from_scan(sc, capi.Scan.FULL, origin, R, t, dict(CFG, apply=True))
            else:
                twin.insert_from_scan(sc, R.astype(np.float32), t.astype(np.float32))
            b = time.perf_counter()
            left = twin.stats()["n_points"] if side == "apply" else before["n_points"] - want["n_removed"]
            if side == "apply" and got != want:
                sys.exit("map_carve_time: apply and preview disagree: %r against %r" % (got, want))
            twin.release()
        if left != before["n_points"] - want["n_removed"]:
            sys.exit("map_carve_time: the sides disagree: %d points left against %d" % (left, before["n_points"] - want["n_removed"]))
        if i >= warm:
            t_us.append((b - a) * 1e6)
    out["us"] = round(float(np.median(t_us)), 3)
    sc.destroy()
    gm.release()
    ctx.close()
    return out


def child(args, timeout=280) -> dict:
    import subprocess
    print("map_carve_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_carve_time.json"))
    ap.add_argument("--one", default="", choices=("",) + CASES, help="run one case and one side in this process and print its JSON")
    ap.add_argument("--side", default="preview", choices=SIDES)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "map_carve_time", "config": CFG, "cases": []}
    for case in CASES:
        runs = {s: [] for s in SIDES}
        for _ in range(a.rounds):
            for side in SIDES:  # alternating fresh processes
                runs[side].append(child(["--one", case, "--side", side, "--repeats", str(a.host_repeats if side == "host_route" else a.repeats)]))
        first = runs["preview"][0]
        row = {"case": case, "repeats": a.repeats, "host_repeats": a.host_repeats, "rounds": a.rounds, "map_points": first["map_points"],
               "map_voxels": first["map_voxels"], "counters": first["counters"]}
        for side in SIDES:
            vals = [q["us"] for q in runs[side]]
            row[side + "_us"] = round(float(np.median(vals)), 3)
            row[side + "_us_runs"] = vals
        row["host_route_over_apply"] = round(row["host_route_us"] / row["apply_us"], 2)
        row["apply_over_preview"] = round(row["apply_us"] / row["preview_us"], 2)
        row["apply_over_insert"] = round(row["apply_us"] / row["insert_us"], 2)
        out["cases"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
