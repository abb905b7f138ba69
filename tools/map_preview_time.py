"""Times the insert preview on the GPU against the only route the library offered before it.  Every figure is a median host wall
clock over --repeats repeats after warm-up, in us.

Cases:
  small   a 64 x 512 scan's body cloud (every 4th point) against the map of one 12 x 10 x 3 m room: the replays' setting
  large   a 128 x 1024 scan's body cloud (~32 k points) against the 2 x 5-room map (~5 M stored points)
Sides:
  preview      mh_map_preview_insert_from_scan (counts only, no outcome array)
  copy_route   mh_map_copy + mh_map_insert_from_scan + mh_map_get_stats + mh_map_release: what learning the same two numbers took
  insert       mh_map_insert_from_scan alone, on a copy made (and released) outside the timed region: the insert on a map that
               needs no fork, for scale

The sides alternate in fresh child processes, --rounds rounds, each child under a time limit; a failed child ends the run.
Writes profiles/map_preview_time.json (or --out) and prints it.  On a shared machine run it as one step under its own limit:

  timeout -k 10 900 python tools/map_preview_time.py

  python tools/map_preview_time.py [--repeats N] [--rounds R] [--out PATH]
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

CASES = ("small", "large")
SIDES = ("preview", "copy_route", "insert")
WARMUP = 5


def one(case: str, side: str, repeats: int) -> dict:
    from mimosa_amd import capi, synth

    ctx = capi.Context(0)
    gm = capi.VoxelMap(ctx)
    if case == "small":
        room = (12.0, 10.0, 3.0)
        gm.insert(synth.make_room(synth.BASE_SEED, 0, 0, room=np.asarray(room)))
        raw, aux = synth.make_raw_scan(64, n_cols=512, room=room, sensor_local=np.array([2.3, 2.6, 1.2]))
    else:
        for _, _, xyz in synth.make_map_rooms(2, 5):
            gm.insert(xyz)
        raw, aux = synth.make_raw_scan(128)
    sc = capi.Scan(ctx)
    sc.prepare_input(raw, capi.make_input_config())
    sc.deskew(aux["Rt12"][np.searchsorted(aux["unique_ns"], sc.unique_ns())])
    sc.preprocess_geometric(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    R, t = synth.query_pose(aux["R_W_L"], aux["t_W_L"])
    before = gm.stats()
    out = {"case": case, "side": side, "repeats": repeats, "map_points": before["n_points"], "map_voxels": before["n_voxels"]}
    pv = gm.preview_insert_from_scan(sc, R, t)
    out["body_points"] = pv["n_points"]
    out["preview"] = pv
    t_us = []
    for i in range(repeats + WARMUP):
        if side == "preview":
            a = time.perf_counter()
            got = gm.preview_insert_from_scan(sc, R, t)
            b = time.perf_counter()
            added, new = got["n_added"], got["n_new_voxels"]
        elif side == "copy_route":
            a = time.perf_counter()
            twin = gm.copy()
            twin.insert_from_scan(sc, R, t)
            s = twin.stats()
            twin.release()
            b = time.perf_counter()
            added, new = s["n_points"] - before["n_points"], s["n_voxels"] - before["n_voxels"]
        else:
            twin = gm.copy()
            ctx.check(ctx.L.mh_synchronize(ctx.h))
            a = time.perf_counter()
            twin.insert_from_scan(sc, R, t)
            b = time.perf_counter()
            s = twin.stats()
            twin.release()
            added, new = s["n_points"] - before["n_points"], s["n_voxels"] - before["n_voxels"]
        if (added, new) != (pv["n_added"], pv["n_new_voxels"]):
            sys.exit("map_preview_time: the sides disagree: %r against %r" % ((added, new), (pv["n_added"], pv["n_new_voxels"])))
        if i >= WARMUP:
            t_us.append((b - a) * 1e6)
    out["us"] = round(float(np.median(t_us)), 3)
    sc.destroy()
    gm.release()
    ctx.close()
    return out


def child(args, timeout=280) -> dict:
    import subprocess
    print("map_preview_time:", " ".join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_preview_time.json"))
    ap.add_argument("--one", default="", choices=("",) + CASES, help="run one case and one side in this process and print its JSON")
    ap.add_argument("--side", default="preview", choices=SIDES)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.side, a.repeats)))
        return
    out = {"tool": "map_preview_time", "cases": []}
    for case in CASES:
        runs = {s: [] for s in SIDES}
        for _ in range(a.rounds):
            for side in SIDES:  # alternating fresh processes
                runs[side].append(child(["--one", case, "--side", side, "--repeats", str(a.repeats)]))
        first = runs["preview"][0]
        row = {"case": case, "repeats": a.repeats, "rounds": a.rounds, "body_points": first["body_points"], "map_points": first["map_points"],
               "map_voxels": first["map_voxels"], "preview": first["preview"]}
        for side in SIDES:
            vals = [q["us"] for q in runs[side]]
            row[side + "_us"] = round(float(np.median(vals)), 3)
            row[side + "_us_runs"] = vals
        row["copy_route_over_preview"] = round(row["copy_route_us"] / row["preview_us"], 2)
        row["insert_over_preview"] = round(row["insert_us"] / row["preview_us"], 2)
        row["preview_not_slower_than_copy_route"] = bool(row["preview_us"] <= row["copy_route_us"])
        out["cases"].append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
