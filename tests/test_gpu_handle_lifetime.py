"""-m gpu: the host bookkeeping of the handles, through the C ABI.  (1) Pinned staging that grows: on every entry point whose
staging grows with the batch, a small call, a call past the first 64 KiB class and the small call again on ONE handle give what
the same call gives on a fresh handle, bit for bit (a recycled pinned block is not zeroed: a path that read before it wrote
would show here).  (2) One context with a place database, a pose graph and two keyframe stores is shut down under them.  (3) A
process that creates, uses and destroys one of every handle type round after round asks the runtime for nothing once it is warm."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import handle_lifetime_worker as worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL, BIG = 500, 6000  # points: 6 000 x 12 B of packed xyz = 72 000 B, past the first class (65 536 B)


def _clouds(seed):
    """small, big, small again: three clouds in regions of their own (1 km apart), so that what a map holds of one of them is what
    a fresh map holds of it alone"""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate((SMALL, BIG, SMALL)):
        xyz = rng.uniform(-20.0, 20.0, (n, 3)).astype(np.float32)
        xyz[:, 2] = rng.uniform(-1.5, 8.0, n).astype(np.float32)
        xyz[:, 0] += np.float32(1024.0 * k)
        out.append(np.ascontiguousarray(xyz))
    return out


def _rows_sorted(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))].tobytes()


# ---- 1. staging growth ---------------------------------------------------------------------------------------------------------
def test_map_insert_staging_growth(ctx):
    from mimosa_amd import capi
    clouds = _clouds(1)
    one = capi.VoxelMap(ctx)
    for k, xyz in enumerate(clouds):
        one.insert(xyz)
        got = one.get_cloud()
        mine = got[(got[:, 0] > 1024.0 * k - 512.0) & (got[:, 0] < 1024.0 * k + 512.0)]
        fresh = capi.VoxelMap(ctx)
        fresh.insert(xyz)
        ref = fresh.get_cloud()
        assert len(ref) > 0.5 * len(xyz) and _rows_sorted(mine) == _rows_sorted(ref), k
        fresh.release()
    one.release()


def test_place_describe_add_staging_growth(ctx):
    from mimosa_amd import capi
    clouds = [c - np.float32([1024.0 * k, 0, 0]) for k, c in enumerate(_clouds(2))]  # (back around the sensor: the descriptor's range)
    one = capi.PlaceDatabase(ctx, capacity=4)
    for k, xyz in enumerate(clouds):
        d = one.describe(xyz)
        i = one.add(d, tag=k)
        fresh = capi.PlaceDatabase(ctx, capacity=4)
        ref = fresh.describe(xyz)
        j = fresh.add(ref, tag=k)
        assert d.any() and d.tobytes() == ref.tobytes(), k
        assert one.get(i)[0].tobytes() == fresh.get(j)[0].tobytes() == d.tobytes() and one.get(i)[1] == k
        fresh.destroy()
    one.destroy()


def test_keyframes_add_get_staging_growth(ctx):
    from mimosa_amd import capi
    one = capi.KeyframeStore(ctx, capacity_keyframes=4, capacity_points=1 << 14)
    for k, xyz in enumerate(_clouds(3)):
        i = one.add(xyz, tag=10 + k)
        got, tag = one.get(i)  # (the read-back stages float4: 6 000 x 16 B crosses the class as well)
        fresh = capi.KeyframeStore(ctx, capacity_keyframes=4, capacity_points=1 << 14)
        ref, _ = fresh.get(fresh.add(xyz, tag=10 + k))
        assert tag == 10 + k and got.tobytes() == ref.tobytes() == xyz.tobytes(), k
        fresh.destroy()
    one.destroy()


def test_pose_graph_set_poses_staging_growth(ctx):
    from mimosa_amd import capi, synth
    rng = np.random.default_rng(4)
    one = capi.PoseGraph(ctx, 1024, 8)
    for k, n in enumerate((10, 1000, 10)):  # 1 000 poses x 96 B = 96 000 B of staging
        R = np.stack([synth.so3_exp(w) for w in rng.normal(0.0, 0.3, (n, 3))])
        t = rng.normal(0.0, 5.0, (n, 3))
        one.set_poses(R, t)
        gR, gt = one.poses()
        fresh = capi.PoseGraph(ctx, 1024, 8)
        fresh.set_poses(R, t)
        fR, ft = fresh.poses()
        assert gR.tobytes() == fR.tobytes() == R.tobytes() and gt.tobytes() == ft.tobytes() == t.tobytes(), k
        fresh.destroy()
    one.destroy()


def test_score_poses_staging_growth(ctx, small_world):
    from mimosa_amd import capi, synth
    w = small_world
    gmap = capi.VoxelMap(ctx)
    gmap.insert(w["map_xyz"])
    rc = capi.make_reg_config(**w["cfg"])
    rng = np.random.default_rng(5)
    one = capi.ICPFactor(ctx, gmap, w["pts"], rc)
    for k, n in enumerate((8, 600, 8)):  # 256 + 600 x 96 + 600 x 24 B = 72 256 B of staging
        R = np.stack([w["R"] @ synth.rot_z(a) for a in rng.normal(0.0, 0.05, n)])
        t = w["t"] + rng.normal(0.0, 0.2, (n, 3))
        scores, best = one.score_poses(R, t, 1.0, top_k=4)
        fresh = capi.ICPFactor(ctx, gmap, w["pts"], rc)
        fs, fb = fresh.score_poses(R, t, 1.0, top_k=4)
        assert scores.tobytes() == fs.tobytes() and np.array_equal(best, fb) and best[0] >= 0, k
        fresh.destroy()
    one.destroy()
    gmap.release()


def test_photo_preprocess_staging_growth(ctx):
    """32 x 1 024 is the smallest image whose corrected intensities (4 B per point) pass the first class; the small calls hand over
    its first eight rows"""
    from mimosa_amd import capi, synth_photo as sp
    cfg = sp.photo_config(rows=32, cols=1024)
    fr = sp.make_frame(cfg, 0)
    n_all = len(fr["raw"])
    assert n_all * 4 > 65536

    def intensities(P, n):
        return P.preprocess(fr["raw"][:n], fr["deskewed"][:n], fr["unique_ns"], fr["T_Le_Lt"])["intensity"].tobytes()

    one = capi.Photo(ctx, cfg)
    for k, n in enumerate((8 * 1024, n_all, 8 * 1024)):
        got = intensities(one, n)
        fresh = capi.Photo(ctx, cfg)
        assert got == intensities(fresh, n) and got != fr["deskewed"][:n]["intensity"].tobytes(), k
        fresh.destroy()
    one.destroy()


# ---- 2. mixed teardown ---------------------------------------------------------------------------------------------------------
def test_mixed_teardown():
    from mimosa_amd import capi
    L, p, OK, INV = capi.load(), capi._p, capi.MH_OK, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    h, db, pg, k1, k2 = (C.c_void_p() for _ in range(5))
    assert L.mh_init(0, C.byref(h)) == OK
    pcfg, kcfg = capi.make_place_config(capacity=4), capi.KeyframesConfig(4, 0, 64)
    assert L.mh_place_db_create(h, C.byref(pcfg), C.byref(db)) == OK
    assert L.mh_pose_graph_create(h, 4, 2, C.byref(pg)) == OK
    assert L.mh_keyframes_create(h, C.byref(kcfg), C.byref(k1)) == OK
    assert L.mh_keyframes_create(h, C.byref(kcfg), C.byref(k2)) == OK
    xyz, desc = np.ones((4, 3), np.float32), np.zeros(capi.PLACE_CELLS, np.float32)
    desc[:60] = 1.0
    R, t = np.tile(np.eye(3).ravel(), (2, 1)), np.zeros((2, 3))
    assert L.mh_place_db_add(db, p(desc), 1, None) == OK
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 2) == OK
    assert L.mh_keyframes_add(k1, p(xyz), 4, 3, 1, None) == OK and L.mh_keyframes_add(k2, p(xyz), 4, 3, 2, None) == OK
    L.mh_keyframes_destroy(k1)  # the list must not keep it: mh_shutdown would write through a dangling entry
    L.mh_shutdown(h)
    # every remaining handle refuses a call with its own text
    assert L.mh_place_db_add(db, p(desc), 1, None) == INV
    assert L.mh_last_error(None) == b"mh_place_db_add: the database's context was shut down; the handle can only be destroyed"
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 2) == INV
    assert L.mh_last_error(None) == b"mh_pose_graph_set_poses: the graph's context was shut down; the handle can only be destroyed"
    assert L.mh_keyframes_add(k2, p(xyz), 4, 3, 2, None) == INV
    assert L.mh_last_error(None) == b"mh_keyframes_add: the store's context was shut down; the handle can only be destroyed"
    assert L.mh_place_db_size(db) == 0 and L.mh_keyframes_size(k2) == 0
    # not in the order they were created in
    L.mh_keyframes_destroy(k2)
    L.mh_place_db_destroy(db)
    L.mh_pose_graph_destroy(pg)
    # a second context works
    h2, k3, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert L.mh_init(0, C.byref(h2)) == OK
    assert L.mh_keyframes_create(h2, C.byref(kcfg), C.byref(k3)) == OK
    assert L.mh_keyframes_add(k3, p(xyz), 4, 3, 3, None) == OK and L.mh_keyframes_size(k3) == 1
    out = np.zeros((4, 3), np.float32)
    assert L.mh_keyframes_get(k3, 0, p(out), 4, C.byref(n), None) == OK and n.value == 4 and np.array_equal(out, xyz)
    L.mh_keyframes_destroy(k3)
    L.mh_shutdown(h2)


# ---- 3. nothing leaks ----------------------------------------------------------------------------------------------------------
def test_nothing_leaks():
    """Ten rounds of every handle type behind three warm-up rounds: every block of every round comes from the caches, device and
    pinned, so the allocation trace is silent behind the marker.  (A member a teardown forgets is one line per round here.)"""
    env = dict(os.environ, MH_ALLOC_TRACE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "handle_lifetime_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    before, marker, after = r.stderr.partition(worker.MARKER)
    assert marker, r.stderr[-2000:]
    warm = [ln for ln in before.splitlines() if ln.startswith("AllocCache:")]
    late = [ln for ln in after.splitlines() if ln.startswith("AllocCache:")]
    print(f"allocation trace: {len(warm)} lines while warming up, {len(late)} behind the marker")
    for ln in late:
        print(ln)
    assert any("hipMalloc" in ln for ln in warm) and any("hipHostMalloc" in ln for ln in warm)  # the trace is on, both paths
    assert late == []
