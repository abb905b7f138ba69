"""One create / use once / destroy round of every handle type of the C ABI at small shapes (make_cycle), and, run as a script, the
child process of tests/test_gpu_handle_lifetime.py::test_nothing_leaks: WARM rounds, a marker line on stderr, ROUNDS more rounds,
shutdown.  With MH_ALLOC_TRACE=1 in its environment every trip of the allocation cache to the runtime is a line on stderr; the
parent counts the lines behind the marker.  tools/leak_check.py runs the same round."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MARKER = "handle_lifetime_worker: warm"
WARM, ROUNDS = 3, 10


def make_cycle(ctx):
    """The inputs are made once; no block of a round comes near the 64 MiB the device cache refuses."""
    from mimosa_amd import capi, synth, synth_photo as sp, synth_radar as sr

    m, pts, aux = synth.small_world()
    R, t = synth.query_pose(aux["R_W_L"], aux["t_W_L"])
    rc = capi.make_reg_config(**synth.enwide_config())
    raw, _ = synth.make_raw_scan(16, n_cols=256)
    icfg = capi.make_input_config()
    pcfg = sp.photo_config(rows=32, cols=256)
    fr = [sp.make_frame(pcfg, k) for k in range(2)]
    rng = np.random.default_rng(5)
    scene = sr.make_scene(n_static=300, n_dynamic=10, seed=3)
    rraw, rlay = sr.pack(scene["points"], "mmwave")
    rcfg, rst = capi.make_radar_config(**scene["cfg"]), sr.random_state(rng)
    poses_R = np.stack([R @ synth.rot_z(0.01 * k) for k in range(8)])
    poses_t = np.stack([t + np.array([0.05 * k, 0.0, 0.0]) for k in range(8)])
    acfg = capi.make_align_config(max_iters=3)
    xyz = synth.points_xyz(pts)
    edges = [dict(a=0, b=1, Z=(np.eye(3), np.array([1.0, 0.0, 0.0])), info=np.eye(6))]

    def cycle():
        gm = capi.VoxelMap(ctx)
        gm.insert(m)
        g2 = gm.copy()
        g2.insert(m[:500] + np.float32(0.3))
        f = capi.ICPFactor(ctx, g2, pts, rc)
        f.linearize(R, t)
        c = f.clone()
        capi.linearize_batch([f, c], [R] * 2, [t] * 2)
        f.align(R, t, acfg)
        c.score_poses(poses_R, poses_t, 1.0, top_k=2)
        sc = capi.Scan(ctx)
        sc.prefetch(raw)
        sc.prepare_input_prefetched(icfg)
        sc.deskew(np.tile(np.r_[np.eye(3).ravel(), np.zeros(3)], (len(sc.unique_ns()), 1)))
        P = capi.Photo(ctx, pcfg)
        P.preprocess(fr[0]["raw"], fr[0]["deskewed"], fr[0]["unique_ns"], fr[0]["T_Le_Lt"])
        P.detect(20, fr[0]["R_W_Be"], fr[0]["t_W_Be"], sp.BIAS_DIRECTIONS)
        P.preprocess(fr[1]["raw"], fr[1]["deskewed"], fr[1]["unique_ns"], fr[1]["T_Le_Lt"])
        pf = P.make_factor() if P.features() else None
        if pf:
            pf.linearize(fr[1]["R_W_Be"], fr[1]["t_W_Be"])
        rs = capi.RadarScan(ctx)
        rs.prepare_input(rraw, sr.capi_layout(rlay), rcfg)
        rf = capi.RadarFactor(ctx, rs, rst["R_B_S"], rst["t_B_S"], rst["omega"], 0.1)
        rf.linearize(rst["R_W_B"], rst["v_W"], rst["bias_gyro"])
        db = capi.PlaceDatabase(ctx, capacity=8)
        db.add(db.describe(xyz), tag=1)
        db.query(db.describe(xyz), top_k=1)
        pg = capi.PoseGraph(ctx, 8, 4)
        pg.set_poses(np.stack([np.eye(3)] * 2), np.array([[0.0, 0.0, 0.0], [1.1, 0.0, 0.0]]))
        pg.set_fixed([1, 0])
        pg.set_edges(edges)
        pg.optimise(iters=2)
        ks = capi.KeyframeStore(ctx, capacity_keyframes=4, capacity_points=1 << 14)
        ks.add(xyz, tag=2)
        ks.get(0)
        for h in (ks, pg, db, rf, rs, pf, P, sc, c, f):
            if h:
                h.destroy()
        g2.release()
        gm.release()

    return cycle


if __name__ == "__main__":
    from mimosa_amd import capi

    ctx = capi.Context(0)
    cycle = make_cycle(ctx)
    for _ in range(WARM):
        cycle()
    ctx.synchronize()
    print(MARKER, file=sys.stderr, flush=True)
    for _ in range(ROUNDS):
        cycle()
    ctx.close()
    print("handle_lifetime_worker: done", flush=True)
