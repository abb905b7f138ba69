"""-m gpu: map carving (mh_map_carve*): the map points a scan sees through, removed on the device.  Removed sets and counters
against the numpy restatement (tests/map_carve_ref.py) fed from the map's own get_cloud(), exactly; every internal structure
against a twin built by one insert of the carved map's cloud; the preview against the apply form; the LRU stamps through the next
purge; the three entry forms against each other.  The scenes are tests/map_carve_scenes.py."""
import ctypes as C
import os

import numpy as np
import pytest

import map_carve_ref as ref
import map_carve_scenes as scenes

pytestmark = pytest.mark.gpu

LIN_KEYS = ("H_ss", "b_s", "f", "status_hist", "loc_trans_comp", "loc_rot_comp")
I9, Z3 = np.eye(3).ravel(), np.zeros(3)


def expected(gm, S, leaf=0.5):
    """(counters, removed mask over gm.get_cloud(), the cloud) by the restatement"""
    cloud = gm.get_cloud()
    counters, removed = ref.carve(cloud, ref.voxel_counts(cloud, leaf), S["obs"], S["origin"], S["R"], S["t"], S["cfg"])
    return counters, removed, cloud


def carve(gm, S, apply):
    return gm.carve(S["obs"], S["origin"], S["R"], S["t"], dict(S["cfg"], apply=apply))


def check_carve(gm, S):
    """preview and apply on gm against the restatement: counters exact, the cloud afterwards is the old one minus the removed set,
    in order.  Returns (counters, removed mask, cloud before)."""
    want, removed, cloud0 = expected(gm, S)
    stats0 = gm.stats()
    assert carve(gm, S, False) == want
    assert gm.stats() == stats0 and np.array_equal(gm.get_cloud(), cloud0)
    assert carve(gm, S, True) == want
    cloud1 = gm.get_cloud()
    assert np.array_equal(cloud1, cloud0[~removed])
    st = gm.stats()
    assert st["n_points"] == len(cloud1) == stats0["n_points"] - want["n_removed"]
    assert st["n_voxels"] == stats0["n_voxels"] - want["n_voxels_emptied"]
    assert (st["uploads"], st["upload_bytes"]) == (stats0["uploads"], stats0["upload_bytes"])
    return want, removed, cloud0


def knn_queries(cloud, seed=4, n=80):
    rng = np.random.default_rng(seed)
    if len(cloud) == 0:
        return rng.normal(0, 3.0, (n, 3))
    return cloud[rng.integers(0, len(cloud), n)].astype(np.float64) + rng.normal(0, 0.2, (n, 3))


def assert_same_map(a, b, q, ks=(1, 5)):
    sa, sb = a.stats(), b.stats()
    for k in ("n_voxels", "n_points", "n_blocks"):
        assert sa[k] == sb[k], k
    assert np.array_equal(a.get_cloud(), b.get_cloud())
    for k in ks:
        for x, y in zip(a.knn(q, k), b.knn(q, k)):
            assert np.array_equal(x, y)


def twin_of(ctx, gm, **kw):
    from mimosa_amd import capi
    tw = capi.VoxelMap(ctx, **kw)
    tw.insert(gm.get_cloud())
    return tw


def designed_map(ctx, with_lone, **kw):
    from mimosa_amd import capi
    S = scenes.designed(with_lone)
    gm = capi.VoxelMap(ctx, min_dist=0.0, **kw)
    gm.insert(S["points"])
    assert gm.stats()["n_points"] == len(S["points"])       # every point is in: nothing was too close, no voxel over the cap
    return gm, S


# ---- 1. the designed scene ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lone", [True, False])
def test_designed_scene(ctx, with_lone):
    gm, S = designed_map(ctx, with_lone)
    cloud = gm.get_cloud()
    row = {p.tobytes(): k for k, p in enumerate(S["points"])}
    order = np.array([row[p.tobytes()] for p in cloud])     # cloud row -> batch row
    if with_lone:
        assert order[0] == 0 and order[-1] == len(S["points"]) - 1   # voxel id 0 and the last voxel hold the two points put there
    img, n_used = ref.image(S["obs"], S["origin"], S["cfg"])
    dec = ref.decide(cloud, img, S["origin"], S["R"], S["t"], S["cfg"])
    wrong = [(S["label"][order[k]], int(dec[k])) for k in range(len(cloud)) if dec[k] != S["want"][order[k]]]
    assert not wrong, wrong                                   # the scene is what it says: each case gets its designed decision
    want, removed, _ = check_carve(gm, S)
    assert want["n_obs_used"] == n_used == len(S["obs"]) - S["n_obs_unused"] and want["n_cells_hit"] == S["n_cells_hit"]
    assert want["n_removed"] == int((S["want"] == ref.SEEN_THROUGH).sum()) and want["n_tested"] == int((S["want"] != ref.UNTESTED).sum())
    assert (want["n_voxels_emptied"] > 0) == with_lone
    # the voxel at the cap lost its slots 0, 7 and 19 and keeps the other seventeen in order
    cap = [k for k in range(len(cloud)) if S["label"][order[k]].startswith("cap slot")]
    assert [S["label"][order[k]] for k in cap] == ["cap slot %d" % s for s in range(20)]
    assert np.flatnonzero(removed[cap]).tolist() == [0, 7, 19]
    tw = twin_of(ctx, gm, min_dist=0.0)
    assert_same_map(gm, tw, np.concatenate([knn_queries(gm.get_cloud()), cloud[cap].astype(np.float64) + 0.01]))
    tw.release()
    gm.release()


# ---- 2. the twin ------------------------------------------------------------------------------------------------------------
def scene_map(ctx, S, **kw):
    from mimosa_amd import capi
    gm = capi.VoxelMap(ctx, **kw)
    for b in S["map_batches"]:
        gm.insert(b)
    return gm


@pytest.mark.parametrize("mode", [7, 19, 27])
def test_twin_holds_every_structure_to_the_inserts_own(ctx, small_world, mode):
    from mimosa_amd import capi
    S = scenes.random_scene(7, small_world)
    gm = scene_map(ctx, S, mode=mode)
    want, removed, cloud0 = check_carve(gm, S)
    assert want["n_removed"] > 100 and want["n_voxels_emptied"] > 0 and want["n_voxels_touched"] > want["n_voxels_emptied"]
    tw = twin_of(ctx, gm, mode=mode)
    q = np.concatenate([knn_queries(gm.get_cloud()), cloud0[removed][:40].astype(np.float64)])   # also where points were taken away
    assert_same_map(gm, tw, q)
    cfg = capi.make_reg_config(**small_world["cfg"])
    fa, fb = capi.ICPFactor(ctx, gm, small_world["pts"], cfg), capi.ICPFactor(ctx, tw, small_world["pts"], cfg)
    la, lb = fa.linearize(small_world["R"], small_world["t"]), fb.linearize(small_world["R"], small_world["t"])
    for k in LIN_KEYS:
        assert np.array_equal(la[k], lb[k]), k
    fa.destroy()
    fb.destroy()
    tw.release()
    gm.release()


# ---- 3. the preview -----------------------------------------------------------------------------------------------------------
def test_preview_moves_nothing(ctx, small_world):
    S = scenes.random_scene(8, small_world)
    base = scene_map(ctx, S)
    gm, never, applied = base.copy(), base.copy(), base.copy()   # three copies: their eight stats start out equal, device_bytes included
    base.release()
    q = knn_queries(gm.get_cloud())
    stats0 = gm.stats()
    assert len(stats0) == 8
    pv = carve(gm, S, False)
    assert pv == carve(gm, S, False) == carve(applied, S, True) and pv["n_removed"] > 0
    assert gm.stats() == stats0 == never.stats()
    assert_same_map(gm, never, q)
    batch = small_world["map_xyz"][:1500] + np.float32(0.04)
    assert gm.preview_insert(batch) == never.preview_insert(batch)
    gm.insert(batch)
    never.insert(batch)
    assert gm.stats() == never.stats()
    assert_same_map(gm, never, q)
    for g in (gm, never, applied):
        g.release()


# ---- 4. nothing seen through ------------------------------------------------------------------------------------------------
def test_nothing_seen_through_leaves_the_map_alone(ctx, small_world):
    S = scenes.random_scene(9, small_world)
    S["map_batches"] = S["map_batches"][:1]                  # the room alone, seen by its own scan with a margin wider than its noise
    S["cfg"] = dict(S["cfg"], ring=1, margin_abs=0.5, margin_rel=0.0, range_max=8.0)
    gm = scene_map(ctx, S)
    never = gm.copy()
    stats0 = gm.stats()
    want, removed, _ = expected(gm, S)
    assert want["n_removed"] == 0 and want["n_tested"] > 1000 and want["n_cells_hit"] > 0
    assert carve(gm, S, True) == want and want["n_voxels_emptied"] == 0 == want["n_voxels_touched"]
    assert gm.stats() == stats0                              # device_bytes too: no array was replaced, no compaction ran
    assert_same_map(gm, never, knn_queries(gm.get_cloud()))
    gm.release()
    never.release()


# ---- 5. everything seen through ---------------------------------------------------------------------------------------------
def test_everything_seen_through_leaves_a_new_map(ctx, small_world):
    from mimosa_amd import capi
    rng = np.random.default_rng(3)
    d = rng.standard_normal((300, 3))
    pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (300, 1))).astype(np.float32)
    S = dict(obs=np.array([12.0 * scenes.cell_dir(f, i, j) for f in range(6) for j in range(8) for i in range(8)], np.float32), origin=Z3, R=I9, t=Z3,
             cfg=dict(grid=8, ring=2, range_min=0.5, range_max=10.0, margin_abs=0.3, margin_rel=0.01))
    gm = capi.VoxelMap(ctx)
    gm.insert(pts)
    n0 = gm.stats()["n_points"]
    want, removed, _ = check_carve(gm, S)
    assert removed.all() and want["n_removed"] == n0 and want["n_voxels_emptied"] == want["n_voxels_touched"] > 1
    st = gm.stats()
    assert (st["n_voxels"], st["n_points"], st["n_blocks"]) == (0, 0, 0) and len(gm.get_cloud()) == 0
    q = knn_queries(pts)
    assert not gm.knn(q, 1)[2].any()
    new = capi.VoxelMap(ctx)
    batch = small_world["map_xyz"][:2000]
    gm.insert(batch)
    new.insert(batch)
    assert_same_map(gm, new, knn_queries(batch))
    assert carve(gm, S, True)["n_removed"] == carve(new, S, True)["n_removed"]    # and it can be carved again
    assert_same_map(gm, new, knn_queries(batch))
    gm.release()
    new.release()


# ---- 6. the LRU stamps ------------------------------------------------------------------------------------------------------
def test_lru_generations_survive_the_carve(ctx, small_world):
    """an old generation (x voxels below the middle, stamped at insert 0) and a young one (stamped at insert 1), both carved
    partly; horizon 3, purge at every fourth insert (stamp + 3 < 4 only for stamp 0): at the fourth insert the old generation goes, in the carved map and in
    the uncarved copy alike, and the young one stays"""
    from mimosa_amd import capi
    S = scenes.random_scene(10, small_world)
    allp = np.concatenate(S["map_batches"])
    vx = np.floor(allp[:, 0].astype(np.float64) * 2.0)
    mid = np.median(vx)
    old, young = allp[vx < mid], allp[vx >= mid]
    gm = capi.VoxelMap(ctx, lru_horizon=3, lru_clear_cycle=4)
    gm.insert(old)
    gm.insert(young)
    plain = gm.copy()
    want, removed, cloud0 = check_carve(gm, S)
    is_old = lambda c: np.floor(c[:, 0].astype(np.float64) * 2.0) < mid
    assert (removed & is_old(cloud0)).sum() > 20 and (removed & ~is_old(cloud0)).sum() > 20 and want["n_voxels_emptied"] > 0
    n_old = int(is_old(gm.get_cloud()).sum())
    assert 0 < n_old < int(is_old(plain.get_cloud()).sum())
    far = np.array([500.0, 0.0, 0.0], np.float32)
    for k in (2, 3):                                         # the third insert, then the fourth, which purges
        batch = small_world["map_xyz"][:300] + far * np.float32(k)
        gm.insert(batch)
        plain.insert(batch)
        cg, cp = gm.get_cloud(), plain.get_cloud()
        near_g, near_p = cg[cg[:, 0] < 400.0], cp[cp[:, 0] < 400.0]
        if k == 2:
            assert int(is_old(near_g).sum()) == n_old and int(is_old(near_p).sum()) > n_old
        else:
            assert int(is_old(near_g).sum()) == 0 == int(is_old(near_p).sum())
        assert np.array_equal(near_g[~is_old(near_g)], cloud0[~removed & ~is_old(cloud0)])      # the young survivors stay, in order
        assert np.array_equal(near_p[~is_old(near_p)], cloud0[~is_old(cloud0)])
    tw = twin_of(ctx, gm, lru_horizon=3, lru_clear_cycle=4)
    assert_same_map(gm, tw, knn_queries(gm.get_cloud()))
    for g in (gm, plain, tw):
        g.release()


# ---- 7. a factor from before the carve --------------------------------------------------------------------------------------
def test_factor_created_before_the_carve(ctx, small_world):
    from mimosa_amd import capi
    S = scenes.random_scene(11, small_world)
    gm = scene_map(ctx, S)
    cfg = capi.make_reg_config(**small_world["cfg"])
    before = capi.ICPFactor(ctx, gm, small_world["pts"], cfg)
    before.linearize(small_world["R"], small_world["t"])   # it holds associations into the uncarved map now
    want, _, _ = check_carve(gm, S)
    assert want["n_removed"] > 100 and want["n_voxels_emptied"] > 0
    before.reset()
    lin1 = before.linearize(small_world["R"], small_world["t"])
    fresh = capi.ICPFactor(ctx, gm, small_world["pts"], cfg)
    lin2 = fresh.linearize(small_world["R"], small_world["t"])
    for k in LIN_KEYS:
        assert np.array_equal(lin1[k], lin2[k]), k
    before.destroy()
    fresh.destroy()
    gm.release()


# ---- 8. the entry forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_entry_forms_agree(ctx, small_world, which):
    from mimosa_amd import capi, synth
    raw, aux = synth.make_raw_scan(16, n_cols=64, room=(6.0, 5.0, 3.0), sensor_local=np.array([2.3, 2.6, 1.2]))
    sc = capi.Scan(ctx)
    sc.prepare_input(raw, capi.make_input_config())
    sc.deskew(aux["Rt12"][np.searchsorted(aux["unique_ns"], sc.unique_ns())])
    sc.preprocess_geometric(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    rec = sc.points(which)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    assert len(xyz) > 200                                    # the body cloud is the geometric subset: a few hundred of the 1024
    S = scenes.random_scene(12, small_world)
    S.update(obs=xyz, origin=np.array([0.01, -0.02, 0.03]), R=aux["R_W_L"].ravel(), t=aux["t_W_L"])
    maps = [scene_map(ctx, S) for _ in range(3)]
    want, removed, cloud0 = expected(maps[0], S)
    assert want["n_removed"] > 0
    d, n = C.c_void_p(), C.c_size_t()
    ctx.check(ctx.L.mh_scan_device_points(sc.h, which, C.byref(d), C.byref(n)))
    assert n.value == len(xyz)
    for apply in (False, True):
        cfg = dict(S["cfg"], apply=apply)
        got = [maps[0].carve(xyz, S["origin"], S["R"], S["t"], cfg),
               maps[1].carve_device(d, n.value, rec.dtype.itemsize // 4, S["origin"], S["R"], S["t"], cfg),
               maps[2].carve_from_scan(sc, which, S["origin"], S["R"], S["t"], cfg)]
        assert got == [want] * 3
    for g in maps:
        assert np.array_equal(g.get_cloud(), cloud0[~removed])
    assert_same_map(maps[0], maps[1], knn_queries(cloud0))
    assert_same_map(maps[0], maps[2], knn_queries(cloud0))
    for g in maps:
        g.release()
    sc.destroy()


# ---- 9. random scenes -------------------------------------------------------------------------------------------------------
def fuzz_seeds():
    return [21, 22, 23] + [1000 + i for i in range(int(os.environ.get("MH_FUZZ_EXTRA", "0")))]


@pytest.mark.parametrize("seed", fuzz_seeds())
def test_random_scenes(ctx, small_world, seed):
    S = scenes.random_scene(seed, small_world)
    gm = scene_map(ctx, S)
    want, removed, _ = check_carve(gm, S)
    print(seed, S["cfg"], want)
    assert want["n_tested"] > 500 and want["n_obs_used"] > 500
    tw = twin_of(ctx, gm)
    assert_same_map(gm, tw, knn_queries(gm.get_cloud()))
    tw.release()
    gm.release()


# ---- 10. a mover ------------------------------------------------------------------------------------------------------------
def test_a_mover_is_carved_and_the_static_room_is_not(ctx):
    from mimosa_amd import capi
    gm = capi.VoxelMap(ctx)
    for pose in scenes.MOVER_POSES[:3]:
        gm.insert(scenes.cast(pose, True)[0])
    P4 = scenes.MOVER_POSES[3]
    scan_W = scenes.cast(P4, False)[0]
    S = dict(obs=(scan_W.astype(np.float64) - P4).astype(np.float32), origin=Z3, R=I9, t=P4, cfg=dict(scenes.MOVER_CFG))
    plain = gm.copy()
    cloud0 = gm.get_cloud()
    box = scenes.on_box(cloud0)
    assert box.sum() > 100
    # ring 0 trusts one cell: it takes static points too (what the header warns of) — by the restatement, the map stays as it is
    loose = ref.carve(cloud0, ref.voxel_counts(cloud0, 0.5), S["obs"], Z3, I9, P4, dict(S["cfg"], ring=0))[1]
    assert (loose & ~box).sum() > 0
    want, removed, _ = check_carve(gm, S)
    print(want, "cabinet", int(box.sum()), "removed", int((removed & box).sum()))
    assert (removed & ~box).sum() == 0
    assert 2 * (removed & box).sum() >= box.sum()
    a, b = plain.preview_insert(scan_W), gm.preview_insert(scan_W)
    print(a, b)
    assert b["n_added"] > a["n_added"] and b["n_voxel_full"] < a["n_voxel_full"]
    gm.release()
    plain.release()


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_usable(ctx, small_world):
    from mimosa_amd import capi
    S = scenes.random_scene(13, small_world)
    gm, twin = scene_map(ctx, S), scene_map(ctx, S)
    L, p = ctx.L, capi._p
    obs, o, R, t = np.ascontiguousarray(S["obs"]), S["origin"].copy(), S["R"].copy(), S["t"].copy()
    good, out = capi.make_carve_config(**S["cfg"]), capi.MapCarveResult()
    call = lambda cfg=good, o=o, R=R, t=t, out=out, n=len(obs), xyz=obs, stride=3: L.mh_map_carve(
        gm.h, p(xyz), n, stride, p(o), p(R), p(t), C.byref(cfg) if cfg is not None else None, C.byref(out) if out is not None else None)
    INV = capi.MH_ERR_INVALID_ARG
    assert call(cfg=None) == INV and call(out=None) == INV and call(o=None) == INV and call(R=None) == INV and call(t=None) == INV
    assert call(xyz=None) == INV and call(stride=2) == INV
    for bad in (dict(grid=3), dict(grid=513), dict(ring=-1), dict(ring=3), dict(range_min=0.0), dict(range_min=-1.0), dict(range_min=5.0, range_max=5.0),
                dict(range_max=np.inf), dict(range_min=np.nan), dict(margin_abs=-0.1), dict(margin_rel=-0.1), dict(margin_abs=np.nan),
                dict(margin_rel=np.inf), dict(apply=2), dict(apply=-1)):
        kw = dict(S["cfg"], **bad)
        cfg = capi.make_carve_config(**{k: v for k, v in kw.items() if k != "apply"})
        cfg.apply = int(kw.get("apply", 1))
        assert call(cfg=cfg) == INV, bad
        with pytest.raises(capi.MhError):
            gm.carve(obs, o, R, t, cfg)
    for k in range(9):
        Rb = R.copy()
        Rb[k] = np.nan
        assert call(R=Rb) == INV
    for k in range(3):
        tb, ob = t.copy(), o.copy()
        tb[k], ob[k] = np.inf, -np.inf
        assert call(t=tb) == INV and call(o=ob) == INV
    assert call(n=0x40000000) == capi.MH_ERR_UNSUPPORTED      # refused before a byte of the batch is looked at
    assert L.mh_map_carve_device(gm.h, p(obs), 0x40000000, 3, p(o), p(R), p(t), C.byref(good), C.byref(out)) == capi.MH_ERR_UNSUPPORTED
    sc = capi.Scan(ctx)
    from_scan = lambda which: L.mh_map_carve_from_scan(gm.h, sc.h, which, p(o), p(R), p(t), C.byref(good), C.byref(out))
    assert from_scan(0) == INV and from_scan(1) == INV       # nothing prepared yet
    assert from_scan(2) == INV and from_scan(-1) == INV
    from mimosa_amd import synth
    raw, _ = synth.make_raw_scan(16, n_cols=64, room=(6.0, 5.0, 3.0), sensor_local=np.array([2.3, 2.6, 1.2]))
    sc.prepare_input(raw, capi.make_input_config())
    assert from_scan(1) == INV                               # prepared, not preprocessed: no body cloud
    assert L.mh_map_carve_from_scan(gm.h, None, 0, p(o), p(R), p(t), C.byref(good), C.byref(out)) == INV
    sc.destroy()
    # none of it touched the map, and the next carve works; zero observations remove nothing
    assert gm.stats() == twin.stats()
    assert_same_map(gm, twin, knn_queries(gm.get_cloud()))
    assert gm.carve(obs[:0], o, R, t, S["cfg"]) == dict.fromkeys(ref.COUNTERS, 0)
    assert gm.stats() == twin.stats()
    want, _, _ = check_carve(gm, S)
    assert want["n_removed"] > 0
    gm.release()
    twin.release()
