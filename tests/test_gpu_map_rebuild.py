"""-m gpu: the keyframe cloud store (mh_keyframes_*) and the map rebuilt from it at given poses (mh_map_rebuild_from_keyframes).
Every rebuild is compared with its twin — a fresh VoxelMap plus one mh_map_insert_device per keyframe, fed from the store's own
device_points — and "equal" means: get_cloud bit for bit, the stats in every field but device_bytes, knn (k = 5) on a seeded
query set, one linearize of a small factor.  The LRU stamps and the counter, which nothing reads back, are compared by carrying
both maps on through further inserts and purges.  The corridor scene and the oracle build are tests/map_rebuild_ref.py."""
import ctypes as C

import numpy as np
import pytest

import map_rebuild_ref as ref
import place_scenes as hall
from oracle import numpy_ref

pytestmark = pytest.mark.gpu

LIN_KEYS = ("H_ss", "b_s", "f", "status_hist", "loc_trans_comp", "loc_rot_comp")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def insert_entry(ctx, vmap, store, i, R, t):
    from mimosa_amd import capi
    d, n = store.device_points(i)
    ctx.check(ctx.L.mh_map_insert_device(vmap.h, d, n, 4, capi._p(f32(R)), capi._p(f32(t))))


def twin_of(ctx, store, Rs, ts, order=None, **cfg):
    from mimosa_amd import capi
    tw = capi.VoxelMap(ctx, **cfg)
    for j, i in enumerate(range(store.size()) if order is None else order):
        insert_entry(ctx, tw, store, int(i), Rs[j], ts[j])
    return tw


def factor_points(cloud, seed, n=300):
    from mimosa_amd import synth
    rng = np.random.default_rng(seed)
    xyz = cloud[rng.integers(0, len(cloud), n)] + rng.normal(0, 0.03, (n, 3)).astype(np.float32)
    pts = np.zeros(n, synth.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["pad"], pts["intensity"], pts["idx"] = 1.0, 100.0, np.arange(n)
    pts["range"] = np.linalg.norm(xyz, axis=1)
    return pts


def assert_equal_maps(ctx, a, b, seed=5):
    from mimosa_amd import capi, synth
    ca, cb = a.get_cloud(), b.get_cloud()
    assert ca.shape == cb.shape and np.array_equal(bits(ca), bits(cb))
    sa, sb = a.stats(), b.stats()
    for k in sa:
        if k != "device_bytes":
            assert sa[k] == sb[k], (k, sa[k], sb[k])
    if len(ca) == 0:
        return
    rng = np.random.default_rng(seed)
    q = ca[rng.integers(0, len(ca), 120)].astype(np.float64) + rng.normal(0, 0.2, (120, 3))
    for x, y in zip(a.knn(q, 5), b.knn(q, 5)):
        assert np.array_equal(x, y)
    cfg = capi.make_reg_config(**synth.enwide_config())
    pts = factor_points(ca, seed)
    fa, fb = capi.ICPFactor(ctx, a, pts, cfg), capi.ICPFactor(ctx, b, pts, cfg)
    la, lb = fa.linearize(np.eye(3), np.zeros(3)), fb.linearize(np.eye(3), np.zeros(3))
    for k in LIN_KEYS:
        assert np.array_equal(la[k], lb[k]), k
    fa.destroy()
    fb.destroy()


def raw_rebuild(ctx, store, R, t, order=None, n_order=None, chunk_points=0, cfg=None, rc=True):
    """the C call itself: (return code, map handle, result)"""
    from mimosa_amd import capi
    cfg = cfg or capi.MapConfig(0.5, 0.15, 20, 19, 1000, 10, 0)
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    n_order = (0 if order is None else len(order)) if n_order is None else n_order
    h, res = C.c_void_p(), capi.MapRebuildResult()
    rcfg = capi.MapRebuildConfig(chunk_points, 0)
    code = ctx.L.mh_map_rebuild_from_keyframes(store.h, C.byref(cfg), capi._p(order), n_order, capi._p(None if R is None else f32(R)),
                                               capi._p(None if t is None else f32(t)), C.byref(rcfg) if rc else None, C.byref(h), C.byref(res))
    return code, h, res


def check_rebuild(ctx, store, Rs, ts, order=None, budgets=(0, 1), **cfg):
    """the rebuild with each budget against the twin; returns the results"""
    tw = twin_of(ctx, store, Rs, ts, order, **cfg)
    out = []
    for budget in budgets:
        gm, res = store.rebuild_map((Rs, ts), order=order, chunk_points=budget, **cfg)
        K = store.size() if order is None else len(order)
        assert res["keyframes"] == K and res["n_points"] == tw.stats()["n_points"] and res["n_voxels"] == tw.stats()["n_voxels"]
        assert_equal_maps(ctx, gm, tw)
        gm.release()
        out.append(res)
    tw.release()
    return out


def random_keyframes(K, seed):
    """K seeded clouds of 300 to 2 000 points in a 6 x 6 x 2 m box around the sensor; poses with rotation, offsets of 0 and 100 m"""
    from mimosa_amd import synth
    rng = np.random.default_rng(seed)
    clouds, Rs, ts = [], [], []
    for k in range(K):
        n = int(rng.integers(300, 2001))
        clouds.append(f32(rng.uniform([-3, -3, 0], [3, 3, 2], (n, 3))))
        Rs.append(synth.so3_exp(rng.normal(0, 0.3, 3)))
        ts.append(np.array([100.0 if k % 3 == 1 else 0.0, 100.0 if k % 3 == 2 else 0.0, 0.0]) + rng.normal(0, 0.4, 3) * (k > 0))
    return clouds, f32(Rs), f32(ts)


def store_of(ctx, clouds, **kw):
    from mimosa_amd import capi
    st = capi.KeyframeStore(ctx, capacity_keyframes=kw.get("capacity_keyframes", max(len(clouds), 1)),
                            capacity_points=kw.get("capacity_points", max(sum(len(c) for c in clouds), 1)))
    for i, c in enumerate(clouds):
        assert st.add(c, tag=100 + i) == i
    return st


# ---- 1. the store -----------------------------------------------------------------------------------------------------------
def raw_scan_of(cloud, rows=32):
    from mimosa_amd import synth
    cloud = np.asarray(cloud, np.float32)
    raw = np.zeros(len(cloud), synth.OUSTER_DTYPE)
    raw["x"], raw["y"], raw["z"] = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    raw["pad"], raw["intensity"] = 1.0, 100.0
    raw["ring"] = (np.arange(len(cloud)) // (len(cloud) // rows)).astype(np.uint16)
    return raw


def scan_of(ctx, cloud):
    from mimosa_amd import capi
    sc = capi.Scan(ctx)
    sc.prepare_input(raw_scan_of(cloud), capi.make_input_config())
    sc.preprocess_geometric(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    return sc


def scan_xyz(sc, which):
    rec = sc.points(which)
    return np.stack([rec["x"], rec["y"], rec["z"]], 1)


@pytest.mark.parametrize("which", [0, 1])
def test_store_entry_forms_agree(ctx, which):
    from mimosa_amd import capi
    sc = scan_of(ctx, hall.keyframes()[7][2])
    xyz = scan_xyz(sc, which)
    n = len(xyz)
    assert n > (6000 if which == 0 else 200)
    st = capi.KeyframeStore(ctx, capacity_keyframes=8, capacity_points=5 * n)
    d, dn = C.c_void_p(), C.c_size_t()
    ctx.check(ctx.L.mh_scan_device_points(sc.h, which, C.byref(d), C.byref(dn)))
    assert dn.value == n
    wide = np.full((n, 5), 7.0, np.float32)  # a host stride that is not 3
    wide[:, :3] = xyz
    assert [st.add(xyz, tag=-5), st.add_device(d, n, sc.points(which).dtype.itemsize // 4, tag=6), st.add_from_scan(sc, which, tag=2 ** 40),
            st.add(wide, tag=8)] == [0, 1, 2, 3]
    assert st.add(np.zeros((0, 3), np.float32), tag=9) == 4  # a cloud of 0 points is a valid entry
    assert st.size() == 5
    info = st.info()
    assert (info["keyframes"], info["points"], info["capacity_keyframes"], info["capacity_points"]) == (5, 4 * n, 8, 5 * n)
    assert info["device_bytes"] >= 5 * n * 16
    for i, tag in enumerate([-5, 6, 2 ** 40, 8]):
        got, t = st.get(i)
        assert t == tag and got.shape == (n, 3) and np.array_equal(bits(got), bits(xyz)), i
    got, t = st.get(4)
    assert got.shape == (0, 3) and t == 9 and st.device_points(4)[1] == 0
    # device_points: entry 2's address, read through the stride-4 device form into a new entry
    dp, np_ = st.device_points(2)
    assert np_ == n and dp.value
    only_count = C.c_size_t()
    ctx.check(ctx.L.mh_keyframes_get(st.h, 2, None, 0, C.byref(only_count), None))
    assert only_count.value == n
    assert st.add_device(dp, np_, 4, tag=1) == 5 and np.array_equal(bits(st.get(5)[0]), bits(xyz))
    # a short read
    part = np.zeros((10, 3), np.float32)
    ctx.check(ctx.L.mh_keyframes_get(st.h, 0, capi._p(part), 10, C.byref(only_count), None))
    assert only_count.value == n and np.array_equal(bits(part), bits(xyz[:10]))
    st.destroy()
    sc.destroy()


def test_store_refusals_leave_it_as_it_was(ctx):
    from mimosa_amd import capi
    L, p, INV = ctx.L, capi._p, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    xyz = f32(np.random.default_rng(1).normal(0, 2, (100, 3)))
    st = capi.KeyframeStore(ctx, capacity_keyframes=3, capacity_points=250)
    assert st.add(xyz, 1) == 0 and st.add(xyz, 2) == 1
    before, idx = st.info(), C.c_int32(-7)
    add = lambda a=xyz, n=100, stride=3: L.mh_keyframes_add(st.h, p(a), n, stride, 0, C.byref(idx))
    assert add() == INV and b"full (points)" in L.mh_last_error(ctx.h)                # 200 + 100 > 250
    assert add(stride=2) == INV and add(a=None) == INV
    n_out, tag, d = C.c_size_t(), C.c_int64(), C.c_void_p()
    for bad in (-1, 2, 3):
        assert L.mh_keyframes_get(st.h, bad, None, 0, C.byref(n_out), C.byref(tag)) == INV
        assert L.mh_keyframes_device_points(st.h, bad, C.byref(d), C.byref(n_out)) == INV
    assert L.mh_keyframes_device_points(st.h, 0, None, C.byref(n_out)) == INV
    sc = capi.Scan(ctx)
    for which in (-1, 0, 1, 2):                                                      # no stage has run; which outside 0..1
        assert L.mh_keyframes_add_from_scan(st.h, sc.h, which, 0, C.byref(idx)) == INV
    sc.prepare_input(raw_scan_of(hall.keyframes()[0][2]), capi.make_input_config())
    assert L.mh_keyframes_add_from_scan(st.h, sc.h, 1, 0, C.byref(idx)) == INV       # prepared, not preprocessed
    assert L.mh_keyframes_add_from_scan(st.h, sc.h, 0, 0, C.byref(idx)) == INV and b"full (points)" in L.mh_last_error(ctx.h)
    sc.destroy()
    other = capi.Context(0)                                                          # a scan of another context
    so = scan_of(other, hall.keyframes()[0][2])
    assert L.mh_keyframes_add_from_scan(st.h, so.h, 1, 0, C.byref(idx)) == INV and b"another context" in L.mh_last_error(ctx.h)
    so.destroy()
    other.close()
    assert idx.value == -7 and st.info() == before
    assert st.add(xyz[:50], 3) == 2                                                  # exactly full in points, and in keyframes
    assert L.mh_keyframes_add(st.h, None, 0, 3, 0, C.byref(idx)) == INV and b"full (keyframes)" in L.mh_last_error(ctx.h)
    assert st.info()["points"] == 250 and st.size() == 3
    for i, (c, tg) in enumerate([(xyz, 1), (xyz, 2), (xyz[:50], 3)]):
        got, t = st.get(i)
        assert t == tg and np.array_equal(bits(got), bits(c))
    st.destroy()


def test_use_after_shutdown_is_refused():
    """a store is registered on its context: after mh_shutdown every call but destroy refuses it"""
    from mimosa_amd import capi
    L, p, INV = capi.load(), capi._p, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    h, st = C.c_void_p(), C.c_void_p()
    assert L.mh_init(0, C.byref(h)) == capi.MH_OK
    cfg = capi.KeyframesConfig(4, 0, 64)
    assert L.mh_keyframes_create(h, C.byref(cfg), C.byref(st)) == capi.MH_OK
    xyz = np.ones((4, 3), np.float32)
    assert L.mh_keyframes_add(st, p(xyz), 4, 3, 9, None) == capi.MH_OK and L.mh_keyframes_size(st) == 1
    L.mh_shutdown(h)
    assert L.mh_keyframes_size(st) == 0
    n, d, info, m, res = C.c_size_t(), C.c_void_p(), capi.KeyframesInfo(), C.c_void_p(), capi.MapRebuildResult()
    mcfg, R, t = capi.MapConfig(0.5, 0.15, 20, 19, 1000, 10, 0), f32(np.eye(3)), f32(np.zeros(3))
    assert L.mh_keyframes_add(st, p(xyz), 4, 3, 9, None) == INV and b"shut down" in L.mh_last_error(None)
    assert L.mh_keyframes_add_device(st, p(xyz), 4, 3, 9, None) == INV
    assert L.mh_keyframes_get(st, 0, None, 0, C.byref(n), None) == INV
    assert L.mh_keyframes_device_points(st, 0, C.byref(d), C.byref(n)) == INV
    assert L.mh_keyframes_get_info(st, C.byref(info)) == INV
    assert L.mh_map_rebuild_from_keyframes(st, C.byref(mcfg), None, 0, p(R), p(t), None, C.byref(m), C.byref(res)) == INV and not m.value
    assert b"shut down" in L.mh_last_error(None)
    L.mh_keyframes_destroy(st)


# ---- 2. rebuild equals the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 7])
def test_rebuild_equals_the_twin(ctx, K):
    clouds, Rs, ts = random_keyframes(K, 40 + K)
    st = store_of(ctx, clouds)
    default, single = check_rebuild(ctx, st, Rs, ts)
    assert default["chunks"] == 1 and single["chunks"] == K and default["points_offered"] == sum(len(c) for c in clouds)
    if K == 7:
        check_rebuild(ctx, st, Rs, ts, budgets=(3000,), lru_clear_cycle=3, lru_horizon=1)   # cut by the budget and by the cycle
    st.destroy()


def test_empty_store_and_empty_list(ctx):
    from mimosa_amd import capi
    st = capi.KeyframeStore(ctx, capacity_keyframes=2, capacity_points=16)
    gm, res = st.rebuild_map((np.zeros((0, 3, 3)), np.zeros((0, 3))))
    assert res == dict(keyframes=0, points_offered=0, chunks=0, purges=0, n_points=0, n_voxels=0) and gm.stats()["n_points"] == 0
    gm.release()
    st.add(np.ones((3, 3), np.float32))
    gm, res = st.rebuild_map((np.zeros((0, 3, 3)), np.zeros((0, 3))), order=np.zeros(0, np.int32))
    assert res["keyframes"] == 0 and gm.stats()["n_voxels"] == 0 and gm.stats()["uploads"] == 0
    gm.release()
    st.destroy()


# ---- 3. the segment classes -------------------------------------------------------------------------------------------------
def designed_keyframes(n_voxel, fill, seed=3):
    """One voxel ((3, 2, 1) at leaf 0.5) that receives n_voxel points within one chunk, spread over three keyframes, among 200
    background points each; the first cloud twice at the same pose; an empty keyframe in the middle.  fill = False: the points
    coincide, so the bucket never fills and every trip of the segment runs.  fill = True: distinct points 0.1 m apart (min_dist
    0.05), twelve positions in the first keyframe, the rest from the second on: the bucket fills there."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij"), -1).reshape(-1, 3)   # 32 positions
    pos = f32(np.array([1.55, 1.05, 0.55]) + 0.1 * g)
    share = [n_voxel // 4, n_voxel // 4, n_voxel - 3 * (n_voxel // 4)]   # the first cloud is listed twice: n_voxel points in all
    clouds = []
    for k, m in enumerate(share):
        if fill:
            pick = (np.arange(m) % 12) if k == 0 else 12 + (np.arange(m) % 20)
            inside = pos[pick]
        else:
            inside = np.tile(f32([[1.7, 1.2, 0.7]]), (m, 1))
        back = f32(rng.uniform(-5, 5, (200, 3)))
        back = back[~np.all(np.floor(back.astype(np.float64) * 2.0) == [3, 2, 1], axis=1)]
        c = np.concatenate([inside, back])
        clouds.append(c[rng.permutation(len(c))])
    return [clouds[0], clouds[0], np.zeros((0, 3), np.float32), clouds[1], clouds[2]]


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("n_voxel", [40, 500, 1500])
def test_segment_classes(ctx, n_voxel, fill):
    clouds = designed_keyframes(n_voxel, fill)
    st = store_of(ctx, clouds)
    Rs, ts = f32(np.tile(np.eye(3), (5, 1, 1))), f32(np.zeros((5, 3)))
    default, single = check_rebuild(ctx, st, Rs, ts, min_dist=0.05)
    assert default["chunks"] == 1 and single["chunks"] == 5
    # the designed voxel holds what the design says; the second copy of the first cloud added nothing
    gm, _ = st.rebuild_map((Rs, ts), min_dist=0.05)
    cloud = gm.get_cloud()
    inside = np.all(np.floor(cloud.astype(np.float64) * 2.0) == [3, 2, 1], axis=1)
    assert inside.sum() == (20 if fill else 1)
    one, _ = st.rebuild_map((Rs[:1], ts[:1]), order=[0], min_dist=0.05)
    two, _ = st.rebuild_map((Rs[:2], ts[:2]), order=[0, 1], min_dist=0.05)
    assert np.array_equal(bits(one.get_cloud()), bits(two.get_cloud())) and two.stats()["uploads"] == 2
    for m in (gm, one, two):
        m.release()
    st.destroy()


# ---- 4. LRU -----------------------------------------------------------------------------------------------------------------
def test_lru_purges_inside_the_sequence(ctx):
    from mimosa_amd import capi
    clouds, Rs, ts = ref.corridor_scene()
    cfg = dict(ref.CORRIDOR_MAP)
    st = store_of(ctx, clouds)
    oracle = ref.sequential_build(numpy_ref.VoxelMap(**cfg), ref.corridor_world(clouds, Rs, ts))
    for budget in (0, 1000, 1):
        gm, res = st.rebuild_map((Rs, ts), chunk_points=budget, **cfg)
        tw = twin_of(ctx, st, Rs, ts, **cfg)
        assert res["purges"] == 5 and res["chunks"] == len(ref.plan([len(c) for c in clouds], 0, 5, budget or ref.DEFAULT_CHUNK_POINTS))
        assert res["chunks"] == {0: 5, 1: 25}.get(budget, res["chunks"]) and res["chunks"] >= 5
        assert (res["n_voxels"], res["n_points"]) == (len(oracle.order), oracle.num_points)       # the oracle's counts
        assert_equal_maps(ctx, gm, tw)
        # carry both on: five more inserts across the next purge (counter 30), a preview, a carve preview
        for m in (gm, tw):
            for i in range(3, 8):
                insert_entry(ctx, m, st, i, Rs[i], ts[i])
        assert gm.stats()["uploads"] == 30
        assert_equal_maps(ctx, gm, tw, seed=6)
        d, n = st.device_points(20)
        assert gm.preview_insert_device(d, n, 4, Rs[20], ts[20]) == tw.preview_insert_device(d, n, 4, Rs[20], ts[20])
        carve = dict(grid=64, ring=1, range_min=0.5, range_max=30.0, margin_abs=0.3, margin_rel=0.0, apply=False)
        origin, R64, t64 = np.zeros(3), Rs[5].astype(np.float64), ts[5].astype(np.float64)
        ca, cb = gm.carve_device(d, n, 4, origin, R64, t64, carve), tw.carve_device(d, n, 4, origin, R64, t64, carve)
        assert ca == cb and ca["n_tested"] > 0
        assert_equal_maps(ctx, gm, tw, seed=7)
        gm.release()
        tw.release()
    st.destroy()


# ---- 5. order ---------------------------------------------------------------------------------------------------------------
def test_order(ctx):
    from mimosa_amd import capi
    clouds, Rs, ts = random_keyframes(7, 77)
    st = store_of(ctx, clouds)
    for order in ([4, 0, 6, 2, 5, 1, 3], [5, 1, 3], [4, 5, 6]):      # a permutation, a subset, the last M
        check_rebuild(ctx, st, Rs[order], ts[order], order=order, lru_clear_cycle=3, lru_horizon=1)
    INV = capi.MH_ERR_INVALID_ARG
    for bad in ([0, 1, 0], [0, 7], [-1]):
        code, h, _ = raw_rebuild(ctx, st, Rs[:len(bad)], ts[:len(bad)], order=bad)
        assert code == INV and not h.value, bad
    code, h, _ = raw_rebuild(ctx, st, Rs, ts, order=None, n_order=3)  # n_order > 0 with a NULL order
    assert code == INV and not h.value
    st.destroy()


# ---- 6. insert_from_scan parity ---------------------------------------------------------------------------------------------
def test_insert_from_scan_parity(ctx):
    from mimosa_amd import capi
    st = capi.KeyframeStore(ctx, capacity_keyframes=6, capacity_points=6 * 8192)
    grown = capi.VoxelMap(ctx)
    Rs, ts = [], []
    for k in (0, 1, 6, 7, 12, 13):
        xy, yaw, cloud = hall.keyframes()[k]
        R, t = hall.pose_of(xy, yaw)
        sc = scan_of(ctx, cloud)
        grown.insert_from_scan(sc, R, t)
        st.add_from_scan(sc, capi.Scan.BODY, tag=k)
        sc.destroy()
        Rs.append(R)
        ts.append(t)
    gm, res = st.rebuild_map((Rs, ts))
    assert res["keyframes"] == 6 and res["n_points"] > 1000
    assert_equal_maps(ctx, gm, grown)
    gm.release()
    grown.release()
    st.destroy()


# ---- 7. nothing else moves --------------------------------------------------------------------------------------------------
def test_nothing_else_moves(ctx, small_world):
    from mimosa_amd import capi
    old = capi.VoxelMap(ctx)
    old.insert(small_world["map_xyz"])
    f = capi.ICPFactor(ctx, old, small_world["pts"], capi.make_reg_config(**small_world["cfg"]))
    lin0, cloud0, stats0 = f.linearize(small_world["R"], small_world["t"]), old.get_cloud(), old.stats()
    q = cloud0[::50].astype(np.float64) + 0.01
    knn0 = old.knn(q, 5)
    clouds, Rs, ts = random_keyframes(3, 5)
    st = store_of(ctx, clouds)
    gm, _ = st.rebuild_map((Rs, ts))
    f.reset()
    lin1 = f.linearize(small_world["R"], small_world["t"])
    for k in LIN_KEYS:
        assert np.array_equal(lin0[k], lin1[k]), k
    assert np.array_equal(bits(old.get_cloud()), bits(cloud0)) and old.stats() == stats0
    for x, y in zip(old.knn(q, 5), knn0):
        assert np.array_equal(x, y)
    for i, c in enumerate(clouds):                                   # ... and the store is what it was
        assert np.array_equal(bits(st.get(i)[0]), bits(c))
    f.destroy()
    gm.release()
    old.release()
    st.destroy()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_rebuild_refusals(ctx):
    from mimosa_amd import capi
    L, INV, UNS = ctx.L, capi.MH_ERR_INVALID_ARG, capi.MH_ERR_UNSUPPORTED
    L.mh_last_error.restype = C.c_char_p
    clouds, Rs, ts = random_keyframes(3, 9)
    st = store_of(ctx, clouds)
    before = st.info()
    for arr, k in ((Rs, 13), (ts, 4)):
        for v in (np.nan, np.inf):
            bad = arr.copy()
            bad.reshape(-1)[k] = v
            code, h, _ = raw_rebuild(ctx, st, bad if arr is Rs else Rs, bad if arr is ts else ts)
            assert code == INV and not h.value and b"not finite" in L.mh_last_error(ctx.h)
    assert raw_rebuild(ctx, st, None, ts)[0] == INV and raw_rebuild(ctx, st, Rs, None)[0] == INV     # NULL poses with a non-empty list
    assert raw_rebuild(ctx, st, Rs, ts, chunk_points=-1)[0] == INV
    for change in (dict(leaf_size=0.0), dict(max_points_in_cell=21), dict(neighbor_voxel_mode=5), dict(lru_clear_cycle=0), dict(lru_horizon=-1)):
        cfg = capi.MapConfig(0.5, 0.15, 20, 19, 1000, 10, 0)
        for k, v in change.items():
            setattr(cfg, k, v)
        code, h, _ = raw_rebuild(ctx, st, Rs, ts, cfg=cfg)
        assert code == INV and not h.value, change
    h, res = C.c_void_p(), capi.MapRebuildResult()
    cfg = capi.MapConfig(0.5, 0.15, 20, 19, 1000, 10, 0)
    assert L.mh_map_rebuild_from_keyframes(st.h, None, None, 0, capi._p(Rs), capi._p(ts), None, C.byref(h), C.byref(res)) == INV
    assert L.mh_map_rebuild_from_keyframes(st.h, C.byref(cfg), None, 0, capi._p(Rs), capi._p(ts), None, None, C.byref(res)) == INV
    assert L.mh_map_rebuild_from_keyframes(st.h, C.byref(cfg), None, 0, capi._p(Rs), capi._p(ts), None, C.byref(h), None) == INV
    # a pose that throws the second chunk's points beyond 2^20 voxels: no map comes back, the store stays usable
    far = ts.copy()
    far[1, 0] = 1.0e6
    code, h, res = raw_rebuild(ctx, st, Rs, far, chunk_points=1)
    assert code == UNS and not h.value and b"2^20" in L.mh_last_error(ctx.h) and res.keyframes == 0
    assert st.info() == before
    code, h, res = raw_rebuild(ctx, st, Rs, ts, rc=False)                                             # rc = NULL: the defaults
    assert code == capi.MH_OK and h.value and res.keyframes == 3 and res.chunks == 1
    gm = capi.VoxelMap(ctx, _h=h)
    tw = twin_of(ctx, st, Rs, ts)
    assert_equal_maps(ctx, gm, tw)
    gm.release()
    tw.release()
    st.destroy()


# ---- 9. end to end in the hall ----------------------------------------------------------------------------------------------
def test_end_to_end_in_the_hall(ctx):
    """Drifted keyframe poses, a pose graph with one loop edge, optimise, rebuild at the corrected poses: the rebuilt map lies on the
    map built at the true poses.  The measure is the RMS distance from the rebuilt map's points to their nearest point of the true
    map (mh_map_knn, k = 1; capped at one leaf, where that search ends).  tests/test_map_rebuild_cpu.py chose the drift so that the
    restated graph and the oracle map give a corrected RMS below a quarter of the drifted one; the device is held to a half, the
    factor of two being the margin for the device solver's stop test."""
    from mimosa_amd import capi
    case = ref.hall_case()
    st = store_of(ctx, case["clouds"])
    pg = capi.PoseGraph(ctx, 36, 36)
    pg.set_poses(*case["drifted"])
    pg.set_fixed(case["fixed"])
    pg.set_edges([{"a": a, "b": b, "Z": (ZR, Zt), "info": info} for a, b, ZR, Zt, info in case["edges"]])
    got = pg.optimise(iters=16)
    # the loop's error, spread evenly over the 36 edges of the cycle, leaves 1 / 36 of the cost it had on the one edge
    assert got["f_last"] < 1.01 * got["f_first"] / 36.0
    maps = {name: st.rebuild_map(poses, mode=27)[0] for name, poses in (("true", case["true"]), ("drifted", case["drifted"]), ("corrected", (got["R"], got["t"])))}

    def rms(m):
        cloud = m.get_cloud().astype(np.float64)
        _, sq, found = maps["true"].knn(cloud, 1)
        return ref.capped_rms(np.where(found > 0, np.sqrt(sq[:, 0]), ref.HALL_CAP)), float((found > 0).mean())

    (rms_d, found_d), (rms_c, found_c) = rms(maps["drifted"]), rms(maps["corrected"])
    print("hall, device: RMS to the true map drifted %.4f m (%.0f %% within a voxel), corrected %.4f m (%.0f %%)" % (rms_d, 100 * found_d, rms_c, 100 * found_c))
    assert rms(maps["true"])[0] == 0.0
    assert rms_d > 0.1 and rms_c < 0.5 * rms_d
    tw = twin_of(ctx, st, *[f32(a) for a in (got["R"], got["t"])], mode=27)     # ... and it is the twin's map, like every rebuild
    assert_equal_maps(ctx, maps["corrected"], tw)
    tw.release()
    for m in maps.values():
        m.release()
    pg.destroy()
    st.destroy()
