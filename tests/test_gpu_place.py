"""-m gpu: place recognition (mh_place_*): scan descriptors and a keyframe database searched on the device.  Descriptors against the
numpy restatement (tests/place_ref.py) bit for bit; {D, shift} of every searched entry to 1e-12 and, under the gap conditions
tests/test_place_cpu.py verifies for these very inputs, shifts and hits exactly; bit reproducibility across database sizes and
positions; persistence through get / add; and from hits to a pose with capi.place_relocalise in a cluttered hall.  The inputs
are tests/place_scenes.py."""
import ctypes as C

import numpy as np
import pytest

import place_ref as ref
import place_scenes as scenes

pytestmark = pytest.mark.gpu

LIN_KEYS = ("H_ss", "b_s", "f", "status_hist", "loc_trans_comp", "loc_rot_comp")
D_TOL = 1e-12   # see tests/test_place_cpu.py


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_db(ctx, **cfg):
    from mimosa_amd import capi
    return capi.PlaceDatabase(ctx, **cfg)


def raw_scan_of(cloud, rows=32):
    """a level cloud as the raw records mh_scan_prepare_input reads: one timestamp, ring = row"""
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


def tilted_R():
    from mimosa_amd import synth
    return synth.so3_exp(np.array([0.21, -0.13, 0.9]))


# ---- 1. the descriptor ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", scenes.DESIGNED_SIZES)
def test_descriptor_against_the_restatement_bit_for_bit(ctx, n):
    xyz, R = scenes.designed_cloud(n)
    db = make_db(ctx, **scenes.DESIGNED_CFG)
    for Rm in (R, tilted_R()):
        want = ref.describe(xyz, Rm, scenes.DESIGNED_CFG)
        got = db.describe(xyz, Rm)
        assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:10]
        assert np.array_equal(bits(db.describe(xyz[::-1], Rm)), bits(want))                 # the other point order
        wide = np.full((n, 5), 7.0, np.float32)                                              # a stride that is not 3
        wide[:, :3] = xyz
        out = np.empty(ref.CELLS, np.float32)
        from mimosa_amd import capi
        ctx.check(ctx.L.mh_place_describe(db.h, capi._p(wide) if n else None, n, 5, capi._p(np.ascontiguousarray(Rm, np.float64)), capi._p(out)))
        assert np.array_equal(bits(out), bits(want))
    if n == 0:
        assert not got.any()
    assert db.size() == 0
    db.destroy()


@pytest.mark.parametrize("which", [0, 1])
def test_entry_forms_agree(ctx, which):
    from mimosa_amd import capi
    kxy, kyaw, cloud = scenes.keyframes()[7]
    sc = scan_of(ctx, cloud)
    xyz = scan_xyz(sc, which)
    assert len(xyz) > (6000 if which == 0 else 200)
    db = make_db(ctx, **scenes.SCENE_CFG)
    R = tilted_R() if which else np.eye(3)
    want = ref.describe(xyz, R, scenes.SCENE_CFG)
    assert (want > 0).sum() > 100
    d, n = C.c_void_p(), C.c_size_t()
    ctx.check(ctx.L.mh_scan_device_points(sc.h, which, C.byref(d), C.byref(n)))
    assert n.value == len(xyz)
    forms = [db.describe(xyz, R), db.describe_device(d, n.value, sc.points(which).dtype.itemsize // 4, R), db.describe_from_scan(sc, which, R)]
    for got in forms:
        assert np.array_equal(bits(got), bits(want))
    # ... and the forms that never leave the device: add_from_scan's entry, query_from_scan's query
    i = db.add_from_scan(sc, which, R, tag=-5)
    assert i == 0 and db.size() == 1
    desc, tag = db.get(0)
    assert np.array_equal(bits(desc), bits(want)) and tag == -5
    hits, all_ = db.query_from_scan(sc, which, R, top_k=2, want_all=True)
    D, shift, _ = ref.distances(want, want[None], scenes.SCENE_CFG["min_overlap"])
    assert hits["index"].tolist() == [0, -1] and hits["shift"][0] == 0 == shift[0] and hits["tag"].tolist() == [-5, 0]
    assert abs(all_["dist"][0] - D[0]) <= D_TOL and abs(hits["dist"][0]) < 1e-12 and hits["dist"][1] == 2.0
    db.destroy()
    sc.destroy()


# ---- 2. the query ---------------------------------------------------------------------------------------------------------------
def filled(ctx, E, tags=None, capacity=None):
    db = make_db(ctx, **dict(scenes.DESIGNED_CFG, min_overlap=scenes.QUERY_MIN_OVERLAP, capacity=capacity or max(len(E), 1)))
    for i, e in enumerate(E):
        assert db.add(e, tag=(tags[i] if tags is not None else 1000 + i)) == i
    return db


@pytest.fixture(scope="module")
def query_ref():
    q, E = scenes.query_set()
    D, shift, gap = ref.distances(q, E, scenes.QUERY_MIN_OVERLAP)
    return dict(q=q, E=E, D=D, shift=shift, gap=gap)


@pytest.mark.parametrize("M", scenes.QUERY_SIZES)
def test_query_against_the_restatement(ctx, query_ref, M):
    q, E, D, shift = query_ref["q"], query_ref["E"][:M], query_ref["D"][:M], query_ref["shift"][:M]
    db = filled(ctx, E)
    assert db.size() == M
    worst = 0.0
    for top_k in (1, 4, 16):
        hits, all_ = db.query(q, top_k=top_k, want_all=True)
        assert len(all_) == M and len(hits) == top_k
        worst = max(worst, np.abs(all_["dist"] - D).max())
        assert np.abs(all_["dist"] - D).max() <= D_TOL
        assert np.array_equal(all_["dist"] == 2.0, D == 2.0)
        assert np.array_equal(all_["shift"], shift)      # (every shift of this set is decided by more than 1e-9: test_place_cpu.py)
        want = ref.rank(D, top_k)
        assert hits["index"].tolist() == want.tolist()
        real = want >= 0
        assert np.array_equal(hits["shift"][real], shift[want[real]]) and np.array_equal(hits["tag"][real], 1000 + want[real])
        assert np.array_equal(hits["dist"][real], all_["dist"][want[real]])
        assert (hits["dist"][~real] == 2.0).all() and (hits["shift"][~real] == 0).all() and (hits["tag"][~real] == 0).all()
        if real.any():
            assert real[:real.sum()].all()               # -1 entries sit behind the last real hit
    print("M = %d: largest |D - restatement| %.3g" % (M, worst))
    if M >= 65:
        idx = hits["index"].tolist()
        assert idx[:6] == [5, 9, 40, 41, 3, 17]          # the rotated copies, then the duplicate pair: the lower index first
        for e, s in scenes.ROTATED.items():
            assert all_["shift"][e] == s
        assert all_["dist"][3] == all_["dist"][17] and all_["dist"][0] == 2.0 == all_["dist"][1]
        # n_search cuts the search: the first n entries only, as a database of that size answers
        for n_search in (1, 4, 10, 41, M):
            h2, a2 = db.query(q, top_k=16, n_search=n_search, want_all=True)
            assert len(a2) == n_search and np.array_equal(a2, all_[:n_search])
            assert h2["index"].tolist() == ref.rank(D[:n_search], 16).tolist()
            assert (h2["index"] < n_search).all()
    # a query that matches nothing: all zero
    hits, all_ = db.query(np.zeros(ref.CELLS, np.float32), top_k=4, want_all=True)
    assert (hits["index"] == -1).all() and (all_["dist"] == 2.0).all() and (all_["shift"] == 0).all()
    db.destroy()


def test_bit_reproducibility(ctx, query_ref):
    """an entry's {dist, shift} is identical alone, in a database of 300, at another position and on a repeat"""
    q, E = query_ref["q"], query_ref["E"]
    big = filled(ctx, E)
    _, a300 = big.query(q, top_k=1, want_all=True)
    _, again = big.query(q, top_k=16, want_all=True)
    assert np.array_equal(a300, again)
    for e in (3, 5, 103, 299, 1):
        alone = filled(ctx, E[e:e + 1])
        _, a1 = alone.query(q, top_k=1, want_all=True)
        assert a1[0] == a300[e], (e, a1, a300[e])
        alone.destroy()
    perm = np.random.default_rng(8).permutation(300)
    moved = filled(ctx, E[perm])
    _, am = moved.query(q, top_k=1, want_all=True)
    assert np.array_equal(am, a300[perm])
    moved.destroy()
    big.destroy()


def test_persistence(ctx, query_ref):
    """a database rebuilt with add from what get returned answers every query bit for bit as the original; adds leave earlier entries alone"""
    q, E = query_ref["q"], query_ref["E"][:65]
    tags = [(-1) ** i * (2 ** 40 + i) for i in range(len(E))]
    a = filled(ctx, E[:30], tags, capacity=len(E))
    first = [a.get(i) for i in range(30)]
    for i in range(30, len(E)):
        a.add(E[i], tags[i])
    for i in range(30):                                  # adds leave earlier entries as they were
        d, t = a.get(i)
        assert np.array_equal(bits(d), bits(first[i][0])) and t == first[i][1] == tags[i]
        assert np.array_equal(bits(d), bits(E[i]))
    saved = [a.get(i) for i in range(len(E))]
    b = filled(ctx, [d for d, _ in saved], [t for _, t in saved])
    for query in (q, E[44], E[3], E[0]):
        ha, aa = a.query(query, top_k=16, want_all=True)
        hb, ab = b.query(query, top_k=16, want_all=True)
        assert np.array_equal(ha, hb) and np.array_equal(aa, ab)
    a.destroy()
    b.destroy()


# ---- 3. nothing else moves ------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(ctx, small_world):
    from mimosa_amd import capi
    gm = capi.VoxelMap(ctx)
    gm.insert(small_world["map_xyz"])
    f = capi.ICPFactor(ctx, gm, small_world["pts"], capi.make_reg_config(**small_world["cfg"]))
    sc = scan_of(ctx, scenes.keyframes()[0][2])
    qs = np.random.default_rng(4).normal(0, 2.0, (60, 3)) + small_world["t"]

    def snapshot():
        lin = f.linearize(small_world["R"], small_world["t"])
        f.reset()
        return gm.stats(), gm.knn(qs, 5), {k: np.array(lin[k]) for k in LIN_KEYS}, scan_xyz(sc, 0), scan_xyz(sc, 1)

    before = snapshot()
    db = make_db(ctx, **scenes.SCENE_CFG)
    db.describe(scan_xyz(sc, 0))
    db.describe_from_scan(sc, 1)
    db.add_from_scan(sc, 0, tag=1)
    db.add(ref.describe(scan_xyz(sc, 1), np.eye(3), scenes.SCENE_CFG), tag=2)
    db.query_from_scan(sc, 0, top_k=4, want_all=True)
    db.query(db.get(1)[0], top_k=2)
    after = snapshot()
    assert before[0] == after[0]
    for x, y in zip(before[1], after[1]):
        assert np.array_equal(x, y)
    for k in LIN_KEYS:
        assert np.array_equal(before[2][k], after[2][k]), k
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    db.destroy()
    sc.destroy()
    f.destroy()
    gm.release()


# ---- 4. end to end: from a scan to a pose in a map of 36 keyframes --------------------------------------------------------------
def test_end_to_end_in_the_hall(ctx):
    from mimosa_amd import capi, synth
    gm = capi.VoxelMap(ctx)
    db = make_db(ctx, **scenes.SCENE_CFG)
    poses = []
    for k, (xy, yaw, cloud) in enumerate(scenes.keyframes()):
        sc = scan_of(ctx, cloud)
        R, t = scenes.pose_of(xy, yaw)
        gm.insert_from_scan(sc, R, t)
        assert db.add_from_scan(sc, capi.Scan.FULL, tag=100 + k) == k
        poses.append((R, t))
        sc.destroy()
    assert db.size() == 36
    K = scenes.keyframe_descriptors()
    for k in (0, 17, 35):                                # the device built what the restatement builds from the same clouds
        assert np.array_equal(bits(db.get(k)[0]), bits(K[k]))
    reg = capi.make_reg_config(**synth.enwide_config())
    errs = []
    for c in scenes.queries():
        sc = scan_of(ctx, c["cloud"])
        hits, all_ = db.query_from_scan(sc, capi.Scan.FULL, top_k=4, want_all=True)
        assert np.abs(all_["dist"] - c["D"]).max() <= D_TOL
        top = c["top"][:4]
        assert hits["index"].tolist() == top.tolist() and np.array_equal(hits["shift"], c["shift"][top]) and np.array_equal(hits["tag"], 100 + top)
        f = sc.make_factor(gm, reg)
        r = capi.place_relocalise(f, hits, poses)
        assert r is not None
        R_true, t_true = scenes.pose_of(c["xy"], c["yaw"])
        dt = float(np.linalg.norm(r["t"] - t_true))
        dr = float(np.rad2deg(np.arccos(np.clip((np.trace(R_true.T @ r["R"]) - 1.0) / 2.0, -1.0, 1.0))))
        errs.append((dt, dr, r["hit"], r["index"], c["nearest"]))
        f.destroy()
        sc.destroy()
    for e in errs:
        print("pose error %.4f m %.3f deg; winning hit rank %d (keyframe %d, nearest %d)" % e)
    assert all(e[0] < 0.1 for e in errs), errs           # found the basin (the gate is 1 m, the grid step 0.5 m)
    db.destroy()
    gm.release()


# ---- 5. refusals that need a device ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_database_as_it_was(ctx, query_ref):
    from mimosa_amd import capi
    L, p, INV = ctx.L, capi._p, capi.MH_ERR_INVALID_ARG
    q, E = query_ref["q"], query_ref["E"]
    db = filled(ctx, E[:3], capacity=4)
    _, before = db.query(q, top_k=1, want_all=True)
    hits, desc, R = np.zeros(16, capi.PLACE_HIT_DTYPE), np.ascontiguousarray(q), np.eye(3).ravel()
    query = lambda d=desc, n_search=0, top_k=4, h=hits: L.mh_place_db_query(db.h, p(d), n_search, top_k, p(h), None)
    assert query(top_k=0) == INV and query(top_k=17) == INV and query(top_k=-1) == INV
    assert query(n_search=4) == INV and query(d=None) == INV and query(h=None) == INV
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        d = desc.copy()
        d[777] = bad
        assert query(d=d) == INV and L.mh_place_db_add(db.h, p(d), 0, None) == INV
    d = desc.copy()
    d[0] = -0.0                                          # minus zero is not negative
    assert query(d=d) == capi.MH_OK
    assert L.mh_place_db_get(db.h, 3, p(desc.copy()), None) == INV and L.mh_place_db_get(db.h, -1, None, None) == INV
    xyz = np.zeros((4, 3), np.float32)
    out = np.empty(ref.CELLS, np.float32)
    assert L.mh_place_describe(db.h, p(xyz), 4, 2, p(R), p(out)) == INV
    assert L.mh_place_describe(db.h, None, 4, 3, p(R), p(out)) == INV and L.mh_place_describe(db.h, p(xyz), 4, 3, None, p(out)) == INV
    assert L.mh_place_describe(db.h, p(xyz), 0x40000000, 3, p(R), p(out)) == capi.MH_ERR_UNSUPPORTED
    for k in range(9):
        Rb = R.copy()
        Rb[k] = np.nan
        assert L.mh_place_describe(db.h, p(xyz), 4, 3, p(Rb), p(out)) == INV
    # a scan without that stage
    sc = capi.Scan(ctx)
    idx = C.c_int32()
    from_scan = lambda which: (L.mh_place_describe_from_scan(db.h, sc.h, which, p(R), p(out)), L.mh_place_db_add_from_scan(db.h, sc.h, which, p(R), 0, C.byref(idx)),
                               L.mh_place_db_query_from_scan(db.h, sc.h, which, p(R), 0, 4, p(hits), None))
    assert from_scan(0) == (INV,) * 3 and from_scan(1) == (INV,) * 3 and from_scan(2) == (INV,) * 3 and from_scan(-1) == (INV,) * 3
    sc.prepare_input(raw_scan_of(scenes.keyframes()[0][2]), capi.make_input_config())
    assert from_scan(1) == (INV,) * 3                    # prepared, not preprocessed: no body cloud
    assert db.size() == 3
    # a full database
    assert db.add(E[3], 5) == 3 and db.size() == 4
    assert L.mh_place_db_add(db.h, p(np.ascontiguousarray(E[4])), 0, None) == INV and b"full" in L.mh_last_error(ctx.h)
    assert L.mh_place_db_add_from_scan(db.h, sc.h, 0, p(R), 0, None) == INV and b"full" in L.mh_last_error(ctx.h)
    assert db.size() == 4
    _, after = db.query(q, top_k=1, want_all=True)
    assert np.array_equal(after[:3], before)
    # a query on an empty database; zero points are no error
    empty = make_db(ctx, **scenes.DESIGNED_CFG)
    assert L.mh_place_db_query(empty.h, p(desc), 0, 4, p(hits), None) == INV and b"empty" in L.mh_last_error(ctx.h)
    assert not empty.describe(np.zeros((0, 3), np.float32)).any()
    empty.destroy()
    sc.destroy()
    db.destroy()


def test_use_after_shutdown_is_refused():
    """a database is registered on its context: after mh_shutdown every call but destroy refuses it"""
    from mimosa_amd import capi
    L, p, INV = capi.load(), capi._p, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    h, db = C.c_void_p(), C.c_void_p()
    assert L.mh_init(0, C.byref(h)) == capi.MH_OK
    cfg = capi.make_place_config(capacity=4)
    assert L.mh_place_db_create(h, C.byref(cfg), C.byref(db)) == capi.MH_OK
    desc = np.zeros(ref.CELLS, np.float32)
    desc[:60] = 1.0
    assert L.mh_place_db_add(db, p(desc), 9, None) == capi.MH_OK and L.mh_place_db_size(db) == 1
    L.mh_shutdown(h)
    hits, out, R, xyz = np.zeros(4, capi.PLACE_HIT_DTYPE), np.empty(ref.CELLS, np.float32), np.eye(3).ravel(), np.zeros((4, 3), np.float32)
    assert L.mh_place_db_size(db) == 0
    assert L.mh_place_db_add(db, p(desc), 9, None) == INV and b"shut down" in L.mh_last_error(None)
    assert L.mh_place_db_query(db, p(desc), 0, 1, p(hits), None) == INV
    assert L.mh_place_db_get(db, 0, p(out), None) == INV
    assert L.mh_place_describe(db, p(xyz), 4, 3, p(R), p(out)) == INV
    assert L.mh_place_describe_device(db, p(xyz), 4, 3, p(R), p(out)) == INV
    L.mh_place_db_destroy(db)
