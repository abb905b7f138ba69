"""-m gpu: the insert preview (mh_map_preview_insert*): what the next insert of a batch would do, computed read-only on the
device.  Counts against the stats diff of copy() + insert() on the device and against the CPU oracle's insert; per-point outcomes
against the numpy restatement of the sequential rule (tests/map_preview_ref.py) fed from the map's own get_cloud(); the points the
insert really adds against the points with outcome 1; and nothing observable moving.  Every map here is one whose next insert
triggers no LRU purge (at most two inserts at lru_clear_cycle = 10)."""
import collections

import numpy as np
import pytest

import map_preview_ref as ref

pytestmark = pytest.mark.gpu

COUNTS = ("n_points", "n_added", "n_too_close", "n_voxel_full", "n_touched_voxels", "n_new_voxels")
ORIGIN = np.array([2.05, 2.05, 2.05])            # the hand-made cases live in voxel (4, 4, 4) of the 0.5 m grid: [2.0, 2.5)^3


def lattice():
    """27 points 0.16 m apart (> min_dist 0.15 m, so each one is acceptable beside all the others), all in one voxel"""
    g = np.array([[i, j, k] for i in range(3) for j in range(3) for k in range(3)], np.float64) * 0.16
    return (ORIGIN + g).astype(np.float32)


def elsewhere():
    return np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [7.2, 0.4, 1.1]], np.float32)


def check_against_restatement(gm, batch):
    """preview(batch) on gm == the restatement on gm.get_cloud(), counts and outcomes; returns the preview"""
    pv = gm.preview_insert(batch, want_outcome=True)
    counts, outcome, _ = ref.preview(ref.cells_of(gm.get_cloud()), batch)
    assert {k: pv[k] for k in COUNTS} == counts
    assert np.array_equal(pv["outcome"], outcome), np.flatnonzero(pv["outcome"] != outcome)[:10]
    assert pv["n_added"] + pv["n_too_close"] + pv["n_voxel_full"] == pv["n_points"] == len(batch)
    no = gm.preview_insert(batch)                # without the outcome array: the same counts
    assert "outcome" not in no and no == {k: pv[k] for k in COUNTS}
    return pv


def check_against_insert(gm, batch, pv):
    """the counts are the stats diff of copy() + insert(); the rows the insert adds are the batch rows with outcome 1"""
    before, cloud0 = gm.stats(), gm.get_cloud()
    twin = gm.copy()
    twin.insert(batch)
    after, cloud1 = twin.stats(), twin.get_cloud()
    twin.release()
    assert after["n_points"] - before["n_points"] == pv["n_added"]
    assert after["n_voxels"] - before["n_voxels"] == pv["n_new_voxels"]
    rows = lambda a: collections.Counter(r.tobytes() for r in np.ascontiguousarray(a, np.float32).reshape(-1, 3))
    added = rows(cloud1)
    added.subtract(rows(cloud0))
    assert min(added.values()) >= 0
    batch = np.ascontiguousarray(batch, np.float32).reshape(-1, 3)
    assert +added == rows(batch[pv["outcome"] == ref.ADDED])


# ---- hand-made voxel cases: leaf 0.5, min_dist 0.15, cap 20 --------------------------------------------------------------
def test_long_segment_fills_its_voxel_in_the_second_trip(ctx):
    """One segment longer than a trip of 64: 12 lattice points, each followed by four copies jittered by < 0.01 m (60 entries), then
    the lattice's 15 other points — 75 candidates of one voxel the map does not hold yet.  Acceptances 1 .. 12 fall into the
    first 60 entries, the 20th is entry 68 (index 67, in the second trip), and the last 7 meet a full voxel."""
    from mimosa_amd import capi
    L = lattice()
    rng = np.random.default_rng(2)
    rows = []
    for p in L[:12]:
        rows.append(p)
        rows.extend(p + rng.uniform(-0.005, 0.005, (4, 3)).astype(np.float32))
    batch = np.concatenate([np.array(rows, np.float32), L[12:]])
    assert len(batch) == 75
    gm = capi.VoxelMap(ctx)
    gm.insert(elsewhere())
    pv = check_against_restatement(gm, batch)
    want = np.full(75, ref.TOO_CLOSE, np.uint8)
    want[np.arange(12) * 5] = ref.ADDED
    want[60:68] = ref.ADDED
    want[68:] = ref.VOXEL_FULL
    assert np.array_equal(pv["outcome"], want)
    assert (pv["n_added"], pv["n_too_close"], pv["n_voxel_full"], pv["n_touched_voxels"], pv["n_new_voxels"]) == (20, 48, 7, 1, 1)
    check_against_insert(gm, batch, pv)
    # the same segment into the voxel when the map holds it already (3 resident points that block nothing new)
    gm.insert(L[24:27])
    pv2 = check_against_restatement(gm, batch)
    assert pv2["n_new_voxels"] == 0 and pv2["n_added"] == 17 and pv2["n_voxel_full"] == 10
    check_against_insert(gm, batch, pv2)
    gm.release()


def test_full_nearly_full_and_resident_copies(ctx):
    from mimosa_amd import capi
    L = lattice()
    full = capi.VoxelMap(ctx)
    full.insert(np.concatenate([elsewhere(), L[:20]]))
    assert full.stats()["n_points"] == 23
    batch = np.concatenate([L[20:25], L[:3]])          # acceptable points and copies alike: the voxel is full for all of them
    pv = check_against_restatement(full, batch)
    assert np.array_equal(pv["outcome"], np.full(8, ref.VOXEL_FULL, np.uint8)) and pv["n_voxel_full"] == 8
    check_against_insert(full, batch, pv)
    full.release()

    nearly = capi.VoxelMap(ctx)
    nearly.insert(np.concatenate([elsewhere(), L[:19]]))
    pv = check_against_restatement(nearly, L[20:23])   # three acceptable points, one free slot
    assert pv["outcome"].tolist() == [ref.ADDED, ref.VOXEL_FULL, ref.VOXEL_FULL]
    check_against_insert(nearly, L[20:23], pv)
    nearly.release()

    some = capi.VoxelMap(ctx)
    some.insert(np.concatenate([elsewhere(), L[:10]]))
    batch = np.concatenate([L[:10], elsewhere()])      # exact copies of resident points, in two voxels... and a third
    pv = check_against_restatement(some, batch)
    assert np.array_equal(pv["outcome"], np.full(13, ref.TOO_CLOSE, np.uint8))
    assert (pv["n_touched_voxels"], pv["n_new_voxels"]) == (3, 0)
    check_against_insert(some, batch, pv)
    some.release()


def test_empty_map_and_tiny_batches(ctx, small_world):
    from mimosa_amd import capi
    gm = capi.VoxelMap(ctx)                              # never inserted into
    batch = small_world["map_xyz"][:700]
    pv = check_against_restatement(gm, batch)
    assert pv["n_new_voxels"] == pv["n_touched_voxels"] > 1 and pv["n_added"] > 0
    check_against_insert(gm, batch, pv)
    zero = gm.preview_insert(batch[:0], want_outcome=True)
    assert {k: zero[k] for k in COUNTS} == dict.fromkeys(COUNTS, 0) and len(zero["outcome"]) == 0
    assert gm.stats()["n_points"] == 0 and gm.stats()["uploads"] == 0
    gm.insert(batch)
    for one in (batch[5:6], batch[5:6] + np.float32(0.07), np.array([[40.0, 1.0, 1.0]], np.float32)):
        pv = check_against_restatement(gm, one)
        assert pv["n_points"] == 1 == pv["n_touched_voxels"]
        check_against_insert(gm, one, pv)
    zero = gm.preview_insert(batch[:0])
    assert zero == dict.fromkeys(COUNTS, 0)
    gm.release()


# ---- random cases on small_world -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded(ctx, small_world):
    """the device map and the oracle's, both holding small_world's map, and the restatement's cells of the device map"""
    from mimosa_amd import capi
    from oracle import ref_cpu
    gm, rm = capi.VoxelMap(ctx), ref_cpu.Map()
    gm.insert(small_world["map_xyz"])
    rm.insert(small_world["map_xyz"])
    yield dict(gm=gm, rm=rm, cells=ref.cells_of(gm.get_cloud()), stats=gm.stats(), cloud=gm.get_cloud())
    gm.release()


def random_batch(name, world):
    from mimosa_amd import synth
    m = world["map_xyz"]
    rng = np.random.default_rng(21)
    if name == "scan":                                   # the scan at its true pose
        R, t = world["aux"]["R_W_L"].astype(np.float32), world["aux"]["t_W_L"].astype(np.float32)
        return (synth.points_xyz(world["pts"]).astype(np.float32) @ R.T + t).astype(np.float32)
    if name == "dense":                                  # near-duplicates of resident points: min-distance rule + cap
        return m[:3000] + rng.normal(0, 0.01, (3000, 3)).astype(np.float32)
    # more than 256 touched voxels (several workgroups of four waves, one wave per voxel), some of them new, input order shuffled
    wide = np.concatenate([m[::2][:2500] + np.float32(0.04), m[:1200] + np.array([20.0, 0.0, 0.0], np.float32)])
    return wide[rng.permutation(len(wide))]


@pytest.mark.parametrize("name", ["scan", "dense", "wide"])
def test_random_batches(ctx, small_world, seeded, name):
    gm, rm = seeded["gm"], seeded["rm"]
    batch = random_batch(name, small_world)
    pv = gm.preview_insert(batch, want_outcome=True)
    print(name, {k: pv[k] for k in COUNTS})
    counts, outcome, _ = ref.preview(seeded["cells"], batch)
    assert {k: pv[k] for k in COUNTS} == counts
    assert np.array_equal(pv["outcome"], outcome), np.flatnonzero(pv["outcome"] != outcome)[:10]
    r2 = rm.copy()
    np0, nv0 = r2.num_points, r2.num_voxels
    r2.insert(batch)
    assert (r2.num_points - np0, r2.num_voxels - nv0) == (pv["n_added"], pv["n_new_voxels"])
    check_against_insert(gm, batch, pv)
    assert pv["n_added"] > 0 and pv["n_too_close"] > 0
    if name == "wide":
        assert pv["n_touched_voxels"] > 256 and 0 < pv["n_new_voxels"] < pv["n_touched_voxels"]
    assert gm.stats() == seeded["stats"] and np.array_equal(gm.get_cloud(), seeded["cloud"])


def test_nothing_observable_moves(ctx, small_world):
    """all eight stats, the cloud, k-NN answers and a factor's linearize result are bit-identical before and after previews; a real
    insert afterwards gives the map a never-previewed twin gets"""
    from mimosa_amd import capi
    m = small_world["map_xyz"]
    gm, twin = capi.VoxelMap(ctx), capi.VoxelMap(ctx)
    for g in (gm, twin):
        g.insert(m)
    gf = capi.ICPFactor(ctx, gm, small_world["pts"], capi.make_reg_config(**small_world["cfg"]))
    R, t = small_world["R"], small_world["t"]
    rng = np.random.default_rng(4)
    q = m[rng.integers(0, len(m), 60)].astype(np.float64) + rng.normal(0, 0.15, (60, 3))
    keys = ("H_ss", "b_s", "f", "status_hist", "loc_trans_comp", "loc_rot_comp")
    stats0, cloud0, knn0 = gm.stats(), gm.get_cloud(), gm.knn(q, 5)
    lin0 = gf.linearize(R, t)
    assert len(stats0) == 8
    for name in ("scan", "dense", "wide"):
        gm.preview_insert(random_batch(name, small_world), want_outcome=(name != "dense"))
    assert gm.stats() == stats0
    assert np.array_equal(gm.get_cloud(), cloud0)
    for a, b in zip(gm.knn(q, 5), knn0):
        assert np.array_equal(a, b)
    gf.reset()
    lin1 = gf.linearize(R, t)
    for k in keys:
        assert np.array_equal(lin0[k], lin1[k]), k
    gf.destroy()
    batch = random_batch("wide", small_world)
    gm.insert(batch)
    twin.insert(batch)
    assert gm.stats() == twin.stats() and np.array_equal(gm.get_cloud(), twin.get_cloud())
    for a, b in zip(gm.knn(q, 5), twin.knn(q, 5)):
        assert np.array_equal(a, b)
    gm.release()
    twin.release()


def test_transform_variants_agree(ctx, small_world):
    """the device variant with (R, t) == the host variant on ctx.transform_f32 of the same points; preview_insert_from_scan == the
    device variant on the scan's body cloud"""
    import ctypes as C
    from mimosa_amd import capi, synth
    raw, aux = synth.make_raw_scan(16, n_cols=64, room=(6.0, 5.0, 3.0), sensor_local=np.array([2.3, 2.6, 1.2]))
    sc = capi.Scan(ctx)
    sc.prepare_input(raw, capi.make_input_config())
    sc.deskew(aux["Rt12"][np.searchsorted(aux["unique_ns"], sc.unique_ns())])
    sc.preprocess_geometric(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    body = sc.points(capi.Scan.BODY)
    R, t = aux["R_W_L"].astype(np.float32), aux["t_W_L"].astype(np.float32)
    gm = capi.VoxelMap(ctx)
    gm.insert(small_world["map_xyz"])
    stats0 = gm.stats()
    W = ctx.transform_f32(body, R, t)
    host = gm.preview_insert(np.stack([W["x"], W["y"], W["z"]], 1), want_outcome=True)
    d, n = C.c_void_p(), C.c_size_t()
    ctx.check(ctx.L.mh_scan_device_points(sc.h, capi.Scan.BODY, C.byref(d), C.byref(n)))
    assert n.value == len(body)
    dev = gm.preview_insert_device(d, n.value, body.dtype.itemsize // 4, R, t, want_outcome=True)
    scan = gm.preview_insert_from_scan(sc, R, t, want_outcome=True)
    for other in (dev, scan):
        assert {k: other[k] for k in COUNTS} == {k: host[k] for k in COUNTS}
        assert np.array_equal(other["outcome"], host["outcome"])
    assert host["n_points"] == len(body) and 0 < host["n_added"] < len(body)
    assert gm.preview_insert_from_scan(sc, R, t) == {k: host[k] for k in COUNTS}
    # R without t is refused
    out = capi.MapInsertPreview()
    rc = ctx.L.mh_map_preview_insert_device(gm.h, d, n.value, body.dtype.itemsize // 4, capi._p(R), None, C.byref(out), None)
    assert rc == capi.MH_ERR_INVALID_ARG
    assert gm.stats() == stats0
    twin = gm.copy()
    twin.insert_from_scan(sc, R, t)
    assert twin.stats()["n_points"] - stats0["n_points"] == host["n_added"]
    twin.release()
    gm.release()
    sc.destroy()


def test_refusals_leave_the_map_usable(ctx, small_world):
    import ctypes as C
    from mimosa_amd import capi
    m = small_world["map_xyz"]
    gm, twin = capi.VoxelMap(ctx), capi.VoxelMap(ctx)
    for g in (gm, twin):
        g.insert(m)
    bad = m[:100].copy()
    bad[37, 1] = np.nan
    far = m[:100].copy()
    far[5, 0] = 1.0e7                                    # 2e7 voxels from the origin: outside the 21-bit key
    out = capi.MapInsertPreview()
    oc = np.zeros(100, np.uint8)
    for batch in (bad, far):
        rc = ctx.L.mh_map_preview_insert(gm.h, capi._p(batch), 100, 3, C.byref(out), capi._p(oc))
        assert rc == capi.MH_ERR_UNSUPPORTED
        with pytest.raises(capi.MhError):
            gm.preview_insert(batch)
    assert ctx.L.mh_map_preview_insert(gm.h, capi._p(bad), 100, 3, None, None) == capi.MH_ERR_INVALID_ARG   # no `out`
    assert gm.stats() == twin.stats() and np.array_equal(gm.get_cloud(), twin.get_cloud())
    good = m[:500] + np.float32(0.05)
    pv = check_against_restatement(gm, good)             # the next preview works
    gm.insert(good)
    twin.insert(good)
    assert gm.stats() == twin.stats() and np.array_equal(gm.get_cloud(), twin.get_cloud())
    assert pv["n_added"] > 0
    gm.release()
    twin.release()
