"""-m gpu: the entry points that take a point cloud — as host xyz with a stride, as a device pointer with a stride, or as a stage of
a device-resident mh_scan: mh_map_insert*, mh_map_preview_insert*, mh_map_carve*, mh_place_describe* / mh_place_db_{add,query}_from_scan,
mh_keyframes_add*, with mh_map_insert_shard*, mh_scan_get_points, mh_scan_device_points and mh_icp_create_from_scan.

1. The refusal table: one row per single fault of an argument that describes the cloud, with the return code and the COMPLETE
   text of mh_last_error; a few rows with two faults at once, which pin the code alone (the header promises no order of checks).
2. Three forms, one answer: for n in {0, 1, 257} (257: one full workgroup of 256 and a tail of one) the host form at strides 3, 4
   and 8, the device form at the same strides and the from-scan form on the stage that holds the cloud give the same bits.

Nothing here launches more than a few hundred points."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 0x40000000   # the first batch size every form refuses
STRIDES = (3, 4, 8)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def f64(a):
    return np.ascontiguousarray(a, np.float64)


def cloud_of(n, seed=11):
    """n points 1.5 to 6 m from the sensor, none on a coordinate plane"""
    rng = np.random.default_rng(seed)
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True) if n else 1.0
    return f32(d * rng.uniform(1.5, 6.0, (n, 1)))


def raw_of(cloud):
    from mimosa_amd import synth
    raw = np.zeros(len(cloud), synth.OUSTER_DTYPE)
    raw["x"], raw["y"], raw["z"] = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    raw["pad"], raw["intensity"] = 1.0, 100.0
    raw["ring"] = (np.arange(len(cloud)) % 32).astype(np.uint16)
    return raw


def scan_of(ctx, cloud, preprocess=True):
    """a scan whose stages both hold every point of the cloud (no skip divisors)"""
    from mimosa_amd import capi
    sc = capi.Scan(ctx)
    sc.prepare_input(raw_of(cloud), capi.make_input_config(point_skip_divisor=1, ring_skip_divisor=1))
    if preprocess:
        sc.preprocess_geometric(np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    return sc


def scan_xyz(sc, which):
    rec = sc.points(which)
    return np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32).reshape(-1, 3)


def strided(xyz, stride):
    wide = np.full((len(xyz), stride), 7.0, np.float32)
    wide[:, :3] = xyz
    return wide


class DeviceCopies:
    """the cloud in device memory at each stride (freed by close)"""

    def __init__(self, ctx, xyz):
        self.L, self.ctx, self.ptr = ctx.L, ctx, {}
        for s in STRIDES:
            a = strided(xyz, s)
            d = C.c_void_p()
            assert self.L.hipMalloc(C.byref(d), C.c_size_t(max(a.nbytes, 64))) == 0
            if a.nbytes:
                assert self.L.hipMemcpy(d, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
            self.ptr[s] = d

    def close(self):
        self.ctx.synchronize()
        for d in self.ptr.values():
            assert self.L.hipFree(d) == 0


@pytest.fixture(scope="module")
def base_xyz():
    """what the maps of this module hold before the batch arrives: 300 points, half of them half way along the rays of the 257-point
    cloud (a carve sees through those), half beside its points (an insert meets occupied voxels)"""
    c = cloud_of(257)
    rng = np.random.default_rng(5)
    return f32(np.concatenate([0.5 * c[:150], c[100:250] + rng.normal(0, 0.1, (150, 3))]))


def map_of(ctx, base_xyz):
    from mimosa_amd import capi
    m = capi.VoxelMap(ctx)
    m.insert(base_xyz)
    return m


# ---- 1. the refusal table -----------------------------------------------------------------------------------------------------
WHICH_TEXT = ": which must be 0 (points_full_) or 1 (Be_cloud_)"
STAGE_TEXT = ": that stage has not run"
NO_PRE_TEXT = ": no mh_scan_preprocess_geometric before"


@pytest.fixture(scope="module")
def world(ctx, base_xyz):
    """the handles every row of the table is tried on, the scans in their states, and arguments that are in order"""
    from mimosa_amd import capi, synth
    L = ctx.L
    L.mh_last_error.restype = C.c_char_p
    xyz = cloud_of(257)
    w = dict(ctx=ctx, L=L, capi=capi, xyz=xyz)
    w["map"] = map_of(ctx, base_xyz)
    w["db"] = capi.PlaceDatabase(ctx, capacity=4)
    w["db"].add(np.zeros(capi.PLACE_CELLS, np.float32), tag=1)      # (a query of an empty database is refused before its cloud)
    w["kf"] = capi.KeyframeStore(ctx, capacity_keyframes=4, capacity_points=4096)
    w["fresh"] = capi.Scan(ctx)                                     # no stage has run
    w["prepared"] = scan_of(ctx, xyz, preprocess=False)             # prepared, not preprocessed
    w["ready"] = scan_of(ctx, xyz)
    w["other_ctx"] = capi.Context(0)
    w["foreign"] = scan_of(w["other_ctx"], xyz)                     # a scan of a second context on the same device
    w["foreign_fresh"] = capi.Scan(w["other_ctx"])
    w["dev"] = DeviceCopies(ctx, xyz)
    w["reg"] = capi.make_reg_config(**synth.enwide_config())
    yield w
    w["dev"].close()
    for k in ("fresh", "prepared", "ready", "foreign", "foreign_fresh"):
        w[k].destroy()
    w["other_ctx"].close()
    w["kf"].destroy()
    w["db"].destroy()
    w["map"].release()


class Call:
    """One entry point with arguments that are in order; row(name=value) is the call with one of them replaced."""

    def __init__(self, w, fn, **args):
        self.w, self.fn, self.args = w, fn, args

    def __call__(self, **change):
        a = dict(self.args, **change)
        p = self.w["capi"]._p
        vals = [p(v) if isinstance(v, np.ndarray) else (v.h if hasattr(v, "h") else v) for v in a.values()]
        rc = getattr(self.w["L"], self.fn)(*vals)
        return rc, (self.w["L"].mh_last_error(None) or b"").decode()


def calls_of(w):
    """every entry point of the table, by name, with arguments that pass"""
    capi = w["capi"]
    xyz, d3 = w["xyz"], w["dev"].ptr[3]
    R32, t32 = f32(np.eye(3)), f32(np.zeros(3))
    o, R64, t64, carve = f64(np.zeros(3)), f64(np.eye(3)), f64(np.zeros(3)), capi.make_carve_config(apply=False)
    pv, cr = capi.MapInsertPreview(), capi.MapCarveResult()
    desc, hits = np.zeros(capi.PLACE_CELLS, np.float32), np.zeros(4, capi.PLACE_HIT_DTYPE)
    idx, n_out, dptr, icp = C.c_int32(-7), C.c_size_t(), C.c_void_p(), C.c_void_p()
    out_pts = np.zeros(257 * 8, np.float32)
    m, db, kf, sc = w["map"], w["db"], w["kf"], w["ready"]
    w["keep"] = (pv, cr, idx, n_out, dptr, icp, carve)
    c = {}
    c["mh_map_insert"] = Call(w, "mh_map_insert", map=m, xyz=xyz, n=257, stride=3)
    c["mh_map_insert_device"] = Call(w, "mh_map_insert_device", map=m, d=d3, n=257, stride=3, R=None, t=None)
    c["mh_map_insert_from_scan"] = Call(w, "mh_map_insert_from_scan", map=m, scan=sc, R=R32, t=t32)
    c["mh_map_insert_shard"] = Call(w, "mh_map_insert_shard", map=m, xyz=xyz, n=257, stride=3, world=2, rank=0, block_log2=3)
    c["mh_map_insert_shard_from_scan"] = Call(w, "mh_map_insert_shard_from_scan", map=m, scan=sc, R=R32, t=t32, world=2, rank=0, block_log2=3)
    c["mh_map_preview_insert"] = Call(w, "mh_map_preview_insert", map=m, xyz=xyz, n=257, stride=3, out=C.byref(pv), outcome=None)
    c["mh_map_preview_insert_device"] = Call(w, "mh_map_preview_insert_device", map=m, d=d3, n=257, stride=3, R=None, t=None, out=C.byref(pv), outcome=None)
    c["mh_map_preview_insert_from_scan"] = Call(w, "mh_map_preview_insert_from_scan", map=m, scan=sc, R=R32, t=t32, out=C.byref(pv), outcome=None)
    c["mh_map_carve"] = Call(w, "mh_map_carve", map=m, xyz=xyz, n=257, stride=3, origin=o, R=R64, t=t64, cfg=C.byref(carve), out=C.byref(cr))
    c["mh_map_carve_device"] = Call(w, "mh_map_carve_device", map=m, d=d3, n=257, stride=3, origin=o, R=R64, t=t64, cfg=C.byref(carve), out=C.byref(cr))
    c["mh_map_carve_from_scan"] = Call(w, "mh_map_carve_from_scan", map=m, scan=sc, which=1, origin=o, R=R64, t=t64, cfg=C.byref(carve), out=C.byref(cr))
    c["mh_place_describe"] = Call(w, "mh_place_describe", db=db, xyz=xyz, n=257, stride=3, R=R64, desc=desc)
    c["mh_place_describe_device"] = Call(w, "mh_place_describe_device", db=db, d=d3, n=257, stride=3, R=R64, desc=desc)
    c["mh_place_describe_from_scan"] = Call(w, "mh_place_describe_from_scan", db=db, scan=sc, which=1, R=R64, desc=desc)
    c["mh_place_db_add_from_scan"] = Call(w, "mh_place_db_add_from_scan", db=db, scan=sc, which=1, R=R64, tag=5, index=C.byref(idx))
    c["mh_place_db_query_from_scan"] = Call(w, "mh_place_db_query_from_scan", db=db, scan=sc, which=1, R=R64, n_search=0, top_k=1, hits=hits, all=None)
    c["mh_keyframes_add"] = Call(w, "mh_keyframes_add", kf=kf, xyz=xyz, n=257, stride=3, tag=5, index=C.byref(idx))
    c["mh_keyframes_add_device"] = Call(w, "mh_keyframes_add_device", kf=kf, d=d3, n=257, stride=3, tag=5, index=C.byref(idx))
    c["mh_keyframes_add_from_scan"] = Call(w, "mh_keyframes_add_from_scan", kf=kf, scan=sc, which=1, tag=5, index=C.byref(idx))
    c["mh_scan_get_points"] = Call(w, "mh_scan_get_points", scan=sc, which=1, out=out_pts, capacity=257, n_out=C.byref(n_out))
    c["mh_scan_device_points"] = Call(w, "mh_scan_device_points", scan=sc, which=1, d=C.byref(dptr), n_out=C.byref(n_out))
    c["mh_icp_create_from_scan"] = Call(w, "mh_icp_create_from_scan", ctx=w["ctx"].h, map=m, scan=sc, cfg=C.byref(w["reg"]), is_binary=0, out=C.byref(icp))
    return c


def single_faults(w):
    """(entry point, the argument replaced, its value, code, complete text)"""
    capi = w["capi"]
    INV, UNS = capi.MH_ERR_INVALID_ARG, capi.MH_ERR_UNSUPPORTED
    R32, t32 = f32(np.eye(3)), f32(np.zeros(3))
    rows = []

    def nulls(fn, *names):
        rows.extend((fn, {k: None}, INV, fn + ": NULL argument") for k in names)

    # host forms: each NULL argument, a stride of 2
    nulls("mh_map_insert", "map", "xyz")
    nulls("mh_map_insert_shard", "map", "xyz")
    nulls("mh_map_preview_insert", "map", "xyz", "out")
    nulls("mh_map_carve", "map", "xyz", "origin", "R", "t", "cfg", "out")
    nulls("mh_place_describe", "db", "xyz", "R", "desc")
    nulls("mh_keyframes_add", "kf", "xyz")
    nulls("mh_map_insert_device", "map", "d")
    nulls("mh_map_preview_insert_device", "map", "d", "out")
    nulls("mh_map_carve_device", "map", "d", "origin", "R", "t", "cfg", "out")
    nulls("mh_place_describe_device", "db", "d", "R", "desc")
    nulls("mh_keyframes_add_device", "kf", "d")
    nulls("mh_map_insert_from_scan", "map", "scan")
    nulls("mh_map_insert_shard_from_scan", "map", "scan", "R", "t")
    nulls("mh_map_preview_insert_from_scan", "map", "scan", "out")
    nulls("mh_map_carve_from_scan", "map", "scan", "origin", "R", "t", "cfg", "out")
    nulls("mh_place_describe_from_scan", "db", "scan", "R", "desc")
    nulls("mh_place_db_add_from_scan", "db", "scan", "R")
    nulls("mh_place_db_query_from_scan", "db", "scan", "R", "hits")
    nulls("mh_keyframes_add_from_scan", "kf", "scan")
    nulls("mh_scan_get_points", "scan", "n_out")
    nulls("mh_scan_device_points", "scan", "d", "n_out")
    nulls("mh_icp_create_from_scan", "ctx", "map", "scan", "cfg", "out")
    for fn in ("mh_map_insert", "mh_map_insert_shard", "mh_map_preview_insert", "mh_map_carve", "mh_place_describe", "mh_keyframes_add",
               "mh_map_insert_device", "mh_map_preview_insert_device", "mh_map_carve_device", "mh_place_describe_device", "mh_keyframes_add_device"):
        rows.append((fn, dict(stride=2), INV, fn + ": stride_floats must be >= 3"))
    # R and t go together: the device forms, and the from-scan forms that go through them
    for fn, said_by in (("mh_map_insert_device", "mh_map_insert_device"), ("mh_map_insert_from_scan", "mh_map_insert_device"),
                        ("mh_map_preview_insert_device", "mh_map_preview_insert_device"), ("mh_map_preview_insert_from_scan", "mh_map_preview_insert_device")):
        rows.append((fn, dict(R=R32, t=None), INV, said_by + ": R and t go together"))
        rows.append((fn, dict(R=None, t=t32), INV, said_by + ": R and t go together"))
    # n = 2^30, in the forms that refuse before they touch the batch (the host forms of mh_map_insert and mh_map_insert_shard stage first)
    rows.append(("mh_map_insert_device", dict(n=BIG), UNS, "mh_map_insert: batch too large"))   # insert_device speaks as mh_map_insert
    for fn in ("mh_map_preview_insert", "mh_map_preview_insert_device", "mh_map_carve", "mh_map_carve_device", "mh_place_describe", "mh_place_describe_device"):
        rows.append((fn, dict(n=BIG), UNS, fn + ": batch too large"))
    # (a store asks first whether the entry fits, and an arena for 2^30 points is 16 GiB: this store answers that it is full)
    for fn in ("mh_keyframes_add", "mh_keyframes_add_device"):
        rows.append((fn, dict(n=BIG), INV, fn + ": the store is full (points)"))
    rows.append(("mh_keyframes_add_device", dict(n=1, stride=1 << 32), UNS, "mh_keyframes_add_device: batch too large"))
    # which
    with_which = ("mh_map_carve_from_scan", "mh_place_describe_from_scan", "mh_place_db_add_from_scan", "mh_place_db_query_from_scan", "mh_keyframes_add_from_scan")
    for fn in with_which:
        for which in (-1, 2):
            rows.append((fn, dict(which=which), INV, fn + WHICH_TEXT))
    for fn in ("mh_scan_get_points", "mh_scan_device_points"):
        for which in (-1, 3):
            rows.append((fn, dict(which=which), INV, fn + STAGE_TEXT))
    # a scan no stage of which has run; one that is prepared and not preprocessed, asked for its body cloud
    for fn in with_which + ("mh_scan_get_points", "mh_scan_device_points"):
        rows.append((fn, dict(scan=w["fresh"], which=0), INV, fn + STAGE_TEXT))
        rows.append((fn, dict(scan=w["fresh"], which=1), INV, fn + STAGE_TEXT))
        rows.append((fn, dict(scan=w["prepared"], which=1), INV, fn + STAGE_TEXT))
    for fn in ("mh_scan_get_points", "mh_scan_device_points"):
        rows.append((fn, dict(scan=w["prepared"], which=2), INV, fn + STAGE_TEXT))
    for fn in ("mh_map_insert_from_scan", "mh_map_insert_shard_from_scan", "mh_map_preview_insert_from_scan", "mh_icp_create_from_scan"):
        rows.append((fn, dict(scan=w["fresh"]), INV, fn + NO_PRE_TEXT))
        rows.append((fn, dict(scan=w["prepared"]), INV, fn + NO_PRE_TEXT))
    # residence: a store takes the scans of its own context only (every other consumer asks for the same device)
    rows.append(("mh_keyframes_add_from_scan", dict(scan=w["foreign"]), INV, "mh_keyframes_add_from_scan: scan belongs to another context"))
    return rows


def double_faults(w):
    """(entry point, the arguments replaced, code): two faults at once, the code alone"""
    INV = w["capi"].MH_ERR_INVALID_ARG
    rows = [("mh_keyframes_add_from_scan", dict(scan=w["foreign_fresh"], which=0), INV),      # wrong residence and wrong stage
            ("mh_keyframes_add_from_scan", dict(scan=w["foreign_fresh"], which=1), INV)]
    for fn in ("mh_map_carve_from_scan", "mh_place_describe_from_scan", "mh_place_db_add_from_scan", "mh_place_db_query_from_scan", "mh_keyframes_add_from_scan",
               "mh_scan_get_points", "mh_scan_device_points"):
        for which in (-1, 3):
            rows.append((fn, dict(scan=w["fresh"], which=which), INV))                          # wrong which and an unprepared scan
    return rows


def test_refusal_table(world):
    w = world
    calls = calls_of(w)
    state = lambda: (w["map"].stats(), bits(w["map"].get_cloud()).tobytes(), w["db"].size(), w["kf"].info())   # noqa: E731
    before = state()
    singles, doubles = single_faults(w), double_faults(w)
    assert {r[0] for r in singles} == set(calls)                    # every entry point has rows
    wrong = []
    for fn, change, code, text in singles:
        rc, said = calls[fn](**change)
        if (rc, said) != (code, text):
            wrong.append((fn, {k: (v if isinstance(v, (int, type(None))) else type(v).__name__) for k, v in change.items()}, rc, said, code, text))
    for fn, change, code in doubles:
        rc, _ = calls[fn](**change)
        if rc != code:
            wrong.append((fn, sorted(change), rc, code))
    assert not wrong, wrong
    assert w["keep"][2].value == -7 and state() == before           # no refusal wrote an index or moved a handle
    # ... and the calls of the table pass as they stand (the ones that only read)
    for fn in ("mh_map_preview_insert", "mh_map_preview_insert_device", "mh_map_preview_insert_from_scan", "mh_map_carve", "mh_map_carve_device",
               "mh_map_carve_from_scan", "mh_place_describe", "mh_place_describe_device", "mh_place_describe_from_scan", "mh_place_db_query_from_scan",
               "mh_scan_get_points", "mh_scan_device_points"):
        assert calls[fn]()[0] == w["capi"].MH_OK, fn


# ---- 2. three forms, one answer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1, 257])
def source(request, ctx):
    """a cloud of n points: in a scan (both stages hold all of it), on the host, and on the device at every stride"""
    n = request.param
    sc = scan_of(ctx, cloud_of(n))
    xyz = scan_xyz(sc, 1)
    assert len(xyz) == n and np.array_equal(bits(scan_xyz(sc, 0)), bits(xyz))     # the identity extrinsic: one cloud in both stages
    s = dict(n=n, scan=sc, xyz=xyz, dev=DeviceCopies(ctx, xyz))
    yield s
    s["dev"].close()
    sc.destroy()


def host_forms(s):
    """(label, pointer argument, stride) of the host forms"""
    from mimosa_amd import capi
    s["_host"] = [strided(s["xyz"], st) for st in STRIDES]
    return [("host/%d" % st, capi._p(a) if s["n"] else None, st) for st, a in zip(STRIDES, s["_host"])]


def device_forms(s):
    return [("device/%d" % st, s["dev"].ptr[st] if s["n"] else None, st) for st in STRIDES]


def all_same(results):
    """results: (label, value) pairs; every value equals the first"""
    first = results[0]
    for label, value in results[1:]:
        assert value == first[1], (first[0], label)


def map_state(m):
    st = m.stats()
    return ({k: v for k, v in st.items() if k not in ("device_bytes", "upload_bytes")}, bits(m.get_cloud()).tobytes())


def test_map_insert_forms(ctx, source, base_xyz):
    from mimosa_amd import capi, synth
    L, n, p = ctx.L, source["n"], capi._p
    R, t = f32(synth.so3_exp(np.array([0.1, -0.2, 0.3]))), f32([0.4, -0.3, 0.2])
    results, moved = [], []
    base_bytes = None

    def run(label, fn, *args):
        nonlocal base_bytes
        m = map_of(ctx, base_xyz)
        base_bytes = m.stats()["upload_bytes"]
        ctx.check(getattr(L, fn)(m.h, *args))
        assert m.stats()["uploads"] == 2
        out = (label, map_state(m), m.stats()["upload_bytes"])
        m.release()
        return out

    for label, ptr, st in host_forms(source):
        label, state, up = run(label, "mh_map_insert", ptr, n, st)
        assert up == base_bytes + 12 * n, label                    # a host batch counts as packed xyz, whatever its stride
        results.append((label, state))
    for label, ptr, st in device_forms(source):
        label, state, up = run(label, "mh_map_insert_device", ptr, n, st, None, None)
        assert up == base_bytes, label
        results.append((label, state))
        moved.append(run(label + "/Rt", "mh_map_insert_device", ptr, n, st, p(R), p(t))[:2])
    label, state, up = run("scan", "mh_map_insert_from_scan", source["scan"].h, None, None)
    assert up == base_bytes
    results.append((label, state))
    moved.append(run("scan/Rt", "mh_map_insert_from_scan", source["scan"].h, p(R), p(t))[:2])
    all_same(results)
    all_same(moved)
    if n == 257:
        assert results[0][1][0]["n_points"] > len(base_xyz) and moved[0][1] != results[0][1]


@pytest.mark.parametrize("rank", [0, 1])
def test_map_insert_shard_forms(ctx, source, base_xyz, rank):
    """this rank's share of the batch: the host form at each stride, and the from-scan form at the identity pose"""
    from mimosa_amd import capi
    L, n, p = ctx.L, source["n"], capi._p
    results = []
    for label, ptr, st in host_forms(source):
        m = map_of(ctx, base_xyz)
        ctx.check(L.mh_map_insert_shard(m.h, ptr, n, st, 2, rank, 3))
        results.append((label, map_state(m)))
        m.release()
    m = map_of(ctx, base_xyz)
    ctx.check(L.mh_map_insert_shard_from_scan(m.h, source["scan"].h, p(f32(np.eye(3))), p(f32(np.zeros(3))), 2, rank, 3))
    results.append(("scan", map_state(m)))
    m.release()
    all_same(results)


def test_map_preview_forms(ctx, source, base_xyz):
    from mimosa_amd import capi, synth
    L, n, p = ctx.L, source["n"], capi._p
    R, t = f32(synth.so3_exp(np.array([0.1, -0.2, 0.3]))), f32([0.4, -0.3, 0.2])
    m = map_of(ctx, base_xyz)
    before = map_state(m)

    def run(fn, *args):
        pv, oc = capi.MapInsertPreview(), np.full(max(n, 1), 9, np.uint8)
        ctx.check(getattr(L, fn)(m.h, *args, C.byref(pv), p(oc)))
        return bytes(pv), oc[:n].tobytes()

    results = [(label, run("mh_map_preview_insert", ptr, n, st)) for label, ptr, st in host_forms(source)]
    results += [(label, run("mh_map_preview_insert_device", ptr, n, st, None, None)) for label, ptr, st in device_forms(source)]
    results.append(("scan", run("mh_map_preview_insert_from_scan", source["scan"].h, None, None)))
    moved = [(label, run("mh_map_preview_insert_device", ptr, n, st, p(R), p(t))) for label, ptr, st in device_forms(source)]
    moved.append(("scan/Rt", run("mh_map_preview_insert_from_scan", source["scan"].h, p(R), p(t))))
    all_same(results)
    all_same(moved)
    pv = capi.MapInsertPreview.from_buffer_copy(results[0][1][0])
    assert pv.n_points == n and pv.n_added + pv.n_too_close + pv.n_voxel_full == n
    if n == 257:
        assert 0 < pv.n_added < n and set(results[0][1][1]) >= {1, 2}
    assert map_state(m) == before
    m.release()


@pytest.mark.parametrize("which", [0, 1])
def test_map_carve_forms(ctx, source, base_xyz, which):
    from mimosa_amd import capi
    L, n, p = ctx.L, source["n"], capi._p
    o, R, t = f64(np.zeros(3)), f64(np.eye(3)), f64(np.zeros(3))
    for apply in (False, True):
        # ring 0: the cloud is sparse, and a map point half way along the ray of an observation shares its cell
        cfg = capi.make_carve_config(grid=64, ring=0, range_min=0.5, range_max=30.0, margin_abs=0.3, margin_rel=0.0, apply=apply)

        def run(fn, *args):
            m, out = map_of(ctx, base_xyz), capi.MapCarveResult()
            ctx.check(getattr(L, fn)(m.h, *args, p(o), p(R), p(t), C.byref(cfg), C.byref(out)))
            got = (bytes(out), map_state(m))
            m.release()
            return got, out.n_removed

        results = [(label, run("mh_map_carve", ptr, n, st)) for label, ptr, st in host_forms(source)]
        results += [(label, run("mh_map_carve_device", ptr, n, st)) for label, ptr, st in device_forms(source)]
        results.append(("scan", run("mh_map_carve_from_scan", source["scan"].h, which)))
        all_same(results)
        removed = results[0][1][1]
        assert removed > 0 if n == 257 else (removed == 0 or n == 1)   # the points half way along the rays are seen through
        if not apply or removed == 0:
            m = map_of(ctx, base_xyz)
            assert results[0][1][0][1] == map_state(m)             # a preview, and a carve that removes nothing, leave the map as it was
            m.release()


@pytest.mark.parametrize("which", [0, 1])
def test_place_forms(ctx, source, which):
    from mimosa_amd import capi, synth
    L, n, p = ctx.L, source["n"], capi._p
    R = f64(synth.so3_exp(np.array([0.05, -0.04, 0.6])))
    db = capi.PlaceDatabase(ctx, r_min=0.5, r_max=10.0, z_min=-8.0, z_max=8.0, min_overlap=1, capacity=4)

    def run(fn, *args):
        desc = np.full(capi.PLACE_CELLS, -1.0, np.float32)
        ctx.check(getattr(L, fn)(db.h, *args, p(R), p(desc)))
        return bits(desc).tobytes()

    results = [(label, run("mh_place_describe", ptr, n, st)) for label, ptr, st in host_forms(source)]
    results += [(label, run("mh_place_describe_device", ptr, n, st)) for label, ptr, st in device_forms(source)]
    results.append(("scan", run("mh_place_describe_from_scan", source["scan"].h, which)))
    assert db.add_from_scan(source["scan"], which, R, tag=3) == 0                      # ... the entry that never leaves the device
    results.append(("add_from_scan", bits(db.get(0)[0]).tobytes()))
    all_same(results)
    desc = np.frombuffer(results[0][1], np.float32)
    assert (desc > 0).sum() > 50 if n == 257 else (desc > 0).sum() <= n
    # the query described from the scan is the query with that descriptor
    a, a_all = db.query(desc, top_k=2, want_all=True)
    b, b_all = db.query_from_scan(source["scan"], which, R, top_k=2, want_all=True)
    assert a.tobytes() == b.tobytes() and a_all.tobytes() == b_all.tobytes()
    db.destroy()


@pytest.mark.parametrize("which", [0, 1])
def test_keyframes_forms(ctx, source, which):
    from mimosa_amd import capi
    L, n = ctx.L, source["n"]
    st_ = capi.KeyframeStore(ctx, capacity_keyframes=8, capacity_points=7 * max(n, 1))
    idx = C.c_int32(-1)
    labels = []
    for label, ptr, st in host_forms(source):
        ctx.check(L.mh_keyframes_add(st_.h, ptr, n, st, 10 + len(labels), C.byref(idx)))
        assert idx.value == len(labels)
        labels.append(label)
    for label, ptr, st in device_forms(source):
        ctx.check(L.mh_keyframes_add_device(st_.h, ptr, n, st, 10 + len(labels), C.byref(idx)))
        assert idx.value == len(labels)
        labels.append(label)
    assert st_.add_from_scan(source["scan"], which, tag=10 + len(labels)) == len(labels)
    labels.append("scan")
    assert st_.size() == 7 and st_.info()["points"] == 7 * n
    for i, label in enumerate(labels):
        got, tag = st_.get(i)
        assert tag == 10 + i and got.shape == (n, 3) and np.array_equal(bits(got), bits(source["xyz"])), label
    st_.destroy()
