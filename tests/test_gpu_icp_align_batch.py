"""-m gpu: mh_icp_align_batch — B independent alignments in one chain of launches — against mh_icp_align on a clone of each
member from the same start pose, and mh_icp_relocalise_batch against mh_icp_relocalise.

Scene: the room of test_gpu_icp_align.py (mimosa_amd/synth.py) as the map, scans cast from the ground-truth pose and thinned to
1 .. 24 576 points, started from the truth perturbed by 0.05-0.5 m and 1-5 degrees.

Bars per member: iters, converged and every trace row's degenerate / n_knn equal; trace poses, f, step norms, first, last, the
final status / mean / normal arrays and the final pose bit for bit (same_bits below).  That holds wherever the batch gives a
member the launch class a call of its own gets — every case here but test_launch_classes, where the batch's total point count
moves the members from the two-lanes-per-point class to the 256- and the 512-thread class.  There K3 adds its rows in another
order: mh_icp_linearize_batch on that exact window differs from separate mh_icp_linearize calls in the last bits (the test measures
and prints it first), and the members are held to the project's chain bar instead: 1e-9 m / 1e-9 rad per trace pose, equal iters /
converged, equal status arrays (same_chain below)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = np.array([0.0, 0.0, -1.0])


def expmap(w):
    w = np.asarray(w, float)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    return np.eye(3) + A * K + B * (K @ K)


def rot_angle(Ra, Rb):
    M = Ra.T @ Rb
    return float(np.arctan2(np.linalg.norm(M - M.T) / (2.0 * np.sqrt(2.0)), (np.trace(M) - 1.0) / 2.0))


def perturbed(truth, seed, dist=None, deg=None):
    rng = np.random.default_rng(seed)
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    w = ax / np.linalg.norm(ax) * np.deg2rad(rng.uniform(1.0, 5.0) if deg is None else deg)
    dt = d / np.linalg.norm(d) * (rng.uniform(0.05, 0.5) if dist is None else dist)
    R, t = truth
    return R @ expmap(w), t + dt


def align_cfg(**kw):
    from mimosa_amd import capi
    base = dict(max_iters=30, eps_rot=1e-6, eps_trans=1e-6, damping=1e-9)
    base.update(kw)
    return capi.make_align_config(**base)


@pytest.fixture(scope="module")
def world():
    from mimosa_amd import capi, synth
    ctx = capi.Context(0)
    room = synth.make_room(synth.BASE_SEED, 0, 0)
    maps = {}
    mid, _ = synth.make_scan(64)

    def cloud(n):
        c = np.ascontiguousarray(mid[:: max(1, len(mid) // n)][:n])
        assert len(c) == n
        return c

    def gmap(mode):
        if mode not in maps:
            maps[mode] = capi.VoxelMap(ctx, mode=mode)
            maps[mode].insert(room)
        return maps[mode]

    factors = {}

    def factor(n, k=5, mode=19, reg4=0, binary=False):
        key = (n, k, mode, reg4, binary)
        if key not in factors:
            cfg = dict(synth.enwide_config(), num_corres_points=k, reg_4_dof=reg4)
            factors[key] = capi.ICPFactor(ctx, gmap(mode), cloud(n), capi.make_reg_config(**cfg), binary=binary)
        return factors[key]

    yield dict(ctx=ctx, gmap=gmap, factor=factor, cloud=cloud, truth=synth.sensor_pose_gt(), capi=capi, synth=synth)
    for f in factors.values():
        f.destroy()
    for m in maps.values():
        m.release()
    ctx.close()


def same_result(a, b, tag):
    for key in b:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), (tag, key)


def same_bits(got, ref, tag):
    """a member's result against mh_icp_align's from the same start, bit for bit"""
    assert (got["iters"], got["converged"]) == (ref["iters"], ref["converged"]), tag
    assert len(got["trace"]) == len(ref["trace"]) == ref["iters"]
    for i, (a, b) in enumerate(zip(got["trace"], ref["trace"])):
        assert a["degenerate"] == b["degenerate"] and a["n_knn"] == b["n_knn"], (tag, i)
        for key in ("R", "t", "f", "step_rot", "step_trans"):
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (tag, i, key)
    assert np.array_equal(got["R"], ref["R"]) and np.array_equal(got["t"], ref["t"]), tag
    same_result(got["first"], ref["first"], (tag, "first"))
    same_result(got["last"], ref["last"], (tag, "last"))


def same_state(a, b, tag):
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y, equal_nan=True), tag


def same_chain(got, ref, tag):
    """the project's chain bar: 1e-9 m / 1e-9 rad per trace pose, equal iters / converged"""
    worst_t = worst_r = 0.0
    for a, b in zip(got["trace"], ref["trace"]):
        worst_t = max(worst_t, float(np.linalg.norm(a["t"] - b["t"])))
        worst_r = max(worst_r, rot_angle(a["R"], b["R"]))
    print(tag, "iters", got["iters"], ref["iters"], "worst trace difference: %.3e m %.3e rad" % (worst_t, worst_r))
    assert (got["iters"], got["converged"]) == (ref["iters"], ref["converged"]), tag
    assert worst_t <= 1e-9 and worst_r <= 1e-9, tag


def run_pair(world, bases, starts, cfg, wait=True):
    """(members, their results, reference factors, their results): the batch on clones of `bases`, mh_icp_align on second clones"""
    capi = world["capi"]
    members, refs = [b.clone() for b in bases], [b.clone() for b in bases]
    got = capi.align_batch(members, starts, cfg, G, wait=wait)
    if not wait:
        got = got.wait()
    ref = [r.align(R0, t0, cfg, G) for r, (R0, t0) in zip(refs, starts)]
    return members, got, refs, ref


def destroy(*lists):
    for l in lists:
        for f in l:
            f.destroy()


def device_factors(world):
    """(from_device, free): from_device() makes a factor of the 257-point cloud with mh_icp_create_from_device, which keeps the
    caller's point order as the pieces of a map-sharded factor do; free() gives the device cloud back once those factors are gone"""
    capi, synth = world["capi"], world["synth"]
    ctx, L = world["ctx"], world["ctx"].L
    pts = world["cloud"](257)
    d_pts = C.c_void_p()
    assert L.hipMalloc(C.byref(d_pts), C.c_size_t(pts.nbytes)) == 0
    assert L.hipMemcpy(d_pts, C.c_void_p(pts.ctypes.data), C.c_size_t(pts.nbytes), 1) == 0
    reg = capi.make_reg_config(**synth.enwide_config())

    def from_device():
        h = C.c_void_p()
        ctx.check(L.mh_icp_create_from_device(ctx.h, world["gmap"](19).h, d_pts, len(pts), C.byref(reg), 0, C.byref(h)))
        return capi.ICPFactor(ctx, world["gmap"](19), None, None, _h=h, _n=len(pts))

    def free():
        ctx.synchronize()
        assert L.hipFree(d_pts) == 0

    return from_device, free


def count_of(f, world):
    """the factor's linearize count (one more linearize shows it)"""
    return f.linearize(*world["truth"], G)["linearize_count"] - 1


def test_one_member_is_mh_icp_align(world):
    base = world["factor"](1024)
    start = perturbed(world["truth"], 7)
    members, got, refs, ref = run_pair(world, [base], [start], align_cfg())
    assert len(got) == 1
    same_bits(got[0], ref[0], "B=1")
    same_state(members[0], refs[0], "B=1")
    assert got[0]["last"]["linearize_count"] == ref[0]["last"]["linearize_count"] == got[0]["iters"]
    assert count_of(members[0], world) == count_of(refs[0], world) == got[0]["iters"]
    destroy(members, refs)


CLONE_STARTS = [(0.05, 1.0), (0.15, 2.3), (0.3, 3.6), (0.5, 5.0)]  # m, degrees


def test_four_clones_stop_on_their_own(world):
    base = world["factor"](1024)
    starts = [perturbed(world["truth"], 11 + i, dist=d, deg=a) for i, (d, a) in enumerate(CLONE_STARTS)]
    members, got, refs, ref = run_pair(world, [base] * 4, starts, align_cfg())
    print("reference iters", [r["iters"] for r in ref], "converged", [r["converged"] for r in ref])
    assert len({r["iters"] for r in ref}) >= 2  # the references alone: the members do not all stop together
    for m in range(4):
        same_bits(got[m], ref[m], f"clone {m}")
        same_state(members[m], refs[m], f"clone {m}")
        assert len(got[m]["trace"]) == got[m]["iters"]  # its n_knn rows stop where it stopped
        assert count_of(members[m], world) == got[m]["iters"]  # its count advanced by its own iters
    destroy(members, refs)


def test_unlike_members(world):
    """k 5 / 8 / 3, neighbour modes 7 / 19 / 27, 1 / 257 / 1 024 points, one member with reg_4_dof (the prior on the rotation
    serves it and, as cfg is the call's, every member).  Three launch groups per iteration: {0, 3}, {1}, {2} — member 3 rides in
    slot 1, member 1 in slot 2."""
    f = world["factor"]
    bases = [f(1024, 5, 7), f(257, 8, 19, reg4=1), f(1, 3, 27), f(257, 5, 7)]
    starts = [perturbed(world["truth"], 21 + i) for i in range(4)]
    members, got, refs, ref = run_pair(world, bases, starts, align_cfg(prior_sigma_rot=0.1))
    print("iters", [r["iters"] for r in ref])
    for m in range(4):
        same_bits(got[m], ref[m], f"unlike {m}")
        same_state(members[m], refs[m], f"unlike {m}")
    destroy(members, refs)


def test_singular_member_stops_alone(world):
    """member 1 is the singular case of test_gpu_icp_align.py's degenerate scene: a rough floor as the map, the scan's floor hits,
    project_on_degneneracy on with a threshold no plane's x, y reach, no prior, no damping"""
    capi, synth = world["capi"], world["synth"]
    ctx = world["ctx"]
    Rt, tt = world["truth"]
    gx, gy = np.meshgrid(np.arange(-10.0, 10.0, 0.08), np.arange(-10.0, 10.0, 0.08))
    origin = synth.room_origin(0, 0)
    rough = np.random.default_rng(0).normal(0.0, 0.004, gx.size)
    plane = np.stack([gx.ravel() + tt[0], gy.ravel() + tt[1], origin[2] + rough], axis=1).astype(np.float32)
    gm = capi.VoxelMap(ctx)
    gm.insert(plane)
    scan, _ = synth.make_scan(64)
    pw = synth.points_xyz(scan).astype(np.float64) @ Rt.T + tt
    room = np.asarray(synth.ROOM, float)
    inside = np.all((pw[:, :2] > origin[:2] + 0.3) & (pw[:, :2] < origin[:2] + room[:2] - 0.3), axis=1)
    near = np.linalg.norm(synth.points_xyz(scan), axis=1) < 8.0
    floor = np.ascontiguousarray(scan[inside & near & (np.abs(pw[:, 2] - origin[2]) < 0.06)][:2048])
    assert len(floor) == 2048
    cfg = dict(synth.enwide_config(), project_on_degneneracy=1, degen_thresh_trans=1e6)
    sing = capi.ICPFactor(ctx, gm, floor, capi.make_reg_config(**cfg))
    Rs, ts = Rt @ expmap([0.002, -0.003, 0.0]), tt + np.array([0.0, 0.0, 0.03])
    room_f = world["factor"](1024)
    starts = [perturbed(world["truth"], 31), (Rs, ts), perturbed(world["truth"], 32)]
    members, got, refs, ref = run_pair(world, [room_f, sing, room_f], starts, align_cfg(damping=0.0))
    s = got[1]
    assert s["iters"] == 1 and s["converged"] == 0 and s["trace"][-1]["degenerate"] & 4
    assert np.array_equal(s["R"], Rs) and np.array_equal(s["t"], ts)
    for m in range(3):
        same_bits(got[m], ref[m], f"singular {m}")
        same_state(members[m], refs[m], f"singular {m}")
    assert got[0]["converged"] == 1 and got[2]["converged"] == 1 and got[0]["iters"] > 1 and got[2]["iters"] > 1
    destroy(members, refs, [sing])
    gm.release()


@pytest.mark.parametrize("B,n", [(4, 12288), (3, 24576)])
def test_launch_classes(world, B, n):
    """4 x 12 288 points, k = 5: 49 152 in all, the 256-thread class where a call of its own gets the two-lanes-per-point class;
    3 x 24 576: more than 65 536, the 512-thread class.  Held to the chain bar (the module's docstring)."""
    capi = world["capi"]
    base = world["factor"](n)
    starts = [perturbed(world["truth"], 41 + i) for i in range(B)]
    # what moves the bits: K3's batch form in the window's class against separate calls, on this exact window
    a, b = [base.clone() for _ in range(B)], [base.clone() for _ in range(B)]
    for f in a + b:
        f.set_components(False)
    lb = capi.linearize_batch(a, [s[0] for s in starts], [s[1] for s in starts])
    ls = [f.linearize(R0, t0, G) for f, (R0, t0) in zip(b, starts)]
    rel = max(float(np.abs(x["H_ss"] - y["H_ss"]).max() / np.abs(y["H_ss"]).max()) for x, y in zip(lb, ls))
    print(f"B={B} n={n}: mh_icp_linearize_batch against separate calls, worst |dH| / |H| = {rel:.3e}")
    assert rel <= 1e-12
    destroy(a, b)
    members, got, refs, ref = run_pair(world, [base] * B, starts, align_cfg(max_iters=6))
    for m in range(B):
        same_chain(got[m], ref[m], f"B={B} n={n} member {m}")
        assert np.array_equal(members[m].state()[0], refs[m].state()[0])
        assert got[m]["trace"][0]["n_knn"] == ref[m]["trace"][0]["n_knn"] == n
    destroy(members, refs)


def test_check_every_and_async(world):
    capi = world["capi"]
    base = world["factor"](1024)
    starts = [perturbed(world["truth"], 11 + i, dist=d, deg=a) for i, (d, a) in enumerate(CLONE_STARTS)]
    runs = []
    for ce, wait in ((0, True), (1, True), (3, True), (0, False)):
        members = [base.clone() for _ in range(4)]
        cfg = align_cfg(check_every=ce)
        if wait:
            got = capi.align_batch(members, starts, cfg, G)
        else:
            call = capi.align_batch(members, starts, cfg, G, wait=False)
            other = base.clone()  # a factor outside the call is free
            other.linearize(*starts[0], G)
            other.destroy()
            for what in (lambda: members[1].reset(), lambda: members[1].linearize(*starts[1], G), lambda: members[2].wait(),
                         lambda: capi.align_batch([members[1]], [starts[1]], cfg, G), lambda: capi.align_batch([base], [starts[0]], cfg, G)):
                with pytest.raises(capi.MhError) as e:
                    what()
                assert e.value.code == capi.MH_ERR_INVALID_ARG
            got = call.wait()
            with pytest.raises(capi.MhError):  # nothing in flight any more
                call.wait()
        runs.append((members, got))
    for members, got in runs[1:]:
        for m in range(4):
            same_bits(got[m], runs[0][1][m], f"run member {m}")
            same_state(members[m], runs[0][0][m], f"run member {m}")
    # after the wait the members work
    members, got = runs[-1]
    members[1].reset()
    assert members[1].linearize(*starts[1], G)["linearize_count"] == got[1]["iters"] + 1
    again = capi.align_batch([members[1]], [starts[1]], align_cfg(), G)
    assert again[0]["iters"] >= 1
    for members, _ in runs:
        destroy(members)


def test_destroying_a_member_abandons_the_call(world):
    """a member destroyed inside a call nobody waited for: the call is over as a whole, the other members are free again (their
    books did not move: after a reset they are fresh clones), and the context takes the next batch call"""
    capi = world["capi"]
    ctx, L = world["ctx"], world["ctx"].L
    base = world["factor"](257)
    members, fresh = [base.clone() for _ in range(3)], base.clone()
    starts = [perturbed(world["truth"], 61 + i) for i in range(3)]
    cfg = align_cfg()
    call = capi.align_batch(members, starts, cfg, G, wait=False)
    members[1].destroy()
    assert L.mh_icp_align_batch_wait(ctx.h) == capi.MH_ERR_INVALID_ARG  # nothing is in flight any more
    del call
    probe = perturbed(world["truth"], 64)
    ref = fresh.linearize(*probe, G)
    for m in (members[0], members[2]):
        m.wait()  # no longer refused: nothing pending
        m.reset()
        same_result(m.linearize(*probe, G), ref, "a member of the abandoned call")
    got = capi.align_batch([members[0], members[2]], [starts[0], starts[2]], cfg, G)
    assert all(r["iters"] >= 1 for r in got)
    destroy([members[0], members[2], fresh])


def test_refusals(world):
    capi, synth = world["capi"], world["synth"]
    L, ctx = world["ctx"].L, world["ctx"]
    base = world["factor"](257)
    fs, twins = [base.clone() for _ in range(3)], [base.clone() for _ in range(3)]
    start = perturbed(world["truth"], 51)
    cfg = align_cfg()
    probe = perturbed(world["truth"], 52)

    def still_answer():
        for f, tw in zip(fs, twins):
            same_result(f.linearize(*probe, G), tw.linearize(*probe, G), "after a refusal")

    def refused(code, factors, poses=None, c=cfg, word=None):
        with pytest.raises(capi.MhError) as e:
            capi.align_batch(factors, poses if poses is not None else [start] * len(factors), c, G)
        assert e.value.code == code, str(e.value)
        assert word is None or word in str(e.value)
        still_answer()

    # NULL arguments and a NULL member, straight at the ABI
    R = np.ascontiguousarray(np.tile(start[0].reshape(9), (3, 1)))
    t = np.ascontiguousarray(np.tile(start[1], (3, 1)))
    handles = (C.c_void_p * 3)(*[f.h for f in fs])
    out = (capi.AlignResult * 3)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [handles, 3, vp(R), vp(t), vp(G), C.byref(cfg), out]
    for i in (0, 2, 3, 4, 5, 6):
        args = list(good)
        args[i] = None
        assert L.mh_icp_align_batch(*args) == capi.MH_ERR_INVALID_ARG
        assert L.mh_icp_align_batch_async(*args) == capi.MH_ERR_INVALID_ARG
        still_answer()
    holed = (C.c_void_p * 3)(fs[0].h, None, fs[2].h)
    assert L.mh_icp_align_batch(holed, 3, vp(R), vp(t), vp(G), C.byref(cfg), out) == capi.MH_ERR_INVALID_ARG
    assert L.mh_icp_align_batch(handles, 0, vp(R), vp(t), vp(G), C.byref(cfg), out) == capi.MH_ERR_INVALID_ARG
    assert L.mh_icp_align_batch_wait(None) == capi.MH_ERR_INVALID_ARG
    assert L.mh_icp_align_batch_wait(ctx.h) == capi.MH_ERR_INVALID_ARG  # none in flight
    still_answer()
    # B above the maximum
    many = [base.clone() for _ in range(capi.MH_ALIGN_BATCH_MAX + 1)]
    refused(capi.MH_ERR_INVALID_ARG, many, word="1..16")
    full = capi.align_batch(many[:-1], [start] * capi.MH_ALIGN_BATCH_MAX, align_cfg(max_iters=2), G)  # 16 is accepted
    assert len(full) == capi.MH_ALIGN_BATCH_MAX and all(r["iters"] >= 1 for r in full)
    destroy(many)
    refused(capi.MH_ERR_INVALID_ARG, [fs[0], fs[1], fs[0]], word="twice")
    # factors of different contexts
    ctx2 = capi.Context(0)
    gm2 = capi.VoxelMap(ctx2)
    gm2.insert(synth.make_room(synth.BASE_SEED, 0, 0))
    foreign = capi.ICPFactor(ctx2, gm2, world["cloud"](257), capi.make_reg_config(**synth.enwide_config()))
    refused(capi.MH_ERR_INVALID_ARG, [fs[0], foreign], word="contexts")
    foreign.destroy()
    gm2.release()
    ctx2.close()
    # a member with a call in flight; a member without points
    pending = fs[1].linearize_async(*probe, G)
    with pytest.raises(capi.MhError) as e:
        capi.align_batch(fs, [start] * 3, cfg, G)
    assert e.value.code == capi.MH_ERR_INVALID_ARG and "in flight" in str(e.value)
    fs[1].wait()
    same_result(pending.as_dict(), twins[1].linearize(*probe, G), "the call that was in flight")
    still_answer()
    empty = capi.ICPFactor(ctx, world["gmap"](19), world["cloud"](257)[:0], capi.make_reg_config(**synth.enwide_config()))
    refused(capi.MH_ERR_INVALID_ARG, [fs[0], empty], word="no points")
    empty.destroy()
    # a batch call already in flight on the context
    others = [base.clone() for _ in range(2)]
    call = capi.align_batch(others, [start] * 2, cfg, G, wait=False)
    refused(capi.MH_ERR_INVALID_ARG, fs, word="in flight")
    call.wait()
    destroy(others)
    # the cfg ranges of mh_icp_align
    for bad in (dict(max_iters=0), dict(max_iters=65), dict(damping=-1.0), dict(eps_rot=-1.0), dict(eps_trans=float("nan")), dict(prior_sigma_rot=-0.1),
                dict(prior_sigma_trans=-0.1), dict(check_every=-1)):
        refused(capi.MH_ERR_INVALID_ARG, fs, c=align_cfg(**bad))
    # binary factors
    binary = world["factor"](257, binary=True)
    refused(capi.MH_ERR_UNSUPPORTED, [fs[0], binary], word="unary")
    # the factors of the map-sharded path: mh_icp_create_from_device keeps the caller's point order, as the sharded factor's
    # pieces do.  Alone and among ordinary members; afterwards it still linearizes as a twin made from the same device cloud
    from_device, free_device_cloud = device_factors(world)
    kept, kept_twin = from_device(), from_device()
    same_result(kept.linearize(*probe, G), kept_twin.linearize(*probe, G), "device factors")
    for members in ([kept], [fs[0], kept, fs[1]], [kept, fs[2]]):
        refused(capi.MH_ERR_UNSUPPORTED, members, word="map-sharded")
        same_result(kept.linearize(*probe, G), kept_twin.linearize(*probe, G), "the device factor after a refusal")
    destroy([kept, kept_twin])
    free_device_cloud()
    destroy(fs, twins)


# ---- mh_icp_align and mh_icp_align_batch are one chain driver: where the two forms meet -----------------------------------
def test_chains_side_by_side(world):
    """two mh_icp_align_async chains (each on its factor's own storage) and one mh_icp_align_batch_async chain (on the context's)
    in flight at once with a plain linearize between them, collected in the reverse of the order they were started: everything
    as blocking calls on fresh clones from the same starts give it"""
    capi = world["capi"]
    big, one = world["factor"](257), world["factor"](1, 3, 27)
    bases = [big, one, big, one, big]
    starts = [perturbed(world["truth"], 71 + i) for i in range(5)]
    cfg = align_cfg()
    fs, refs = [b.clone() for b in bases], [b.clone() for b in bases]
    singles = [fs[0].align_async(*starts[0], cfg, G), fs[1].align_async(*starts[1], cfg, G)]
    call = capi.align_batch(fs[2:4], starts[2:4], cfg, G, wait=False)
    lin = fs[4].linearize(*starts[4], G)
    got_batch = call.wait()
    fs[1].wait()
    fs[0].wait()
    got = [singles[0].as_dict(), singles[1].as_dict()] + got_batch
    ref = [refs[0].align(*starts[0], cfg, G), refs[1].align(*starts[1], cfg, G)] + capi.align_batch(refs[2:4], starts[2:4], cfg, G)
    print("iters", [r["iters"] for r in ref])
    for m in range(4):
        same_bits(got[m], ref[m], f"side by side {m}")
    same_result(lin, refs[4].linearize(*starts[4], G), "the linearize between the chains")
    for m in range(5):
        same_state(fs[m], refs[m], f"side by side {m}")
    destroy(fs, refs)


def test_one_landing_slot_is_enough(world):
    """all 64 iterations evaluated (eps = 0: nothing converges), queued at once and one by one: K3's words of every iteration
    land in the same device slot, told apart by the iteration's sequence number; a one-member batch gives the same trace"""
    capi = world["capi"]
    base = world["factor"](257)
    start = perturbed(world["truth"], 81)
    runs = []
    for ce in (0, 1):
        f = base.clone()
        runs.append((f, f.align(*start, align_cfg(max_iters=64, eps_rot=0.0, eps_trans=0.0, check_every=ce), G)))
    member = base.clone()
    batch = capi.align_batch([member], [start], align_cfg(max_iters=64, eps_rot=0.0, eps_trans=0.0), G)
    assert runs[0][1]["iters"] == 64 and runs[1][1]["iters"] == 64
    same_bits(runs[1][1], runs[0][1], "check_every 1 against 0")
    same_state(runs[1][0], runs[0][0], "check_every 1 against 0")
    same_bits(batch[0], runs[0][1], "one-member batch")
    same_state(member, runs[0][0], "one-member batch")
    destroy([f for f, _ in runs], [member])


def test_order_of_the_refusals(world):
    """which refusal comes first where an argument earns two: each entry point keeps its own order (codes and texts as the
    commit before the two forms shared a driver gave them)"""
    capi, synth = world["capi"], world["synth"]
    ctx = world["ctx"]
    base = world["factor"](257)
    good, twin, busy = base.clone(), base.clone(), base.clone()
    start, probe = perturbed(world["truth"], 91), perturbed(world["truth"], 92)
    from_device, free_device_cloud = device_factors(world)
    kept = from_device()
    binary = world["factor"](257, binary=True)
    empty = capi.ICPFactor(ctx, world["gmap"](19), world["cloud"](257)[:0], capi.make_reg_config(**synth.enwide_config()))

    def refused(call, code, word, without=None):
        with pytest.raises(capi.MhError) as e:
            call()
        print(e.value.code, str(e.value))
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert without is None or without not in str(e.value), str(e.value)
        same_result(good.linearize(*probe, G), twin.linearize(*probe, G), "the good factor after a refusal")

    # mh_icp_align: NULL, unary, in flight, max_iters, the other ranges, the sharded path, no points
    refused(lambda: binary.align(*start, align_cfg(max_iters=0), G), capi.MH_ERR_UNSUPPORTED, "unary")
    refused(lambda: kept.align(*start, align_cfg(max_iters=0), G), capi.MH_ERR_INVALID_ARG, "max_iters")
    refused(lambda: kept.align(*start, align_cfg(), G), capi.MH_ERR_UNSUPPORTED, "map-sharded")
    refused(lambda: empty.align(*start, align_cfg(damping=-1.0), G), capi.MH_ERR_INVALID_ARG, "must be >= 0", without="no points")
    # mh_icp_align_batch: the factors before the config
    refused(lambda: capi.align_batch([good, kept], [start] * 2, align_cfg(max_iters=0), G), capi.MH_ERR_UNSUPPORTED, "map-sharded")
    pending = busy.linearize_async(*probe, G)
    refused(lambda: capi.align_batch([good, busy], [start] * 2, align_cfg(max_iters=0), G), capi.MH_ERR_INVALID_ARG, "in flight")
    busy.wait()
    fresh = base.clone()
    same_result(pending.as_dict(), fresh.linearize(*probe, G), "the call that was in flight")
    destroy([kept, empty])
    free_device_cloud()
    destroy([good, twin, busy, fresh])


def test_held_factors_every_holder(world):
    """a factor held by each of the four calls that take its whole ring — mh_icp_align_async, mh_icp_align_batch_async, a window
    call, mh_icp_score_poses_async — refuses reset, linearize, align, score_poses, clone (and wait, where the holder's own wait is
    the context's) with the code and the words it always had; after the holder's own wait every one of them works"""
    capi = world["capi"]
    base = world["factor"](257)
    start, probe = perturbed(world["truth"], 95), perturbed(world["truth"], 96)
    cfg = align_cfg()
    I = (np.eye(3), np.zeros(3))

    def hold_align(f, mate):
        f.align_async(*start, cfg, G)
        return f.wait

    def hold_batch(f, mate):
        return capi.align_batch([mate, f], [start] * 2, cfg, G, wait=False).wait

    def hold_window(f, mate):
        return capi.optimise_window([mate, f], [start] * 2, capi.make_window_config(iters=3), has_Z=[0, 1], Z=[I, I], wait=False).wait

    def hold_score(f, mate):
        f.score_poses_async(start[0][None], start[1][None], 1.0)
        return f.wait

    # holder: (how it takes hold, mh_icp_reset's words, mh_icp_wait's where it refuses)
    holders = {"align": (hold_align, "an alignment is in flight", None),
               "align_batch": (hold_batch, "batch alignment in flight", "mh_icp_align_batch_wait collects it"),
               "window": (hold_window, "window call in flight", "mh_icp_window_wait collects it"),
               "score": (hold_score, "pose scoring call is in flight", None)}
    for name, (hold, reset_words, wait_words) in holders.items():
        f, mate = base.clone(), base.clone()
        calls = {"reset": (f.reset, reset_words),
                 "linearize": (lambda: f.linearize(*probe, G), "too many calls in flight"),
                 "align": (lambda: f.align(*start, cfg, G), "mh_icp_align: the factor has calls in flight"),
                 "score_poses": (lambda: f.score_poses(start[0][None], start[1][None], 1.0), "mh_icp_score_poses: the factor has calls in flight"),
                 "clone": (lambda: f.clone().destroy(), "source has linearize calls in flight")}
        release = hold(f, mate)
        for what, (call, words) in list(calls.items()) + ([("wait", (f.wait, wait_words))] if wait_words else []):
            with pytest.raises(capi.MhError) as e:
                call()
            print(name, what, e.value.code, str(e.value))
            assert e.value.code == capi.MH_ERR_INVALID_ARG and words in str(e.value), (name, what, str(e.value))
        release()
        for what, (call, _) in calls.items():
            call()
        f.wait()  # nothing pending: not refused
        destroy([f, mate])


# ---- mh_icp_relocalise_batch on the scene of test_gpu_reloc.py's test_relocalise_recovers_the_pose ------------------------
GUESS_OFF = np.array([1.2, -0.9, 0.0])
GUESS_YAW = np.deg2rad(20.0)
GRID = dict(half_xy=2.0, step_xy=0.5, half_yaw=np.deg2rad(30.0), step_yaw=np.deg2rad(7.5))
COARSE = dict(gate=1.0, stride=4, top_k=4)
FINAL_GATE = 0.1


def test_relocalise_batch(world):
    capi, synth = world["capi"], world["synth"]
    ctx = capi.Context(0)
    m, pts, aux = synth.small_world()
    gm = capi.VoxelMap(ctx, mode=19)
    gm.insert(m)
    reg = capi.make_reg_config(**synth.enwide_config())
    Rg, tg = aux["R_W_L"], aux["t_W_L"]
    Rs, ts = capi.pose_grid(synth.rot_z(GUESS_YAW) @ Rg, tg + GUESS_OFF, **GRID)
    cfg = capi.make_reloc_config(align=capi.make_align_config(max_iters=30, eps_rot=1e-9, eps_trans=1e-9, damping=1e-9), final_gate=FINAL_GATE, **COARSE)
    f, twin = capi.ICPFactor(ctx, gm, np.ascontiguousarray(pts), reg), capi.ICPFactor(ctx, gm, np.ascontiguousarray(pts), reg)
    # a warm factor with a count: what must not move
    warm = (Rg, tg + np.array([0.02, 0.0, 0.0]))
    f.linearize(*warm, G)
    untouched = f.clone()
    ref = twin.relocalise(Rs, ts, cfg, G)
    out = f.relocalise(Rs, ts, cfg, G, batch=True)
    assert out["n_candidates"] == ref["n_candidates"] == COARSE["top_k"] and out["best"] == ref["best"]
    for c, r in zip(out["cand"], ref["cand"]):
        assert c["index"] == r["index"] and (c["iters"], c["converged"]) == (r["iters"], r["converged"])
        for name in ("n_points", "n_occupied", "n_inliers", "sum_sq"):
            assert c["coarse"][name] == r["coarse"][name], name  # bit for bit
        dt, dr = float(np.linalg.norm(c["t"] - r["t"])), rot_angle(c["R"], r["R"])
        print("candidate %d: iters %d, aligned pose differs by %.3e m %.3e rad" % (c["index"], c["iters"], dt, dr))
        assert dt <= 1e-9 and dr <= 1e-9
        for name in ("n_points", "n_occupied", "n_inliers"):
            assert c["fine"][name] == r["fine"][name], name
        assert abs(c["fine"]["sum_sq"] - r["fine"]["sum_sq"]) <= 1e-9 * r["fine"]["sum_sq"]
    w = out["cand"][out["best"]]
    assert np.array_equal(out["R"], w["R"]) and np.array_equal(out["t"], w["t"])
    # the work factors: counts advanced by their own iters
    for wk, c in zip(f._reloc_work, out["cand"]):
        assert wk.linearize(*warm, G)["linearize_count"] == 1 + c["iters"] + 1
    # icp was only read: state, count and a following linearize are an untouched clone's
    same_state(f, untouched, "the scored factor")
    same_result(f.linearize(*warm, G), untouched.linearize(*warm, G), "the scored factor")
    same_state(f, untouched, "the scored factor")

    # the refusals of work[]
    L = ctx.L
    Rc, tc = np.ascontiguousarray(Rs.reshape(-1, 9)), np.ascontiguousarray(ts.reshape(-1, 3))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    res = capi.RelocResult()
    err = lambda: (L.mh_last_error(ctx.h) or b"").decode()

    def call(work, icp=f):
        h = (C.c_void_p * max(len(work), 1))(*[w.h if w is not None else None for w in work])
        return L.mh_icp_relocalise_batch(icp.h, h, len(work), vp(Rc), vp(tc), len(Rc), vp(G), C.byref(cfg), C.byref(res))

    work = list(f._reloc_work)
    assert len(work) == 4
    assert call(work) == capi.MH_OK
    assert call(work[:3]) == capi.MH_ERR_INVALID_ARG and "fewer" in err()  # too few
    assert call(work[:3] + [twin]) == capi.MH_ERR_INVALID_ARG and "not a clone" in err()  # a foreign factor of equal size
    assert call(work[:3] + [f]) == capi.MH_ERR_INVALID_ARG and "itself" in err()
    assert call(work[:3] + [None]) == capi.MH_ERR_INVALID_ARG
    assert call(work[:3] + [work[0]]) == capi.MH_ERR_INVALID_ARG and "twice" in err()
    # (a different config: the public calls cannot make a CLONE with another config, so this factor's identity differs as well and
    # the library's comparison of the configs is never the deciding check; it is kept as the contract lists it)
    other_cfg = capi.ICPFactor(ctx, gm, np.ascontiguousarray(pts), capi.make_reg_config(**dict(synth.enwide_config(), num_corres_points=8)))
    assert call(work[:3] + [other_cfg]) == capi.MH_ERR_INVALID_ARG and "not a clone" in err()
    assert L.mh_icp_relocalise_batch(f.h, None, 4, vp(Rc), vp(tc), len(Rc), vp(G), C.byref(cfg), C.byref(res)) == capi.MH_ERR_INVALID_ARG
    # every refusal left the scored factor alone
    same_result(f.linearize(*warm, G), untouched.linearize(*warm, G), "after the refusals")
    for x in (other_cfg, untouched, twin, f):
        x.destroy()
    gm.release()
    ctx.close()
