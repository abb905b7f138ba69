"""-m gpu: mh_icp_window_optimise_joint and mh_icp_window_marginalise_joint — the fixed-lag chain with ONE dense factor on up to
four poses, and the call that produces it: the marginal of the oldest pose on its separator.

Scene: that of tests/test_gpu_icp_window.py (synth.small_world(): a map of ~5 k points, a 1 024-point scan); the factors here
take every fourth point of the scan (256 points), the first consumer case the whole scan (1 024 points).

1.  joint == NULL is mh_icp_window_optimise_edges bit for bit (poses, trace, first / last, masks, factor state); a one-member joint
    factor is mh_icp_window_optimise_edges with the same data as the last linear factor, bit for bit.
2.  The marginal without far edges and without a joint factor is mh_icp_window_marginalise bit for bit; `oldest` is
    mh_icp_linearize of a fresh clone bit for bit.
3.  Six consumer cases against the host-driven loop written here: SEPARATE mh_icp_linearize calls per factor and iteration, the
    restatement of tests/window_joint_ref.py (numpy, dense, written independently of the header) for assembly and the refined
    solve of tests/test_gpu_icp_window.py.  Every pose of every iteration within 1e-9 m / 1e-9 rad; under thresholds equal masks;
    an early stop with iterations queued behind it; an empty factor on a member pose.  Sync, async and check_every = 1: same bits.
4.  Producer cases as in tests/test_icp_window_joint_cpu.py, fed with the device's `oldest`: 1e-9 relative to ||A_SS'||_F,
    ||g_S'||, |c|; cond(A00) <= 1e6 asserted.  (The rank-3 H_ss of the CPU test cannot be asked of a real scan; its stand-in here
    is the empty oldest factor — rank 0 — held by the prior.)
5.  The elimination identity through the two public calls with iters = 1: 1e-9 m / 1e-9 rad, more than 1e-4 m without the marginal.
6.  Async and the C++ mirror (tests/cpp/window_joint_pipeline.cpp) give the blocking call's bits."""
import ctypes as C
import json
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_icp_window as base
import test_gpu_icp_window_relin as relin_base
import window_edge_ref as edge_ref
import window_joint_ref as ref
import window_lin_ref as lin_ref
from test_gpu_icp_window import world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G = base.G
RELIN = relin_base.RELIN
FIXED = dict(iters=6, eps_rot=0.0, eps_trans=0.0)
ZERO = [0.0] * 6


def small_base(world, empty=False):
    """a 256-point factor on the small map (every fourth point of the scan), kept with the world's bases"""
    key = ("joint-small", empty)
    if key not in world.bases:
        capi = world.capi
        cfg = dict(world.synth.enwide_config(), num_corres_points=5, reg_4_dof=0, project_on_degneneracy=0)
        pts = np.ascontiguousarray(world.small_scan[::4])
        world.bases[key] = capi.ICPFactor(world.ctx, world.small_map, pts[:0] if empty else pts, capi.make_reg_config(**cfg))
        assert world.bases[key].n == (0 if empty else 256)
    return world.bases[key]


def optimise_joint_null(world, fs, poses, cfg, has_Z, Z, relin, linear, edges, wait=True):
    """mh_icp_window_optimise_joint[_async] with joint == NULL, through the entry point itself"""
    capi = world.capi
    W = len(fs)
    R = np.ascontiguousarray(np.array([np.asarray(p[0], np.float64).reshape(9) for p in poses]))
    t = np.ascontiguousarray(np.array([np.asarray(p[1], np.float64).reshape(3) for p in poses]))
    hz = np.ascontiguousarray(np.asarray(has_Z).astype(np.int32))
    ZR = np.ascontiguousarray(np.array([np.asarray(z[0], np.float64).reshape(9) for z in Z]))
    Zt = np.ascontiguousarray(np.array([np.asarray(z[1], np.float64).reshape(3) for z in Z]))
    handles = (C.c_void_p * W)(*[f.h for f in fs])
    out = capi.WindowResult()
    trace = np.full((int(cfg.iters), W, 12), np.nan)
    rl = None if relin is None else capi.WindowRelin(float(relin[0]), float(relin[1]))
    masks = None if relin is None else np.zeros(int(cfg.iters), np.uint32)
    lin, ed = capi.make_window_linear(linear), capi.make_window_edge(edges)
    L = world.ctx.L
    fn = L.mh_icp_window_optimise_joint if wait else L.mh_icp_window_optimise_joint_async
    world.ctx.check(fn(handles, W, capi._p(R), capi._p(t), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(G), C.byref(cfg), None if rl is None else C.byref(rl), lin,
                       len(linear), ed, len(edges), C.byref(out), capi._p(trace), capi._p(masks), None))
    if not wait:
        world.ctx.check(L.mh_icp_window_wait(world.ctx.h))
    d = out.as_dict()
    d["poses"] = trace[:d["iters"]]
    if masks is not None:
        d["evaluated"] = masks[:d["iters"]].copy()
    return d


def same_states(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x.state(), y.state()):
            assert np.array_equal(u, v, equal_nan=True)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relin", [None, RELIN])
def test_no_joint_factor_is_the_edges_call_bit_for_bit(world, relin):
    capi = world.capi
    W = 3
    poses, Z, has_Z = base.scene(world, W, 141)
    rng = np.random.default_rng(141)
    for edges in ([], [edge_ref.random_edge(rng, 0, 2, poses), edge_ref.random_edge(rng, 1, 2, poses)]):
        linear = [lin_ref.random_linear(rng, i, poses[i]) for i in (0, 2)]
        cfg = base.window_cfg(True, **FIXED)
        a, b, c = ([small_base(world).clone() for _ in range(W)] for _ in range(3))
        want = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, edges=edges)
        got = optimise_joint_null(world, b, poses, cfg, has_Z, Z, relin, linear, edges)
        got_async = optimise_joint_null(world, c, poses, cfg, has_Z, Z, relin, linear, edges, wait=False)
        relin_base.same_bits(got, want)
        relin_base.same_bits(got_async, want)
        assert got["iters"] == 6 and ("evaluated" in got) == (relin is not None)
        same_states(a, b)
        for f in a + b + c:
            f.destroy()


@pytest.mark.parametrize("relin", [None, RELIN])
def test_one_member_is_the_last_linear_factor_bit_for_bit(world, relin):
    capi = world.capi
    W = 3
    poses, Z, has_Z = base.scene(world, W, 142)
    rng = np.random.default_rng(142)
    linear = [lin_ref.random_linear(rng, i, poses[i]) for i in (1, 2, 1)]
    edges = [edge_ref.random_edge(rng, 0, 2, poses)]
    for edge_list in ([], edges):
        l = lin_ref.random_linear(rng, 1, poses[1])
        joint = dict(poses=[1], at=[l["at"]], H=l["H"], b=l["b"], f=l["f"])
        cfg = base.window_cfg(True, **FIXED)
        a, b = ([small_base(world).clone() for _ in range(W)] for _ in range(2))
        want = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear + [l], edges=edge_list)
        got = capi.optimise_window(b, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, edges=edge_list, joint=joint)
        relin_base.same_bits(got, want)
        same_states(a, b)
        for f in a + b:
            f.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def same_icp(a, b):
    for k in a:
        if not k.startswith("gpu_ms"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_marginal_without_far_edges_is_the_existing_call_bit_for_bit(world):
    capi = world.capi
    W = 3
    poses, Z, has_Z = base.scene(world, W, 143)
    rng = np.random.default_rng(143)
    linear = [lin_ref.random_linear(rng, 1, poses[1]), lin_ref.random_linear(rng, 0, poses[0]), lin_ref.random_linear(rng, 0, poses[0])]
    edges = [edge_ref.random_edge(rng, 0, 1, poses), edge_ref.random_edge(rng, 1, 2, poses), edge_ref.random_edge(rng, 0, 1, poses)]
    cfg = base.window_cfg(False, iters=1, eps_rot=0.0, eps_trans=0.0)
    a, b = ([small_base(world).clone() for _ in range(W)] for _ in range(2))
    want = capi.marginalise_window(a, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges)
    got = capi.marginalise_window_joint(b, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges)
    assert got["valid"] == want["valid"] == 1 and got["n_ties"] == want["n_ties"] == 3
    assert got["joint_here"]["poses"] == [1] and got["joint"]["poses"] == [0]
    for k in ("H", "b"):
        assert np.asarray(got["joint"][k]).tobytes() == np.asarray(want["linear"][k]).tobytes(), k
    assert got["joint"]["f"] == want["linear"]["f"]
    assert np.array_equal(got["joint"]["at"][0][0], poses[1][0]) and np.array_equal(got["joint"]["at"][0][1], poses[1][1])
    same_icp(got["oldest"], want["oldest"])
    fresh = small_base(world).clone()
    fresh.set_components(False)
    same_icp(got["oldest"], fresh.linearize(*poses[0], G))
    same_states(a, b)
    for f in a + b + [fresh]:
        f.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def host_loop(factors, have, poses, Z, has_Z, cfg, linear, edges, joint, relin=None):
    """the loop a caller writes around SEPARATE mh_icp_linearize calls; with `relin` the rule of mh_icp_window_optimise_relin; the
    stopping rule of the chain"""
    for f in factors:
        f.set_components(False)
    poses = [(np.array(R, float), np.array(t, float)) for R, t in poses]
    W = len(poses)
    Wb, prior = np.array(cfg.between_info), np.array(cfg.prior_info)
    kept = [None] * W
    trace, masks, margin, converged = [], [], np.inf, 0
    thr = None if relin is None else np.array([relin[0]] * 3 + [relin[1]] * 3)
    for it in range(cfg.iters):
        icp, mask = [], 0
        for i in range(W):
            if not have[i]:
                icp.append(None)
                continue
            d = None if (relin is None or it == 0) else relin_base.local(kept[i][0], poses[i])
            if d is not None:
                margin = min(margin, float(np.abs(np.abs(d) - thr).min()))
            if d is None or bool(np.any(np.abs(d) > thr)):
                r = factors[i].linearize(*poses[i], G)
                kept[i] = (poses[i], np.array(r["H_ss"], float).reshape(6, 6), np.array(r["b_s"], float), float(r["f"]))
                icp.append(kept[i][1:])
                mask |= 1 << i
            else:
                icp.append(lin_ref.transport(kept[i][1], kept[i][2], kept[i][3], kept[i][0], poses[i]))
        poses, xi, cost = ref.iteration(poses, icp, has_Z, Z, Wb, prior, cfg.damping, linear, edges, joint, solve=base.solve_refined)
        trace.append(dict(poses=poses, f=cost))
        masks.append(mask)
        if np.all(np.linalg.norm(xi[:, :3], axis=1) < cfg.eps_rot) and np.all(np.linalg.norm(xi[:, 3:], axis=1) < cfg.eps_trans):
            converged = 1
            break
    return dict(poses=poses, iters=len(trace), converged=converged, trace=trace, masks=masks, margin=margin)


def consumer_case(world, name):
    """(make factor i, W, have, poses, Z, has_Z, linear, edges, joint, relin, cfg keywords)"""
    seed = {"a_two_members": 151, "b_three_members_beside_edges": 152, "c_sixteen_poses": 153, "d_relin": 154, "e_early_stop": 155, "f_empty_member": 156}[name]
    rng = np.random.default_rng(seed)
    small = lambda i: small_base(world).clone()  # noqa: E731
    if name == "a_two_members":  # the 1 024-point factors
        W = 3
        poses, Z, has_Z = base.scene(world, W, seed)
        return (lambda i: world.base(5).clone()), W, [True] * W, poses, Z, has_Z, [], [], ref.random_joint(rng, [0, 2], poses), None, FIXED
    if name == "c_sixteen_poses":
        W = 16
        poses, Z, has_Z = base.scene(world, W, seed)
        pairs = [(0, s) for s in range(1, W)] + [(W - 1 - s, W - 1) for s in range(1, W)] + [(3, 9), (3, 9)]
        edges = [edge_ref.random_edge(rng, a, b, poses) for a, b in pairs]
        linear = [lin_ref.random_linear(rng, int(p), poses[int(p)]) for p in rng.integers(0, W, 32)]
        return small, W, [True] * W, poses, Z, has_Z, linear, edges, ref.random_joint(rng, [0, 5, 10, 15], poses), None, FIXED
    W = 5
    poses, Z, has_Z = base.scene(world, W, seed)
    edges = [edge_ref.random_edge(rng, 0, 2, poses), edge_ref.random_edge(rng, 1, 4, poses)]
    joint = ref.random_joint(rng, [0, 1, 3], poses)
    if name == "b_three_members_beside_edges":
        return small, W, [True] * W, poses, Z, has_Z, [lin_ref.random_linear(rng, 2, poses[2])], edges, joint, None, FIXED
    if name == "d_relin":
        return small, W, [True] * W, poses, Z, has_Z, [], edges, joint, RELIN, FIXED
    if name == "e_early_stop":  # the loose prior: the chain converges; twelve iterations are queued at once, the stop (0.1 mrad / 0.1 mm) comes earlier
        return small, W, [True] * W, poses, Z, has_Z, [], edges, joint, None, dict(iters=12, eps_rot=1e-4, eps_trans=1e-4)
    mk = lambda i: small_base(world, empty=(i == 3)).clone()  # noqa: E731
    return mk, W, [i != 3 for i in range(W)], poses, Z, has_Z, [], edges, joint, None, FIXED


@pytest.mark.parametrize("name", ["a_two_members", "b_three_members_beside_edges", "c_sixteen_poses", "d_relin", "e_early_stop", "f_empty_member"])
def test_joint_against_the_host_loop(world, name):
    capi = world.capi
    mk, W, have, poses, Z, has_Z, linear, edges, joint, relin, kw = consumer_case(world, name)
    a, b, c = ([mk(i) for i in range(W)] for _ in range(3))
    cfg = base.window_cfg(False, **kw)
    got = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, edges=edges, joint=joint)
    bare = capi.optimise_window(c, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, edges=edges)
    want = host_loop(b, have, poses, Z, has_Z, cfg, linear, edges, joint, relin)
    n = min(got["iters"], bare["iters"])
    moved = float(np.abs(got["poses"][n - 1] - bare["poses"][n - 1]).max())
    print(name, "final poses moved by the joint factor: %.3e" % moved)
    base.compare(got, want, name)
    assert moved > 1e-6
    worst_f = max(abs(got["trace"][it]["f"] - want["trace"][it]["f"]) / max(1.0, abs(want["trace"][it]["f"])) for it in range(got["iters"]))
    print(name, "worst relative cost difference over the iterations: %.3e" % worst_f)
    assert worst_f <= 1e-6  # (the sums follow poses 1e-9 apart; the bar of tests/test_gpu_icp_window_lin.py)
    assert all(r["flags"] == 0 for r in got["trace"])
    if relin is not None:
        print(name, "masks", [bin(m) for m in want["masks"]], "margin %.3e" % want["margin"])
        assert want["margin"] > 1e-7  # no decision so close to its threshold that poses 1e-9 apart could take it differently
        assert [int(m) for m in got["evaluated"]] == want["masks"]
        assert any(m != want["masks"][0] for m in want["masks"])  # some factor was kept
    if name == "e_early_stop":
        assert got["converged"] == 1 and 1 < got["iters"] < cfg.iters
    for i in range(W):
        assert np.array_equal(a[i].state()[0], b[i].state()[0]), (name, i)
    for f in a + b + c:
        f.destroy()


@pytest.mark.parametrize("name", ["b_three_members_beside_edges", "d_relin", "e_early_stop"])
def test_check_every_and_async_do_not_change_the_result(world, name):
    capi = world.capi
    mk, W, have, poses, Z, has_Z, linear, edges, joint, relin, kw = consumer_case(world, name)
    runs = []
    for ce, wait in ((0, True), (1, True), (0, False)):
        fs = [mk(i) for i in range(W)]
        got = capi.optimise_window(fs, poses, base.window_cfg(False, check_every=ce, **kw), has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear,
                                   edges=edges, joint=joint, wait=wait)
        runs.append(got if wait else got.wait())
        for f in fs:
            f.destroy()
    for r in runs[1:]:
        relin_base.same_bits(r, runs[0])


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def icp_of(r, have=True):
    return (np.array(r["H_ss"], float).reshape(6, 6), np.array(r["b_s"], float), float(r["f"])) if have else None


def producer_case(world, name):
    """(W, has_Z[1], empty oldest, edge pairs, joint members or None, the separator expected)"""
    return {"s1": (3, True, False, [(0, 1), (1, 2)], None, [1]),
            "s12": (4, True, False, [(0, 2)], None, [1, 2]),
            "s13_three_on_one_pair_no_tie": (5, False, False, [(0, 3), (0, 3), (2, 4), (0, 3)], None, [1, 3]),
            "s1234": (6, True, False, [(0, 4), (0, 2), (0, 3), (0, 1), (3, 5)], None, [1, 2, 3, 4]),
            "joint_overlaps_and_extends": (5, True, False, [(0, 2), (0, 2)], [0, 2, 3], [1, 2, 3]),
            "joint_and_far_edge": (5, True, False, [(0, 4)], [0, 1, 2, 3], [1, 2, 3, 4]),
            "joint_sixteen_poses_no_tie": (16, False, False, [], [0, 5, 10, 15], [1, 5, 10, 15]),
            "no_tie_at_all": (3, False, False, [(1, 2)], None, [1]),
            "empty_oldest_with_prior": (4, True, True, [(0, 2)], [0, 3], [1, 2, 3])}[name]


PRODUCER = ["s1", "s12", "s13_three_on_one_pair_no_tie", "s1234", "joint_overlaps_and_extends", "joint_and_far_edge", "joint_sixteen_poses_no_tie", "no_tie_at_all",
            "empty_oldest_with_prior"]


@pytest.mark.parametrize("name", PRODUCER)
def test_marginal_against_the_numpy_restatement(world, name):
    capi = world.capi
    W, tie, empty0, pairs, members, sep = producer_case(world, name)
    seed = 160 + PRODUCER.index(name)
    rng = np.random.default_rng(seed)
    poses, Z, has_Z = base.scene(world, W, seed)
    has_Z = [0, int(tie)] + list(has_Z[2:])
    edges = [edge_ref.random_edge(rng, a, b, poses, info=edge_ref.random_info(rng, 1e2, 1e5)) for a, b in pairs]
    linear = [lin_ref.random_linear(rng, 0, poses[0]), lin_ref.random_linear(rng, 1, poses[1])]
    joint = None if members is None else ref.random_joint(rng, members, poses)
    fs = [small_base(world, empty=(empty0 and i == 0)).clone() for i in range(W)]
    cfg = base.window_cfg(False, iters=1, eps_rot=0.0, eps_trans=0.0)
    m = capi.marginalise_window_joint(fs, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges, joint=joint)
    want = ref.marginal(poses, icp_of(m["oldest"], not empty0), bool(tie), Z[1], np.array(cfg.between_info), np.array(cfg.prior_info), cfg.damping, linear, edges,
                        joint)
    cond = np.linalg.cond(want["A00"])
    here = m["joint_here"]
    dev = ref.deviation(dict(H=here["H"], b=here["b"], f=here["f"]), want)
    print(f"{name}: cond(A00) {cond:.3e}  H {dev[0]:.3e}  b {dev[1]:.3e}  f {dev[2]:.3e}")
    assert cond <= 1e6, (name, cond)
    assert here["poses"] == sep == want["sep"] and m["joint"]["poses"] == [i - 1 for i in sep]
    assert m["valid"] == 1 and want["valid"] == 1 and m["n_ties"] == want["n_ties"] == int(tie) + sum(1 for a, _ in pairs if a == 0)
    assert np.array_equal(here["H"], here["H"].T)
    for k, i in enumerate(sep):
        assert np.array_equal(here["at"][k][0], poses[i][0]) and np.array_equal(here["at"][k][1], poses[i][1])
    if name == "no_tie_at_all":
        assert not np.any(here["H"]) and not np.any(here["b"])
    assert max(dev) <= 1e-9, (name, dev)
    assert empty0 or m["oldest"]["linearize_count"] == 1
    for f in fs:
        f.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_elimination_identity_through_the_public_calls(world):
    capi = world.capi
    W = 5
    poses, Z, has_Z = base.scene(world, W, 171)
    rng = np.random.default_rng(171)
    edges = [edge_ref.random_edge(rng, 0, 2, poses), edge_ref.random_edge(rng, 0, 3, poses), edge_ref.random_edge(rng, 1, 4, poses)]
    a, b, c, d = ([small_base(world).clone() for _ in range(W)] for _ in range(4))
    cfg = base.window_cfg(False, iters=1, eps_rot=0.0, eps_trans=0.0)
    cfg0 = base.window_cfg(False, iters=1, eps_rot=0.0, eps_trans=0.0, prior_info=ZERO)
    full = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, linear=[], edges=edges)
    m = capi.marginalise_window_joint(b, poses, cfg, has_Z=has_Z, Z=Z, linear=[], edges=edges)
    assert m["valid"] == 1 and m["n_ties"] == 3 and m["joint"]["poses"] == [0, 1, 2]
    rest = dict(has_Z=[0] + list(has_Z[2:]), Z=Z[1:], edges=[dict(edges[2], a=0, b=3)])
    with_m = capi.optimise_window(c[1:], poses[1:], cfg0, joint=m["joint"], **rest)
    without = capi.optimise_window(d[1:], poses[1:], cfg0, **rest)
    assert full["iters"] == with_m["iters"] == without["iters"] == 1
    worst_r = max(base.rot_angle(with_m["R"][i], full["R"][i + 1]) for i in range(W - 1))
    worst_t = max(float(np.linalg.norm(with_m["t"][i] - full["t"][i + 1])) for i in range(W - 1))
    apart = max(float(np.linalg.norm(without["t"][i] - full["t"][i + 1])) for i in range(W - 1))
    print(f"reduced window with the joint marginal against the full window: {worst_r:.3e} rad, {worst_t:.3e} m; without the marginal {apart:.3e} m")
    assert apart > 1e-4, apart
    assert worst_r <= 1e-9 and worst_t <= 1e-9, (worst_r, worst_t)
    for f in a + b + c + d:
        f.destroy()


@pytest.mark.parametrize("span, want", [(2, [[1, 2]] * 4), (3, [[1, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3]]), (4, [[1, 4], [1, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]])])
def test_sliding_separators_settle_at_the_edge_span(world, span, want):
    """an odometry edge (k - span, k) ending on EVERY pose, a window of 5 sliding four times with the marginal carried: the
    separator settles at `span` poses — {1,2} for span 2, {1,3} -> {1,2,3} -> {1,2,3} for span 3 — and a bound of four poses
    covers span 4; every marginal agrees with the restatement fed with the same carried factor"""
    capi = world.capi
    W, n_slides = 5, 4
    n_scans = W + n_slides
    rng = np.random.default_rng(180 + span)
    track = [base.perturbed(world.truth(), 18000 + 100 * span + k) for k in range(n_scans)]
    Z = [(np.eye(3), np.zeros(3))] * W
    has_Z = [0] + [1] * (W - 1)
    all_edges = {(k - span, k): edge_ref.random_edge(rng, k - span, k, track) for k in range(span, n_scans)}
    cfg = base.window_cfg(False, iters=1, eps_rot=0.0, eps_trans=0.0)
    cfg0 = base.window_cfg(False, iters=1, eps_rot=0.0, eps_trans=0.0, prior_info=ZERO)
    carried, seps = None, []
    for s in range(n_slides):
        poses = track[s:s + W]
        edges = [dict(e, a=a - s, b=b - s) for (a, b), e in all_edges.items() if a >= s and b < s + W]
        fs = [small_base(world).clone() for _ in range(W)]
        c = cfg if carried is None else cfg0
        m = capi.marginalise_window_joint(fs, poses, c, has_Z=has_Z, Z=Z, edges=edges, joint=carried)
        want_m = ref.marginal(poses, icp_of(m["oldest"]), True, Z[1], np.array(c.between_info), np.array(c.prior_info), c.damping, [], edges, carried)
        here = m["joint_here"]
        dev = ref.deviation(dict(H=here["H"], b=here["b"], f=here["f"]), want_m)
        assert m["valid"] == 1 and np.linalg.cond(want_m["A00"]) <= 1e6 and max(dev) <= 1e-9, (s, dev)
        seps.append(here["poses"])
        carried = m["joint"]
        for f in fs:
            f.destroy()
    print(f"span {span}: separators {seps}")
    assert seps == want


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def same_marginal(a, b):
    assert a["valid"] == b["valid"] and a["n_ties"] == b["n_ties"]
    relin_base.same_bits(a["joint_here"], b["joint_here"])
    relin_base.same_bits(a["joint"], b["joint"])
    same_icp(a["oldest"], b["oldest"])


def test_async_marginal_gives_the_same_bits_and_holds_the_context(world):
    capi = world.capi
    W, tie, _, pairs, members, _ = producer_case(world, "joint_overlaps_and_extends")
    poses, Z, has_Z = base.scene(world, W, 172)
    rng = np.random.default_rng(172)
    edges = [edge_ref.random_edge(rng, a, b, poses) for a, b in pairs]
    joint = ref.random_joint(rng, members, poses)
    cfg = base.window_cfg(False, iters=1, eps_rot=0.0, eps_trans=0.0)
    fs, gs = ([small_base(world).clone() for _ in range(W)] for _ in range(2))
    want = capi.marginalise_window_joint(fs, poses, cfg, has_Z=has_Z, Z=Z, edges=edges, joint=joint)
    call = capi.marginalise_window_joint(gs, poses, cfg, has_Z=has_Z, Z=Z, edges=edges, joint=joint, wait=False)
    for attempt in (lambda: capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, joint=joint), lambda: capi.marginalise_window_joint(fs, poses, cfg, has_Z=has_Z, Z=Z),
                    lambda: gs[1].linearize(*poses[1], G)):
        with pytest.raises(capi.MhError) as e:
            attempt()
        assert e.value.code == capi.MH_ERR_INVALID_ARG and ("in flight" in str(e.value) or "window call" in str(e.value)), str(e.value)
    same_marginal(call.wait(), want)
    with pytest.raises(capi.MhError):
        world.ctx.check(world.ctx.L.mh_icp_window_wait(world.ctx.h))  # collected: nothing is in flight
    # refusals leave the handles alone: a valid call afterwards counts from where the first left the factors
    with pytest.raises(capi.MhError) as e:
        capi.marginalise_window_joint(fs, poses, cfg, has_Z=has_Z, Z=Z, edges=edges, joint=dict(joint, poses=[1, 2, 3]))
    assert e.value.code == capi.MH_ERR_UNSUPPORTED and "without pose 0" in str(e.value)
    again = capi.marginalise_window_joint(fs, poses, cfg, has_Z=has_Z, Z=Z, edges=edges, joint=joint)
    assert again["oldest"]["linearize_count"] == 2
    for f in fs + gs:
        f.destroy()


def test_cpp_mirror_gives_the_c_abi_calls_bits(world, tmp_path):
    from test_gpu_host_cpp import build_exe
    capi, synth = world.capi, world.synth
    m, scan, aux = synth.small_world()
    pts = np.ascontiguousarray(scan[::4])
    W = 5
    poses, Z, has_Z = base.scene(world, W, 173)
    rng = np.random.default_rng(173)
    linear = [lin_ref.random_linear(rng, i, poses[i]) for i in (0, 1, 0)]
    edges = [edge_ref.random_edge(rng, a, b, poses) for a, b in ((0, 2), (1, 4), (0, 1))]
    joint = ref.random_joint(rng, [0, 2, 3], poses)
    reg = capi.make_reg_config(**dict(synth.enwide_config(), num_corres_points=5, reg_4_dof=0, project_on_degneneracy=0))
    cfg = capi.make_window_config(iters=3, prior_sigma_rot=0.017453292519943295, prior_sigma_trans=0.1)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            f.write(struct.pack("<Q", arr.size if arr.dtype.itemsize != 32 else len(arr)))
            f.write(arr.tobytes())
        w(m.astype(np.float32).ravel())
        w(pts)
        w(np.frombuffer(bytes(reg), np.uint8))
        w(np.concatenate([np.concatenate([R.ravel(), t]) for R, t in poses]))
        w(np.concatenate([np.concatenate([[float(h)], R.ravel(), t]) for h, (R, t) in zip(has_Z, Z)]))
        w(np.array([cfg.iters] + list(cfg.between_info) + list(cfg.prior_info) + [cfg.damping, cfg.eps_rot, cfg.eps_trans, cfg.check_every], float))
        w(np.concatenate([np.concatenate([[float(l["pose"])], l["at"][0].ravel(), l["at"][1], l["H"].ravel(), l["b"], [l["f"]]]) for l in linear]))
        w(np.concatenate([np.concatenate([[float(e["a"]), float(e["b"])], e["Z"][0].ravel(), e["Z"][1], e["info"].ravel()]) for e in edges]))
        w(np.concatenate([[float(len(joint["poses"]))]] + [np.concatenate([[float(i)], L[0].ravel(), L[1]]) for i, L in zip(joint["poses"], joint["at"])]
                         + [joint["H"].ravel(), joint["b"], [joint["f"]]]))
    out = subprocess.run([build_exe("window_joint_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    blocking, asynchronous = got["runs"]
    assert blocking == asynchronous and got["slid"][0] == got["slid"][1]

    fs = [capi.ICPFactor(world.ctx, world.small_map, pts, reg) for _ in range(W)]
    for f in fs:
        f.set_components(False)
    want = capi.marginalise_window_joint(fs, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges, joint=joint)
    here = want["joint_here"]
    assert blocking["valid"] == want["valid"] == 1 and blocking["n_ties"] == want["n_ties"] == 3
    assert blocking["poses"] == here["poses"] == [1, 2, 3] and blocking["rebased"] == want["joint"]["poses"]
    assert np.array_equal(np.array(blocking["H"]).reshape(18, 18), here["H"]) and np.array_equal(np.array(blocking["b"]), here["b"])
    assert blocking["f"] == here["f"] and blocking["oldest_f"] == want["oldest"]["f"]
    assert np.array_equal(np.array(blocking["at"]), np.concatenate([np.concatenate([R.ravel(), t]) for R, t in here["at"]]))
    assert blocking["counts"][0] == want["oldest"]["linearize_count"] == 1
    cfg0 = capi.make_window_config(iters=3, prior_info=ZERO)
    slid = capi.optimise_window(fs[1:], poses[1:], cfg0, has_Z=[0] + list(has_Z[2:]), Z=Z[1:], edges=[dict(edges[1], a=0, b=3)], joint=want["joint"])
    assert got["slid"][0]["iters"] == slid["iters"] == 3
    for i, p in enumerate(got["slid"][0]["poses"]):
        assert np.array_equal(np.array(p["R"]).reshape(3, 3), slid["R"][i]) and np.array_equal(np.array(p["t"]), slid["t"][i])
    for f in fs:
        f.destroy()
