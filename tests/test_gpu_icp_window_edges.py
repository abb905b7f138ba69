"""-m gpu: mh_icp_window_optimise_edges — the fixed-lag chain with between factors on any pair of poses, each with a dense
information matrix, solved over the row profile of the system.

Scene: that of tests/test_gpu_icp_window.py (synth.small_world(): a map of ~5 k points, a 1 024-point scan cloned W times);
the W = 16 case takes every fourth point of the scan (256-point factors) and 32 edges.

1.  n_edges = 0: poses, trace, first / last (and masks), factor state bit-identical to optimise_window(..., linear=...).
2.  Against the host-driven loop written here: mh_icp_linearize_batch (per-factor mh_icp_linearize where thresholds select the
    factors), the edge terms, assembly and retraction of tests/window_edge_ref.py (numpy, dense, written independently of the
    header) with the refined solve of tests/test_gpu_icp_window.py.  Every pose of every iteration within 1e-9 m / 1e-9 rad.
    Cases for W = 3: (a) one edge (0, 2) beside the has_Z ties, (b) two edges on one pair and one parallel to a has_Z tie,
    with linear factors, (c) an edge as the only tie across a has_Z gap, (d) an edge ending on the pose of an empty ICP factor,
    (e) case (b) under the reference's thresholds (1.75e-2 rad, 5e-3 m) with equal masks and the smallest decision margin
    above 1e-7; and W = 16 with 32 edges of every span.  In each the final poses differ from the same call without edges by
    more than 1e-6.  The edges: dense random SPD information matrices with eigenvalues between 1e2 and 1e6, measurements a
    degree / centimetres off the start poses' own relative pose.
3.  Sync, async + mh_icp_window_wait and check_every = 1: the same bits.
4.  Every refusal of the contract: MH_ERR_INVALID_ARG, and a valid call on the same factors afterwards."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_icp_window as base
import test_gpu_icp_window_lin as lin_base
import test_gpu_icp_window_relin as relin_base
import window_edge_ref as ref
import window_lin_ref as lin_ref
from test_gpu_icp_window import world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G = base.G
RELIN = relin_base.RELIN
FIXED = lin_base.FIXED


def host_loop(factors, have, poses, Z, has_Z, cfg, linear, edges, relin=None):
    """the loop a caller writes around the library's linearize calls; with `relin` the rule of mh_icp_window_optimise_relin"""
    from mimosa_amd import capi
    for f in factors:
        f.set_components(False)
    poses = [(np.array(R, float), np.array(t, float)) for R, t in poses]
    W = len(poses)
    Wb, prior = np.array(cfg.between_info), np.array(cfg.prior_info)
    kept = [None] * W
    trace, masks, margin = [], [], np.inf
    thr = None if relin is None else np.array([relin[0]] * 3 + [relin[1]] * 3)
    for it in range(cfg.iters):
        if relin is None:
            res = capi.linearize_batch(factors, [p[0] for p in poses], [p[1] for p in poses])
            icp = [(np.array(r["H_ss"], float).reshape(6, 6), np.array(r["b_s"], float), float(r["f"])) if have[i] else None for i, r in enumerate(res)]
            mask = sum(1 << i for i in range(W) if have[i])
        else:
            icp, mask = [], 0
            for i in range(W):
                if not have[i]:
                    icp.append(None)
                    continue
                d = None if it == 0 else relin_base.local(kept[i][0], poses[i])
                if it:
                    margin = min(margin, float(np.abs(np.abs(d) - thr).min()))
                if it == 0 or bool(np.any(np.abs(d) > thr)):
                    r = factors[i].linearize(*poses[i], G)
                    kept[i] = (poses[i], np.array(r["H_ss"], float).reshape(6, 6), np.array(r["b_s"], float), float(r["f"]))
                    icp.append(kept[i][1:])
                    mask |= 1 << i
                else:
                    icp.append(lin_ref.transport(kept[i][1], kept[i][2], kept[i][3], kept[i][0], poses[i]))
        poses, xi, cost = ref.iteration(poses, icp, has_Z, Z, Wb, prior, cfg.damping, linear, edges, solve=base.solve_refined)
        trace.append(dict(poses=poses, f=cost))
        masks.append(mask)
    return dict(poses=poses, iters=len(trace), converged=0, trace=trace, masks=masks, margin=margin)


def case_edges(name, poses, seed):
    """(edges, linear factors, has_Z override or None)"""
    rng = np.random.default_rng(seed)
    W = len(poses)
    if name == "a_far_edge":
        return [ref.random_edge(rng, 0, W - 1, poses)], [], None
    if name in ("b_shared_pair_and_parallel", "e_relin"):
        edges = [ref.random_edge(rng, 0, 2, poses), ref.random_edge(rng, 0, 2, poses), ref.random_edge(rng, 1, 2, poses)]
        return edges, [lin_ref.random_linear(rng, i, poses[i]) for i in (0, 2, 2)], None
    if name == "c_across_a_gap":
        return [ref.random_edge(rng, 0, 2, poses)], [], [False, True, False]
    if name == "d_on_an_empty_factor":
        return [ref.random_edge(rng, 0, 1, poses)], [], None
    raise KeyError(name)


# name -> (seed, empty_at, relin)
CASES = {"a_far_edge": (1, None, None), "b_shared_pair_and_parallel": (2, None, None), "c_across_a_gap": (3, None, None), "d_on_an_empty_factor": (4, 1, None),
         "e_relin": (2, None, RELIN)}


def run_against_host_loop(world, mk, W, poses, Z, has_Z, linear, edges, have, relin, tag):
    capi = world.capi
    a, b, c = [mk(i) for i in range(W)], [mk(i) for i in range(W)], [mk(i) for i in range(W)]
    cfg = base.window_cfg(False, **FIXED)
    got = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, edges=edges)
    bare = capi.optimise_window(c, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, edges=[])
    want = host_loop(b, have, poses, Z, has_Z, cfg, linear, edges, relin)
    moved = float(np.abs(got["poses"][-1] - bare["poses"][-1]).max())
    print(tag, "final poses moved by the edges: %.3e" % moved)
    base.compare(got, want, tag)
    assert moved > 1e-6
    worst_f = max(abs(got["trace"][it]["f"] - want["trace"][it]["f"]) / max(1.0, abs(want["trace"][it]["f"])) for it in range(got["iters"]))
    print(tag, "worst relative cost difference over the iterations: %.3e" % worst_f)
    assert worst_f <= 1e-6  # (the sums follow poses 1e-9 apart; the bar of tests/test_gpu_icp_window_lin.py)
    if relin is not None:
        print(tag, "masks", [bin(m) for m in want["masks"]], "margin %.3e" % want["margin"])
        assert want["margin"] > 1e-7  # no decision so close to its threshold that poses 1e-9 apart could take it differently
        assert [int(m) for m in got["evaluated"]] == want["masks"]
    for i in range(W):
        assert np.array_equal(a[i].state()[0], b[i].state()[0]), (tag, i)
    for f in a + b + c:
        f.destroy()
    return got, want


@pytest.mark.parametrize("name", list(CASES))
def test_edges_against_the_host_loop(world, name):
    seed, empty_at, relin = CASES[name]
    W = 3
    mk = lambda i: (world.base(5, empty=True) if i == empty_at else world.base(5)).clone()  # noqa: E731
    poses, Z, has_Z = base.scene(world, W, 60 + seed)
    edges, linear, hz = case_edges(name, poses, seed)
    has_Z = has_Z if hz is None else hz
    run_against_host_loop(world, mk, W, poses, Z, has_Z, linear, edges, [i != empty_at for i in range(W)], relin, name)


def test_sixteen_poses_and_thirty_two_edges(world):
    capi = world.capi
    W = 16
    cfg = dict(world.synth.enwide_config(), num_corres_points=5, reg_4_dof=0, project_on_degneneracy=0)
    small = capi.ICPFactor(world.ctx, world.small_map, np.ascontiguousarray(world.small_scan[::4]), capi.make_reg_config(**cfg))
    assert small.n == 256
    poses, Z, has_Z = base.scene(world, W, 71)
    rng = np.random.default_rng(71)
    pairs = [(0, s) for s in range(1, W)] + [(W - 1 - s, W - 1) for s in range(1, W)] + [(3, 9), (3, 9)]
    assert len(pairs) == 32 and {b - a for a, b in pairs} == set(range(1, W))
    edges = [ref.random_edge(rng, a, b, poses) for a, b in pairs]
    run_against_host_loop(world, lambda i: small.clone(), W, poses, Z, has_Z, [], edges, [True] * W, None, "W=16 n_edges=32")
    small.destroy()


# ---- no edge: the lin chain, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("relin", [None, RELIN])
def test_no_edge_is_the_lin_chain_bit_for_bit(world, relin):
    capi = world.capi
    W, empty_at = 3, 1
    for with_empty in (False, True):
        mk = lambda i: (world.base(5, empty=True) if with_empty and i == empty_at else world.base(5)).clone()  # noqa: E731
        poses, Z, has_Z = base.scene(world, W, 41)
        linear = lin_base.case_linear("b_one_per_pose", poses, 5)
        cfg = base.window_cfg(True, **FIXED)
        a, b = [mk(i) for i in range(W)], [mk(i) for i in range(W)]
        want = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear)
        got = capi.optimise_window(b, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, edges=[])
        relin_base.same_bits(got, want)
        assert got["iters"] == 6 and ("evaluated" in got) == (relin is not None)
        for x, y in zip(a, b):
            for u, v in zip(x.state(), y.state()):
                assert np.array_equal(u, v, equal_nan=True)
        for f in a + b:
            f.destroy()


# ---- how the host drives the chain does not show in the result ------------------------------------------------------------------
@pytest.mark.parametrize("relin", [None, RELIN])
def test_check_every_and_async_do_not_change_the_result(world, relin):
    capi = world.capi
    W = 3
    poses, Z, has_Z = base.scene(world, W, 43)
    edges, linear, _ = case_edges("b_shared_pair_and_parallel", poses, 5)
    runs = []
    for ce, wait in ((0, True), (1, True), (0, False)):
        fs = [world.base(5).clone() for _ in range(W)]
        got = capi.optimise_window(fs, poses, base.window_cfg(True, check_every=ce, **FIXED), has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear,
                                   edges=edges, wait=wait)
        runs.append(got if wait else got.wait())
        for f in fs:
            f.destroy()
    assert runs[0]["iters"] == 6
    for r in runs[1:]:
        relin_base.same_bits(r, runs[0])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handles_usable(world):
    capi = world.capi
    W = 3
    fs = [world.base(5).clone() for _ in range(W)]
    poses, Z, has_Z = base.scene(world, W, 47)
    good, linear, _ = case_edges("b_shared_pair_and_parallel", poses, 7)
    cfg = base.window_cfg(True, iters=3, eps_rot=0.0, eps_trans=0.0)

    def refused(edges, **kw):
        for wait in (True, False):
            with pytest.raises(capi.MhError) as e:
                capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, edges=edges, wait=wait, **kw)
            assert e.value.code == capi.MH_ERR_INVALID_ARG, str(e.value)
        return str(e.value)

    assert "32" in refused([good[0]] * 33)
    for a, b in ((-1, 1), (0, W), (0, 16), (1, 1), (2, 1)):
        assert "pose_a" in refused([good[0], dict(good[1], a=a, b=b)])
    for bad in (np.nan, np.inf, -np.inf):
        info = np.array(good[1]["info"], float).copy()
        info[5, 5] = bad
        assert "finite" in refused([good[0], dict(good[1], info=info)])
        ZR, Zt = good[2]["Z"][0].copy(), good[2]["Z"][1].copy()
        ZR[1, 2] = bad
        assert "finite" in refused([dict(good[2], Z=(ZR, Zt))])
        ZR, Zt = good[2]["Z"][0].copy(), good[2]["Z"][1].copy()
        Zt[0] = bad
        assert "finite" in refused([dict(good[2], Z=(ZR, Zt))])
    info = np.array(good[0]["info"], float).copy()
    info[1, 4] += 1.0
    assert "symmetric" in refused([dict(good[0], info=info)])
    # everything the lin call refuses
    assert "relin" in refused(good, relin=(-1.0, 5e-3))
    assert "pose" in refused(good, linear=[dict(linear[0], pose=W)])
    # edges == NULL with n_edges > 0, through the entry points themselves
    R = np.ascontiguousarray(np.array([p[0].reshape(9) for p in poses]))
    t = np.ascontiguousarray(np.array([p[1] for p in poses]))
    hz = np.ascontiguousarray(np.array(has_Z, np.int32))
    ZR = np.ascontiguousarray(np.array([z[0].reshape(9) for z in Z]))
    Zt = np.ascontiguousarray(np.array([z[1] for z in Z]))
    handles = (C.c_void_p * W)(*[f.h for f in fs])
    out = capi.WindowResult()
    L = world.ctx.L
    for fn in (L.mh_icp_window_optimise_edges, L.mh_icp_window_optimise_edges_async):
        rc = fn(handles, W, capi._p(R), capi._p(t), capi._p(hz), capi._p(ZR), capi._p(Zt), capi._p(G), C.byref(cfg), None, None, 0, None, 2, C.byref(out), None, None)
        assert rc == capi.MH_ERR_INVALID_ARG
    with pytest.raises(capi.MhError):
        world.ctx.check(L.mh_icp_window_wait(world.ctx.h))  # nothing was enqueued
    # the handles are unchanged: a valid call on the same factors, and their counts start from zero
    r = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=good)
    assert r["iters"] == 3 and all(r["first"][i]["linearize_count"] == 1 and r["last"][i]["linearize_count"] == 3 for i in range(W))
    for f in fs:
        f.destroy()
