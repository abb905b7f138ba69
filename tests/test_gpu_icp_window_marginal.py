"""-m gpu: mh_icp_window_marginalise — the marginal prior the oldest pose of a fixed-lag window leaves on the pose behind it,
computed on the device: one K3 launch of the oldest factor, one one-wave kernel, one wait.

Scene: that of tests/test_gpu_icp_window.py (synth.small_world(): a map of ~5 k points, a 1 024-point scan cloned W times); the
case of 32 linear factors and 32 edges takes every fourth point of the scan (256-point factors).

1.  `oldest` is mh_icp_linearize (components off) of a fresh clone of factor 0 at T_0, bit for bit; factor 0's count is + 1 and
    its state that clone's; every other factor's count and state are untouched.
2.  `prior` against the numpy restatement (tests/window_marginal_ref.py) fed with that `oldest`: 1e-9 relative to the uncancelled
    scales ||A11'||_F, ||g1'||, c — the bar and the metric of tests/test_icp_window_marginal_cpu.py; cond(A00) <= 1e6 asserted.
3.  The elimination identity through the public calls: one iteration of mh_icp_window_optimise_edges on the full window and one
    on the window without its oldest pose, with the marginal as a linear factor and no prior, move poses 1 .. W - 1 alike to
    1e-9 m / 1e-9 rad; without the marginal they differ by more than 1e-6 m.
4.  Two slides: the second marginalise call carries the first marginal as a linear factor on pose 0, away from its L.
5.  Async + mh_icp_window_wait: the same bits.  Refusals leave counts and state alone; a window call is refused while a
    marginalise call has not been waited for."""
import numpy as np
import pytest

import test_gpu_icp_window as base
import window_edge_ref as edge_ref
import window_lin_ref as lin_ref
import window_marginal_ref as ref
from test_gpu_icp_window import world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G = base.G
ZERO = [0.0] * 6


def cfg_of(prior=True, iters=1):
    kw = dict(iters=iters, eps_rot=0.0, eps_trans=0.0)
    if not prior:
        kw["prior_info"] = ZERO
    return base.window_cfg(False, **kw)


def icp_of(r, have=True):
    return (np.array(r["H_ss"], float).reshape(6, 6), np.array(r["b_s"], float), float(r["f"])) if have else None


def restated(m, have0, poses, Z, has_Z, cfg, linear, edges):
    return ref.marginal(poses, icp_of(m["oldest"], have0), bool(has_Z[1]), Z[1], np.array(cfg.between_info), np.array(cfg.prior_info), cfg.damping,
                        linear, edges)


def check_against_restatement(m, want, tag):
    cond = np.linalg.cond(want["A00"])
    got = dict(H=m["linear"]["H"], b=m["linear"]["b"], f=m["linear"]["f"])
    dev = ref.deviation(got, want)
    print(f"{tag}: cond(A00) {cond:.3e}  H {dev[0]:.3e}  b {dev[1]:.3e}  f {dev[2]:.3e}  (||A11'|| {np.linalg.norm(want['A11']):.3e}, c {want['c']:.3e})")
    assert cond <= 1e6, (tag, cond)
    assert m["valid"] == 1 and want["valid"] == 1 and m["n_ties"] == want["n_ties"], tag
    assert np.array_equal(m["linear"]["H"], m["linear"]["H"].T), tag
    assert max(dev) <= 1e-9, (tag, dev)


def same_result(a, b):
    assert a["valid"] == b["valid"] and a["n_ties"] == b["n_ties"]
    for k in ("H", "b", "f"):
        assert np.array_equal(np.asarray(a["linear"][k]), np.asarray(b["linear"][k]))
    for k in (0, 1):
        assert np.array_equal(a["linear"]["at"][k], b["linear"]["at"][k])
    same_icp(a["oldest"], b["oldest"])


def same_icp(a, b):
    for k in a:
        if not k.startswith("gpu_ms"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_oldest_is_one_linearize_of_factor_0_and_nothing_else_moves(world):
    capi = world.capi
    W = 3
    fs = [world.base(5).clone() for _ in range(W)]
    poses, Z, has_Z = base.scene(world, W, 81)
    fs[2].set_components(False)
    fs[2].linearize(*poses[2], G)  # a factor with a history: count 1, warm state
    before = [f.state() for f in fs]
    m = capi.marginalise_window(fs, poses, cfg_of(), has_Z=has_Z, Z=Z)
    fresh = world.base(5).clone()
    fresh.set_components(False)
    want = fresh.linearize(*poses[0], G)
    same_icp(m["oldest"], want)
    assert m["oldest"]["linearize_count"] == 1
    assert m["linear"]["pose"] == 0 and np.array_equal(m["linear"]["at"][0], poses[1][0]) and np.array_equal(m["linear"]["at"][1], poses[1][1])
    for u, v in zip(fs[0].state(), fresh.state()):
        assert np.array_equal(u, v, equal_nan=True)
    for i in (1, 2):
        for u, v in zip(fs[i].state(), before[i]):
            assert np.array_equal(u, v, equal_nan=True)
    for f in fs:
        f.set_components(False)
    counts = [f.linearize(*p, G)["linearize_count"] for f, p in zip(fs, poses)]
    assert counts == [2, 1, 2], counts
    for f in fs + [fresh]:
        f.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def marginal_case(world, name):
    """(factors, have0, poses, Z, has_Z, linear, edges)"""
    capi = world.capi
    rng = np.random.default_rng({"tie_only": 1, "mixed": 2, "empty_oldest": 3, "full_lists": 4}[name])
    if name == "tie_only":
        W = 2
        poses, Z, has_Z = base.scene(world, W, 82)
        return [world.base(5).clone() for _ in range(W)], True, poses, Z, has_Z, [], []
    if name == "mixed":  # two linear factors on pose 0, two edges on (0, 1), ignored terms on pose 1 and (1, 2), reg_4_dof on pose 0
        W = 3
        poses, Z, has_Z = base.scene(world, W, 83)
        linear = [lin_ref.random_linear(rng, 1, poses[1]), lin_ref.random_linear(rng, 0, poses[0]), lin_ref.random_linear(rng, 0, poses[0])]
        edges = [edge_ref.random_edge(rng, 0, 1, poses), edge_ref.random_edge(rng, 1, 2, poses), edge_ref.random_edge(rng, 0, 1, poses)]
        return [world.base(5, reg4=1).clone()] + [world.base(5).clone() for _ in range(W - 1)], True, poses, Z, has_Z, linear, edges
    if name == "empty_oldest":
        W = 3
        poses, Z, has_Z = base.scene(world, W, 84)
        return [world.base(5, empty=True).clone()] + [world.base(5).clone() for _ in range(W - 1)], False, poses, Z, has_Z, [], [edge_ref.random_edge(rng, 0, 1, poses)]
    W = 2
    cfg = dict(world.synth.enwide_config(), num_corres_points=5, reg_4_dof=0, project_on_degneneracy=0)
    small = capi.ICPFactor(world.ctx, world.small_map, np.ascontiguousarray(world.small_scan[::4]), capi.make_reg_config(**cfg))
    assert small.n == 256
    poses, Z, has_Z = base.scene(world, W, 85)
    linear = [lin_ref.random_linear(rng, 0, poses[0]) for _ in range(32)]
    edges = [edge_ref.random_edge(rng, 0, 1, poses, info=edge_ref.random_info(rng, 1e2, 1e5)) for _ in range(32)]
    fs = [small.clone() for _ in range(W)]
    small.destroy()
    return fs, True, poses, Z, has_Z, linear, edges


@pytest.mark.parametrize("name", ["tie_only", "mixed", "empty_oldest", "full_lists"])
def test_prior_against_the_numpy_restatement(world, name):
    fs, have0, poses, Z, has_Z, linear, edges = marginal_case(world, name)
    cfg = cfg_of()
    m = world.capi.marginalise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges)
    want = restated(m, have0, poses, Z, has_Z, cfg, linear, edges)
    check_against_restatement(m, want, name)
    assert m["n_ties"] == 1 + sum(1 for e in edges if (e["a"], e["b"]) == (0, 1))
    if not have0:
        assert not np.any(m["oldest"]["H_ss"]) and m["oldest"]["f"] == 0.0
    for f in fs:
        f.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_elimination_identity_through_the_public_calls(world):
    capi = world.capi
    W = 3
    poses, Z, has_Z = base.scene(world, W, 86)
    rng = np.random.default_rng(86)
    edges = [edge_ref.random_edge(rng, 0, 1, poses), edge_ref.random_edge(rng, 1, 2, poses)]
    a, b, c, d = ([world.base(5).clone() for _ in range(W)] for _ in range(4))
    cfg = cfg_of()
    full = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, linear=[], edges=edges)
    m = capi.marginalise_window(b, poses, cfg, has_Z=has_Z, Z=Z, linear=[], edges=edges)
    assert m["valid"] == 1 and m["n_ties"] == 2
    rest = dict(has_Z=[0] + list(has_Z[2:]), Z=Z[1:], edges=[dict(edges[1], a=0, b=1)])
    with_m = capi.optimise_window(c[1:], poses[1:], cfg_of(prior=False), linear=[m["linear"]], **rest)
    without = capi.optimise_window(d[1:], poses[1:], cfg_of(prior=False), linear=[], **rest)
    assert full["iters"] == with_m["iters"] == without["iters"] == 1
    worst_r = max(base.rot_angle(with_m["R"][i], full["R"][i + 1]) for i in range(W - 1))
    worst_t = max(float(np.linalg.norm(with_m["t"][i] - full["t"][i + 1])) for i in range(W - 1))
    apart = max(float(np.linalg.norm(without["t"][i] - full["t"][i + 1])) for i in range(W - 1))
    print(f"reduced window with the marginal against the full window: {worst_r:.3e} rad, {worst_t:.3e} m; without the marginal {apart:.3e} m")
    assert apart > 1e-6, apart
    assert worst_r <= 1e-9 and worst_t <= 1e-9, (worst_r, worst_t)
    for f in a + b + c + d:
        f.destroy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_two_slides_carry_the_prior(world):
    capi = world.capi
    W = 3
    fs = [world.base(5).clone() for _ in range(W)]
    poses, Z, has_Z = base.scene(world, W, 87)
    cfg = cfg_of()
    m1 = capi.marginalise_window(fs, poses, cfg, has_Z=has_Z, Z=Z)
    check_against_restatement(m1, restated(m1, True, poses, Z, has_Z, cfg, [], []), "slide 1")
    # drop the oldest pose, optimise what is left with the carried prior
    live, Zl, hzl = fs[1:], Z[1:], [0] + list(has_Z[2:])
    opt = capi.optimise_window(live, poses[1:], cfg_of(prior=False, iters=3), has_Z=hzl, Z=Zl, linear=[m1["linear"]])
    assert opt["iters"] == 3 and all(r["flags"] == 0 for r in opt["trace"])
    now = [(opt["R"][i], opt["t"][i]) for i in range(W - 1)]
    moved = lin_ref.pose_error(now[0], m1["linear"]["at"])
    assert moved[1] > 1e-6, moved  # the carried prior is now transported: d != 0
    cfg2 = cfg_of(prior=False)
    m2 = capi.marginalise_window(live, now, cfg2, has_Z=hzl, Z=Zl, linear=[m1["linear"]])
    check_against_restatement(m2, restated(m2, True, now, Zl, hzl, cfg2, [m1["linear"]], []), "slide 2")
    assert m2["oldest"]["linearize_count"] == 4
    for f in fs:
        f.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_async_gives_the_same_bits(world):
    capi = world.capi
    fs, _, poses, Z, has_Z, linear, edges = marginal_case(world, "mixed")
    gs, *_ = marginal_case(world, "mixed")
    cfg = cfg_of()
    want = capi.marginalise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges)
    call = capi.marginalise_window(gs, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges, wait=False)
    # one window call per context at a time, and the marginalise call is one
    for attempt in (lambda: capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z), lambda: capi.marginalise_window(fs, poses, cfg, has_Z=has_Z, Z=Z),
                    lambda: gs[1].linearize(*poses[1], G)):
        with pytest.raises(capi.MhError) as e:
            attempt()
        assert e.value.code == capi.MH_ERR_INVALID_ARG and ("in flight" in str(e.value) or "window call" in str(e.value)), str(e.value)
    same_result(call.wait(), want)
    with pytest.raises(capi.MhError):
        world.ctx.check(world.ctx.L.mh_icp_window_wait(world.ctx.h))  # collected: nothing is in flight
    for f in fs + gs:
        f.destroy()


def test_refusals_leave_counts_and_state_alone(world):
    capi = world.capi
    W = 3
    fs = [world.base(5).clone() for _ in range(W)]
    poses, Z, has_Z = base.scene(world, W, 88)
    rng = np.random.default_rng(88)
    cfg = cfg_of()
    for f in fs:
        f.set_components(False)
        f.linearize(*poses[0], G)
    before = [f.state() for f in fs]

    def refused(code, word, factors=fs, p=poses, **kw):
        for wait in (True, False):
            with pytest.raises(capi.MhError) as e:
                capi.marginalise_window(factors, p, cfg, has_Z=has_Z[:len(factors)], Z=Z[:len(factors)], wait=wait, **kw)
            assert e.value.code == code and word in str(e.value), str(e.value)

    refused(capi.MH_ERR_INVALID_ARG, "behind the oldest", factors=fs[:1], p=poses[:1])
    refused(capi.MH_ERR_UNSUPPORTED, "beyond pose 1", edges=[edge_ref.random_edge(rng, 0, 1, poses), edge_ref.random_edge(rng, 0, 2, poses)])
    bad = lin_ref.random_linear(rng, 0, poses[0])
    bad["H"][2, 3] = np.nan
    refused(capi.MH_ERR_INVALID_ARG, "finite", linear=[bad])
    bad = edge_ref.random_edge(rng, 0, 1, poses)
    bad["Z"][1][1] = np.inf
    refused(capi.MH_ERR_INVALID_ARG, "finite", edges=[bad])
    fs[1].linearize_async(*poses[1], G)
    refused(capi.MH_ERR_INVALID_ARG, "in flight")
    fs[1].wait()
    with pytest.raises(capi.MhError):
        world.ctx.check(world.ctx.L.mh_icp_window_wait(world.ctx.h))  # nothing was enqueued
    for i in (0, 2):
        for u, v in zip(fs[i].state(), before[i]):
            assert np.array_equal(u, v, equal_nan=True)
    # a valid call on the same factors: the counts are where the linearize calls above left them
    m = capi.marginalise_window(fs, poses, cfg, has_Z=has_Z, Z=Z)
    assert m["valid"] == 1 and m["oldest"]["linearize_count"] == 2
    assert [f.linearize(*p, G)["linearize_count"] for f, p in zip(fs, poses)] == [3, 3, 2]
    for f in fs:
        f.destroy()
