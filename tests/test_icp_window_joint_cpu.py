"""CPU: the joint-factor phases of mh_icp_window_optimise_joint and mh_icp_window_marginalise_joint (mimosa_amd/csrc/window_device.hpp:
window_joint_transport, the JOINT branches of the assembly and of the profile, window_marginal_joint_impl; compiled by g++ through
tests/cpp/window_joint_step.cpp) against a numpy restatement written independently of the header (tests/window_joint_ref.py:
dense matrices, numpy.linalg.solve); a one-member factor against the same data as the last linear factor, bit for bit; the
marginal without far edges against window_marginal_impl, bit for bit; the elimination identity; every refusal; the ABI additions.

Bars.  Consumer: poses after each of 4 iterations against the restatement, 1e-9 rad / 1e-9 m, and the cost to 1e-9 relative —
the bar and the conditioning rule of tests/test_icp_window_edges_cpu.py.  The joint factors have eigenvalues between 1e2 and 1e6
(scale 1e3 .. 1e4 times a spread of 1e2), inside the range the between weights and the ICP factors already span, so the systems
keep condition numbers of about 1e6 and an unrefined numpy.linalg.solve is good to about 1e-11 per iteration.  Producer: H_m,
b_m, f_m to 1e-9 relative to the uncancelled scales ||A_SS'||_F, ||g_S'||, |c|; every case has cond(A00) <= 1e6 (asserted, none
dropped), so two fp64 routes through A00^-1 agree to about 1e6 x 1e-16 x a small factor.  Elimination identity: 1e-9 m / 1e-9 rad,
and the step without the marginal is more than 1e-4 m away.

Measured: see the print of each test (pytest -s) and DESIGN.md."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_icp_window_cpu as base
import test_icp_window_edges_cpu as edges_base
import test_icp_window_lin_cpu as lin_base
import window_edge_ref as edge_ref
import window_joint_ref as ref
import window_lin_ref as lin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELIN = (1.75e-2, 5e-3)


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("window_joint_step")


@pytest.fixture(scope="module")
def exe_edges():
    from mimosa_amd import build
    return build.build_host_test("window_edge_step")


@pytest.fixture(scope="module")
def exe_marginal():
    from mimosa_amd import build
    return build.build_host_test("window_marginal_step")


def joint_vals(joint):
    if joint is None:
        return [0.0]
    vals = [float(len(joint["poses"]))]
    for i, (R, t) in zip(joint["poses"], joint["at"]):
        vals += [float(i)] + list(np.asarray(R).ravel()) + list(t)
    return vals + list(np.asarray(joint["H"]).ravel()) + list(joint["b"]) + [joint["f"]]


def chain_vals(c, linear, edges, joint, relin=None):
    return [0.0] + joint_vals(joint) + edges_base.chain_vals(c, linear, edges, relin)


def marginal_vals(c, linear, edges, joint):
    import test_icp_window_marginal_cpu as marg_base
    return [1.0] + joint_vals(joint) + marg_base.case_vals(c, linear, edges)


def run(exe, cases):
    return edges_base.run(exe, cases)


def poses_of(c):
    return list(zip(c["R"], c["t"]))


def row_pose(row, i):
    row = np.asarray(row)
    return row[8 + 12 * i:17 + 12 * i].reshape(3, 3), row[17 + 12 * i:20 + 12 * i]


# ---- the consumer ----------------------------------------------------------------------------------------------------------------
def restated(c, linear, edges, joint, n_it, relin=None):
    """tests/test_icp_window_edges_cpu.py's restated chain with the joint factor"""
    W = c["W"]
    poses, Z = poses_of(c), list(zip(c["ZR"], c["Zt"]))
    kept, evaluate, out = [None] * W, [True] * W, []
    for it in range(n_it):
        icp, mask = [], 0
        for i in range(W):
            if not c["have"][i]:
                icp.append(None)
            elif relin is None or evaluate[i]:
                H, b, f, _, _ = base.ref_hessian(c["sums"][it][i], poses[i][0], c["gz"], c["reg4"][i], c["project"][i], c["thresh_rot"][i], c["thresh_trans"][i])
                kept[i] = (H, b, f, poses[i])
                icp.append((H, b, f))
                mask |= 1 << i
            else:
                H, b, f, L = kept[i]
                icp.append(lin_ref.transport(H, b, f, L, poses[i]))
        poses, xi, cost = ref.iteration(poses, icp, c["has_Z"], Z, c["Wb"], c["prior"], c["damping"], linear, edges, joint)
        if relin is not None:
            for i in range(W):
                if c["have"][i]:
                    d = np.abs(lin_ref.local(kept[i][3], poses[i]))
                    evaluate[i] = bool(d[:3].max() > relin[0] or d[3:].max() > relin[1])
        out.append((poses, xi, cost, mask))
    return out


def member_sets(W):
    """n_poses 1 .. 4 (as far as W allows): the ends of the window, neighbours, the widest spread"""
    sets = [[W // 2], [0, W - 1], [W - 2, W - 1], [0, 1, W - 1]]
    if W >= 4:
        sets += [[0, W // 3, (2 * W) // 3, W - 1], [W - 4, W - 3, W - 2, W - 1]]
    return sets


def joint_cases(rng, W):
    """(case, linear, edges, joint, thresholds, what)"""
    out = []

    def case(has_Z):
        return base.window_case(rng, W, has_Z, prior=base.LOOSE, n_it=4, cond=1e2)

    full = [True] * W
    for k, members in enumerate(member_sets(W)):
        gap = list(full)
        if k % 2 and W > 2:
            gap[1 + k % (W - 1)] = False  # a has_Z gap the joint factor may have to bridge
        c = case(gap if members[0] == 0 and members[-1] == W - 1 else full)
        poses = poses_of(c)
        lin32 = [lin_ref.random_linear(rng, int(p), poses[int(p)]) for p in rng.integers(0, W, 32)]
        pairs = [(0, s) for s in range(1, W)] + [(W - 1 - s, W - 1) for s in range(1, W)]
        ed32 = [edge_ref.random_edge(rng, *pairs[j % len(pairs)], poses) for j in range(32)]
        linear, edges = (lin32 if k % 2 == 0 else []), (ed32 if k in (1, 2, 4) else [])
        out.append((c, linear, edges, ref.random_joint(rng, members, poses), RELIN if k in (2, 4) else None,
                    f"W={W} members={members} n_lin={len(linear)} n_edges={len(edges)} relin={k in (2, 4)}"))
    return out


@pytest.mark.parametrize("W", [3, 4, 5, 9, 16])
def test_chain_matches_the_numpy_restatement(exe, W):
    rng = np.random.default_rng(3100 + W)
    cases = joint_cases(rng, W)
    assert {len(j["poses"]) for _, _, _, j, _, _ in cases} == ({1, 2, 3, 4} if W >= 4 else {1, 2, 3})
    assert W != 16 or any(j["poses"] == [0, 5, 10, 15] and len(e) == 32 for _, _, e, j, _, _ in cases)
    assert any(rl is not None for *_, rl, _ in cases) and any(len(l) == 32 for _, l, *_ in cases) and any(len(l) == 0 for _, l, *_ in cases)
    got = run(exe, [chain_vals(c, lin, ed, jt, rl) for c, lin, ed, jt, rl, _ in cases])
    bare = run(exe, [chain_vals(c, lin, ed, None, rl) for c, lin, ed, jt, rl, _ in cases])
    worst = [0.0, 0.0, 0.0]
    for (c, lin, ed, jt, rl, what), g, g0 in zip(cases, got, bare):
        want = restated(c, lin, ed, jt, 4, rl)
        # L away from the poses: the transport is exercised
        assert min(np.abs(lin_ref.local(L, poses_of(c)[i])).max() for i, L in zip(jt["poses"], jt["at"])) > 1e-3, what
        for it in range(4):
            assert g[it]["flags"] == 0 and g[it]["ok"] == 1, what
            if rl is not None:
                assert g[it]["eval"] == want[it][3], what
            for i in range(W):
                er, et = lin_ref.pose_error(row_pose(g[it]["row"], i), want[it][0][i])
                worst = [max(worst[0], er), max(worst[1], et), worst[2]]
            ec = abs(g[it]["cost"] - want[it][2]) / max(1.0, abs(want[it][2]))
            worst[2] = max(worst[2], ec)
            assert ec <= 1e-9, (what, ec)
        # the profile: a member row reaches down to the smallest member
        lo0 = g0[0]["lo"]
        assert g[0]["lo"] == [min(lo0[i], jt["poses"][0]) if i in jt["poses"][1:] else lo0[i] for i in range(W)], what
        moved = max(np.abs(np.array(g[3]["row"])[8:] - np.array(g0[3]["row"])[8:]))
        assert moved > 1e-6, (what, moved)  # the joint factor moved the answer: the bar tests something
    print(f"W={W}: worst deviation from the restatement {worst[0]:.3e} rad, {worst[1]:.3e} m, cost {worst[2]:.3e} relative")
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9, worst


@pytest.mark.parametrize("relin", [None, RELIN])
@pytest.mark.parametrize("W", [3, 5, 16])
def test_one_member_is_the_last_linear_factor_bit_for_bit(exe, exe_edges, W, relin):
    rng = np.random.default_rng(3200 + W)
    cases, lins, eds, joints = [], [], [], []
    for k in range(4):
        c = base.window_case(rng, W, [True] * W, prior=base.LOOSE, n_it=4, cond=1e2)
        poses = poses_of(c)
        p = int(rng.integers(0, W))
        at = poses[p] if k == 3 else None  # L exactly at the pose: the untouched branch, in the first iteration
        l = lin_ref.random_linear(rng, p, poses[p])
        if at is not None:
            l["at"] = at
        cases.append(c)
        lins.append(lin_base.linear_sets(rng, c)[:31] if k % 2 else [])
        eds.append([edge_ref.random_edge(rng, 0, W - 1, poses), edge_ref.random_edge(rng, 1, 2, poses)] if k >= 1 else [])
        joints.append((l, dict(poses=[p], at=[l["at"]], H=l["H"], b=l["b"], f=l["f"])))
    got = run(exe, [chain_vals(c, lin, ed, j, relin) for c, lin, ed, (_, j) in zip(cases, lins, eds, joints)])
    want = run(exe_edges, [edges_base.chain_vals(c, lin + [l], ed, relin) for c, lin, ed, (l, _) in zip(cases, lins, eds, joints)])
    for gc, rc in zip(got, want):
        assert len(gc) == len(rc) == 4
        for g, r in zip(gc, rc):
            assert g == r


def test_no_joint_factor_is_the_edges_chain_bit_for_bit(exe, exe_edges):
    rng = np.random.default_rng(3250)
    cases = edges_base.edge_cases(rng, 5)
    got = run(exe, [chain_vals(c, lin, ed, None, rl) for c, lin, ed, rl, _ in cases])
    want = run(exe_edges, [edges_base.chain_vals(c, lin, ed, rl) for c, lin, ed, rl, _ in cases])
    assert got == want


def test_singular_system_takes_no_step_and_reports_bit_4(exe):
    """both factors empty, no prior, no damping, a joint factor that sees only the relative pose (H = J^T Om J with J = [-I, I] at
    d = 0, powers of two: every product exact): the gauge is free, the second pivot block is exactly zero"""
    rng = np.random.default_rng(3300)
    c = base.window_case(rng, 2, [False, False], prior=np.zeros(6), n_it=2, damping=0.0)
    c["have"] = [False, False]
    Om = np.diag([2.0 ** k for k in (8, 10, 12, 9, 11, 7)])
    J = np.hstack([-np.eye(6), np.eye(6)])
    joint = dict(poses=[0, 1], at=poses_of(c), H=J.T @ Om @ J, b=np.zeros(12), f=1.0)
    g = run(exe, [chain_vals(c, [], [], joint)])[0]
    assert g[0]["ok"] == 0 and int(g[0]["row"][3]) & 4 and g[0]["flags"] & 1
    for i in range(2):
        R, t = row_pose(g[0]["row"], i)
        assert np.array_equal(R, c["R"][i]) and np.array_equal(t, c["t"][i])
    assert g[1]["flags"] & 4 and g[1]["row"][8:] == g[0]["row"][8:]


# ---- the producer ----------------------------------------------------------------------------------------------------------------
def icp0_of(c):
    if not c["have"][0]:
        return None
    return base.ref_hessian(c["sums"][0][0], c["R"][0], c["gz"], c["reg4"][0], c["project"][0], c["thresh_rot"][0], c["thresh_trans"][0])[:3]


def restated_marginal(c, linear, edges, joint):
    return ref.marginal(poses_of(c), icp0_of(c), c["has_Z"][1], (c["ZR"][1], c["Zt"][1]), c["Wb"], c["prior"], c["damping"], linear, edges, joint)


def rank3_sums(rng):
    V = np.linalg.qr(rng.standard_normal((6, 6)))[0][:, :3]
    H = (V * (1e3 * np.array([1.0, 3.0, 10.0]))) @ V.T
    H = (H + H.T) / 2.0
    return base.pack(H, H @ (rng.standard_normal(6) * 0.05), 4.0)


def marginal_cases(rng):
    """(case, linear, edges, joint, the separator expected, what)"""
    out = []

    def case(W, tie=True, rank3=False):
        c = base.window_case(rng, W, [False, tie] + [True] * (W - 2), prior=base.LOOSE if rank3 or len(out) % 2 == 0 else np.zeros(6), cond=1e3, scale=None,
                             reg4=0, project=0 if rank3 else 1)
        if rank3:
            c["sums"][0][0] = rank3_sums(rng)
        return c

    def E(c, a, b, **kw):
        return edge_ref.random_edge(rng, a, b, poses_of(c), info=edge_ref.random_info(rng, 1e2, 1e5), **kw)

    for rank3 in (False, True):
        c = case(3, rank3=rank3)
        out.append((c, [lin_ref.random_linear(rng, 0, poses_of(c)[0])], [E(c, 0, 1), E(c, 1, 2)], None, [1], f"S={{1}} rank3={rank3}"))
        c = case(4, rank3=rank3)
        out.append((c, [], [E(c, 0, 2)], None, [1, 2], f"S={{1,2}} rank3={rank3}"))
        c = case(5, tie=False, rank3=rank3)
        out.append((c, [lin_ref.random_linear(rng, 1, poses_of(c)[1])], [E(c, 0, 3), E(c, 0, 3), E(c, 2, 4), E(c, 0, 3)], None, [1, 3],
                    f"S={{1,3}}, three edges on (0, 3), no has_Z tie, rank3={rank3}"))
        c = case(6, rank3=rank3)
        out.append((c, [lin_ref.random_linear(rng, 0, poses_of(c)[0]) for _ in range(3)], [E(c, 0, 4), E(c, 0, 2), E(c, 0, 3), E(c, 0, 1), E(c, 3, 5)], None,
                    [1, 2, 3, 4], f"S={{1,2,3,4}} by edges, rank3={rank3}"))
        # a carried joint factor with pose 0 whose other members overlap ({2}) and extend ({3}) the edges' separator {1, 2}
        c = case(5, rank3=rank3)
        out.append((c, [], [E(c, 0, 2), E(c, 0, 2)], ref.random_joint(rng, [0, 2, 3], poses_of(c)), [1, 2, 3], f"joint {{0,2,3}} beside edges (0,2), rank3={rank3}"))
        c = case(16, tie=False, rank3=rank3)
        out.append((c, [lin_ref.random_linear(rng, 0, poses_of(c)[0])], [], ref.random_joint(rng, [0, 5, 10, 15], poses_of(c)), [1, 5, 10, 15],
                    f"joint {{0,5,10,15}} alone, no tie, rank3={rank3}"))
        c = case(5, rank3=rank3)
        out.append((c, [], [E(c, 0, 4)], ref.random_joint(rng, [0, 1, 2, 3], poses_of(c)), [1, 2, 3, 4], f"joint {{0,1,2,3}} and an edge (0,4), rank3={rank3}"))
        c = case(3, rank3=rank3)
        out.append((c, [], [E(c, 1, 2)], ref.random_joint(rng, [0], poses_of(c)), [1], f"a one-member joint factor on pose 0, rank3={rank3}"))
    return out


def test_marginal_matches_the_numpy_restatement(exe):
    rng = np.random.default_rng(3400)
    cases = marginal_cases(rng)
    got = run(exe, [marginal_vals(c, l, e, j) for c, l, e, j, _, _ in cases])
    worst, worst_cond = [0.0, 0.0, 0.0], 0.0
    for (c, lin, ed, jt, sep, what), g in zip(cases, got):
        want = restated_marginal(c, lin, ed, jt)
        cond = np.linalg.cond(want["A00"])
        worst_cond = max(worst_cond, cond)
        assert cond <= 1e6, (what, cond)
        assert g["sep"] == sep == want["sep"], what
        assert g["valid"] == 1 and want["valid"] == 1 and g["stray"] == 0, what
        assert g["n_ties"] == want["n_ties"], what
        n = 6 * len(sep)
        H = np.array(g["H"]).reshape(n, n)
        assert np.array_equal(H, H.T), what
        dev = ref.deviation(g, want)
        print(f"{what}: cond {cond:.2e}  dH {dev[0]:.2e}  db {dev[1]:.2e}  df {dev[2]:.2e}")
        worst = [max(a, b) for a, b in zip(worst, dev)]
        for k, shape in (("A00", (6, 6)), ("AS0", (n, 6)), ("ASS", (n, n))):
            assert np.allclose(np.array(g[k]).reshape(shape), want[k], rtol=0, atol=1e-12 * max(1.0, np.abs(want[k]).max())), (what, k)
    print(f"worst deviation from the restatement: H {worst[0]:.3e}, b {worst[1]:.3e}, f {worst[2]:.3e}; worst cond(A00) {worst_cond:.3e}")
    assert max(worst) <= 1e-9, worst


def test_marginal_without_far_edges_is_window_marginal_impl_bit_for_bit(exe, exe_marginal):
    import test_icp_window_marginal_cpu as marg_base
    rng = np.random.default_rng(3500)
    cases = marg_base.random_cases(rng)
    got = run(exe, [marginal_vals(c, l, e, None) for c, l, e, _ in cases])
    want = marg_base.run(exe_marginal, [marg_base.case_vals(c, l, e) for c, l, e, _ in cases])
    for g, r, (_, _, _, what) in zip(got, want, cases):
        assert g["sep"] == [1], what
        for k in ("H", "b", "f", "valid", "n_ties", "A00", "g0", "c"):
            assert g[k] == r[k], (what, k)
        assert g["AS0"] == r["A10"] and g["ASS"] == r["A11"] and g["gS"] == r["g1"], what


def test_no_tie_at_all_leaves_zeros_on_pose_1(exe):
    rng = np.random.default_rng(3600)
    c = base.window_case(rng, 3, [False, False, True], prior=base.LOOSE, cond=1e2, scale=1e3)
    poses = poses_of(c)
    lin, ed = [lin_ref.random_linear(rng, 0, poses[0])], [edge_ref.random_edge(rng, 1, 2, poses)]
    g = run(exe, [marginal_vals(c, lin, ed, None)])[0]
    want = restated_marginal(c, lin, ed, None)
    assert g["sep"] == [1] and g["valid"] == 1 and g["n_ties"] == 0
    assert not np.any(np.array(g["H"])) and not np.any(np.array(g["b"]))
    assert want["n_ties"] == 0 and not np.any(want["H"]) and abs(g["f"] - want["f"]) <= 1e-9 * abs(want["c"])


def test_no_positive_pivot_gives_valid_0_and_zeros(exe):
    rng = np.random.default_rng(3700)
    c = base.window_case(rng, 4, [False] * 4, prior=np.zeros(6), damping=0.0)
    c["have"] = [False, True, True, True]
    g = run(exe, [marginal_vals(c, [], [], None)])[0]
    assert g["valid"] == 0 and g["n_ties"] == 0 and g["f"] == 0.0 and g["stray"] == 0
    assert not np.any(np.array(g["H"])) and not np.any(np.array(g["b"]))
    assert restated_marginal(c, [], [], None)["valid"] == 0


def test_elimination_identity(exe):
    rng = np.random.default_rng(3800)
    W = 5
    c = base.window_case(rng, W, [False] + [True] * (W - 1), prior=base.LOOSE, cond=1e2, n_it=1)
    poses, Z = poses_of(c), list(zip(c["ZR"], c["Zt"]))
    edges = [edge_ref.random_edge(rng, 0, 2, poses), edge_ref.random_edge(rng, 0, 3, poses), edge_ref.random_edge(rng, 1, 4, poses)]
    icp = [base.ref_hessian(c["sums"][0][i], c["R"][i], c["gz"], 0, 1, 0.0, 0.0)[:3] for i in range(W)]
    full, _, _ = ref.iteration(poses, icp, c["has_Z"], Z, c["Wb"], c["prior"], c["damping"], [], edges, None)
    g = run(exe, [marginal_vals(c, [], edges, None)])[0]
    assert g["valid"] == 1 and g["n_ties"] == 3 and g["sep"] == [1, 2, 3]
    joint = ref.as_joint(g, poses)
    assert joint["poses"] == [0, 1, 2]
    rest_edges = [dict(edges[2], a=0, b=3)]
    hz, Zr = [False] + c["has_Z"][2:], Z[1:]
    with_m, _, _ = ref.iteration(poses[1:], icp[1:], hz, Zr, c["Wb"], np.zeros(6), c["damping"], [], rest_edges, joint)
    without, _, _ = ref.iteration(poses[1:], icp[1:], hz, Zr, c["Wb"], np.zeros(6), c["damping"], [], rest_edges, None)
    # the same reduced step through the host build of the consuming chain
    red = dict(c, W=W - 1, has_Z=hz, have=c["have"][1:], reg4=c["reg4"][1:], project=c["project"][1:], prior=np.zeros(6), thresh_rot=c["thresh_rot"][1:],
               thresh_trans=c["thresh_trans"][1:], R=c["R"][1:], t=c["t"][1:], ZR=c["ZR"][1:], Zt=c["Zt"][1:], sums=[c["sums"][0][1:]])
    chain = run(exe, [chain_vals(red, [], rest_edges, joint)])[0][0]
    assert chain["flags"] == 0 and chain["ok"] == 1
    worst = [max(lin_ref.pose_error(with_m[i], full[i + 1])[k] for i in range(W - 1)) for k in (0, 1)]
    worst_chain = [max(lin_ref.pose_error(row_pose(chain["row"], i), full[i + 1])[k] for i in range(W - 1)) for k in (0, 1)]
    apart = max(lin_ref.pose_error(without[i], full[i + 1])[1] for i in range(W - 1))
    print(f"reduced step with the joint marginal against the full step: {worst[0]:.3e} rad, {worst[1]:.3e} m (numpy), {worst_chain[0]:.3e} rad, "
          f"{worst_chain[1]:.3e} m (host build of the chain); without the marginal {apart:.3e} m")
    assert apart > 1e-4, apart
    assert max(worst) <= 1e-9 and max(worst_chain) <= 1e-9, (worst, worst_chain)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
JOINT_FUNCS = ["mh_icp_window_optimise_joint", "mh_icp_window_optimise_joint_async", "mh_icp_window_marginalise_joint", "mh_icp_window_marginalise_joint_async"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in JOINT_FUNCS:
        assert hasattr(L, f), f
    assert set(JOINT_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr
    for f in JOINT_FUNCS:
        assert f"int {f}(" in hdr


def test_struct_sizes_match_the_header(tmp_path):
    from mimosa_amd import capi
    src = tmp_path / "sz.c"
    F, M = "mh_window_joint_factor", "mh_window_joint_marginal"
    fields = [f"sizeof({F})"] + [f"offsetof({F}, {k})" for k in ("n_poses", "pose", "L_R", "L_t", "H", "b", "f")]
    fields += [f"sizeof({M})"] + [f"offsetof({M}, {k})" for k in ("prior", "valid", "n_ties", "oldest")] + ["(size_t)MH_WINDOW_JOINT_POSES"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) { printf("' + "%zu " * len(fields) + '\\n", ' + ", ".join(fields)
                   + "); return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    J, Q = capi.WindowJointFactor, capi.WindowJointMarginal
    assert got == [C.sizeof(J), J.n_poses.offset, J.pose.offset, J.L_R.offset, J.L_t.offset, J.H.offset, J.b.offset, J.f.offset, C.sizeof(Q), Q.prior.offset,
                   Q.valid.offset, Q.n_ties.offset, Q.oldest.offset, capi.MH_WINDOW_JOINT_POSES]


def bad_joints():
    """(joint as capi.WindowJointFactor, code name, a word of the message) for W = 3: every refusal of the joint argument"""
    from mimosa_amd import capi
    I, z = np.eye(3), np.zeros(3)

    def make(poses, H=None, b=None, f=1.0, n=None, at=None):
        m = len(poses)
        q = capi.make_window_joint(dict(poses=poses, at=at or [(I, z)] * m, H=np.eye(6 * m) * 4.0 if H is None else H, b=np.zeros(6 * m) if b is None else b, f=f))
        if n is not None:
            q.n_poses = n
        return q

    asym = np.eye(12) * 4.0
    asym[1, 8] = 1.0
    out = [(make([0], n=0), b"n_poses"), (make([0, 1], n=5), b"n_poses"), (make([0, 1], n=-1), b"n_poses"), (make([1, 1]), b"ascending"),
           (make([2, 1]), b"ascending"), (make([0, 3]), b"ascending"), (make([-1, 1]), b"ascending"), (make([0, 2], H=asym), b"symmetric")]
    for bad in (np.nan, np.inf):
        H, b = np.eye(12) * 4.0, np.zeros(12)
        H[7, 7] = bad
        b[9] = bad
        out += [(make([0, 2], H=H), b"not finite"), (make([0, 2], b=b), b"not finite"), (make([0, 2], f=bad), b"not finite"),
                (make([0, 2], at=[(I, z), (np.full((3, 3), bad), z)]), b"not finite"), (make([0, 2], at=[(I, z + bad), (I, z)]), b"not finite")]
    # entries behind the members in use are ignored: not finite there is no error (the call goes on to the NULL argument)
    q = make([0])
    q.H[24 * 6 + 6] = np.nan
    q.b[6] = np.inf
    q.pose[1] = -7
    out.append((q, b"NULL argument"))
    return out


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out, mout = capi.make_window_config(), capi.WindowResult(), capi.WindowJointMarginal()
    I, z, g = np.tile(np.eye(3).ravel(), 3), np.zeros(9), np.array([0.0, 0.0, -1.0])
    hz = np.zeros(3, np.int32)
    common = (None, C.c_size_t(3), capi._p(I), capi._p(z), hz.ctypes.data_as(C.c_void_p), capi._p(I), capi._p(z), capi._p(g), C.byref(cfg))
    good_edge = dict(a=0, b=2, Z=(np.eye(3), np.zeros(3)), info=np.diag([4.0] * 6))
    bad_edge = dict(good_edge, a=2, b=1)

    def optimise(fn, edges, joint):
        return fn(*common, None, None, C.c_size_t(0), capi.make_window_edge(edges), C.c_size_t(len(edges)), C.byref(out), None, None, C.byref(joint))

    def marginalise(fn, edges, joint, W=3):
        args = list(common)
        args[1] = C.c_size_t(W)
        return fn(*args, None, C.c_size_t(0), capi.make_window_edge(edges), C.c_size_t(len(edges)), None if joint is None else C.byref(joint), C.byref(mout))

    calls = [(lambda e, j, fn=fn: optimise(fn, e, j)) for fn in (L.mh_icp_window_optimise_joint, L.mh_icp_window_optimise_joint_async)]
    calls += [(lambda e, j, fn=fn: marginalise(fn, e, j)) for fn in (L.mh_icp_window_marginalise_joint, L.mh_icp_window_marginalise_joint_async)]
    for call in calls:
        for joint, word in bad_joints():
            assert call([good_edge], joint) == capi.MH_ERR_INVALID_ARG, word
            assert word in L.mh_last_error(None), (word, L.mh_last_error(None))
            assert b"joint" in L.mh_last_error(None) or word == b"NULL argument"
        # behind the edges: a call with both wrong reports the edge; before icps / W: a bad joint factor with icps == NULL reports the joint factor
        assert call([bad_edge], bad_joints()[0][0]) == capi.MH_ERR_INVALID_ARG and b"pose_a" in L.mh_last_error(None)
    # the marginal's own refusals
    two = capi.make_window_joint(dict(poses=[1, 2], at=[(np.eye(3), np.zeros(3))] * 2, H=np.eye(12), b=np.zeros(12), f=0.0))
    wide = capi.make_window_joint(dict(poses=[0, 5, 6], at=[(np.eye(3), np.zeros(3))] * 3, H=np.eye(18), b=np.zeros(18), f=0.0))
    for fn in (L.mh_icp_window_marginalise_joint, L.mh_icp_window_marginalise_joint_async):
        assert marginalise(fn, [good_edge], two) == capi.MH_ERR_UNSUPPORTED and b"without pose 0" in L.mh_last_error(None)
        far = [dict(good_edge, b=k) for k in (2, 3, 4)]
        assert marginalise(fn, far + [dict(good_edge, b=5)], None, W=7) == capi.MH_ERR_UNSUPPORTED and b"more than 4 poses" in L.mh_last_error(None)
        assert marginalise(fn, far, wide, W=7) == capi.MH_ERR_UNSUPPORTED and b"more than 4 poses" in L.mh_last_error(None)
        # four poses are taken: the call goes on to the NULL argument
        assert marginalise(fn, far, None, W=7) == capi.MH_ERR_INVALID_ARG and b"NULL argument" in L.mh_last_error(None)
    # mh_icp_window_marginalise itself still refuses the far edge
    rc = L.mh_icp_window_marginalise(*common, None, C.c_size_t(0), capi.make_window_edge([good_edge]), C.c_size_t(1), C.byref(capi.WindowMarginal()))
    assert rc == capi.MH_ERR_UNSUPPORTED and b"beyond pose 1" in L.mh_last_error(None)
