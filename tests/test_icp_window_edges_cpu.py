"""CPU: the edge phases and the profile solve of mh_icp_window_optimise_edges (mimosa_amd/csrc/window_device.hpp, compiled by
g++ through tests/cpp/window_edge_step.cpp): no edge is window_advance_lin bit for bit; the chain against a numpy restatement
written independently of the header (tests/window_edge_ref.py: a dense assembly and numpy.linalg.solve, no profile); a span-1
edge against the has_Z tie it restates; the singular system; the ABI additions.

Bars.  Poses after each of 4 iterations against the restatement: 1e-9 rad / 1e-9 m and the cost to 1e-9 relative, the bar and
the conditioning rule of tests/test_icp_window_lin_cpu.py (reg_4_dof only where between factors tie every pose).  The edges'
information matrices have eigenvalues between 1e2 and 1e6, inside the range the between weights (2.5e5 / 1e4) and the factors
(1 .. 1e4) already span, so the systems keep condition numbers of about 1e6 and an unrefined numpy.linalg.solve is good to
about 1e-11 per iteration.  The span-1 edge against the has_Z tie: the same terms through a dense product instead of a diagonal
one, 1e-9 as the issue sets it.

The singular system.  W = 2, both factors empty, no prior, damping 0, one edge: the gauge is free and the exact system is
singular.  With both poses equal, J_a = -I, and with an information matrix of powers of two every product is exact: S_0 = Om
factorises with L = I, G = -I and S_1 = Om - Om = 0 exactly, so the first pivot of S_1 is 0 whatever the rounding mode; the
chain must report bit 4 and leave the poses alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_icp_window_cpu as base
import test_icp_window_lin_cpu as lin_base
import test_icp_window_relin_cpu as relin_base
import window_edge_ref as ref
import window_lin_ref as lin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELIN = (1.75e-2, 5e-3)


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("window_edge_step")


@pytest.fixture(scope="module")
def exe_lin():
    from mimosa_amd import build
    return build.build_host_test("window_lin_step")


def edge_vals(edges):
    vals = [float(len(edges))]
    for e in edges:
        vals += [float(e["a"]), float(e["b"])] + list(np.asarray(e["Z"][0]).ravel()) + list(e["Z"][1]) + list(np.asarray(e["info"]).ravel())
    return vals


def chain_vals(c, linear, edges, relin=None):
    head = [0.0, 0.0, 0.0] if relin is None else [1.0, relin[0], relin[1]]
    return head + lin_base.lin_vals(linear) + edge_vals(edges) + relin_base.chain_vals(c, (0.0, 0.0))[2:]


def run(exe, cases):
    toks = [str(len(cases))]
    for vals in cases:
        toks += [repr(float(v)) for v in vals]
    out = subprocess.run([exe], input=" ".join(toks), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def poses_of(c):
    return list(zip(c["R"], c["t"]))


@pytest.mark.parametrize("with_lin", [False, True])
@pytest.mark.parametrize("relin", [None, RELIN])
@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_no_edge_is_window_advance_lin_bit_for_bit(exe, exe_lin, W, relin, with_lin):
    rng = np.random.default_rng(1100 + W)
    cases = lin_base.mixed_cases(rng, W)
    lins = [lin_base.linear_sets(rng, c) if with_lin else [] for c in cases]
    want = lin_base.run(exe_lin, [(1, lin_base.chain_vals(c, l, relin)) for c, l in zip(cases, lins)])
    got = run(exe, [chain_vals(c, l, [], relin) for c, l in zip(cases, lins)])
    kept = 0
    for c, gc, rc in zip(cases, got, want):
        assert len(gc) == len(rc)
        for g, r in zip(gc, rc):
            assert g["flags"] == r["flags"] and g["row"] == r["row"]
            if "xi" in r:
                assert g["xi"] == r["xi"] and g["H"] == r["H"] and g["cost"] == r["cost"] and g["ok"] == r["ok"]
                # the profile of a window without edges: the has_Z ties, nothing else
                assert g["lo"] == [i - 1 if c["has_Z"][i] else i for i in range(W)]
                if relin is not None:
                    assert g["eval"] == r["eval"] and g["next"] == r["next"]
                    kept += g["eval"] != int(base.mask(c["have"]))
    assert relin is None or kept or W == 1


def restated(c, linear, edges, n_it, relin=None):
    """the chain in numpy: per iteration (poses, xi, cost, evaluated mask).  With thresholds a factor whose pose stayed within
    them of its last evaluation (component-wise, strict) is carried from there instead of being evaluated."""
    W = c["W"]
    poses, Z = poses_of(c), list(zip(c["ZR"], c["Zt"]))
    kept = [None] * W  # (H, b, f, L)
    evaluate = [True] * W
    out = []
    for it in range(n_it):
        icp, mask = [], 0
        for i in range(W):
            if not c["have"][i]:
                icp.append(None)
                continue
            if relin is None or evaluate[i]:
                H, b, f, _, _ = base.ref_hessian(c["sums"][it][i], poses[i][0], c["gz"], c["reg4"][i], c["project"][i], c["thresh_rot"][i], c["thresh_trans"][i])
                kept[i] = (H, b, f, poses[i])
                icp.append((H, b, f))
                mask |= 1 << i
            else:
                H, b, f, L = kept[i]
                icp.append(lin_ref.transport(H, b, f, L, poses[i]))
        poses, xi, cost = ref.iteration(poses, icp, c["has_Z"], Z, c["Wb"], c["prior"], c["damping"], linear, edges)
        if relin is not None:
            for i in range(W):
                if c["have"][i]:
                    d = np.abs(lin_ref.local(kept[i][3], poses[i]))
                    evaluate[i] = bool(d[:3].max() > relin[0] or d[3:].max() > relin[1])
        out.append((poses, xi, cost, mask))
    return out


def edge_cases(rng, W):
    """(case, linear factors, edges, thresholds, what it is there for) — every kind of edge the contract names"""
    out = []

    def case(has_Z, reg4=0):
        return base.window_case(rng, W, has_Z, prior=base.LOOSE, reg4=int(reg4 and all(has_Z[1:])), n_it=4, cond=1e2)

    full, none = [True] * W, [False] * W
    # one edge over the whole window, beside the has_Z ties
    c = case(full, reg4=1)
    out.append((c, [], [ref.random_edge(rng, 0, W - 1, poses_of(c))], None, "one edge (0, W - 1)"))
    # 32 edges: every span 1 .. W - 1 from both ends of the window, two on one pair, linear factors present
    c = case(full)
    pairs = [(0, s) for s in range(1, W)] + [(W - 1 - s, W - 1) for s in range(1, W)]
    pairs = [pairs[j % len(pairs)] for j in range(32)]
    pairs[31] = pairs[0]
    out.append((c, lin_base.linear_sets(rng, c), [ref.random_edge(rng, a, b, poses_of(c)) for a, b in pairs], None, "32 edges, every span"))
    # an edge parallel to a has_Z tie, and two edges on one pair
    c = case(full, reg4=1)
    k = int(rng.integers(0, W - 1))
    out.append((c, [], [ref.random_edge(rng, k, k + 1, poses_of(c)), ref.random_edge(rng, 0, W - 1, poses_of(c)), ref.random_edge(rng, 0, W - 1, poses_of(c))], None,
                "parallel to a has_Z tie; two on one pair"))
    # an edge as the only tie across a has_Z gap
    gap = list(full)
    i = int(rng.integers(1, W))
    gap[i] = False
    c = case(gap)
    a, b = int(rng.integers(0, i)), int(rng.integers(i, W))
    out.append((c, lin_base.linear_sets(rng, c)[:3], [ref.random_edge(rng, a, b, poses_of(c))], None, "the only tie across a has_Z gap"))
    # no has_Z tie at all: a far edge and a chain of edges hold the window together
    c = case(none)
    out.append((c, [], [ref.random_edge(rng, j, j + 1, poses_of(c)) for j in range(W - 1)] + [ref.random_edge(rng, 0, W - 1, poses_of(c))], None, "edges only"))
    # an edge ending on a pose without an ICP factor
    c = case(full)
    e = int(rng.integers(1, W))
    c["have"][e] = False
    out.append((c, [], [ref.random_edge(rng, int(rng.integers(0, e)), e, poses_of(c))], None, "ends on a pose without an ICP factor"))
    # thresholds present, with linear factors and edges of several spans
    c = case(full)
    spans = [(max(0, j - 1 - j % 3), j) for j in range(1, W)]
    out.append((c, lin_base.linear_sets(rng, c), [ref.random_edge(rng, a, b, poses_of(c)) for a, b in spans], RELIN, "thresholds"))
    return out


@pytest.mark.parametrize("W", [2, 3, 5, 16])
def test_chain_matches_the_numpy_restatement(exe, W):
    rng = np.random.default_rng(1200 + W)
    cases = edge_cases(rng, W)
    assert any(len(e) == 1 for _, _, e, _, _ in cases) and any(len(e) == 32 for _, _, e, _, _ in cases)
    assert {q["b"] - q["a"] for _, _, e, _, _ in cases for q in e} == set(range(1, W))
    assert any(len(e) > len({(q["a"], q["b"]) for q in e}) for _, _, e, _, _ in cases)
    assert any(not c["have"][q["b"]] for c, _, e, _, _ in cases for q in e)
    for _, _, e, _, _ in cases:
        for q in e:
            lam = np.linalg.eigvalsh(q["info"])
            assert 0.99e2 <= lam[0] and lam[-1] <= 1.01e6 and np.abs(q["info"] - np.diag(np.diag(q["info"]))).max() > 1.0
    got = run(exe, [chain_vals(c, lin, ed, rl) for c, lin, ed, rl, _ in cases])
    bare = run(exe, [chain_vals(c, lin, [], rl) for c, lin, ed, rl, _ in cases])
    worst = [0.0, 0.0, 0.0]
    for (c, lin, ed, rl, what), g, g0 in zip(cases, got, bare):
        want = restated(c, lin, ed, 4, rl)
        for it in range(4):
            assert g[it]["flags"] == 0 and g[it]["ok"] == 1, what
            if rl is not None:
                assert g[it]["eval"] == want[it][3], what
            row = np.array(g[it]["row"])
            for i in range(W):
                T = (row[8 + 12 * i:17 + 12 * i].reshape(3, 3), row[17 + 12 * i:20 + 12 * i])
                er, et = lin_ref.pose_error(T, want[it][0][i])
                worst = [max(worst[0], er), max(worst[1], et), worst[2]]
            ec = abs(g[it]["cost"] - want[it][2]) / max(1.0, abs(want[it][2]))
            worst[2] = max(worst[2], ec)
            assert ec <= 1e-9, what
        # the edges moved the answer: the bar below tests something
        moved = max(np.abs(np.array(g[3]["row"])[8:] - np.array(g0[3]["row"])[8:]))
        assert moved > 1e-6, (what, moved)
    print(f"W={W}: worst deviation from the restatement {worst[0]:.3e} rad, {worst[1]:.3e} m, cost {worst[2]:.3e} relative")
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9, worst


@pytest.mark.parametrize("W", [2, 5, 16])
def test_profile_is_the_smallest_column_of_each_row(exe, W):
    rng = np.random.default_rng(1300 + W)
    for c, lin, ed, rl, _ in edge_cases(rng, W):
        g = run(exe, [chain_vals(c, lin, ed, rl)])[0][0]
        assert g["lo"] == [min([i - 1 if c["has_Z"][i] else i] + [q["a"] for q in ed if q["b"] == i]) for i in range(W)]


@pytest.mark.parametrize("W", [2, 5, 16])
def test_span_one_edge_with_the_between_weights_is_the_has_Z_tie(exe, W):
    rng = np.random.default_rng(1400 + W)
    c = base.window_case(rng, W, [True] * W, prior=base.LOOSE, n_it=4, cond=1e2)
    tie = run(exe, [chain_vals(c, [], [])])[0]
    e = dict(c, has_Z=[False] * W)
    edges = [dict(a=i - 1, b=i, Z=(c["ZR"][i], c["Zt"][i]), info=np.diag(c["Wb"])) for i in range(1, W)]
    got = run(exe, [chain_vals(e, [], edges)])[0]
    worst = 0.0
    for g, r in zip(got, tie):
        assert g["flags"] == r["flags"] == 0
        worst = max(worst, np.abs(np.array(g["row"])[8:] - np.array(r["row"])[8:]).max())
    print(f"W={W}: span-1 edges against the has_Z ties {worst:.3e}")
    assert worst <= 1e-9


def test_singular_system_takes_no_step_and_reports_bit_4(exe):
    rng = np.random.default_rng(7)
    c = base.window_case(rng, 2, [False, False], prior=np.zeros(6), n_it=2, damping=0.0)
    c["have"] = [False, False]
    c["R"][1], c["t"][1] = c["R"][0].copy(), c["t"][0].copy()
    Om = np.diag([2.0 ** k for k in (8, 10, 12, 9, 11, 7)])
    edge = dict(a=0, b=1, Z=base.random_pose(rng, 0.02, 0.03), info=Om)
    g = run(exe, [chain_vals(c, [], [edge])])[0]
    assert g[0]["ok"] == 0 and int(g[0]["row"][3]) & 4 and g[0]["flags"] & 1
    row = np.array(g[0]["row"])
    for i in range(2):
        assert np.array_equal(row[8 + 12 * i:17 + 12 * i], np.asarray(c["R"][i]).ravel()) and np.array_equal(row[17 + 12 * i:20 + 12 * i], c["t"][i])
    assert g[1]["flags"] & 4 and g[1]["row"][8:] == g[0]["row"][8:]  # queued behind the stop: nothing evaluated


# ---- ABI -------------------------------------------------------------------------------------------------------------------
EDGE_FUNCS = ["mh_icp_window_optimise_edges", "mh_icp_window_optimise_edges_async"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in EDGE_FUNCS:
        assert hasattr(L, f), f
    assert set(EDGE_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr
    for f in EDGE_FUNCS:
        assert f"int {f}(" in hdr


def test_struct_size_matches_the_header(tmp_path):
    from mimosa_amd import capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(mh_window_edge), offsetof(mh_window_edge, pose_a), offsetof(mh_window_edge, pose_b), offsetof(mh_window_edge, Z_R), "
                   "offsetof(mh_window_edge, Z_t), offsetof(mh_window_edge, info), MH_WINDOW_EDGE_MAX); return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    E = capi.WindowEdge
    assert got == [C.sizeof(E), E.pose_a.offset, E.pose_b.offset, E.Z_R.offset, E.Z_t.offset, E.info.offset, capi.MH_WINDOW_EDGE_MAX]


def bad_edges():
    """(edges, n_edges or None for len, a word of the message) for W = 3: every refusal of the edge arguments"""
    I, z, Om = np.eye(3), np.zeros(3), np.diag([4.0] * 6)
    good = dict(a=0, b=2, Z=(I, z), info=Om)
    asym = Om.copy()
    asym[1, 4] = 1.0
    out = [([good] * 33, None, b"at most 32"), (None, 1, b"NULL edges"), ([dict(good, a=-1)], None, b"pose_a"), ([dict(good, b=3)], None, b"pose_a"),
           ([dict(good, a=2, b=2)], None, b"pose_a"), ([dict(good, a=2, b=1)], None, b"pose_a"), ([dict(good, info=asym)], None, b"symmetric")]
    for key in ("ZR", "Zt", "info"):
        for bad in (np.nan, np.inf):
            e = dict(good, Z=(I.copy(), z.copy()), info=Om.copy())
            if key == "ZR":
                e["Z"][0][1, 2] = bad
            elif key == "Zt":
                e["Z"][1][2] = bad
            else:
                e["info"][3, 3] = bad
            out.append(([good, e], None, b"not finite"))
    return out


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out = capi.make_window_config(), capi.WindowResult()
    I, z, g = np.tile(np.eye(3).ravel(), 3), np.zeros(9), np.array([0.0, 0.0, -1.0])
    hz = np.zeros(3, np.int32)
    for fn in (L.mh_icp_window_optimise_edges, L.mh_icp_window_optimise_edges_async):
        for edges, n, word in bad_edges() + [([], None, b"NULL argument")]:
            arr = None if edges is None else capi.make_window_edge(edges)
            rc = fn(None, C.c_size_t(3), capi._p(I), capi._p(z), hz.ctypes.data_as(C.c_void_p), capi._p(I), capi._p(z), capi._p(g), C.byref(cfg), None, None,
                    C.c_size_t(0), arr, C.c_size_t(len(edges) if n is None else n), C.byref(out), None, None)
            assert rc == capi.MH_ERR_INVALID_ARG, word
            assert word in L.mh_last_error(None), (word, L.mh_last_error(None))
