"""CPU: the phases of mh_icp_window_marginalise (mimosa_amd/csrc/window_device.hpp: window_marginal_impl, compiled by g++ through
tests/cpp/window_marginal_step.cpp) against a numpy restatement written independently of the header
(tests/window_marginal_ref.py: dense blocks and numpy.linalg.solve); the elimination identity — a Gauss-Newton step of the
window without its oldest pose, with the marginal as a linear factor, moves the remaining poses as the step of the full window
moves them; the edge conditions; the ABI additions.

Bars.  H_m, b_m, f_m against the restatement: 1e-9, the project's standing bar, relative to the uncancelled scales ||A11'||_F,
||g1'|| and c.  Every case has cond(A00) <= 1e6 (asserted, none is dropped), so two fp64 routes through A00^-1 agree to about
1e6 x 1e-16 x a small factor: three digits of margin.  The elimination identity: 1e-9 m / 1e-9 rad, as the issue sets it; the
full system there has a condition number of about 1e6 as well (tests/test_icp_window_edges_cpu.py)."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import test_icp_window_cpu as base
import window_edge_ref as edge_ref
import window_lin_ref as lin_ref
import window_marginal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("window_marginal_step")


def case_vals(c, linear, edges):
    W = c["W"]
    vals = [float(len(linear))]
    for l in linear:
        vals += [float(l["pose"])] + list(np.asarray(l["at"][0]).ravel()) + list(l["at"][1]) + list(np.asarray(l["H"]).ravel()) + list(l["b"]) + [l["f"]]
    vals.append(float(len(edges)))
    for e in edges:
        vals += [float(e["a"]), float(e["b"])] + list(np.asarray(e["Z"][0]).ravel()) + list(e["Z"][1]) + list(np.asarray(e["info"]).ravel())
    vals += [float(W), base.mask(c["has_Z"]), base.mask(c["have"]), base.mask(c["reg4"]), base.mask(c["project"])] + list(c["gz"]) + list(c["Wb"]) + list(c["prior"])
    vals += [c["damping"], c["thresh_rot"][0], c["thresh_trans"][0]]
    for i in range(W):
        vals += list(np.asarray(c["R"][i]).ravel()) + list(c["t"][i])
    for i in range(W):
        vals += list(np.asarray(c["ZR"][i]).ravel()) + list(c["Zt"][i])
    vals += list(c["sums"][0][0])
    return vals


def run(exe, cases):
    toks = [str(len(cases))]
    for vals in cases:
        toks += [repr(float(v)) for v in vals]
    out = subprocess.run([exe], input=" ".join(toks), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def poses_of(c):
    return list(zip(c["R"], c["t"]))


def icp0_of(c):
    if not c["have"][0]:
        return None
    return base.ref_hessian(c["sums"][0][0], c["R"][0], c["gz"], c["reg4"][0], c["project"][0], c["thresh_rot"][0], c["thresh_trans"][0])[:3]


def restated(c, linear, edges):
    return ref.marginal(poses_of(c), icp0_of(c), c["has_Z"][1], (c["ZR"][1], c["Zt"][1]), c["Wb"], c["prior"], c["damping"], linear, edges)


def rank3_sums(rng):
    """H_ss of rank 3 (three directions of the pose unobserved), b in its range"""
    V = np.linalg.qr(rng.standard_normal((6, 6)))[0][:, :3]
    H = (V * (1e3 * np.array([1.0, 3.0, 10.0]))) @ V.T
    H = (H + H.T) / 2.0
    return base.pack(H, H @ (rng.standard_normal(6) * 0.05), 4.0)


def random_cases(rng):
    """(case, linear, edges, what): H_ss full rank / rank 3 with a prior, 0 / 1 / 32 linear factors on pose 0 linearized away from
    T_0, linear factors on pose 1, has_Z[1] on and off, 0 / 2 / 32 edges on (0, 1), at W = 3 an edge (1, 2)"""
    out = []
    for rank3, n_lin0, tie, n_edge in itertools.product((False, True), (0, 1, 32), (False, True), (0, 2, 32)):
        W = 2 + (len(out) % 2)
        c = base.window_case(rng, W, [False, tie] + [True] * (W - 2), prior=base.LOOSE if rank3 or len(out) % 3 == 0 else np.zeros(6), cond=1e3, scale=None,
                             reg4=0, project=0 if rank3 else 1)
        if rank3:
            c["sums"][0][0] = rank3_sums(rng)
        poses = poses_of(c)
        linear = [lin_ref.random_linear(rng, 0, poses[0]) for _ in range(n_lin0)]
        if n_lin0 < 32:  # on pose 1: to be ignored, in front of and behind the others
            linear = [lin_ref.random_linear(rng, 1, poses[1])] + linear + [lin_ref.random_linear(rng, 1, poses[1])]
        edges = [edge_ref.random_edge(rng, 0, 1, poses, info=edge_ref.random_info(rng, 1e2, 1e6 if n_edge == 2 else 1e5)) for _ in range(n_edge)]
        if W == 3 and n_edge < 32:  # to be ignored
            edges.insert(len(edges) // 2, edge_ref.random_edge(rng, 1, 2, poses))
        out.append((c, linear, edges, f"rank3={rank3} n_lin0={n_lin0} tie={tie} n_edge={n_edge} W={W}"))
    return out


def test_random_cases_match_the_numpy_restatement(exe):
    rng = np.random.default_rng(2100)
    cases = random_cases(rng)
    got = run(exe, [case_vals(c, l, e) for c, l, e, _ in cases])
    worst, worst_cond = [0.0, 0.0, 0.0], 0.0
    for (c, lin, ed, what), g in zip(cases, got):
        want = restated(c, lin, ed)
        cond = np.linalg.cond(want["A00"])
        worst_cond = max(worst_cond, cond)
        assert cond <= 1e6, (what, cond)
        assert g["valid"] == 1 and want["valid"] == 1, what
        assert g["n_ties"] == want["n_ties"], what
        H = np.array(g["H"]).reshape(6, 6)
        assert np.array_equal(H, H.T), what
        dev = ref.deviation(g, want)
        print(f"{what}: cond {cond:.2e}  dH {dev[0]:.2e}  db {dev[1]:.2e}  df {dev[2]:.2e}")
        worst = [max(a, b) for a, b in zip(worst, dev)]
        # the accumulated blocks themselves
        for k in ("A00", "A10", "A11"):
            assert np.allclose(np.array(g[k]).reshape(6, 6), want[k], rtol=0, atol=1e-12 * max(1.0, np.abs(want[k]).max())), (what, k)
    print(f"worst deviation from the restatement: H {worst[0]:.3e}, b {worst[1]:.3e}, f {worst[2]:.3e}; worst cond(A00) {worst_cond:.3e}")
    assert max(worst) <= 1e-9, worst


def test_terms_that_do_not_touch_pose_0_change_nothing(exe):
    rng = np.random.default_rng(2150)
    c = base.window_case(rng, 3, [False, True, True], prior=base.LOOSE, cond=1e2, scale=1e3)
    poses = poses_of(c)
    lin0 = [lin_ref.random_linear(rng, 0, poses[0])]
    e01 = [edge_ref.random_edge(rng, 0, 1, poses)]
    lin_all = [lin_ref.random_linear(rng, 1, poses[1])] + lin0 + [lin_ref.random_linear(rng, 2, poses[2])]
    e_all = [edge_ref.random_edge(rng, 1, 2, poses)] + e01
    bare = dict(c, has_Z=[False, True, False])
    a, b = run(exe, [case_vals(c, lin_all, e_all), case_vals(bare, lin0, e01)])
    assert a == b


def test_elimination_identity(exe):
    rng = np.random.default_rng(2200)
    W = 4
    c = base.window_case(rng, W, [False, True, True, True], prior=base.LOOSE, cond=1e2, n_it=1)
    poses, Z = poses_of(c), list(zip(c["ZR"], c["Zt"]))
    edges = [edge_ref.random_edge(rng, 0, 1, poses), edge_ref.random_edge(rng, 1, 3, poses)]
    icp = [base.ref_hessian(c["sums"][0][i], c["R"][i], c["gz"], 0, 1, 0.0, 0.0)[:3] for i in range(W)]
    full, _, _ = edge_ref.iteration(poses, icp, c["has_Z"], Z, c["Wb"], c["prior"], c["damping"], [], edges)
    g = run(exe, [case_vals(c, [], edges)])[0]
    assert g["valid"] == 1 and g["n_ties"] == 2
    rest_edges = [dict(edges[1], a=0, b=2)]
    hz, Zr = [False] + c["has_Z"][2:], Z[1:]
    with_m, _, _ = edge_ref.iteration(poses[1:], icp[1:], hz, Zr, c["Wb"], np.zeros(6), c["damping"], [ref.as_linear(g, poses[1])], rest_edges)
    without, _, _ = edge_ref.iteration(poses[1:], icp[1:], hz, Zr, c["Wb"], np.zeros(6), c["damping"], [], rest_edges)
    worst = [max(lin_ref.pose_error(with_m[i], full[i + 1])[k] for i in range(W - 1)) for k in (0, 1)]
    apart = max(lin_ref.pose_error(without[i], full[i + 1])[1] for i in range(W - 1))
    print(f"reduced step with the marginal against the full step: {worst[0]:.3e} rad, {worst[1]:.3e} m; without the marginal {apart:.3e} m")
    assert apart > 1e-6, apart
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9, worst


def test_no_positive_pivot_gives_valid_0_and_zeros(exe):
    rng = np.random.default_rng(2300)
    c = base.window_case(rng, 2, [False, False], prior=np.zeros(6), damping=0.0)
    c["have"] = [False, True]
    g = run(exe, [case_vals(c, [], [])])[0]
    assert g["valid"] == 0 and g["n_ties"] == 0 and g["f"] == 0.0
    assert not np.any(np.array(g["H"])) and not np.any(np.array(g["b"]))
    assert restated(c, [], [])["valid"] == 0


def test_no_tie_leaves_a_constant(exe):
    rng = np.random.default_rng(2400)
    c = base.window_case(rng, 3, [False, False, True], prior=base.LOOSE, cond=1e2, scale=1e3)
    poses = poses_of(c)
    lin, ed = [lin_ref.random_linear(rng, 0, poses[0])], [edge_ref.random_edge(rng, 1, 2, poses)]
    g = run(exe, [case_vals(c, lin, ed)])[0]
    want = restated(c, lin, ed)
    assert g["valid"] == 1 and g["n_ties"] == 0
    assert not np.any(np.array(g["H"])) and not np.any(np.array(g["b"]))
    A00, g0 = np.array(g["A00"]).reshape(6, 6), np.array(g["g0"])
    f = g["c"] - g0 @ np.linalg.solve(A00, g0)
    assert abs(g["f"] - f) <= 1e-9 * abs(g["c"])
    assert want["n_ties"] == 0 and not np.any(want["H"]) and abs(g["f"] - want["f"]) <= 1e-9 * abs(want["c"])


# ---- ABI -------------------------------------------------------------------------------------------------------------------
MARGINAL_FUNCS = ["mh_icp_window_marginalise", "mh_icp_window_marginalise_async"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in MARGINAL_FUNCS:
        assert hasattr(L, f), f
    assert set(MARGINAL_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr
    for f in MARGINAL_FUNCS:
        assert f"int {f}(" in hdr


def test_struct_size_matches_the_header(tmp_path):
    from mimosa_amd import capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(mh_window_marginal), offsetof(mh_window_marginal, prior), offsetof(mh_window_marginal, valid), "
                   "offsetof(mh_window_marginal, n_ties), offsetof(mh_window_marginal, oldest)); return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    M = capi.WindowMarginal
    assert got == [C.sizeof(M), M.prior.offset, M.valid.offset, M.n_ties.offset, M.oldest.offset]


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out = capi.make_window_config(), capi.WindowMarginal()
    I, z, g = np.tile(np.eye(3).ravel(), 3), np.zeros(9), np.array([0.0, 0.0, -1.0])
    hz = np.zeros(3, np.int32)
    good = dict(a=0, b=1, Z=(np.eye(3), np.zeros(3)), info=np.diag([4.0] * 6))
    asym = np.diag([4.0] * 6)
    asym[1, 4] = 1.0
    nan = np.diag([4.0] * 6)
    nan[2, 2] = np.nan
    for fn in (L.mh_icp_window_marginalise, L.mh_icp_window_marginalise_async):
        for edges, code, word in [([good] * 33, capi.MH_ERR_INVALID_ARG, b"at most 32"), ([dict(good, a=1, b=1)], capi.MH_ERR_INVALID_ARG, b"pose_a"),
                                  ([dict(good, info=asym)], capi.MH_ERR_INVALID_ARG, b"symmetric"), ([dict(good, info=nan)], capi.MH_ERR_INVALID_ARG, b"not finite"),
                                  ([good, dict(good, b=2)], capi.MH_ERR_UNSUPPORTED, b"beyond pose 1"), ([good], capi.MH_ERR_INVALID_ARG, b"NULL argument")]:
            arr = capi.make_window_edge(edges)
            rc = fn(None, C.c_size_t(3), capi._p(I), capi._p(z), hz.ctypes.data_as(C.c_void_p), capi._p(I), capi._p(z), capi._p(g), C.byref(cfg), None,
                    C.c_size_t(0), arr, C.c_size_t(len(edges)), C.byref(out))
            assert rc == code, word
            assert word in L.mh_last_error(None), (word, L.mh_last_error(None))
