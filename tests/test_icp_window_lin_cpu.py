"""CPU: the linear-factor phases of mh_icp_window_optimise_lin (mimosa_amd/csrc/window_device.hpp, compiled by g++ through
tests/cpp/window_lin_step.cpp): no linear factor is window_advance / window_advance_relin bit for bit; the chain against a
numpy restatement written independently of the header (tests/window_lin_ref.py); the carried model to first order; the ABI
additions.

Bars.  Poses after each of 4 iterations against the restatement: 1e-9 rad / 1e-9 m, the project's bar for this chain.  The
systems here have condition numbers up to about 1e6 (the loose prior of the replay, factors of scale 1 .. 1e4, the between
weights 2.5e5 / 1e4) and steps of a few 1e-2, so an unrefined numpy.linalg.solve is good to about 1e-11 per iteration.
The model: with x(xi) = local(L, retract(T, xi)) the translation part of x is exactly d_t + Exp(d_r) xi_t and the rotation part
d_r + Jr^-1(d_r) xi_r + O(|d| |xi|^2) with a constant below 1, so the stored quadratic at x(xi) differs from the carried one at
xi by at most 2 |b + H d| |xi|^2 (the gradient times the neglected curvature) plus |H| terms of third order; held to
2 |b + H d| |xi|^2 + 1e-13 max(1, |q|) at |xi| = 1e-6, where the first-order term 2 bo . xi it confirms is 1e4 times the bar."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_icp_window_cpu as base
import test_icp_window_relin_cpu as relin_base
import window_lin_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELIN = (1.75e-2, 5e-3)


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("window_lin_step")


@pytest.fixture(scope="module")
def exe_plain():
    from mimosa_amd import build
    return build.build_host_test("window_step")


@pytest.fixture(scope="module")
def exe_relin():
    from mimosa_amd import build
    return build.build_host_test("window_relin_step")


def lin_vals(linear):
    vals = [float(len(linear))]
    for l in linear:
        vals += [float(l["pose"])] + list(np.asarray(l["at"][0]).ravel()) + list(l["at"][1]) + list(np.asarray(l["H"]).ravel()) + list(l["b"]) + [l["f"]]
    return vals


def chain_vals(c, linear, relin=None):
    head = [0.0, 0.0, 0.0] if relin is None else [1.0, relin[0], relin[1]]
    return head + lin_vals(linear) + relin_base.chain_vals(c, (0.0, 0.0))[2:]


def run(exe, cases):
    return relin_base.run(exe, cases)


def mixed_cases(rng, W):
    cases = []
    for i in range(6):
        pat = base.patterns(rng, W)[i % 3]
        cases.append(base.window_case(rng, W, pat, prior=base.TIGHT if i % 2 else base.LOOSE, reg4=i % 2, n_it=5, eps=1e-7 if i == 5 else 0.0))
    empty = base.window_case(rng, W, [True] * W, n_it=4)
    empty["have"][W // 2] = False
    cases.append(empty)
    return cases


@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_no_linear_factor_is_window_advance_bit_for_bit(exe, exe_plain, W):
    cases = mixed_cases(np.random.default_rng(700 + W), W)
    want = base.run_cases(exe_plain, cases)
    got = run(exe, [(1, chain_vals(c, [])) for c in cases])
    for gc, rc in zip(got, want):
        assert len(gc) == len(rc)
        for g, r in zip(gc, rc):
            assert g["flags"] == r["flags"] and g["row"] == r["row"]
            if "xi" in r:
                assert g["xi"] == r["xi"] and g["H"] == r["H"] and g["cost"] == r["cost"] and g["ok"] == r["ok"]


@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_no_linear_factor_with_thresholds_is_window_advance_relin_bit_for_bit(exe, exe_relin, W):
    cases = mixed_cases(np.random.default_rng(800 + W), W)
    want = run(exe_relin, [(3, relin_base.chain_vals(c, RELIN)) for c in cases])
    got = run(exe, [(1, chain_vals(c, [], RELIN)) for c in cases])
    kept = 0
    for c, gc, rc in zip(cases, got, want):
        assert len(gc) == len(rc)
        for g, r in zip(gc, rc):
            assert g["flags"] == r["flags"] and g["row"] == r["row"]
            if "xi" in r:
                assert g["xi"] == r["xi"] and g["H"] == r["H"] and g["cost"] == r["cost"] and g["ok"] == r["ok"]
                assert g["eval"] == r["eval"] and g["next"] == r["next"]
                kept += g["eval"] != int(base.mask(c["have"]))
    assert kept or W == 1  # the thresholds kept some factor somewhere: the relin phases ran


def linear_sets(rng, c):
    """the linear factors of a case: between 1 and 32, two or more sharing a pose, one on a pose without an ICP factor"""
    W = c["W"]
    T = list(zip(c["R"], c["t"]))
    n = int(rng.integers(1, 33))
    poses = [int(p) for p in rng.integers(0, W, n)]
    if n >= 2:
        poses[1] = poses[0]  # two on one pose
    return [ref.random_linear(rng, p, T[p]) for p in poses]


def restated(c, linear, n_it):
    poses = list(zip(c["R"], c["t"]))
    Z = list(zip(c["ZR"], c["Zt"]))
    out = []
    for it in range(n_it):
        icp = []
        for i in range(c["W"]):
            if not c["have"][i]:
                icp.append(None)
                continue
            H, b, f, _, _ = base.ref_hessian(c["sums"][it][i], poses[i][0], c["gz"], c["reg4"][i], c["project"][i], c["thresh_rot"][i], c["thresh_trans"][i])
            icp.append((H, b, f))
        poses, xi, cost = ref.iteration(poses, icp, c["has_Z"], Z, c["Wb"], c["prior"], c["damping"], linear)
        out.append((poses, xi, cost))
    return out


@pytest.mark.parametrize("W", [1, 2, 3, 5, 16])
def test_chain_matches_the_numpy_restatement(exe, W):
    rng = np.random.default_rng(900 + W)
    cases, lins = [], []
    for i in range(8):
        pat = base.patterns(rng, W)[1 if i < 2 else i % 3]
        # (the 4-DoF projection leaves a factor's rotation block with rank 1: only where between factors tie every pose, or the
        # damping of 1e-9 alone would hold two rotation directions and no two solvers agree to 1e-9)
        c = base.window_case(rng, W, pat, prior=base.LOOSE, reg4=int(i % 2 == 1 and all(pat[1:])), n_it=4, cond=1e2)
        if i % 3 == 2 or i == 0:
            c["have"][int(rng.integers(0, W))] = False  # a pose without an ICP factor
        lin = linear_sets(rng, c)
        if i == 0:  # 32 factors, one of them on the pose of the empty ICP factor
            lin = [ref.random_linear(rng, j % W, (c["R"][j % W], c["t"][j % W])) for j in range(32)]
        if not all(c["have"]):
            e = c["have"].index(False)
            lin[-1] = ref.random_linear(rng, e, (c["R"][e], c["t"][e]))
        if i == 1:
            lin = lin[:1]
        cases.append(c)
        lins.append(lin)
    assert any(len(l) == 32 for l in lins) and any(len(l) == 1 for l in lins)
    assert any(not all(c["have"]) and any(not c["have"][l["pose"]] for l in lin) for c, lin in zip(cases, lins))
    assert W == 1 or any(len(l) > len({q["pose"] for q in l}) for l in lins)
    got = run(exe, [(1, chain_vals(c, lin)) for c, lin in zip(cases, lins)])
    bare = run(exe, [(1, chain_vals(c, [])) for c in cases])
    worst = [0.0, 0.0]
    for c, lin, g, g0 in zip(cases, lins, got, bare):
        want = restated(c, lin, 4)
        for it in range(4):
            assert g[it]["flags"] == 0 and g[it]["ok"] == 1
            row = np.array(g[it]["row"])
            for i in range(W):
                T = (row[8 + 12 * i:17 + 12 * i].reshape(3, 3), row[17 + 12 * i:20 + 12 * i])
                er, et = ref.pose_error(T, want[it][0][i])
                worst = [max(worst[0], er), max(worst[1], et)]
            assert abs(g[it]["cost"] - want[it][2]) <= 1e-9 * max(1.0, abs(want[it][2]))
        # the linear factors moved the answer: the bar below tests something
        moved = max(np.abs(np.array(g[3]["row"])[8:] - np.array(g0[3]["row"])[8:]))
        assert moved > 1e-6, moved
    print(f"W={W}: worst deviation from the restatement {worst[0]:.3e} rad, {worst[1]:.3e} m")
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9, worst


def test_thresholds_zero_with_linear_factors_is_the_plain_chain_bit_for_bit(exe):
    """thresholds of 0 evaluate every factor in every iteration: the relin instantiation then carries the linear factors exactly
    as the plain one does"""
    rng = np.random.default_rng(31)
    W = 3
    c = base.window_case(rng, W, [True] * W, prior=base.LOOSE, n_it=4, cond=1e2)
    lin = [ref.random_linear(rng, i, (c["R"][i], c["t"][i])) for i in (0, 1, 1, 2)]
    plain = run(exe, [(1, chain_vals(c, lin))])[0]
    zero = run(exe, [(1, chain_vals(c, lin, (0.0, 0.0)))])[0]
    for g, r in zip(zero, plain):
        assert g["row"] == r["row"] and g["xi"] == r["xi"] and g["cost"] == r["cost"]


def test_carried_model_agrees_with_the_stored_one_to_first_order(exe):
    rng = np.random.default_rng(41)
    cases, meta = [], []
    for n in range(40):
        T = base.random_pose(rng)
        l = ref.random_linear(rng, 0, T)
        cases.append((0, list(l["at"][0].ravel()) + list(l["at"][1]) + list(T[0].ravel()) + list(T[1]) + list(l["H"].ravel()) + list(l["b"]) + [l["f"]]))
        meta.append((T, l))
    first_order = []
    for (T, l), g in zip(meta, run(exe, cases)):
        H, b, f, L = l["H"], l["b"], l["f"], l["at"]
        d = ref.local(L, T)
        assert np.abs(np.array(g["d"]) - d).max() <= 1e-14
        assert 1e-3 < np.linalg.norm(d[:3]) <= 3e-2 + 1e-12 and np.linalg.norm(d[3:]) <= 2e-2 + 1e-12
        Ho, bo, fo = np.array(g["H"]).reshape(6, 6), np.array(g["b"]), g["f"]
        for _ in range(4):
            xi = rng.standard_normal(6)
            xi *= 1e-6 / np.linalg.norm(xi)
            x = ref.local(L, ref.retract(T, xi))
            stored = f + 2.0 * b @ x + x @ H @ x
            carried = fo + 2.0 * bo @ xi + xi @ Ho @ xi
            bar = 2.0 * np.linalg.norm(b + H @ d) * 1e-12 + 1e-13 * max(1.0, abs(stored))
            assert abs(stored - carried) <= bar, (abs(stored - carried), bar)
            first_order.append(abs(2.0 * bo @ xi) / bar)
    assert np.median(first_order) > 1e2  # the term the check confirms stands far above its bar


# ---- ABI -------------------------------------------------------------------------------------------------------------------
LIN_FUNCS = ["mh_icp_window_optimise_lin", "mh_icp_window_optimise_lin_async"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in LIN_FUNCS:
        assert hasattr(L, f), f
    assert set(LIN_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr
    for f in LIN_FUNCS:
        assert f"int {f}(" in hdr


def test_struct_size_matches_the_header(tmp_path):
    from mimosa_amd import capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   "sizeof(mh_window_linear_factor), offsetof(mh_window_linear_factor, L_R), offsetof(mh_window_linear_factor, H), "
                   "offsetof(mh_window_linear_factor, f), MH_WINDOW_LINEAR_MAX); return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    F = capi.WindowLinearFactor
    assert got == [C.sizeof(F), F.L_R.offset, F.H.offset, F.f.offset, capi.MH_WINDOW_LINEAR_MAX]


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out = capi.make_window_config(), capi.WindowResult()
    I, z, g = np.eye(3).ravel().copy(), np.zeros(3), np.array([0.0, 0.0, -1.0])
    hz = np.zeros(1, np.int32)
    for fn in (L.mh_icp_window_optimise_lin, L.mh_icp_window_optimise_lin_async):
        rc = fn(None, C.c_size_t(1), capi._p(I), capi._p(z), hz.ctypes.data_as(C.c_void_p), capi._p(I), capi._p(z), capi._p(g), C.byref(cfg), None, None,
                C.c_size_t(0), C.byref(out), None, None)
        assert rc == capi.MH_ERR_INVALID_ARG
        assert b"NULL" in L.mh_last_error(None)
