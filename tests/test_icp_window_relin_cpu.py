"""CPU: the relinearization phases of mh_icp_window_optimise_relin (mimosa_amd/csrc/window_device.hpp, compiled by g++ through
tests/cpp/window_relin_step.cpp): the inverse right Jacobian, the kept model carried to the current pose, the decision rule, the
thresholds-0 identity with window_advance, and the ABI additions.

Bars.  Jr^-1 against its defining property, Exp(phi + Jr^-1(phi) x) = Exp(phi) Exp(x) + O(|x|^2), by central differences in x
(step 1e-5: truncation 1e-10 relative, rounding 1e-11) held to 1e-8, and against numpy's closed form in longdouble to 1e-14 on
both sides of the series' switch point (1e-2 rad).  The transported gradient and Hessian against central finite differences of
the model cost c(xi) = f + 2 b^T x + x^T H x, x = local(L, T retract xi), written in numpy: the gradient (c'(0) / 2) to 1e-7 |b|
and the Hessian (c''(0) / 2) to 1e-5 |H| — x is not linear in xi, so the second difference of c differs from M^T H M by the
curvature of x times the gradient, (b + H d) . d^2 x, which is of order |d| |b + H d|; the test model has its minimum near d, where
that term is below the bar (Gauss-Newton drops it by construction).  The cost: 1e-13 relative.  Thresholds 0: rows, flags and
steps equal to window_advance's, bit for bit.  The decision: exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import test_icp_window_cpu as base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("window_relin_step")


@pytest.fixture(scope="module")
def exe_plain():
    from mimosa_amd import build
    return build.build_host_test("window_step")


def run(exe, cases):
    toks = [str(len(cases))]
    for kind, vals in cases:
        toks += [str(kind)] + [repr(float(v)) for v in vals]
    out = subprocess.run([exe], input=" ".join(toks), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def chain_vals(c, relin):
    """a window_case of test_icp_window_cpu in the driver's order, behind the two thresholds"""
    W = c["W"]
    vals = [relin[0], relin[1], float(W), base.mask(c["has_Z"]), base.mask(c["have"]), base.mask(c["reg4"]), base.mask(c["project"])]
    vals += list(c["gz"]) + list(c["Wb"]) + list(c["prior"]) + [c["damping"], c["eps_rot"], c["eps_trans"]] + list(c["thresh_rot"]) + list(c["thresh_trans"])
    for i in range(W):
        vals += list(np.asarray(c["R"][i]).ravel()) + list(c["t"][i])
    for i in range(W):
        vals += list(np.asarray(c["ZR"][i]).ravel()) + list(c["Zt"][i])
    vals.append(float(len(c["sums"])))
    for it in c["sums"]:
        for s in it:
            vals += list(s)
    return vals


def jrinv_ref(phi):
    phi = np.asarray(phi, np.longdouble)
    th = np.sqrt(phi @ phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]], np.longdouble)
    if th < 1e-4:
        c = np.longdouble(1) / 12 + th * th / 720
    else:
        c = 1 / (th * th) - (1 + np.cos(th)) / (2 * th * np.sin(th))
    return (np.eye(3, dtype=np.longdouble) + K / 2 + c * (K @ K)).astype(np.float64)


def local(L, T):
    return np.concatenate([base.so3log(L[0].T @ T[0]), L[0].T @ (T[1] - L[1])])


def retract(T, xi):
    return T[0] @ base.rodrigues(xi[:3]), T[1] + T[0] @ xi[3:]


ANGLES = [0.0, 1e-12, 1e-6, 9.9e-3, 9.999999e-3, 1.0000001e-2, 1.01e-2, 0.03, 0.05]  # the switch point of the series is 1e-2


def test_jrinv_against_closed_form_and_finite_differences(exe):
    rng = np.random.default_rng(1)
    phis = []
    for th in ANGLES:
        for _ in range(3):
            ax = rng.standard_normal(3)
            phis.append(ax / np.linalg.norm(ax) * th)
    got = run(exe, [(0, list(np.eye(6).ravel()) + [0.0] * 6 + [0.0] + list(p) + [0.0] * 3) for p in phis])
    h = 1e-5
    for p, g in zip(phis, got):
        J = np.array(g["J"]).reshape(3, 3)
        assert np.abs(J - jrinv_ref(p)).max() <= 1e-14, p
        # d/dx Log(Exp(phi)^T ... ): Exp(phi + J x) = Exp(phi) Exp(x) to first order, column by column
        for k in range(3):
            x = np.zeros(3)
            x[k] = h
            fd = (base.so3log(base.rodrigues(p) @ base.rodrigues(x)) - base.so3log(base.rodrigues(p) @ base.rodrigues(-x))) / (2 * h)
            assert np.abs(fd - J[:, k]).max() <= 1e-8, (p, k)
        assert np.abs(np.array(g["E"]).reshape(3, 3) - base.rodrigues(p)).max() <= 1e-15


def test_transport_against_finite_differences_of_the_model_cost(exe):
    rng = np.random.default_rng(2)
    cases, meta = [], []
    for n, th in enumerate(ANGLES[2:] * 2):
        ax = rng.standard_normal(3)
        dr = ax / np.linalg.norm(ax) * min(th, 0.05)
        dt = rng.uniform(-0.05, 0.05, 3)
        d = np.concatenate([dr, dt])
        H = base.spd(rng, 1e3, 1e2)
        b = -H @ d + rng.standard_normal(6) * 1e-4 * np.sqrt(np.abs(H).max())  # the model's minimum sits near d (see the docstring)
        f = 3.0 + n
        L = base.random_pose(rng)
        cases.append((0, list(H.ravel()) + list(b) + [f] + list(d)))
        meta.append((H, b, f, d, L))
    got = run(exe, cases)
    for (H, b, f, d, L), g in zip(meta, got):
        T = retract(L, d)  # first order in t exactly as the chain retracts; Exp in the rotation
        assert np.abs(local(L, T) - d).max() <= 1e-15

        def cost(xi):
            x = local(L, retract(T, xi))
            return f + 2.0 * b @ x + x @ H @ x

        Ho, bo = np.array(g["H"]).reshape(6, 6), np.array(g["b"])
        assert abs(g["f"] - cost(np.zeros(6))) <= 1e-13 * max(1.0, abs(g["f"]))
        h = 1e-5
        grad = np.array([(cost(h * e) - cost(-h * e)) / (2 * h) for e in np.eye(6)]) / 2.0
        assert np.abs(grad - bo).max() <= 1e-7 * max(np.abs(b).max(), np.abs(H @ d).max()), d
        h = 1e-3
        hess = np.zeros((6, 6))
        for i, ei in enumerate(np.eye(6)):
            for j, ej in enumerate(np.eye(6)):
                hess[i, j] = (cost(h * (ei + ej)) - cost(h * (ei - ej)) - cost(h * (ej - ei)) + cost(-h * (ei + ej))) / (4 * h * h) / 2.0
        assert np.abs(hess - Ho).max() <= 1e-5 * np.abs(H).max(), (d, np.abs(hess - Ho).max() / np.abs(H).max())
        assert np.abs(Ho - Ho.T).max() <= 1e-13 * np.abs(H).max()


def test_zero_offset_leaves_the_model_untouched(exe):
    rng = np.random.default_rng(3)
    H, b = base.spd(rng, 1e6, 10.0), rng.standard_normal(6)
    g = run(exe, [(0, list(H.ravel()) + list(b) + [7.25] + [0.0] * 6)])[0]
    assert np.array_equal(np.array(g["H"]).reshape(6, 6), H) and np.array_equal(np.array(g["b"]), b) and g["f"] == 7.25


def test_decision_rule_is_componentwise_and_strict(exe):
    rr, rt = 1.75e-2, 5.0e-3
    cases, want = [], []
    for k in range(6):
        thr = rr if k < 3 else rt
        for sign in (1.0, -1.0):
            for v, ev in ((thr, 0), (np.nextafter(thr, np.inf), 1), (np.nextafter(thr, 0.0), 0)):
                d = np.zeros(6)
                d[k] = sign * v
                cases.append((1, list(d) + [rr, rt]))
                want.append(ev)
    # component-wise, not the norm: every component just inside its threshold is kept
    cases.append((1, [rr, -rr, rr, rt, rt, -rt, rr, rt]))
    want.append(0)
    # a rotation component between the two thresholds: above the translation threshold, below its own
    cases.append((1, [1e-2, 0, 0, 0, 0, 0, rr, rt]))
    want.append(0)
    cases.append((1, [0, 0, 0, 0, 1e-2, 0, rr, rt]))
    want.append(1)
    for thr0 in ((0.0, 0.0),):
        cases.append((1, [0.0] * 6 + list(thr0)))
        want.append(0)
        cases.append((1, [0, 0, 5e-324, 0, 0, 0] + list(thr0)))
        want.append(1)
    got = run(exe, cases)
    assert [g["evaluate"] for g in got] == want


def test_local_coordinates_invert_the_retraction(exe):
    rng = np.random.default_rng(4)
    cases, ds = [], []
    for _ in range(20):
        L = base.random_pose(rng)
        d = np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.05, 0.05, 3)])
        T = retract(L, d)
        cases.append((2, list(L[0].ravel()) + list(L[1]) + list(T[0].ravel()) + list(T[1])))
        ds.append(d)
    for d, g in zip(ds, run(exe, cases)):
        assert np.abs(np.array(g["d"]) - d).max() <= 1e-14


@pytest.mark.parametrize("W", [1, 2, 5, 16])
def test_thresholds_zero_are_window_advance_bit_for_bit(exe, exe_plain, W):
    rng = np.random.default_rng(500 + W)
    cases = []
    for i in range(6):
        pat = base.patterns(rng, W)[i % 3]
        c = base.window_case(rng, W, pat, prior=base.TIGHT if i % 2 else base.LOOSE, reg4=i % 2, n_it=5, eps=1e-7 if i == 5 else 0.0)
        cases.append(c)
    empty = base.window_case(rng, W, [True] * W, n_it=4)
    empty["have"][W // 2] = False
    cases.append(empty)
    ref = base.run_cases(exe_plain, cases)
    got = run(exe, [(3, chain_vals(c, (0.0, 0.0))) for c in cases])
    for c, gc, rc in zip(cases, got, ref):
        assert len(gc) == len(rc)
        for g, r in zip(gc, rc):
            assert g["flags"] == r["flags"] and g["row"] == r["row"]
            if "xi" in r:
                assert g["xi"] == r["xi"] and g["H"] == r["H"] and g["cost"] == r["cost"] and g["ok"] == r["ok"]
                assert g["eval"] == int(base.mask(c["have"]))  # every non-empty factor, every iteration


def test_kept_factors_use_the_transported_model_and_return_past_the_threshold(exe):
    """three poses without between factors, each following its own quadratic bowl: the sums fed are those of the bowl at the
    pose the chain is at, so an evaluated factor sees the truth and a kept one its stored model.  Pose 0 starts far from its
    minimum (evaluated while it moves), pose 1 at its minimum (kept after iteration 0), an empty factor beside them."""
    rng = np.random.default_rng(6)
    W = 3
    c = base.window_case(rng, W, [False] * W, n_it=1, prior=np.zeros(6), damping=1e-9)  # (the damping holds the empty factor's block)
    c["have"] = [True, True, False]
    Hs = [base.spd(rng, 1e2, 1e4) for _ in range(W)]
    x0 = [np.array([0.03, -0.02, 0.04, 0.05, -0.04, 0.03]), np.zeros(6), np.zeros(6)]
    # a Gauss-Newton step on a bowl H with b = H x lands on its minimum at once; shrink b so that it takes several iterations
    c["sums"] = [[base.pack(Hs[i], 0.5 * Hs[i] @ x0[i], 1.0) for i in range(W)] for _ in range(6)]
    got = run(exe, [(3, chain_vals(c, (1.75e-2, 5e-3)))])[0]
    assert got[0]["eval"] == 0b011
    assert got[1]["eval"] == 0b001      # pose 1 did not move: kept, its offset the rounding of L.R^T R at most
    assert np.abs(np.array(got[1]["d"]).reshape(-1, 6)[1]).max() <= 1e-15
    assert np.abs(np.array(got[1]["H"]).reshape(W, 36)[1] - np.array(got[0]["H"]).reshape(W, 36)[1]).max() <= 1e-12 * np.abs(Hs[1]).max()
    assert not np.any(np.array(got[1]["xi"]).reshape(W, 6)[1:])
    # pose 0: every evaluation sees the same b (the sums are fixed), so it keeps stepping by the same xi and is evaluated while
    # that step exceeds a threshold; the recorded offset is the step just taken
    for it in range(1, 6):
        assert got[it]["eval"] & 1
        d = np.array(got[it]["d"]).reshape(-1, 6)[0]
        xi = np.array(got[it]["xi"]).reshape(W, 6)[0]
        assert np.abs(d[:3] - xi[:3]).max() <= 1e-12 and np.abs(d[3:] - xi[3:]).max() <= 1e-12
    # the same with thresholds nothing reaches: only iteration 0 evaluates; afterwards the kept model's own Newton step
    got = run(exe, [(3, chain_vals(c, (1e9, 1e9)))])[0]
    assert [g["eval"] for g in got] == [0b011, 0, 0, 0, 0, 0]
    H0, b0 = Hs[0], 0.5 * Hs[0] @ x0[0]
    x = np.zeros(6)
    for it in range(6):
        xi = np.array(got[it]["xi"]).reshape(W, 6)[0]
        d_before = x.copy()
        if it:
            # the model's gradient at the offset, seen through M: the step solves M^T H M xi = -M^T (b + H d)
            assert np.abs(np.array(got[it]["cost"]) - (2.0 + 2 * b0 @ d_before + d_before @ H0 @ d_before)) <= 1e-9
        x = np.array(got[it]["d"]).reshape(-1, 6)[0]
    # the kept model is quadratic in L's tangent: its minimum is -H^-1 b, reached to first order by iteration 1 and held
    assert np.abs(x - np.linalg.solve(H0, -b0)).max() <= 1e-6


# ---- ABI -------------------------------------------------------------------------------------------------------------------
RELIN_FUNCS = ["mh_icp_window_optimise_relin", "mh_icp_window_optimise_relin_async"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in RELIN_FUNCS:
        assert hasattr(L, f), f
    assert set(RELIN_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr
    for f in RELIN_FUNCS:
        assert f"int {f}(" in hdr
    assert C.sizeof(capi.WindowRelin) == 16


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out, rl = capi.make_window_config(), capi.WindowResult(), capi.WindowRelin(0.0, 0.0)
    I, z, g = np.eye(3).ravel().copy(), np.zeros(3), np.array([0.0, 0.0, -1.0])
    hz = np.zeros(1, np.int32)
    for fn in (L.mh_icp_window_optimise_relin, L.mh_icp_window_optimise_relin_async):
        rc = fn(None, C.c_size_t(1), capi._p(I), capi._p(z), hz.ctypes.data_as(C.c_void_p), capi._p(I), capi._p(z), capi._p(g), C.byref(cfg), C.byref(rl),
                C.byref(out), None, None)
        assert rc == capi.MH_ERR_INVALID_ARG
        assert b"NULL" in L.mh_last_error(None)
