"""CPU: the step arithmetic of mh_icp_window_optimise (mimosa_amd/csrc/window_device.hpp, compiled by g++ through
tests/cpp/window_step.cpp) against a numpy restatement of one iteration of WindowSmootherT::optimise, and the ABI additions.

Bars.  The assembled system (diagonal blocks, off-diagonal blocks, right-hand side) and the cost: 1e-13 |A| (|A| the largest
entry of the system) — a handful of fp64 products in another order, and acos / sin of the between residual through numpy
instead of libm.  xi: 1e-12 relative to |xi| against numpy.linalg.solve on the dense system refined with residuals in
longdouble, at condition numbers up to 1e8 with the tight (1e8) and the loose prior of the replay next to a damping of 1e-9;
the system solved is the one the header assembled.  Retracted poses: exact — the retraction is restated here in Python floats
in the header's operation order on the header's own xi.  Stop flags, the frozen poses after a stop, the singular case and the
agreement of a one-pose window with align_step: exact."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TIGHT = np.array([1e8] * 6)                                                  # 1 / (1e-4)^2: what marginalisation leaves
LOOSE = np.array([1.0 / 0.017453292519943295 ** 2] * 3 + [1.0 / 0.1 ** 2] * 3)  # while the oldest pose was never optimised
WB = np.array([1.0 / 2e-3 ** 2] * 3 + [1.0 / 1e-2 ** 2] * 3)                  # the replay's between sigmas


# ---- numpy reference -------------------------------------------------------------------------------------------------------
def pack(H, b, f, counters=(7.0, 70.0, 0.0, 35.0)):
    M = np.zeros((7, 7))
    M[:6, :6] = H
    M[:6, 6] = M[6, :6] = b
    M[6, 6] = f
    return np.concatenate([M[np.triu_indices(7)], np.asarray(counters, float)])


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        A, B = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + A * K + B * (K @ K)


def so3log(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    th = np.arccos(c)
    s = 0.5 if th < 1e-9 else th / (2.0 * np.sin(th))
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * s


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def adjoint(R, t):
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def degenerate(block, thresh):
    w = np.linalg.eigh(block)[0]
    with np.errstate(invalid="ignore"):
        return not bool(np.all(np.sqrt(w) > thresh))


def ref_hessian(sums, R, gz, reg4, project, thresh_rot, thresh_trans):
    M = np.zeros((7, 7))
    M[np.triu_indices(7)] = sums[:28]
    M = M + np.triu(M, 1).T
    H, b, f = M[:6, :6].copy(), M[:6, 6].copy(), M[6, 6]
    rd, td = degenerate(H[:3, :3], thresh_rot), degenerate(H[3:, 3:], thresh_trans)
    if reg4:
        lz = R.T @ np.asarray(gz)
        Pi = np.outer(lz, lz)
        Hrr, Hrt, Htr = H[:3, :3].copy(), H[:3, 3:].copy(), H[3:, :3].copy()
        H[:3, :3], H[:3, 3:], H[3:, :3] = Pi @ Hrr @ Pi, Pi @ Hrt, Htr @ Pi
        b[:3] = Pi @ b[:3]
    if project and (rd or td):
        H[:], b[:] = 0.0, 0.0
    return H, b, f, rd, td


def ref_system(c, sums):
    """one iteration of WindowSmootherT::optimise without the photometric terms: dense A, g (before the sign flip), cost"""
    W = c["W"]
    A, g, cost = np.zeros((6 * W, 6 * W)), np.zeros(6 * W), 0.0
    for i in range(W):
        if not c["have"][i]:
            continue
        H, b, f, _, _ = ref_hessian(sums[i], c["R"][i], c["gz"], c["reg4"][i], c["project"][i], c["thresh_rot"][i], c["thresh_trans"][i])
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += H
        g[6 * i:6 * i + 6] += b
        cost += f
    Wb = np.diag(c["Wb"])
    for i in range(1, W):
        if not c["has_Z"][i]:
            continue
        Ra, ta, Rb, tb = c["R"][i - 1], c["t"][i - 1], c["R"][i], c["t"][i]
        abR, abt = Ra.T @ Rb, Ra.T @ (tb - ta)
        ZR, Zt = c["ZR"][i], c["Zt"][i]
        r = np.concatenate([so3log(ZR.T @ abR), ZR.T @ (abt - Zt)])
        Ja, Jb = -adjoint(abR.T, abR.T @ (-abt)), np.eye(6)
        a, b = slice(6 * (i - 1), 6 * i), slice(6 * i, 6 * i + 6)
        A[a, a] += Ja.T @ Wb @ Ja
        A[a, b] += Ja.T @ Wb @ Jb
        A[b, a] += Jb.T @ Wb @ Ja
        A[b, b] += Wb
        g[a] += Ja.T @ Wb @ r
        g[b] += Wb @ r
        cost += r @ Wb @ r
    A[:6, :6] += np.diag(c["prior"])
    A += c["damping"] * np.eye(6 * W)
    return A, g, cost


def dense(got, W):
    A = np.zeros((6 * W, 6 * W))
    gA, gE = np.array(got["A"]).reshape(W, 6, 6), np.array(got["E"]).reshape(W, 6, 6)
    for i in range(W):
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = gA[i]
        if i:
            A[6 * i:6 * i + 6, 6 * i - 6:6 * i] = gE[i]
            A[6 * i - 6:6 * i, 6 * i:6 * i + 6] = gE[i].T
    return A


def solve_refined(A, rhs):
    x = np.linalg.solve(A, rhs)
    Al, rl = A.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(4):
        r = (rl - Al @ x.astype(np.longdouble)).astype(np.float64)
        x = x + np.linalg.solve(A, r)
    return x


def retract_exact(R, t, xi):
    """align_retract / align_expmap in Python floats, operation for operation"""
    R, t, w = [float(v) for v in np.asarray(R).ravel()], [float(v) for v in t], [float(v) for v in xi]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = math.sqrt(th2)
    K = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    if th < 1e-10:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    E = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    for i in range(3):
        for j in range(3):
            kk = 0.0
            for m in range(3):
                kk += K[3 * i + m] * K[3 * m + j]
            E[3 * i + j] += A * K[3 * i + j] + B * kk
    tn = [t[i] + (R[3 * i] * w[3] + R[3 * i + 1] * w[4] + R[3 * i + 2] * w[5]) for i in range(3)]
    Rn = [R[3 * i] * E[j] + R[3 * i + 1] * E[3 + j] + R[3 * i + 2] * E[6 + j] for i in range(3) for j in range(3)]
    return np.array(Rn).reshape(3, 3), np.array(tn)


# ---- driver ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("window_step")


def mask(bits):
    return float(sum(1 << i for i, b in enumerate(bits) if b))


def run_cases(exe, cases):
    toks = [str(len(cases))]
    for c in cases:
        W = c["W"]
        vals = [float(W), mask(c["has_Z"]), mask(c["have"]), mask(c["reg4"]), mask(c["project"])] + list(c["gz"]) + list(c["Wb"]) + list(c["prior"])
        vals += [c["damping"], c["eps_rot"], c["eps_trans"]] + list(c["thresh_rot"]) + list(c["thresh_trans"])
        for i in range(W):
            vals += list(np.asarray(c["R"][i]).ravel()) + list(c["t"][i])
        for i in range(W):
            vals += list(np.asarray(c["ZR"][i]).ravel()) + list(c["Zt"][i])
        vals.append(float(len(c["sums"])))
        for it in c["sums"]:
            for s in it:
                vals += list(s)
        toks += [repr(float(v)) for v in vals]
    out = subprocess.run([exe], input=" ".join(toks), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def spd(rng, cond, scale):
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    lam = scale * np.logspace(0, np.log10(cond), 6)[rng.permutation(6)]
    H = (Q * lam) @ Q.T
    return (H + H.T) / 2


def random_pose(rng, rot=0.7, trans=3.0):
    return rodrigues(rng.standard_normal(3) * rot), rng.standard_normal(3) * trans


def window_case(rng, W, has_Z, prior=TIGHT, cond=1e3, scale=None, reg4=0, project=1, n_it=1, eps=0.0, have=None, thresh=0.0, damping=1e-9):
    """random SPD sums, a random trajectory, between measurements a few degrees / centimetres off the poses' own"""
    R, t = [], []
    Rk, tk = random_pose(rng)
    for i in range(W):
        dR, dt = random_pose(rng, 0.1, 0.5)
        Rk, tk = Rk @ dR, tk + Rk @ dt
        R.append(Rk)
        t.append(tk)
    ZR, Zt = [np.eye(3)], [np.zeros(3)]
    for i in range(1, W):
        nR, nt = random_pose(rng, 0.02, 0.03)
        ZR.append(R[i - 1].T @ R[i] @ nR)
        Zt.append(R[i - 1].T @ (t[i] - t[i - 1]) + nt)
    sums = []
    for it in range(n_it):
        row = []
        for i in range(W):
            H = spd(rng, cond, (10.0 ** rng.uniform(0, 4)) if scale is None else scale)
            b = H @ (rng.standard_normal(6) * 0.05) + rng.standard_normal(6) * 1e-3 * np.sqrt(np.abs(H).max())
            row.append(pack(H, b, 3.0 + i + it))
        sums.append(row)
    return dict(W=W, has_Z=[False] + [bool(z) for z in has_Z[1:]], have=[True] * W if have is None else have, reg4=[reg4] * W, project=[project] * W,
                gz=(0.0, 0.0, 1.0), Wb=WB, prior=prior, damping=damping, eps_rot=eps, eps_trans=eps, thresh_rot=[thresh] * W, thresh_trans=[thresh] * W,
                R=R, t=t, ZR=ZR, Zt=Zt, sums=sums)


def patterns(rng, W):
    return [[False] * W, [True] * W, list(rng.integers(0, 2, W).astype(bool))]


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 5, 16])
def test_assembled_system_matches_numpy(exe, W):
    rng = np.random.default_rng(300 + W)
    cases = []
    for reg4 in (0, 1):
        for prior in (TIGHT, LOOSE):
            for pat in patterns(rng, W):
                cases.append(window_case(rng, W, pat, prior=prior, reg4=reg4))
    empty = window_case(rng, W, [True] * W)
    empty["have"][W // 2] = False  # an empty factor contributes nothing
    cases.append(empty)
    got = run_cases(exe, cases)
    for c, g in zip(cases, got):
        A, gr, cost = ref_system(c, c["sums"][0])
        sA = np.abs(A).max()
        assert np.abs(dense(g[0], W) - A).max() <= 1e-13 * sA
        assert np.abs(-np.array(g[0]["rhs"]) - gr).max() <= 1e-13 * sA
        assert abs(g[0]["cost"] - cost) <= 1e-13 * sA
        assert g[0]["row"][0] == g[0]["cost"]
    assert not np.any(np.array(got[-1][0]["H"]).reshape(W, 36)[W // 2])


@pytest.mark.parametrize("W", [1, 2, 3, 5, 16])
def test_step_matches_refined_solve(exe, W):
    """the step against the refined dense solve of the assembled system, condition numbers up to 1e8: the tight prior (1e8)
    beside a damping of 1e-9 and factors whose smallest eigenvalue is of order one; retracted poses exact"""
    rng = np.random.default_rng(400 + W)
    cases = []
    for i in range(12):
        pat = patterns(rng, W)[i % 3]
        if W == 1 and i % 2:  # one pose: the factor's own condition number, held by the damping alone
            c = window_case(rng, W, pat, prior=np.zeros(6), cond=10.0 ** (1 + i % 8), scale=1e2)
        else:  # smallest eigenvalue of every factor 1, the oldest pose under its prior
            c = window_case(rng, W, pat, prior=TIGHT if i % 2 == 0 else LOOSE, cond=10.0 ** (1 + i % 4), scale=1.0)
        cases.append(c)
    got = run_cases(exe, cases)
    worst = 0.0
    for c, g in zip(cases, got):
        g = g[0]
        A = dense(g, W)
        cond = np.linalg.cond(A)
        worst = max(worst, cond)
        assert cond <= 1.05e8, cond
        assert g["ok"] == 1 and g["flags"] == 0
        rhs, gxi = np.array(g["rhs"]), np.array(g["xi"])
        xi = solve_refined((A + A.T) / 2, rhs)
        n = np.linalg.norm(xi)
        assert np.linalg.norm(gxi - xi) <= 1e-12 * n, (np.linalg.norm(gxi - xi) / n, cond)
        row = np.array(g["row"])
        for i in range(W):
            Rn, tn = retract_exact(c["R"][i], c["t"][i], gxi[6 * i:6 * i + 6])
            assert np.array_equal(row[8 + 12 * i:17 + 12 * i].reshape(3, 3), Rn) and np.array_equal(row[17 + 12 * i:20 + 12 * i], tn)
            assert np.abs(Rn.T @ Rn - np.eye(3)).max() <= 1e-14
        nr, nt = np.linalg.norm(gxi.reshape(W, 6)[:, :3], axis=1), np.linalg.norm(gxi.reshape(W, 6)[:, 3:], axis=1)
        assert abs(row[1] - nr.max()) <= 4e-16 * max(1.0, row[1]) and abs(row[2] - nt.max()) <= 4e-16 * max(1.0, row[2])
    assert worst >= 1e7  # the hard end of the range is in the set


def test_one_pose_window_is_align_step_bit_for_bit(exe):
    rng = np.random.default_rng(7)
    cases = []
    for i in range(24):
        pr = np.array([10.0 ** rng.uniform(0, 8)] * 3 + [10.0 ** rng.uniform(0, 8)] * 3) if i % 3 else np.zeros(6)
        c = window_case(rng, 1, [False], prior=pr, cond=10.0 ** (1 + i % 7), reg4=i % 2, eps=1.0 if i % 4 == 0 else 0.0, thresh=0.5 * (i % 5 == 0),
                        damping=0.0 if i % 2 else 1e-9)
        cases.append(c)
    got = run_cases(exe, cases)
    conv = 0
    for g in got:
        g = g[0]
        row = np.array(g["row"])
        assert g["xi"] == g["align_xi"] or not g["ok"]
        assert np.array_equal(row[8:17], np.array(g["align_R"])) and np.array_equal(row[17:20], np.array(g["align_t"]))
        assert (int(row[3]) & 4) == (g["align_bits"] & 4) and int(row[4]) == (g["align_bits"] & 3)
        assert bool(g["flags"] & 2) == bool(g["align_converged"])
        conv += g["align_converged"]
    assert 0 < conv < len(got)


def test_chain_stops_when_every_pose_has_converged_and_freezes(exe):
    """sums of a quadratic bowl whose gradient shrinks per iteration: the stop needs EVERY pose below eps; the rows queued behind
    the stop carry the same poses bit for bit and flag 4, whatever sums they are fed"""
    rng = np.random.default_rng(21)
    W = 3
    c = window_case(rng, W, [False] * W, n_it=1, eps=1e-6, prior=np.zeros(6))  # no between factor: every pose follows its own factor
    H = [spd(rng, 1e2, 1e4) for _ in range(W)]
    state = [rng.standard_normal(6) * 0.02 for _ in range(W)]
    shrink = [0.01, 0.01, 0.2]  # the last pose converges later than the others
    seq = []
    for it in range(16):
        seq.append([pack(H[i], H[i] @ state[i], float(state[i] @ H[i] @ state[i])) for i in range(W)])
        state = [s * k for s, k in zip(state, shrink)]
    c["sums"] = seq
    got = run_cases(exe, [c])[0]
    stopped_at, partial = None, False
    for it, g in enumerate(got):
        row = np.array(g["row"])
        if stopped_at is not None:
            assert g["flags"] == 7 and "xi" not in g
            assert np.array_equal(row[8:], np.array(got[stopped_at]["row"])[8:]) and row[6] == stopped_at + 1
            continue
        xi = np.array(g["xi"]).reshape(W, 6)
        nr, nt = np.linalg.norm(xi[:, :3], axis=1), np.linalg.norm(xi[:, 3:], axis=1)
        conv = bool(np.all(nr < 1e-6) and np.all(nt < 1e-6))
        assert g["flags"] == (3 if conv else 0) and row[6] == it + 1
        partial = partial or (not conv and bool(np.any((nr < 1e-6) & (nt < 1e-6))))
        if conv:
            stopped_at = it
    assert partial  # some poses were below eps while the chain went on
    assert stopped_at is not None and 3 <= stopped_at < 15


def test_singular_system_takes_no_step_and_stops(exe):
    """degenerate sums with project_on_degeneracy (H = b = 0), no between factor, no prior, no damping: no positive pivot"""
    rng = np.random.default_rng(33)
    W = 3
    c = window_case(rng, W, [False] * W, prior=np.zeros(6), damping=0.0, n_it=3, thresh=1e9)
    got = run_cases(exe, [c])[0]
    poses = np.concatenate([np.concatenate([c["R"][i].ravel(), c["t"][i]]) for i in range(W)])
    assert got[0]["flags"] == 1 and int(got[0]["row"][3]) == 4 and got[0]["ok"] == 0
    assert int(got[0]["row"][4]) == sum(3 << (2 * i) for i in range(W))
    assert [g["flags"] for g in got[1:]] == [5, 5]
    for g in got:
        assert np.array_equal(np.array(g["row"])[8:], poses) and g["row"][6] == 1.0 and g["row"][1] == 0.0 and g["row"][2] == 0.0
    # the same sums held by prior and damping: a zero step, exactly, and no stop with eps = 0
    c2 = dict(c, prior=TIGHT, damping=1e-9)
    got = run_cases(exe, [c2])[0]
    assert [g["flags"] for g in got] == [0, 0, 0]
    for g in got:
        assert not np.any(np.array(g["xi"])) and np.array_equal(np.array(g["row"])[8:], poses)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
WINDOW_FUNCS = ["mh_icp_window_optimise", "mh_icp_window_optimise_async", "mh_icp_window_wait"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in WINDOW_FUNCS:
        assert hasattr(L, f), f
    assert set(WINDOW_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr


def test_struct_sizes_match_the_header(tmp_path):
    from mimosa_amd import capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(mh_icp_window_config), sizeof(mh_icp_window_trace), sizeof(mh_icp_window_result), offsetof(mh_icp_window_config, check_every), "
                   "offsetof(mh_icp_window_result, trace), offsetof(mh_icp_window_result, first), offsetof(mh_icp_window_result, last), MH_WINDOW_MAX); return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.WindowConfig), C.sizeof(capi.WindowTrace), C.sizeof(capi.WindowResult), capi.WindowConfig.check_every.offset,
                   capi.WindowResult.trace.offset, capi.WindowResult.first.offset, capi.WindowResult.last.offset, capi.MH_WINDOW_MAX]


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out = capi.make_window_config(), capi.WindowResult()
    I, z, g = np.eye(3).ravel().copy(), np.zeros(3), np.array([0.0, 0.0, -1.0])
    hz = np.zeros(1, np.int32)
    for fn in (L.mh_icp_window_optimise, L.mh_icp_window_optimise_async):
        rc = fn(None, C.c_size_t(1), capi._p(I), capi._p(z), hz.ctypes.data_as(C.c_void_p), capi._p(I), capi._p(z), capi._p(g), C.byref(cfg), C.byref(out), None)
        assert rc == capi.MH_ERR_INVALID_ARG
        assert b"mh_icp_window_optimise" in L.mh_last_error(None) and b"NULL" in L.mh_last_error(None)
    assert L.mh_icp_window_wait(None) == capi.MH_ERR_INVALID_ARG
