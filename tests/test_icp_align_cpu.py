"""CPU: the step arithmetic of mh_icp_align (mimosa_amd/csrc/align_device.hpp, compiled by g++ through
tests/cpp/align_step.cpp) against numpy, and the ABI additions.

Bars.  xi: 1e-12 relative to |xi| against the solution of the same 6 x 6 system (numpy.linalg.solve, refined with residuals in
extended precision so that the REFERENCE is good to that figure at condition numbers of 1e8 — a plain LU keeps eight digits
there); the system is built from the H, b the header produced, which are compared with numpy's on their own (1e-13 |H|: a
handful of fp64 products in another order).  Retracted R orthonormal to 1e-14.  Flags and the frozen pose: exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def degenerate(block, thresh):
    w = np.linalg.eigh(block)[0]
    with np.errstate(invalid="ignore"):
        return not bool(np.all(np.sqrt(w) > thresh))


def ref_hessian(sums, R, p):
    M = np.zeros((7, 7))
    M[np.triu_indices(7)] = sums[:28]
    M = M + np.triu(M, 1).T
    H, b, f = M[:6, :6].copy(), M[:6, 6].copy(), M[6, 6]
    rd, td = degenerate(H[:3, :3], p["thresh_rot"]), degenerate(H[3:, 3:], p["thresh_trans"])
    if p["reg_4_dof"]:
        lz = R.T @ np.asarray(p["gz"])
        Pi = np.outer(lz, lz)
        Hrr, Hrt, Htr = H[:3, :3].copy(), H[:3, 3:].copy(), H[3:, :3].copy()
        H[:3, :3], H[:3, 3:], H[3:, :3] = Pi @ Hrr @ Pi, Pi @ Hrt, Htr @ Pi
        b[:3] = Pi @ b[:3]
    if p["project"] and (rd or td):
        H[:], b[:] = 0.0, 0.0
    return H, b, f, rd, td


def system(H, b, p):
    A = H.copy()
    for i in range(6):
        A[i, i] = (A[i, i] + (p["prior_rot"] if i < 3 else p["prior_trans"])) + p["damping"]
    return A, -b


def solve_refined(A, rhs):
    x = np.linalg.solve(A, rhs)
    Al, rl = A.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(4):
        r = (rl - Al @ x.astype(np.longdouble)).astype(np.float64)
        x = x + np.linalg.solve(A, r)
    return x


# ---- driver ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("align_step")


def run_cases(exe, cases):
    toks = [str(len(cases))]
    for c in cases:
        p = c["p"]
        vals = list(p["gz"]) + [p["eps_rot"], p["eps_trans"], p["damping"], p["prior_rot"], p["prior_trans"], p["thresh_rot"], p["thresh_trans"],
                                float(p["reg_4_dof"]), float(p["project"])]
        vals += list(np.asarray(c["R"]).ravel()) + list(c["t"]) + [float(len(c["sums"]))]
        for s in c["sums"]:
            vals += list(s)
        toks += [repr(float(v)) for v in vals]
    out = subprocess.run([exe], input=" ".join(toks), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def params(**kw):
    p = dict(gz=(0.0, 0.0, 1.0), eps_rot=0.0, eps_trans=0.0, damping=0.0, prior_rot=0.0, prior_trans=0.0, thresh_rot=0.0, thresh_trans=0.0,
             reg_4_dof=0, project=1)
    p.update(kw)
    return p


def spd(rng, cond, scale):
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    lam = scale * np.logspace(0, np.log10(cond), 6)[rng.permutation(6)]
    H = (Q * lam) @ Q.T
    return (H + H.T) / 2


def rank_deficient(rng, n_rot_dead, n_trans_dead, scale=1e4):
    """J^T J of rows that see nothing along n dead axes of a random basis of the rotation / translation block"""
    Br, Bt = np.linalg.qr(rng.standard_normal((3, 3)))[0], np.linalg.qr(rng.standard_normal((3, 3)))[0]
    J = rng.standard_normal((200, 6))
    J[:, :3] = (J[:, :3] * np.array([0.0] * n_rot_dead + [1.0] * (3 - n_rot_dead))) @ Br.T
    J[:, 3:] = (J[:, 3:] * np.array([0.0] * n_trans_dead + [1.0] * (3 - n_trans_dead))) @ Bt.T
    e = rng.standard_normal(200) * 0.05
    J *= np.sqrt(scale / 200)
    return J.T @ J, J.T @ e, float(e @ e)


def check_step(got, sums, R, t, p):
    """one evaluated iteration against numpy; returns the pose after it"""
    H, b, f, rd, td = ref_hessian(sums, R, p)
    assert (got["rot_degen"], got["trans_degen"]) == (int(rd), int(td))
    gH, gb = np.array(got["H"]).reshape(6, 6), np.array(got["b"])
    sH = max(np.abs(H).max(), np.abs(sums[:28]).max())
    assert np.abs(gH - H).max() <= 1e-13 * sH and np.abs(gb - b).max() <= 1e-13 * max(np.abs(sums[:28]).max(), 1e-300)
    assert np.array_equal(gH, gH.T) or p["reg_4_dof"]
    row = np.array(got["row"])
    A, rhs = system(gH, gb, p)
    singular = not np.all(np.linalg.eigvalsh((A + A.T) / 2) > 0)
    if singular:
        assert int(row[4]) & 4 and got["flags"] == 1
        assert np.array_equal(row[7:16].reshape(3, 3), R) and np.array_equal(row[16:19], t)
        return R, t, True
    xi = solve_refined((A + A.T) / 2 if not p["reg_4_dof"] else A, rhs)
    gxi = np.array(got["xi"])
    n = np.linalg.norm(xi)
    assert np.linalg.norm(gxi - xi) <= 1e-12 * n + 1e-300, (np.linalg.norm(gxi - xi) / max(n, 1e-300), np.linalg.cond(A))
    Rn, tn = R @ rodrigues(gxi[:3]), t + R @ gxi[3:]
    gR, gt = row[7:16].reshape(3, 3), row[16:19]
    assert np.abs(gR - Rn).max() <= 1e-15 * 8 and np.abs(gt - tn).max() <= 1e-15 * 8 * max(1.0, np.abs(tn).max())
    assert np.abs(gR.T @ gR - np.eye(3)).max() <= 1e-14
    assert row[0] == f
    assert abs(row[1] - np.linalg.norm(gxi[:3])) <= 4e-16 * max(1.0, row[1])
    assert abs(row[2] - np.linalg.norm(gxi[3:])) <= 4e-16 * max(1.0, row[2])
    assert int(row[4]) == int(rd) + 2 * int(td)
    conv = bool(row[1] < p["eps_rot"] and row[2] < p["eps_trans"])
    assert got["flags"] == (3 if conv else 0)
    return gR, gt, conv


def random_pose(rng):
    return rodrigues(rng.standard_normal(3) * 0.7), rng.standard_normal(3) * 3


@pytest.mark.parametrize("reg4", [0, 1])
def test_step_matches_numpy_on_spd_sums(exe, reg4):
    """condition numbers 1e1 .. 1e8 of H (of the solved system too: no prior, no damping unless the 4-DoF projection makes
    the rotation block rank one, where a prior of lambda_max / 1e7 keeps the system under 1e8)"""
    rng = np.random.default_rng(11 + reg4)
    cases = []
    for i in range(48):
        cond = 10.0 ** (1 + (i % 8))
        H = spd(rng, cond, 10.0 ** rng.uniform(0, 6))
        if reg4:  # the projected system: condition number set by the prior
            H = spd(rng, 1e3, 10.0 ** rng.uniform(0, 6))
        b = H @ (rng.standard_normal(6) * 0.05) + rng.standard_normal(6) * 1e-3 * np.sqrt(np.abs(H).max())
        R, t = random_pose(rng)
        lam = np.linalg.eigvalsh(H).max()
        p = params(reg_4_dof=reg4, prior_rot=(lam / 10.0 ** (i % 8 + 0.5) if reg4 else 0.0), damping=(0.0 if i % 3 else lam * 1e-9))
        cases.append(dict(p=p, R=R, t=t, sums=[pack(H, b, 3.0 + i)]))
    got = run_cases(exe, cases)
    worst = 0.0
    for c, g in zip(cases, got):
        A, _ = system(*ref_hessian(c["sums"][0], c["R"], c["p"])[:2], c["p"])
        worst = max(worst, np.linalg.cond(A))
        assert np.linalg.cond(A) <= 1.05e8
        check_step(g[0], c["sums"][0], c["R"], c["t"], c["p"])
    assert worst >= 1e7  # the hard end of the range is in the set


@pytest.mark.parametrize("reg4", [0, 1])
@pytest.mark.parametrize("dead", [(1, 0), (2, 0), (0, 1), (0, 2), (1, 1), (2, 2)])
def test_degenerate_sums(exe, dead, reg4):
    """one and two dead directions per block.  project_on_degeneracy: H = b = 0 — with a prior or damping the step
    is exactly zero (and converges at once when eps > 0), without both the system is singular: no step, the chain stops,
    converged stays 0.  Projection off: the prior alone carries the dead directions and the step is numpy's."""
    rng = np.random.default_rng(100 + 10 * dead[0] + dead[1] + 50 * reg4)
    H, b, f = rank_deficient(rng, *dead)
    R, t = random_pose(rng)
    s = pack(H, b, f)
    lam = np.linalg.eigvalsh(H).max()
    th = dict(thresh_rot=0.5, thresh_trans=0.5)
    cases = [
        dict(p=params(reg_4_dof=reg4, prior_rot=1e2, prior_trans=1e2, eps_rot=1e-9, eps_trans=1e-9, **th), R=R, t=t, sums=[s, s]),
        dict(p=params(reg_4_dof=reg4, damping=1.0, **th), R=R, t=t, sums=[s, s]),
        dict(p=params(reg_4_dof=reg4, **th), R=R, t=t, sums=[s, s, s]),
        dict(p=params(reg_4_dof=reg4, project=0, prior_rot=lam / 1e6, prior_trans=lam / 1e6, **th), R=R, t=t, sums=[s]),
    ]
    got = run_cases(exe, cases)
    # prior: zero step, converged, second queued iteration frozen
    g = got[0]
    assert g[0]["rot_degen"] == int(dead[0] > 0) and g[0]["trans_degen"] == int(dead[1] > 0)
    assert not np.any(np.array(g[0]["H"])) and not np.any(np.array(g[0]["b"])) and not np.any(np.array(g[0]["xi"]))
    check_step(g[0], s, R, t, cases[0]["p"])
    assert g[0]["flags"] == 3 and g[1]["flags"] == 7
    assert np.array_equal(np.array(g[0]["row"])[7:19], np.concatenate([R.ravel(), t]))  # Exp(0) = I exactly: the pose does not move
    # damping only, eps = 0: zero steps for ever, never converged
    g = got[1]
    assert [q["flags"] for q in g] == [0, 0] and not np.any(np.array(g[1]["xi"]))
    assert np.array_equal(np.array(g[1]["row"])[7:19], np.concatenate([R.ravel(), t]))
    # neither: singular, stop, pose unchanged, later iterations frozen and not converged
    g = got[2]
    assert g[0]["flags"] == 1 and int(g[0]["row"][4]) & 4 and [q["flags"] for q in g[1:]] == [5, 5]
    for q in g:
        assert np.array_equal(np.array(q["row"])[7:19], np.concatenate([R.ravel(), t]))
    assert g[2]["row"][6] == 1.0  # one executed iteration
    # projection off
    check_step(got[3][0], s, R, t, cases[3]["p"])
    assert int(got[3][0]["row"][4]) == int(dead[0] > 0) + 2 * int(dead[1] > 0)


def test_chain_converges_then_freezes(exe):
    """a quadratic bowl around a target pose, sums rebuilt at every pose the chain reaches; after the converging step the rows of
    iterations queued behind it carry the same pose bit for bit and flag 4, whatever sums they are fed"""
    rng = np.random.default_rng(5)
    H = spd(rng, 1e3, 1e4)
    R, t = random_pose(rng)
    p = params(eps_rot=1e-7, eps_trans=1e-7, damping=1e-9)
    delta = rng.standard_normal(6) * 0.05
    sums, Rk, tk = [], R, t
    state = delta.copy()
    seq = []
    for it in range(12):
        seq.append(pack(H, H @ state, float(state @ H @ state)))
        state = state * 0.02  # what is left after a (nearly exact) Newton step
    got = run_cases(exe, [dict(p=p, R=R, t=t, sums=seq)])[0]
    n_exec = 0
    done = False
    for it, g in enumerate(got):
        if done:
            assert g["flags"] == 7 and "xi" not in g
            assert np.array_equal(np.array(g["row"])[7:19], np.concatenate([Rk.ravel(), tk])) and g["row"][6] == n_exec
            continue
        Rk, tk, done = check_step(g, seq[it], Rk, tk, p)
        n_exec += 1
        assert g["row"][6] == n_exec
    assert done and 2 <= n_exec < 12


# ---- ABI -------------------------------------------------------------------------------------------------------------------
ALIGN_FUNCS = ["mh_icp_align", "mh_icp_align_async"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in ALIGN_FUNCS:
        assert hasattr(L, f), f
    assert set(ALIGN_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr


def test_struct_sizes_match_the_header(tmp_path):
    from mimosa_amd import capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(mh_icp_align_config), sizeof(mh_icp_align_trace), sizeof(mh_icp_align_result), offsetof(mh_icp_align_config, check_every), "
                   "offsetof(mh_icp_align_result, trace), offsetof(mh_icp_align_result, last)); return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.AlignConfig), C.sizeof(capi.AlignTrace), C.sizeof(capi.AlignResult), capi.AlignConfig.check_every.offset,
                   capi.AlignResult.trace.offset, capi.AlignResult.last.offset]


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out = capi.make_align_config(), capi.AlignResult()
    I, z, g = np.eye(3).ravel().copy(), np.zeros(3), np.array([0.0, 0.0, -1.0])
    for fn in (L.mh_icp_align, L.mh_icp_align_async):
        rc = fn(None, capi._p(I), capi._p(z), capi._p(g), C.byref(cfg), C.byref(out))
        assert rc == capi.MH_ERR_INVALID_ARG
        assert b"mh_icp_align" in L.mh_last_error(None) and b"NULL" in L.mh_last_error(None)
