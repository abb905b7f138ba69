"""CPU half of the wide pose graph (mh_pose_graph_create_wide): the blocked phases of mimosa_amd/csrc/pose_graph_device.hpp
(pgo_wide_*) compiled with g++ (tests/cpp/pose_graph_wide_step.cpp) against the dense numpy restatement (tests/pose_graph_ref.py,
tests/pose_graph_robust_ref.py) on the graphs of tests/pose_graph_wide_cases.py — the very graphs
tests/test_gpu_pose_graph_wide.py hands the device — and, bit for bit, against the unblocked pgo_factor_C / pgo_solve_C on the same
graph.  The same program once more as a stand-alone binary under AddressSanitizer and UBSan.  The ABI without a device.  The
conditions the GPU tests rest on are asserted on the restatement alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_wide_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_TOL, W_TOL, f_close = cases.POSE_TOL, cases.W_TOL, cases.f_close


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("pose_graph_wide_step")


def hx(v):
    return float(v).hex()


def graph_text(c, iters, eps=0.0):
    n, E = len(c["R"]), len(c["edges"])
    el = c["edge_loss"] or [(0, 0.0)] * E
    out = ["graph %d %d %d %s %s %s" % (n, E, iters, hx(c["damping"]), hx(eps), hx(eps))]
    out.append(" ".join(hx(v) for i in range(n) for v in list(c["R"][i].ravel()) + list(c["t"][i])))
    out.append(" ".join(str(int(v)) for v in c["fixed"]))
    for (a, b, ZR, Zt, Om), (kind, param) in zip(c["edges"], el):
        out.append("%d %d %s %d %s" % (a, b, " ".join(hx(v) for v in list(ZR.ravel()) + list(Zt) + list(Om.ravel())), kind, hx(param)))
    return "\n".join(out) + "\n"


def fx(v):
    return np.array([float.fromhex(s) for s in v])


def run(exe, text, timeout=600):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    return rows[:-1], rows[-1]


_RUNS = {}


def chain(exe, name, iters=cases.ITERS):
    """the program's run of a case (shared by the tests below, never changed)"""
    if (name, iters) not in _RUNS:
        _RUNS[(name, iters)] = run(exe, graph_text(cases.case(name), iters))
    return _RUNS[(name, iters)]


def split(poses):
    P = fx(poses).reshape(-1, 12)
    return P[:, :9].reshape(-1, 3, 3), P[:, 9:]


# ---- the blocked phases against the dense restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REGULAR)
def test_chain_against_the_restatement(exe, name):
    c, want = cases.case(name), cases.restated(name)
    rows, last = chain(exe, name)
    assert last["iters"] == cases.ITERS == len(rows) and last["converged"] == 0 and last["n_far"] == cases.n_far(c) > 32
    worst = [0.0, 0.0, 0.0]
    for row, w in zip(rows, want["trace"]):
        assert row["flags"] == 0
        R, t = split(row["poses"])
        dt, dr = ref.pose_error(R, t, w["R"], w["t"])
        f = float.fromhex(row["f"])
        worst = [max(worst[0], dt), max(worst[1], dr), max(worst[2], abs(f - w["f"]) / max(abs(w["f"]), 1e-300))]
        assert dt <= POSE_TOL and dr <= POSE_TOL, (name, row["iters"], dt, dr)
        assert f_close(f, w["f"], len(c["edges"])), (name, row["iters"], f, w["f"])
        assert abs(float.fromhex(row["step_rot"]) - w["step_rot"]) <= POSE_TOL and abs(float.fromhex(row["step_trans"]) - w["step_trans"]) <= POSE_TOL
    R, t = split(last["poses"])
    dt, dr = ref.pose_error(R, t, want["R"], want["t"])
    print("%s (%d far edges): largest difference to the restatement over %d iterations: %.3g m, %.3g rad, f %.3g relative; final poses %.3g m, %.3g rad"
          % (name, last["n_far"], cases.ITERS, *worst, dt, dr))
    assert dt <= POSE_TOL and dr <= POSE_TOL
    fixed = np.flatnonzero(c["fixed"])
    assert np.array_equal(R[fixed], c["R"][fixed]) and np.array_equal(t[fixed], c["t"][fixed])   # a fixed pose takes no step: not a bit


def test_robust_case_against_the_restatement(exe):
    name = cases.ROBUST
    c, want = cases.case(name), cases.restated(name)
    rows, last = chain(exe, name)
    assert len(rows) == cases.ITERS and last["same"] == 1
    worst = [0.0, 0.0, 0.0]
    for row, w in zip(rows, want["trace"]):
        assert row["flags"] == 0
        dt, dr = ref.pose_error(*split(row["poses"]), w["R"], w["t"])
        dw = np.abs(fx(row["w"]) - w["w_edges"]).max()
        worst = [max(worst[0], dt), max(worst[1], dr), max(worst[2], dw)]
        assert dt <= POSE_TOL and dr <= POSE_TOL and dw <= W_TOL, (row["iters"], dt, dr, dw)
        assert f_close(float.fromhex(row["f"]), w["f"], len(c["edges"])), (row["iters"], row["f"], w["f"])
    print("%s: largest difference to the restatement: %.3g m, %.3g rad, weights %.3g" % (name, *worst))


# ---- the blocked phases against the unblocked ones, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REGULAR + (cases.ROBUST,) + cases.PLAIN[:3])
def test_blocked_phases_have_the_bits_of_the_unblocked_ones(exe, name):
    """row, poses, the step, u and every entry of C's factor, after every iteration (the program compares; "same" is its verdict)"""
    rows, last = chain(exe, name, cases.ITERS if name in cases.REGULAR + (cases.ROBUST,) else 6)
    assert rows and all(r["same"] == 1 for r in rows) and last["same"] == 1, [r["iters"] for r in rows if r["same"] != 1]
    assert all(r["flags"] & 4 == 0 for r in rows)


@pytest.mark.parametrize("name", cases.SINGULAR)
def test_singular_cases_take_no_step(exe, name):
    c = cases.case(name)
    rows, last = chain(exe, name, 8)
    assert len(rows) == 1 and rows[0]["flags"] == 1 | 4 and rows[0]["same"] == 1 and last["iters"] == 1 and last["converged"] == 0
    R, t = split(last["poses"])
    assert np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined (every array sized to its graph exactly, C and Y
    to its F) and run on what the other tests feed the plain build: same output, no report"""
    from mimosa_amd import build
    san = str(tmp_path / "pose_graph_wide_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "pose_graph_wide_step.cpp"), "-o", san])
    text = "".join(graph_text(cases.case(n), 2) for n in ("n1", "n3_far", "w40_far33", "w80_far70_fixed41", "w90_far64", "w90_far43", "w80_psd_last", "broken_chain"))
    text += graph_text(cases.case("w120_far128"), 1) + graph_text(cases.case(cases.ROBUST), 1)
    a = subprocess.run([san], input=text, capture_output=True, text=True, timeout=900)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0 and a.stdout == b.stdout


# ---- the conditions the GPU tests rest on, on the restatement alone ---------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REGULAR)
def test_regular_cases_converge(name):
    want = cases.restated(name)
    last = want["trace"][-1]
    print("%s: the restatement's step %d: %.3g rad, %.3g m" % (name, cases.ITERS, last["step_rot"], last["step_trans"]))
    assert last["step_rot"] < 1e-12 and last["step_trans"] < 1e-12


def test_case_shapes():
    far = lambda n: [e[:2] for e in cases.case(n)["edges"] if e[1] - e[0] >= 2]
    assert [len(far(n)) for n in cases.REGULAR] == [33, 59, 70, 70, 128, 64, 43]
    assert far("w60_skip2") == [(i, i + 2) for i in range(58)] + [(0, 59)]
    assert all(far(n)[:3] == [(0, len(cases.case(n)["R"]) - 1), (0, 2), (len(cases.case(n)["R"]) - 3, len(cases.case(n)["R"]) - 1)] for n in cases.REGULAR if n != "w60_skip2")
    assert (6 * 64) % cases.NB == 0 and (6 * 43) % cases.NB == 2 and not any((6 * F) % cases.NB == 1 for F in range(1, 513))   # 6 F is even: + 2 is the nearest
    c = cases.case("w80_far70_fixed41")
    assert c["fixed"].nonzero()[0].tolist() == [0, 41] and sum(1 for a, b in far("w80_far70_fixed41") if 41 in (a, b)) >= 1
    assert far("w80_far70_fixed41") == far("w80_far70")
    Om = cases.case("w80_psd_last")["edges"][-1][4]
    w = np.linalg.eigvalsh(Om)
    assert abs(w[0]) < 1e-9 and w[1] > 1.0 and np.array_equal(Om, Om.T) and len(far("w80_psd_last")) - 1 >= 64
    c = cases.case(cases.ROBUST)
    assert all((k == 2 and p == cases.CAUCHY_K) == (e[1] - e[0] >= 2) for e, (k, p) in zip(c["edges"], c["edge_loss"]))
    assert not np.array_equal(c["edges"][-1][3], cases.case("w80_far70")["edges"][-1][3])


# ---- the ABI without a device -----------------------------------------------------------------------------------------------
def test_abi_symbol_and_constants():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    assert hasattr(L, "mh_pose_graph_create_wide") and "mh_pose_graph_create_wide" in capi.EXPORTS
    assert L.mh_abi_version() == 3
    assert (capi.MH_PGO_FAR_MAX, capi.MH_PGO_FAR_LIMIT) == (32, 512)


def test_constants_match_the_header(tmp_path):
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "mimosa_hip.h"\nint main(void) { printf("%d %d %d\\n", MH_PGO_FAR_MAX, MH_PGO_FAR_LIMIT, MH_ABI_VERSION); return 0; }\n')
    out = str(tmp_path / "consts")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", out])
    assert subprocess.run([out], capture_output=True, text=True, check=True).stdout.split() == ["32", "512", "3"]


def test_refusals_that_need_no_device():
    """a NULL argument, and every size mh_pose_graph_create_wide refuses: the sizes are judged before the context is looked at"""
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    INV = capi.MH_ERR_INVALID_ARG
    h = C.c_void_p()
    assert L.mh_pose_graph_create_wide(None, 16, 16, 64, None) == INV and b"mh_pose_graph_create_wide: NULL argument" in L.mh_last_error(None)
    for poses, edges, far, msg in ((0, 16, 64, b"max_poses"), (4097, 16, 64, b"max_poses"), (16, 32769, 64, b"max_edges"), (16, 16, 0, b"max_far"),
                                   (16, 16, 513, b"max_far")):
        assert L.mh_pose_graph_create_wide(None, poses, edges, far, C.byref(h)) == INV and msg in L.mh_last_error(None), (poses, edges, far)
        assert not h.value
    for far in (1, 512):                                   # the ends of the range pass the size check
        assert L.mh_pose_graph_create_wide(None, 4096, 32768, far, C.byref(h)) == INV and b"NULL argument" in L.mh_last_error(None)
