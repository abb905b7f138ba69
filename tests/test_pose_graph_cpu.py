"""CPU half of the pose graph (mh_pose_graph_*): mimosa_amd/csrc/pose_graph_device.hpp compiled with g++
(tests/cpp/pose_graph_step.cpp: every launch of the chain a loop) against the numpy restatement (tests/pose_graph_ref.py: the
same system assembled dense and solved by numpy.linalg.solve) on the graphs of tests/pose_graph_cases.py — the very graphs
tests/test_gpu_pose_graph.py hands the device.  The same program once more as a stand-alone binary under AddressSanitizer and
UBSan.  The ABI without a device.  The conditions the GPU tests rest on are asserted on the restatement alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGO_FUNCS = ("mh_pose_graph_create", "mh_pose_graph_destroy", "mh_pose_graph_set_poses", "mh_pose_graph_set_fixed", "mh_pose_graph_set_edges",
             "mh_pose_graph_get_poses", "mh_pose_graph_residuals", "mh_pose_graph_optimise")
POSE_TOL, F_RTOL, STOP_CASES, f_floor, f_close = cases.POSE_TOL, cases.F_RTOL, cases.STOP_CASES, cases.f_floor, cases.f_close


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("pose_graph_step")


def hx(v):
    return float(v).hex()


def graph_text(c, iters, eps=0.0):
    n, E = len(c["R"]), len(c["edges"])
    out = ["graph %d %d %d %s %s %s" % (n, E, iters, hx(c["damping"]), hx(eps), hx(eps))]
    out.append(" ".join(hx(v) for i in range(n) for v in list(c["R"][i].ravel()) + list(c["t"][i])))
    out.append(" ".join(str(int(v)) for v in c["fixed"]))
    for a, b, ZR, Zt, Om in c["edges"]:
        out.append("%d %d %s" % (a, b, " ".join(hx(v) for v in list(ZR.ravel()) + list(Zt) + list(Om.ravel()))))
    return "\n".join(out) + "\n"


def fx(v):
    return np.array([float.fromhex(s) for s in v])


def run(exe, text, timeout=600):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    return rows[0], rows[1:-1], rows[-1]


def split(poses):
    P = fx(poses).reshape(-1, 12)
    return P[:, :9].reshape(-1, 3, 3), P[:, 9:]


# ---- the header against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REGULAR)
def test_chain_against_the_restatement(exe, name):
    c, want = cases.case(name), cases.restated(name)
    res, rows, last = run(exe, graph_text(c, cases.ITERS))
    assert last["iters"] == cases.ITERS == len(rows) and last["converged"] == 0
    assert last["n_far"] == sum(1 for e in c["edges"] if e[1] - e[0] >= 2)
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
    assert dt <= POSE_TOL and dr <= POSE_TOL
    print("%s: largest difference to the restatement over %d iterations: %.3g m, %.3g rad, f %.3g relative" % (name, cases.ITERS, *worst))
    fixed = np.flatnonzero(c["fixed"])
    assert np.array_equal(R[fixed], c["R"][fixed]) and np.array_equal(t[fixed], c["t"][fixed])   # a fixed pose takes no step: not a bit


@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_test_against_the_restatement(exe, name):
    c, want = cases.case(name), cases.restated(name, 64, cases.STOP_EPS)
    _, rows, last = run(exe, graph_text(c, 64, cases.STOP_EPS))
    assert want["converged"] and want["iters"] < 64
    assert (last["iters"], last["converged"], len(rows)) == (want["iters"], 1, want["iters"])
    assert [r["flags"] for r in rows] == [0] * (want["iters"] - 1) + [3]
    dt, dr = ref.pose_error(*split(last["poses"]), want["R"], want["t"])
    assert dt <= POSE_TOL and dr <= POSE_TOL


@pytest.mark.parametrize("name", cases.REGULAR)
def test_residuals_against_the_restatement(exe, name):
    c = cases.case(name)
    r, chi2, f = cases.restated_residuals(name)
    got, _, _ = run(exe, graph_text(c, 1))
    assert np.abs(fx(got["r"]).reshape(-1, 6) - r).max(initial=0.0) <= POSE_TOL
    assert np.all(np.abs(fx(got["chi2"]) - chi2) <= F_RTOL * chi2 + f_floor(1))
    assert f_close(float.fromhex(got["f"]), f, len(chi2))


@pytest.mark.parametrize("name", cases.SINGULAR)
def test_singular_cases_take_no_step(exe, name):
    """T singular (a gap bridged by a far edge only) or a far edge's info without an inverse: bit 4, no step, the call ends"""
    c = cases.case(name)
    _, rows, last = run(exe, graph_text(c, 8))
    assert len(rows) == 1 and rows[0]["flags"] == 1 | 4 and last["iters"] == 1 and last["converged"] == 0
    assert float.fromhex(rows[0]["step_rot"]) == 0.0 and float.fromhex(rows[0]["step_trans"]) == 0.0
    R, t = split(last["poses"])
    assert np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])
    assert f_close(float.fromhex(rows[0]["f"]), ref.residuals(c["R"], c["t"], c["edges"])[2], len(c["edges"]))
    A, _, _ = ref.system(list(c["R"]), list(c["t"]), c["fixed"], c["edges"], 0.0)
    assert np.linalg.eigvalsh(A).min() > 1e-3          # the whole system is regular: it is the method's limit, stated in the header


def test_damping_mends_the_broken_chain(exe):
    """the documented way out: with damping T is positive definite and the same graph is solved, to the restatement's digits"""
    c = dict(cases.case("broken_chain"), damping=1e-3)
    want = ref.optimise(c["R"], c["t"], c["fixed"], c["edges"], 6, c["damping"])
    _, rows, last = run(exe, graph_text(c, 6))
    assert [r["flags"] for r in rows] == [0] * 6
    dt, dr = ref.pose_error(*split(last["poses"]), want["R"], want["t"])
    assert dt <= POSE_TOL and dr <= POSE_TOL


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined (every array sized to its graph exactly) and run
    on what the other tests feed the plain build: same output, no report"""
    from mimosa_amd import build
    san = str(tmp_path / "pose_graph_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "pose_graph_step.cpp"), "-o", san])
    text = "".join(graph_text(cases.case(n), 3) for n in ("n1", "n2", "n3_far", "n12_far_on_fixed", "n65", "broken_chain", "psd_info"))
    text += graph_text(cases.case("n300_far32"), 1)
    a = subprocess.run([san], input=text, capture_output=True, text=True, timeout=900)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0 and a.stdout == b.stdout


# ---- the conditions the GPU tests rest on, on the restatement alone ---------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REGULAR)
def test_regular_cases_converge(name):
    c = cases.case(name)
    got = ref.optimise(c["R"], c["t"], c["fixed"], c["edges"], 64, c["damping"], 1e-12, 1e-12)
    assert got["converged"] and got["iters"] <= cases.ITERS, got["iters"]
    assert got["trace"][-1]["step_rot"] < 1e-12 and got["trace"][-1]["step_trans"] < 1e-12
    if name in STOP_CASES:  # the stop is decided by a wide margin, not by the last digits: no step norm within a factor 3 of STOP_EPS
        steps = [s for q in got["trace"] for s in (q["step_rot"], q["step_trans"])]
        assert all(not (cases.STOP_EPS / 3 < s < cases.STOP_EPS * 3) for s in steps), steps


@pytest.mark.parametrize("name", cases.CIRCUITS)
def test_loops_pull_the_circuit_towards_the_truth(name):
    c, got = cases.case(name), cases.restated(name)
    free = c["fixed"] == 0
    before = np.linalg.norm(c["t"] - c["truth_t"], axis=1)[free].max()
    after = np.linalg.norm(got["t"] - c["truth_t"], axis=1)[free].max()
    print("%s: largest error against the truth %.3f m integrated, %.3f m optimised" % (name, before, after))
    assert after < before


def test_case_shapes():
    far = lambda n: [e[:2] for e in cases.case(n)["edges"] if e[1] - e[0] >= 2]
    assert len(far("n300_far32")) == 32 and len(set(far("n300_far32"))) == 32
    assert far("n64")[0] == far("n64")[1] and far("n12_far_on_fixed") == [(0, 11)]
    assert sum(1 for e in cases.case("n64")["edges"] if e[:2] == (5, 6)) == 2
    assert cases.case("n257_two_fixed")["fixed"].nonzero()[0].tolist() == [100, 256]
    assert not any(e[:2] == (5, 6) for e in cases.case("broken_chain")["edges"])
    Om = cases.case("psd_info")["edges"][-1][4]
    w = np.linalg.eigvalsh(Om)
    assert abs(w[0]) < 1e-9 and w[1] > 1.0 and np.array_equal(Om, Om.T)
    for n in cases.REGULAR + cases.SINGULAR:
        assert all(np.array_equal(e[4], e[4].T) and np.abs(e[4] - np.diag(np.diag(e[4]))).max() > 1.0 for e in cases.case(n)["edges"])


# ---- the ABI without a device -----------------------------------------------------------------------------------------------
def test_abi_symbols():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in PGO_FUNCS:
        assert hasattr(L, f) and f in capi.EXPORTS, f
    assert L.mh_abi_version() == 3
    assert (capi.MH_PGO_MAX_POSES, capi.MH_PGO_MAX_EDGES, capi.MH_PGO_FAR_MAX) == (4096, 32768, 32)


def test_struct_layouts_match_the_header(tmp_path):
    from mimosa_amd import capi
    structs = [("mh_pose_graph_config", capi.PoseGraphConfig, 32), ("mh_pose_graph_trace", capi.PoseGraphTrace, 32),
               ("mh_pose_graph_result", capi.PoseGraphResult, 32 + 64 * 32), ("mh_window_edge", capi.WindowEdge, 392)]
    items = [("MH_PGO_MAX_POSES", 4096), ("MH_PGO_MAX_EDGES", 32768), ("MH_PGO_FAR_MAX", 32), ("MH_ABI_VERSION", 3)]
    for name, cls, size in structs:
        assert C.sizeof(cls) == size
        items.append(("sizeof(%s)" % name, size))
        items += [("offsetof(%s, %s)" % (name, n), getattr(cls, n).offset) for n, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mimosa_hip.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu\\n", (size_t)%s);\n' % e for e, _ in items) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [v for _, v in items], [(e, g, v) for (e, v), g in zip(items, got) if g != v]


def test_refusals_that_need_no_device():
    """a NULL argument everywhere, and every size mh_pose_graph_create refuses: the sizes are judged before the context is looked at"""
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    INV, p = capi.MH_ERR_INVALID_ARG, capi._p
    h = C.c_void_p()
    assert L.mh_pose_graph_create(None, 16, 16, None) == INV and b"mh_pose_graph_create: NULL argument" in L.mh_last_error(None)
    assert L.mh_pose_graph_create(None, 16, 16, C.byref(h)) == INV and b"NULL argument" in L.mh_last_error(None) and not h.value
    for poses, edges, msg in ((0, 16, b"max_poses"), (4097, 16, b"max_poses"), (16, 32769, b"max_edges")):
        assert L.mh_pose_graph_create(None, poses, edges, C.byref(h)) == INV and msg in L.mh_last_error(None), (poses, edges)
    for poses, edges in ((1, 0), (4096, 32768)):           # the ends of the ranges pass the size check
        assert L.mh_pose_graph_create(None, poses, edges, C.byref(h)) == INV and b"NULL argument" in L.mh_last_error(None)
    R, t, f = np.eye(3).ravel(), np.zeros(3), C.c_double()
    cfg, res = capi.make_pose_graph_config(), capi.PoseGraphResult()
    calls = [("mh_pose_graph_set_poses", lambda: L.mh_pose_graph_set_poses(None, p(R), p(t), 1)),
             ("mh_pose_graph_set_fixed", lambda: L.mh_pose_graph_set_fixed(None, None)),
             ("mh_pose_graph_set_edges", lambda: L.mh_pose_graph_set_edges(None, None, 0)),
             ("mh_pose_graph_get_poses", lambda: L.mh_pose_graph_get_poses(None, p(R), p(t), 1, None)),
             ("mh_pose_graph_residuals", lambda: L.mh_pose_graph_residuals(None, None, None, C.byref(f))),
             ("mh_pose_graph_optimise", lambda: L.mh_pose_graph_optimise(None, C.byref(cfg), C.byref(res), None))]
    for name, call in calls:
        assert call() == INV and (name + ": NULL argument").encode() in L.mh_last_error(None), name
    L.mh_pose_graph_destroy(None)                          # a no-op
