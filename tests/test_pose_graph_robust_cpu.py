"""CPU half of the pose graph's priors and losses (mh_pose_graph_set_priors, _set_loss, _prior_residuals, _weights):
mimosa_amd/csrc/pose_graph_device.hpp compiled with g++ (tests/cpp/pose_graph_robust_step.cpp) against the numpy restatement
(tests/pose_graph_robust_ref.py) on the graphs of tests/pose_graph_robust_cases.py — the very graphs
tests/test_gpu_pose_graph_robust.py hands the device.  The same program once more as a stand-alone binary under AddressSanitizer
and UBSan.  The ABI without a device.  The conditions the GPU tests rest on (a false loop bends the plain solution and not the
robust one) are asserted on the restatement alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_robust_cases as cases
import pose_graph_robust_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCS = ("mh_pose_graph_set_priors", "mh_pose_graph_set_loss", "mh_pose_graph_prior_residuals", "mh_pose_graph_weights")
POSE_TOL, W_TOL, f_close = cases.POSE_TOL, cases.W_TOL, cases.f_close


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("pose_graph_robust_step")


def hx(v):
    return float(v).hex()


def graph_text(c, iters, eps=0.0):
    n, E, P = len(c["R"]), len(c["edges"]), len(c["priors"])
    el = c["edge_loss"] or [(0, 0.0)] * E
    pl = c["prior_loss"] or [(0, 0.0)] * P
    out = ["graph %d %d %d %d %s %s %s" % (n, E, P, iters, hx(c["damping"]), hx(eps), hx(eps))]
    out.append(" ".join(hx(v) for i in range(n) for v in list(c["R"][i].ravel()) + list(c["t"][i])))
    out.append(" ".join(str(int(v)) for v in c["fixed"]))
    for (a, b, ZR, Zt, Om), (kind, param) in zip(c["edges"], el):
        out.append("%d %d %s %d %s" % (a, b, " ".join(hx(v) for v in list(ZR.ravel()) + list(Zt) + list(Om.ravel())), kind, hx(param)))
    for (i, ZR, Zt, Om), (kind, param) in zip(c["priors"], pl):
        out.append("%d %s %d %s" % (i, " ".join(hx(v) for v in list(ZR.ravel()) + list(Zt) + list(Om.ravel())), kind, hx(param)))
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
    first, rows, last = run(exe, graph_text(c, cases.ITERS))
    assert last["iters"] == cases.ITERS == len(rows) and last["converged"] == 0
    worst = [0.0, 0.0, 0.0, 0.0]
    for row, w in zip(rows, want["trace"]):
        assert row["flags"] == 0
        R, t = split(row["poses"])
        dt, dr = ref.pose_error(R, t, w["R"], w["t"])
        f = float.fromhex(row["f"])
        dw = max(np.abs(fx(row["w"]) - w["w_edges"]).max(initial=0.0), np.abs(fx(row["pw"]) - w["w_priors"]).max(initial=0.0))
        worst = [max(worst[0], dt), max(worst[1], dr), max(worst[2], abs(f - w["f"]) / max(abs(w["f"]), 1e-300)), max(worst[3], dw)]
        print("%s iteration %d: %.3g m, %.3g rad, f %.17g against %.17g, weights %.3g" % (name, row["iters"], dt, dr, f, w["f"], dw))
        assert dt <= POSE_TOL and dr <= POSE_TOL, (name, row["iters"], dt, dr)
        assert f_close(f, w["f"], cases.n_terms(c)), (name, row["iters"], f, w["f"])
        assert dw <= W_TOL, (name, row["iters"], dw)
        assert abs(float.fromhex(row["step_rot"]) - w["step_rot"]) <= POSE_TOL and abs(float.fromhex(row["step_trans"]) - w["step_trans"]) <= POSE_TOL
    R, t = split(last["poses"])
    dt, dr = ref.pose_error(R, t, want["R"], want["t"])
    assert dt <= POSE_TOL and dr <= POSE_TOL
    print("%s: largest difference to the restatement over %d iterations: %.3g m, %.3g rad, f %.3g relative, weights %.3g" % (name, cases.ITERS, *worst))
    fixed = np.flatnonzero(c["fixed"])
    assert np.array_equal(R[fixed], c["R"][fixed]) and np.array_equal(t[fixed], c["t"][fixed])   # a fixed pose takes no step: not a bit


@pytest.mark.parametrize("name", cases.REGULAR)
def test_weights_and_prior_residuals_against_the_restatement(exe, name):
    c = cases.case(name)
    we, wp, f = cases.restated_weights(name)
    d, chi2 = rref.prior_residuals(c["R"], c["t"], c["priors"])
    got, _, _ = run(exe, graph_text(c, 1))
    assert np.abs(fx(got["w"]) - we).max(initial=0.0) <= W_TOL and np.abs(fx(got["pw"]) - wp).max(initial=0.0) <= W_TOL
    assert np.abs(fx(got["d"]).reshape(-1, 6) - d).max(initial=0.0) <= POSE_TOL
    assert np.all(np.abs(fx(got["pchi2"]) - chi2) <= cases.F_RTOL * chi2 + cases.base.f_floor(1))
    assert f_close(float.fromhex(got["f"]), f, cases.n_terms(c))


def test_no_anchor_takes_no_step(exe):
    """no fixed pose, no prior, no damping: T is singular, bit 4, the poses untouched"""
    c = cases.case("no_anchor")
    _, rows, last = run(exe, graph_text(c, 8))
    assert len(rows) == 1 and rows[0]["flags"] == 1 | 4 and last["iters"] == 1 and last["converged"] == 0
    R, t = split(last["poses"])
    assert np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])


def test_a_prior_on_a_fixed_pose_acts_on_f_alone(exe):
    c = cases.case("prior_on_fixed")
    _, rows, last = run(exe, graph_text(c, 4))
    _, rows0, last0 = run(exe, graph_text(dict(c, priors=[]), 4))
    assert last["poses"] == last0["poses"]                  # bit for bit
    _, chi2 = rref.prior_residuals(c["R"], c["t"], c["priors"])
    assert chi2[0] > 1.0
    for a, b in zip(rows, rows0):
        assert abs(float.fromhex(a["f"]) - float.fromhex(b["f"]) - chi2[0]) <= 1e-12 * chi2[0] + 1e-9 * abs(float.fromhex(b["f"]))


def test_the_clamp_of_w_is_reached_and_no_pivot_fails(exe):
    c, want = cases.case("huge_chi2"), cases.restated("huge_chi2")
    first, rows, _ = run(exe, graph_text(c, 3))
    far = len(c["edges"]) - 1
    assert fx(first["w"])[far] == rref.MIN_WEIGHT == want["trace"][0]["w_edges"][far]
    assert [r["flags"] for r in rows] == [0, 0, 0]
    s = ref.residuals(c["R"], c["t"], c["edges"])[1][far]
    assert 1.0 / (1.0 + s) < 1e-14                         # the unclamped weight is far below the clamp


def test_kind_0_has_the_bits_of_the_plain_program(exe):
    """with no prior and every kind 0 the chain is the one tests/cpp/pose_graph_step.cpp runs: the same bits in every row"""
    from mimosa_amd import build
    import pose_graph_cases as plain_cases
    from test_pose_graph_cpu import graph_text as plain_text
    plain = build.build_host_test("pose_graph_step")
    for name in ("n3_far", "n65", "n300_far32"):
        c = plain_cases.case(name)
        a = subprocess.run([plain], input=plain_text(c, 6), capture_output=True, text=True, timeout=600)
        assert a.returncode == 0
        want = [json.loads(line) for line in a.stdout.splitlines()]
        _, rows, last = run(exe, graph_text(dict(c, priors=[], edge_loss=None, prior_loss=None), 6))
        assert len(rows) == len(want) - 2
        for r, w in zip(rows + [last], want[1:]):
            assert r["poses"] == w["poses"] and r.get("f") == w.get("f") and r.get("step_rot") == w.get("step_rot"), name


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined (every array sized to its graph exactly) and run
    on what the other tests feed the plain build: same output, no report"""
    from mimosa_amd import build
    san = str(tmp_path / "pose_graph_robust_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "pose_graph_robust_step.cpp"), "-o", san])
    names = ("n1_prior_only", "n2_two_priors_one_pose", "n3_far_cauchy", "n12_far_on_fixed_dcs", "n64_false_loop_huber", "n65_priors_no_fixed", "prior_on_fixed",
             "no_anchor", "huge_chi2")
    text = "".join(graph_text(cases.case(n), 3) for n in names)
    text += graph_text(cases.case("n257_mixed"), 1) + graph_text(cases.case("n300_far32_cauchy"), 1)
    a = subprocess.run([san], input=text, capture_output=True, text=True, timeout=900)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0 and a.stdout == b.stdout


# ---- the conditions the GPU tests rest on, on the restatement alone ---------------------------------------------------------------
def _truth_error(c, t):
    free = c["fixed"] == 0
    return float(np.linalg.norm(np.asarray(t) - c["truth_t"], axis=1)[free].max())


@pytest.mark.parametrize("name", ("n64_false_loop_cauchy", "n64_false_loop_dcs"))
def test_a_false_loop_bends_the_plain_solution_and_not_the_robust_one(name):
    c = cases.case(name)
    start = _truth_error(c, c["t"])
    plain = _truth_error(c, cases.restated("n64_false_loop_plain")["t"])
    got = cases.restated(name)
    robust = _truth_error(c, got["t"])
    w = got["trace"][-1]["w_edges"][-4:]
    print("%s: error against the truth %.3f m at the start, %.3f m plain, %.3f m robust; loop weights %s" % (name, start, plain, robust, w))
    assert plain > start > robust
    assert w[3] < 0.01 and np.all(w[:3] > 0.5)


def test_hall_with_an_aliased_loop():
    """The hall of tests/test_map_rebuild_cpu.py plus one aliased loop (pose_graph_robust_cases.hall_case: ONE true loop, (0, 35)),
    with the restated graph, the oracle map and brute-force nearest distances.  Without a loss the rebuilt map is no better than
    half the drifted one; with Cauchy on the two far edges it lies within a quarter of the drifted map's RMS distance to the true
    map, the aliased loop's weight is below 0.01 and the true loop's above 0.5.  (tests/test_gpu_pose_graph_robust.py asserts a
    half on the device.)"""
    import map_rebuild_ref as mref
    from oracle import numpy_ref
    case = cases.hall_case()
    oracle_points = lambda poses: np.concatenate([np.array(v[0]).reshape(-1, 3) for v in mref.sequential_build(
        numpy_ref.VoxelMap(leaf=0.5, min_dist=0.15, lru_horizon=1000), [mref.world_f32(c, R, t) for c, R, t in zip(case["clouds"], *poses)]).cells.values()])
    true = oracle_points(case["true"])
    rms = lambda poses: mref.capped_rms(mref.nearest_distances(oracle_points(poses)[::10], true))
    plain = rref.optimise(*case["drifted"], case["fixed"], case["edges"], [], None, None, cases.ITERS)
    robust = rref.optimise(*case["drifted"], case["fixed"], case["edges"], [], case["edge_loss"], None, cases.ITERS)
    rms_d, rms_p, rms_r = rms(case["drifted"]), rms((plain["R"], plain["t"])), rms((robust["R"], robust["t"]))
    w = rref.weights(robust["R"], robust["t"], case["edges"], [], case["edge_loss"])[0]
    print("hall, oracle: RMS to the true map drifted %.4f m, plain %.4f m, Cauchy %.4f m; far weights %s" % (rms_d, rms_p, rms_r, w[-2:]))
    assert [q[:2] for q in case["edges"][-2:]] == [(0, 35), cases.HALL_ALIAS[0]]
    assert rms_d > 0.1 and rms_p > 0.5 * rms_d and rms_r < 0.25 * rms_d
    assert w[-1] < 0.01 and w[-2] > 0.5 and np.all(w[:-2] == 1.0)


def test_case_shapes():
    far = lambda c: [e for e, q in enumerate(c["edges"]) if q[1] - q[0] >= 2]
    c = cases.case("n300_far32_cauchy")
    assert len(far(c)) == 32 and all(c["edge_loss"][e] == (rref.CAUCHY, 300.0) for e in far(c))
    c = cases.case("n65_priors_no_fixed")
    assert not c["fixed"].any() and [p[0] for p in c["priors"]] == [0, 64]
    info = c["priors"][1][3]
    assert not info[:3].any() and not info[:, :3].any() and np.linalg.eigvalsh(info[3:, 3:]).min() > 1.0
    c = cases.case("n257_mixed")
    assert c["fixed"].nonzero()[0].tolist() == [100, 256] and len(c["priors"]) == 5 and [p[0] for p in c["priors"]].count(128) == 2
    assert all(k == (rref.CAUCHY if q[1] - q[0] >= 2 else rref.HUBER) for q, (k, _) in zip(c["edges"], c["edge_loss"]))
    assert cases.case("prior_on_fixed")["fixed"][cases.case("prior_on_fixed")["priors"][0][0]] == 1
    c, plain = cases.case("n64_false_loop_cauchy"), cases.case("n64_false_loop_plain")
    assert [q[:2] for q in c["edges"][-4:]] == cases.LOOPS64 and all(np.array_equal(x[3], y[3]) for x, y in zip(c["edges"], plain["edges"]))
    for n in cases.REGULAR + cases.SINGULAR:
        assert all(np.array_equal(p[3], p[3].T) for p in cases.case(n)["priors"])


# ---- the ABI without a device -----------------------------------------------------------------------------------------------
def test_abi_symbols():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in NEW_FUNCS:
        assert hasattr(L, f) and f in capi.EXPORTS, f
    assert L.mh_abi_version() == 3
    assert (capi.MH_PGO_LOSS_NONE, capi.MH_PGO_LOSS_HUBER, capi.MH_PGO_LOSS_CAUCHY, capi.MH_PGO_LOSS_DCS) == (0, 1, 2, 3)


def test_struct_layouts_match_the_header(tmp_path):
    from mimosa_amd import capi
    structs = [("mh_pose_prior", capi.PosePrior, 392), ("mh_pose_graph_loss", capi.PoseGraphLoss, 16)]
    items = [("MH_PGO_LOSS_NONE", 0), ("MH_PGO_LOSS_HUBER", 1), ("MH_PGO_LOSS_CAUCHY", 2), ("MH_PGO_LOSS_DCS", 3), ("MH_ABI_VERSION", 3)]
    for name, cls, size in structs:
        assert C.sizeof(cls) == size
        items.append(("sizeof(%s)" % name, size))
        items += [("offsetof(%s, %s)" % (name, n), getattr(cls, n).offset) for n, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mimosa_hip.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu\\n", (size_t)%s);\n' % e for e, _ in items) + "  return 0;\n}\n")
    out = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", out])
    got = [int(v) for v in subprocess.run([out], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [v for _, v in items], [(e, g, v) for (e, v), g in zip(items, got) if g != v]


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    INV = capi.MH_ERR_INVALID_ARG
    f = C.c_double()
    calls = [("mh_pose_graph_set_priors", lambda: L.mh_pose_graph_set_priors(None, None, 0)),
             ("mh_pose_graph_set_loss", lambda: L.mh_pose_graph_set_loss(None, None, None)),
             ("mh_pose_graph_prior_residuals", lambda: L.mh_pose_graph_prior_residuals(None, None, None)),
             ("mh_pose_graph_weights", lambda: L.mh_pose_graph_weights(None, None, None, C.byref(f)))]
    for name, call in calls:
        assert call() == INV and (name + ": NULL argument").encode() in L.mh_last_error(None), name
