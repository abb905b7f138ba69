"""CPU half of the pose graph's marginal covariances (mh_pose_graph_covariances, rule 10 in include/mimosa_hip.h):
mimosa_amd/csrc/pose_graph_device.hpp compiled with g++ (tests/cpp/pose_graph_cov_step.cpp, pgo_cov_host) against the dense
restatement (tests/pose_graph_cov_ref.py) on the cases of tests/pose_graph_cov_cases.py — the very graphs
tests/test_gpu_pose_graph_cov.py hands the device — to a bar measured per case (16 x the error of numpy.linalg.inv, see
pose_graph_cov_cases).  The same program once more as a stand-alone binary under AddressSanitizer and UBSan.  The ABI without a
device.  The conditions the gate's GPU tests rest on are asserted on the restatement alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pose_graph_cov_cases as cases
import pose_graph_cov_ref as cref
import pose_graph_robust_cases as robust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("pose_graph_cov_step")


def hx(v):
    return float(v).hex()


def graph_text(c, pairs):
    n, E, P = len(c["R"]), len(c["edges"]), len(c["priors"])
    el = c["edge_loss"] or [(0, 0.0)] * E
    pl = c["prior_loss"] or [(0, 0.0)] * P
    out = ["graph %d %d %d %d %s" % (n, E, P, len(pairs), hx(c["damping"]))]
    out.append(" ".join(hx(v) for i in range(n) for v in list(c["R"][i].ravel()) + list(c["t"][i])))
    out.append(" ".join(str(int(v)) for v in c["fixed"]))
    for (a, b, ZR, Zt, Om), (kind, param) in zip(c["edges"], el):
        out.append("%d %d %s %d %s" % (a, b, " ".join(hx(v) for v in list(ZR.ravel()) + list(Zt) + list(Om.ravel())), kind, hx(param)))
    for (i, ZR, Zt, Om), (kind, param) in zip(c["priors"], pl):
        out.append("%d %s %d %s" % (i, " ".join(hx(v) for v in list(ZR.ravel()) + list(Zt) + list(Om.ravel())), kind, hx(param)))
    out.append(" ".join("%d %d" % p for p in pairs))
    return "\n".join(out) + "\n"


def parse(line):
    row = json.loads(line)
    fx = lambda v: np.array([float.fromhex(s) for s in v])
    return row["flags"], row["n_far"], fx(row["cov"]).reshape(-1, 6, 6), fx(row["joint"]).reshape(-1, 12, 12)


def run(exe, text, timeout=600):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return [parse(line) for line in out.stdout.splitlines()]


@pytest.fixture(scope="module")
def computed(exe):
    """every case once, with its 64 pairs (pairs_of first), and once more with its first pair alone"""
    names = list(cases.CASES)
    text = "".join(graph_text(cases.case(n), cases.pairs64(n)) for n in names)
    text += "".join(graph_text(cases.case(n), cases.pairs_of(n)[:1]) for n in names)
    rows = run(exe, text)
    return {n: (rows[k], rows[len(names) + k]) for k, n in enumerate(names)}


# ---- the header against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CASES)
def test_covariances_against_the_restatement(computed, name):
    c, want = cases.case(name), cases.restated(name)
    (flags, n_far, cov, joint), _ = computed[name]
    assert flags == 0 and n_far == sum(1 for e in c["edges"] if e[1] - e[0] >= 2) and len(cov) == len(c["R"])
    err = cases.compare(name, cov, joint)
    print("%s: relative error %.3g; numpy.linalg.inv %.3g; ratio %.2f; bar %.3g; largest entry %.3g" % (name, err, want["err_np"], err / max(want["err_np"], 1e-300),
                                                                                                         want["bar"], want["scale"]))
    assert err <= want["bar"], (name, err, want["err_np"])


@pytest.mark.parametrize("name", cases.CASES)
def test_exact_properties(computed, name):
    (_, _, cov, joint), (_, _, cov1, joint1) = computed[name]
    cases.exact_properties(cases.case(name), cov, cases.pairs64(name), joint)
    assert np.array_equal(cov, cov1)                       # cov does not depend on the pairs
    if len(joint1):
        assert np.array_equal(joint[0], joint1[0])         # a pair alone has the bits it has among 64


@pytest.mark.parametrize("name", [n for n in cases.CASES if len(cases.case(n)["R"]) <= 12])
def test_small_graphs_against_mpmath(computed, name):
    want, mp = cases.restated(name), cref.mp_covariances(cases.case(name))
    (_, _, cov, _), _ = computed[name]
    ref_err = max(np.abs(want["cov"][i] - mp[i]).max() for i in mp) / want["scale"]
    err = max(np.abs(cov[i] - mp[i]).max() for i in mp) / want["scale"]
    print("%s against mpmath: the restatement %.3g, the header %.3g (bar %.3g)" % (name, ref_err, err, want["bar"]))
    assert ref_err <= max(want["err_np"], 1e-15) and err <= want["bar"]


def test_every_free_block_is_positive_definite(computed):
    for name in cases.CASES:
        c = cases.case(name)
        (_, _, cov, _), _ = computed[name]
        for i in np.flatnonzero(c["fixed"] == 0):
            assert np.linalg.eigvalsh(cov[i])[0] > 0.0, (name, i)


@pytest.mark.parametrize("name", cases.SINGULAR)
def test_a_pivot_that_is_not_positive(exe, name):
    c = cases.case(name)
    (flags, _, cov, joint), = run(exe, graph_text(c, [(0, 1), (2, 9)]))
    assert flags == 4 and cov.size == 0 and joint.size == 0


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined (every array sized to its call exactly) and run
    on what the other tests feed the plain build: same output, no report"""
    from mimosa_amd import build
    san = str(tmp_path / "pose_graph_cov_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "pose_graph_cov_step.cpp"), "-o", san])
    names = ("n1_prior_only", "n2_two_priors_one_pose", "n3_far", "n12_far_on_fixed_dcs", "n64_false_loop_cauchy", "n65_priors_no_fixed", "no_anchor", "broken_chain")
    text = "".join(graph_text(cases.case(n), cases.pairs64(n) if len(cases.case(n)["R"]) <= 12 else cases.pairs_of(n)) for n in names)
    text += graph_text(cases.case("n257_mixed"), cases.pairs_of("n257_mixed")[:2]) + graph_text(cases.case("n300_far32"), [(0, 299)])
    a = subprocess.run([san], input=text, capture_output=True, text=True, timeout=900)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0 and a.stdout == b.stdout


# ---- the conditions the gate's GPU tests rest on, on the restatement alone ---------------------------------------------------------
held_out = cases.held_out


def test_the_gate_separates_the_false_loop_of_the_64_pose_circuit():
    """odometry alone, pose 0 fixed, the start poses: each true loop's d2 is below a quarter of the chi^2(6) 0.999 quantile and the
    false loop's above four times it, while every true loop's plain chi2 is above the quantile"""
    g, cand = held_out(cases.case("n64_false_loop_cauchy"))
    assert [q[:2] for q in cand] == robust.LOOPS64
    _, joint = cref.covariances(g, [], [q[:2] for q in cand])
    _, chi2, d2 = cref.gate(g["R"], g["t"], cand, joint)
    print("64-pose circuit: chi2 %s, d2 %s" % (chi2, d2))
    assert np.all(d2[:3] < cref.CHI2_6_999 / 4.0) and d2[3] > 4.0 * cref.CHI2_6_999
    assert np.all(chi2[:3] > cref.CHI2_6_999)


def hall_gate():
    """(graph, candidates) of the hall with an aliased loop: the odometry chain, the true loop (0, 35) and the alias (10, 28) held out"""
    case = robust.hall_case()
    R, t = case["drifted"]
    c = dict(R=np.asarray(R), t=np.asarray(t), fixed=np.asarray(case["fixed"]), edges=list(case["edges"]), priors=[], edge_loss=None, prior_loss=None, damping=0.0)
    return held_out(c)


def test_the_hall_condition_on_the_restatement():
    """The hall does NOT separate by a factor of 4 on both sides, so tests/test_gpu_pose_graph_cov.py keeps the 64-pose circuit as
    its only end-to-end gate scene.  Measured on the restatement: the aliased loop (10, 28) has d2 = 2.0e6, far above 4 x 22.46;
    the true loop (0, 35) has d2 = 17.7 — below the 22.46 threshold, so the gate accepts it, but not below a quarter of it.  The
    hall's drift is a constant (3, 2, 0) cm per keyframe, a bias the odometry's info does not describe as noise, so the true
    loop's d2 is three times its expectation of 6.  (Its plain chi2 is 637.)"""
    g, cand = hall_gate()
    assert [q[:2] for q in cand] == [(0, 35), robust.HALL_ALIAS[0]]
    _, joint = cref.covariances(g, [], [q[:2] for q in cand])
    _, chi2, d2 = cref.gate(g["R"], g["t"], cand, joint)
    print("hall: chi2 %s, d2 %s (true loop, aliased loop)" % (chi2, d2))
    assert d2[1] > 4.0 * cref.CHI2_6_999 and cref.CHI2_6_999 / 4.0 <= d2[0] < cref.CHI2_6_999 < chi2[0]


# ---- the ABI without a device -----------------------------------------------------------------------------------------------
def test_abi_symbols():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    assert hasattr(L, "mh_pose_graph_covariances") and "mh_pose_graph_covariances" in capi.EXPORTS
    assert capi.MH_PGO_COV_PAIRS_MAX == 64


def test_struct_layouts_match_the_header(tmp_path):
    from mimosa_amd import capi
    items = [("MH_PGO_COV_PAIRS_MAX", 64), ("sizeof(mh_pose_graph_cov_info)", 16)]
    assert C.sizeof(capi.PoseGraphCovInfo) == 16
    items += [("offsetof(mh_pose_graph_cov_info, %s)" % n, getattr(capi.PoseGraphCovInfo, n).offset) for n, _ in capi.PoseGraphCovInfo._fields_]
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
    info, cov = capi.PoseGraphCovInfo(), (C.c_double * 36)()
    assert L.mh_pose_graph_covariances(None, 0.0, cov, None, 0, None, C.byref(info)) == capi.MH_ERR_INVALID_ARG
    assert b"mh_pose_graph_covariances: NULL argument" in L.mh_last_error(None)
