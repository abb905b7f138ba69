"""The start of an mh_icp_window_* call without a device: mimosa_amd/csrc/window_request.hpp (the request record and every
payload check, in the order the ABI promises) compiled with g++ (tests/cpp/window_request_check.cpp).  Every refusal with its
exact code and message — the messages are written out here as the library has always worded them, not read from the header;
the order of the checks, pair by adjacent pair; the separator of the joint marginal over every edge set and joint factor of a
window of six poses; an accepted request of each kind.  The same program once more as a stand-alone binary under
AddressSanitizer and UBSan, every array sized to its request exactly."""
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 5
KINDS = ("optimise", "marginal", "marginal_joint")
NULLS = {"icps": 0, "R": 1, "t": 2, "has_Z": 3, "Z_R": 4, "Z_t": 5, "g_unit": 6, "cfg": 7, "out": 8, "lin": 9, "edges": 10}
HOOK = "the factors' own checks"  # what the program's stand-in for the factors' checks refuses with (MH_ERR_UNSUPPORTED)

# ---- the messages, as the library words them ---------------------------------------------------------------------------------
M_RELIN_NULL = "mh_icp_window_optimise_relin: NULL argument"
M_EDGE_MANY = "mh_icp_window_optimise_edges: at most 32 edges per call"
M_EDGE_NULL = "mh_icp_window_optimise_edges: NULL edges"
M_EDGE_RANGE = "mh_icp_window_optimise_edges: an edge needs 0 <= pose_a < pose_b <= W - 1"
M_EDGE_FINITE = "mh_icp_window_optimise_edges: an edge has an entry that is not finite"
M_EDGE_SYMM = "mh_icp_window_optimise_edges: an edge's info is not symmetric"
M_MARG_EDGE = "mh_icp_window_marginalise: an edge from pose 0 beyond pose 1 makes the marginal a joint factor on several poses"
M_JOINT_N = "mh_icp_window_optimise_joint: n_poses must be in 1..4"
M_JOINT_POSES = "mh_icp_window_optimise_joint: the poses must be strictly ascending in 0 .. W - 1"
M_JOINT_FINITE = "mh_icp_window_optimise_joint: the joint factor has an entry that is not finite"
M_JOINT_SYMM = "mh_icp_window_optimise_joint: the joint factor's H is not symmetric"
M_JM_POSE0 = "mh_icp_window_marginalise_joint: a joint factor without pose 0 would stay in the window as a second joint factor"
M_JM_SEP = "mh_icp_window_marginalise_joint: the separator of pose 0 has more than 4 poses"
M_NULL = "mh_icp_window_optimise: NULL argument"
M_NO_POSE = "mh_icp_window_optimise: the window has no pose"
M_MARG_W = "mh_icp_window_marginalise: the window needs a pose behind the oldest"
M_W_MAX = "mh_icp_window_optimise: at most 16 poses per call"
M_NULL_FACTOR = "mh_icp_window_optimise: NULL factor"
M_ITERS = "mh_icp_window_optimise: iters must be in 1..64"
M_CFG = "mh_icp_window_optimise: eps, damping, between_info, prior_info and check_every must be >= 0"
M_RELIN = "mh_icp_window_optimise_relin: relin_rot and relin_trans must be finite and >= 0"
M_LIN_MANY = "mh_icp_window_optimise_lin: at most 32 linear factors per call"
M_LIN_NULL = "mh_icp_window_optimise_lin: NULL linear factors"
M_LIN_POSE = "mh_icp_window_optimise_lin: a linear factor's pose is outside the window"
M_LIN_FINITE = "mh_icp_window_optimise_lin: a linear factor has an entry that is not finite"
M_Z_NULL = "mh_icp_window_optimise: NULL between measurements"


# ---- requests ------------------------------------------------------------------------------------------------------------------
def spd(n, seed):
    A = np.random.default_rng(seed).standard_normal((n, n))
    return A @ A.T + n * np.eye(n)


def edge(a, b, **kw):
    return dict(dict(a=a, b=b, Z_R=np.eye(3), Z_t=np.array([0.1, 0.0, 0.0]), info=spd(6, 100 + 10 * a + b)), **kw)


def linear(pose, **kw):
    return dict(dict(pose=pose, L_R=np.eye(3), L_t=np.zeros(3), H=spd(6, 7), b=np.arange(6.0), f=0.5), **kw)


def joint(poses, n_poses=None, **kw):
    n = len(poses)
    H = np.zeros((24, 24))
    H[:6 * n, :6 * n] = spd(6 * n, n)
    q = dict(n_poses=n if n_poses is None else n_poses, pose=list(poses) + [0] * (4 - n), L_R=np.tile(np.eye(3).ravel(), 4), L_t=np.zeros(12), H=H,
             b=np.zeros(24), f=1.0)
    return dict(q, **kw)


def cfg(**kw):
    return dict(dict(iters=3, check_every=0, between_info=[1.0] * 6, prior_info=[0.0] * 6, damping=0.0, eps_rot=0.0, eps_trans=0.0), **kw)


def request(kind="optimise", W=3, **kw):
    """a request the checks accept; the marginal kinds have a list of linear factors, as their entry points do"""
    q = dict(kind=kind, W=W, relin_required=False, lin_call=kind != "optimise", factors_refuse=False, null_factor=-1, null=(), cfg=cfg(),
             has_Z=[0] + [1] * (W - 1), relin=None, lin=[], n_lin=None, edges=[], n_edges=None, joint=None)
    assert set(kw) <= set(q), set(kw) - set(q)
    return dict(q, **kw)


def nums(*arrays):
    return " ".join(repr(float(v)) for a in arrays for v in np.asarray(a, np.float64).ravel())


def text(q):
    c = q["cfg"]
    out = ["req %d %d %d %d %d %d %d" % (KINDS.index(q["kind"]), q["W"], q["relin_required"], q["lin_call"], q["factors_refuse"], q["null_factor"],
                                         sum(1 << NULLS[n] for n in q["null"])),
           "cfg %d %d %s" % (c["iters"], c["check_every"], nums(c["between_info"], c["prior_info"], c["damping"], c["eps_rot"], c["eps_trans"])),
           "has_Z " + " ".join(str(int(v)) for v in q["has_Z"]),
           "relin 0" if q["relin"] is None else "relin 1 " + nums(q["relin"]),
           "lin %d %d" % (len(q["lin"]) if q["n_lin"] is None else q["n_lin"], len(q["lin"]))]
    out += ["%d %s" % (f["pose"], nums(f["L_R"], f["L_t"], f["H"], f["b"], f["f"])) for f in q["lin"]]
    out.append("edges %d %d" % (len(q["edges"]) if q["n_edges"] is None else q["n_edges"], len(q["edges"])))
    out += ["%d %d %s" % (e["a"], e["b"], nums(e["Z_R"], e["Z_t"], e["info"])) for e in q["edges"]]
    j = q["joint"]
    out.append("joint 0" if j is None else "joint 1 %d %s %s" % (j["n_poses"], " ".join(str(p) for p in j["pose"]), nums(j["L_R"], j["L_t"], j["H"], j["b"], j["f"])))
    return "\n".join(out) + "\n"


def run(exe, requests, timeout=600):
    out = subprocess.run([exe], input="".join(text(q) for q in requests), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    rows = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(rows) == len(requests)
    return rows


# ---- the table: one row per refusal ------------------------------------------------------------------------------------------
def bad(a, where, value):
    a = np.array(a, np.float64)
    a.flat[where] = value
    return a


def refusal_table():
    T = []  # (id, request, code, message)
    W = 3
    good = [edge(0, 1), edge(1, 2), edge(0, 2)]
    T.append(("relin_required", request(relin_required=True), INVALID, M_RELIN_NULL))
    for kind in KINDS:
        # the marginal kinds with edges that stay inside what they take: (0, 2) is the plain marginal's own refusal
        ok = good if kind != "marginal" else good[:2]
        r = lambda edges, **kw: request(kind, edges=edges, **kw)
        T.append((kind + "-33_edges", r([ok[0]] * 33), INVALID, M_EDGE_MANY))
        T.append((kind + "-null_edges", r([], n_edges=2, null=("edges",)), INVALID, M_EDGE_NULL))
        for a, b in ((-1, 1), (0, W), (0, 16), (1, 1), (2, 1)):
            T.append((kind + "-edge_%d_%d" % (a, b), r([ok[0], edge(a, b)]), INVALID, M_EDGE_RANGE))
        for name, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
            T.append((kind + "-edge_info_" + name, r([ok[0], edge(1, 2, info=bad(ok[1]["info"], 7, v))]), INVALID, M_EDGE_FINITE))
            T.append((kind + "-edge_Z_R_" + name, r([edge(1, 2, Z_R=bad(np.eye(3), 4, v))]), INVALID, M_EDGE_FINITE))
            T.append((kind + "-edge_Z_t_" + name, r([edge(1, 2, Z_t=bad(np.zeros(3), 2, v))]), INVALID, M_EDGE_FINITE))
        info = ok[0]["info"].copy()
        info[1, 4] += 1.0
        T.append((kind + "-edge_info_asymmetric", r([edge(0, 1, info=info)]), INVALID, M_EDGE_SYMM))
        # the joint factor
        first = 0 if kind == "marginal_joint" else 1
        for n in (0, 5):
            T.append((kind + "-joint_n_poses_%d" % n, request(kind, W=4, joint=joint([first, 2], n_poses=n)), INVALID, M_JOINT_N))
        T.append((kind + "-joint_not_ascending", request(kind, W=4, joint=joint([first, 3, 2])), INVALID, M_JOINT_POSES))
        T.append((kind + "-joint_pose_twice", request(kind, W=4, joint=joint([first, 2, 2])), INVALID, M_JOINT_POSES))
        T.append((kind + "-joint_pose_W", request(kind, W=4, joint=joint([first, 4])), INVALID, M_JOINT_POSES))
        T.append((kind + "-joint_pose_negative", request(kind, W=4, joint=joint([-1, 2])), INVALID, M_JOINT_POSES))
        g = joint([first, 2])
        for name, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
            T.append((kind + "-joint_H_" + name, request(kind, W=4, joint=dict(g, H=bad(g["H"], 24 * 3 + 11, v))), INVALID, M_JOINT_FINITE))
        T.append((kind + "-joint_b_nan", request(kind, W=4, joint=dict(g, b=bad(g["b"], 11, np.nan))), INVALID, M_JOINT_FINITE))
        T.append((kind + "-joint_L_R_nan", request(kind, W=4, joint=dict(g, L_R=bad(g["L_R"], 17, np.nan))), INVALID, M_JOINT_FINITE))
        T.append((kind + "-joint_L_t_nan", request(kind, W=4, joint=dict(g, L_t=bad(g["L_t"], 5, np.nan))), INVALID, M_JOINT_FINITE))
        T.append((kind + "-joint_f_inf", request(kind, W=4, joint=dict(g, f=np.inf)), INVALID, M_JOINT_FINITE))
        H = g["H"].copy()
        H[2, 9] += 1.0
        T.append((kind + "-joint_H_asymmetric", request(kind, W=4, joint=dict(g, H=H)), INVALID, M_JOINT_SYMM))
        # the arguments and W
        for name in ("icps", "R", "t", "has_Z", "g_unit", "cfg", "out"):
            T.append((kind + "-null_" + name, request(kind, null=(name,)), INVALID, M_NULL))
        T.append((kind + "-W_0", request(kind, W=0, has_Z=[]), INVALID, M_NO_POSE))
        T.append((kind + "-W_17", request(kind, W=17), UNSUPPORTED, M_W_MAX))
        for f in (0, 2):
            T.append((kind + "-null_factor_%d" % f, request(kind, null_factor=f), INVALID, M_NULL_FACTOR))
        # the config
        for iters in (0, -1, 65):
            T.append((kind + "-iters_%d" % iters, request(kind, cfg=cfg(iters=iters)), INVALID, M_ITERS))
        for name, c in (("damping", cfg(damping=-1.0)), ("eps_rot", cfg(eps_rot=-1e-9)), ("eps_trans", cfg(eps_trans=np.nan)), ("check_every", cfg(check_every=-1)),
                        ("between_info", cfg(between_info=[1.0] * 5 + [-1.0])), ("prior_info", cfg(prior_info=[np.nan] + [0.0] * 5))):
            T.append((kind + "-cfg_" + name, request(kind, cfg=c), INVALID, M_CFG))
        # the linear factors
        T.append((kind + "-33_linear", request(kind, lin_call=True, lin=[linear(0)] * 33), INVALID, M_LIN_MANY))
        T.append((kind + "-null_linear", request(kind, lin_call=True, n_lin=2, null=("lin",)), INVALID, M_LIN_NULL))
        for pose in (-1, W):
            T.append((kind + "-linear_pose_%d" % pose, request(kind, lin_call=True, lin=[linear(0), linear(pose)]), INVALID, M_LIN_POSE))
        for name, f in (("H", linear(1, H=bad(spd(6, 7), 35, np.nan))), ("b", linear(1, b=bad(np.zeros(6), 0, np.inf))), ("f", linear(1, f=-np.inf)),
                        ("L_R", linear(1, L_R=bad(np.eye(3), 8, np.nan))), ("L_t", linear(1, L_t=bad(np.zeros(3), 1, np.nan)))):
            T.append((kind + "-linear_%s_not_finite" % name, request(kind, lin_call=True, lin=[linear(0), f]), INVALID, M_LIN_FINITE))
        # the between measurements
        T.append((kind + "-null_Z_R", request(kind, null=("Z_R",)), INVALID, M_Z_NULL))
        T.append((kind + "-null_Z_t", request(kind, null=("Z_t",)), INVALID, M_Z_NULL))
    # what only one kind refuses
    T.append(("marginal-edge_0_2", request("marginal", edges=[edge(0, 1), edge(0, 2)]), UNSUPPORTED, M_MARG_EDGE))
    T.append(("marginal-W_1", request("marginal", W=1), INVALID, M_MARG_W))
    T.append(("marginal_joint-W_1", request("marginal_joint", W=1), INVALID, M_MARG_W))
    T.append(("marginal_joint-joint_1_2_3", request("marginal_joint", W=4, joint=joint([1, 2, 3])), UNSUPPORTED, M_JM_POSE0))
    T.append(("marginal_joint-separator_5", request("marginal_joint", W=6, edges=[edge(0, b) for b in (2, 3, 4, 5)]), UNSUPPORTED, M_JM_SEP))
    for name, rl in (("rot_negative", (-1.0, 5e-3)), ("trans_negative", (1e-3, -1.0)), ("rot_nan", (np.nan, 5e-3)), ("trans_inf", (1e-3, np.inf))):
        T.append(("relin_" + name, request(relin=rl), INVALID, M_RELIN))
    return T


def order_table():
    """for each adjacent pair of steps of the order, a request wrong in both ways: the earlier one is reported.  The steps: 1 relin
    required, 2 edges, 3 the plain marginal's edge, 4 the joint factor, 5 the joint marginal's pose 0 and separator, 6 arguments and
    W, 7 the factors' own checks, 8 config, 9 relin thresholds, 10 linear factors, 11 between measurements.  3 and 5 belong to one
    kind each, so their neighbours are paired across them as well."""
    nan_edge = edge(1, 2, Z_t=[np.nan, 0.0, 0.0])
    wide = [edge(0, b) for b in (2, 3, 4, 5)]
    T = []
    T.append(("1_2", request(relin_required=True, edges=[edge(0, 1)] * 33), INVALID, M_RELIN_NULL))
    T.append(("2_3", request("marginal", edges=[edge(0, 2), nan_edge]), INVALID, M_EDGE_FINITE))
    T.append(("2_4", request(edges=[nan_edge], joint=joint([0, 1], n_poses=0)), INVALID, M_EDGE_FINITE))
    T.append(("3_4", request("marginal", edges=[edge(0, 2)], joint=joint([0, 1], n_poses=0)), UNSUPPORTED, M_MARG_EDGE))
    T.append(("4_5", request("marginal_joint", W=4, joint=joint([1, 3, 2])), INVALID, M_JOINT_POSES))
    T.append(("5_5", request("marginal_joint", W=6, edges=wide, joint=joint([1, 2])), UNSUPPORTED, M_JM_POSE0))
    T.append(("3_6", request("marginal", edges=[edge(0, 2)], null=("R",)), UNSUPPORTED, M_MARG_EDGE))
    T.append(("4_6", request(joint=joint([0, 1], n_poses=5), null=("cfg",)), INVALID, M_JOINT_N))
    T.append(("5_6", request("marginal_joint", W=6, edges=wide, null=("R",)), UNSUPPORTED, M_JM_SEP))
    T.append(("6_6", request("marginal", W=1, null_factor=0, has_Z=[0]), INVALID, M_MARG_W))
    T.append(("6_7", request(null_factor=1, factors_refuse=True), INVALID, M_NULL_FACTOR))
    T.append(("7_8", request(factors_refuse=True, cfg=cfg(iters=0)), UNSUPPORTED, HOOK))
    T.append(("8_8", request(cfg=cfg(iters=0, damping=-1.0)), INVALID, M_ITERS))
    T.append(("8_9", request(cfg=cfg(damping=-1.0), relin=(np.nan, 0.0)), INVALID, M_CFG))
    T.append(("9_10", request(relin=(np.nan, 0.0), lin_call=True, lin=[linear(0)] * 33), INVALID, M_RELIN))
    T.append(("10_11", request(lin_call=True, lin=[linear(3)], null=("Z_R",)), INVALID, M_LIN_POSE))
    return T


def separator_table():
    """W = 6, the joint marginal: every subset of the edges (0, b), b in 1..5, with every joint factor on {0} and up to three of the
    poses 1..5, and with none — 32 x 27 requests"""
    T = []
    subsets = [s for n in range(4) for s in itertools.combinations(range(1, 6), n)]
    assert len(subsets) == 26
    for bs in itertools.chain.from_iterable(itertools.combinations(range(1, 6), n) for n in range(6)):
        for S in [None] + subsets:
            want = sorted({1} | set(bs) | set(S or ()))
            q = request("marginal_joint", W=6, edges=[edge(0, b) for b in bs], joint=None if S is None else joint([0] + list(S)))
            T.append((q, want))
    assert len(T) == 32 * 27
    return T


REFUSALS, ORDER = refusal_table(), order_table()


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("window_request_check")


@pytest.fixture(scope="module")
def answers(exe):
    rows = run(exe, [q for _, q, _, _ in REFUSALS + ORDER])
    return {name: row for (name, _, _, _), row in zip(REFUSALS + ORDER, rows)}


def test_table_ids_are_unique_and_every_message_is_in_it():
    ids = [name for name, _, _, _ in REFUSALS + ORDER]
    assert len(ids) == len(set(ids))
    said = {m for _, _, _, m in REFUSALS}
    assert said == {v for k, v in globals().items() if k.startswith("M_")}


@pytest.mark.parametrize("name,code,message", [(n, c, m) for n, _, c, m in REFUSALS], ids=[n for n, _, _, _ in REFUSALS])
def test_refusal(answers, name, code, message):
    assert (answers[name]["code"], answers[name]["message"]) == (code, message)


@pytest.mark.parametrize("name,code,message", [(n, c, m) for n, _, c, m in ORDER], ids=[n for n, _, _, _ in ORDER])
def test_the_earlier_check_is_reported(answers, name, code, message):
    assert (answers[name]["code"], answers[name]["message"]) == (code, message)


def test_separator_exhaustively_at_six_poses(exe):
    table = separator_table()
    rows = run(exe, [q for q, _ in table])
    refused = 0
    for (q, want), got in zip(table, rows):
        assert got["n_sep"] == len(want)
        assert got["sep"] == (want + [0] * 4)[:4]
        if len(want) > 4:
            refused += 1
            assert (got["code"], got["message"]) == (UNSUPPORTED, M_JM_SEP)
        else:
            assert (got["code"], got["message"], got["zmask"]) == (OK, "", 0b111110)
    assert 0 < refused < len(table)


def accepted_requests():
    full = dict(relin=(1e-3, 5e-3), lin_call=True, lin=[linear(0), linear(3)], edges=[edge(0, 1), edge(1, 3)])
    return [(request(kind, W=4, has_Z=[1, 1, 0, 1]), 0b1010) for kind in KINDS] + \
           [(request(kind, W=2, has_Z=[1, 0], null=("Z_R", "Z_t")), 0) for kind in KINDS] + \
           [(request("optimise", W=1, has_Z=[1], null=("Z_R", "Z_t")), 0),                    # pose 0 has no between measurement
            (request("optimise", W=16, cfg=cfg(iters=64)), 0xfffe),
            (request("optimise", W=4, relin_required=True, **full), 0b1110),
            (request("optimise", W=4, joint=joint([1, 2, 3]), **full), 0b1110),
            (request("marginal", W=4, lin=full["lin"], edges=full["edges"]), 0b1110),
            (request("marginal_joint", W=4, lin=full["lin"], edges=full["edges"] + [edge(0, 3)], joint=joint([0, 2])), 0b1110)]


def test_accepted_requests(exe):
    table = accepted_requests()
    for (q, zmask), got in zip(table, run(exe, [q for q, _ in table])):
        assert (got["code"], got["message"], got["zmask"]) == (OK, "", zmask), q["kind"]
        if q["kind"] != "marginal_joint":
            assert got["n_sep"] == 0 and got["sep"] == [0, 0, 0, 0]
    assert run(exe, [table[-1][0]])[0]["sep"] == [1, 2, 3, 0]


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined, on every request of this file: same output, no
    report.  A check that read behind n_edges edges, n_lin factors or W entries would be one."""
    from mimosa_amd import build
    san = str(tmp_path / "window_request_check_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "window_request_check.cpp"), "-o", san])
    requests = [q for _, q, _, _ in REFUSALS + ORDER] + [q for q, _ in separator_table()] + [q for q, _ in accepted_requests()]
    payload = "".join(text(q) for q in requests)
    a = subprocess.run([san], input=payload, capture_output=True, text=True, timeout=900)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=payload, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) == len(requests)
