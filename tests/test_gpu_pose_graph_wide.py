"""-m gpu: the wide pose graph (mh_pose_graph_create_wide) on the device, through the C ABI.  The graphs of
tests/pose_graph_wide_cases.py against the dense numpy restatement to the bars of tests/test_pose_graph_wide_cpu.py, which also
asserts, on the restatement alone, the conditions these tests rest on; a wide graph of at most MH_PGO_FAR_MAX far edges against a
plain graph, bit for bit; bit reproducibility on a repeat and across check_every; the singular cases; a robust case; residuals and
weights that move nothing; covariances; refusals; use after mh_shutdown."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_robust_ref as rref
import pose_graph_wide_cases as cases
from pose_graph_wide_cases import POSE_TOL, W_TOL, f_close

pytestmark = pytest.mark.gpu


def as_dicts(edges):
    return [{"a": a, "b": b, "Z": (ZR, Zt), "info": Om} for a, b, ZR, Zt, Om in edges]


def graph_of(ctx, c, max_far, slack=0):
    """the case on the device: a wide graph for max_far far edges (None: a plain graph), created for exactly its size (+ slack)"""
    from mimosa_amd import capi
    pg = capi.PoseGraph(ctx, len(c["R"]) + slack, len(c["edges"]) + slack, max_far=max_far)
    pg.set_poses(c["R"], c["t"])
    pg.set_fixed(c["fixed"])
    pg.set_edges(as_dicts(c["edges"]))
    if c["edge_loss"] is not None:
        pg.set_loss(edges=c["edge_loss"])
    return pg


def split(rows):
    rows = np.asarray(rows).reshape(-1, 12)
    return rows[:, :9].reshape(-1, 3, 3), rows[:, 9:]


# ---- 1. against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REGULAR)
def test_chain_against_the_restatement(ctx, name):
    c, want = cases.case(name), cases.restated(name)
    pg = graph_of(ctx, c, cases.n_far(c))              # max_far exactly the case's count: an index past F is past the arrays
    got = pg.optimise(iters=cases.ITERS, eps_rot=0.0, eps_trans=0.0, damping=c["damping"], trace_poses=True)
    assert (got["iters"], got["converged"], got["n_poses"]) == (cases.ITERS, 0, len(c["R"]))
    assert got["n_far"] == cases.n_far(c) > 32
    worst = [0.0, 0.0, 0.0]
    for row, poses, w in zip(got["trace"], got["trace_poses"], want["trace"]):
        assert row["flags"] == 0
        dt, dr = ref.pose_error(*split(poses), w["R"], w["t"])
        worst = [max(worst[0], dt), max(worst[1], dr), max(worst[2], abs(row["f"] - w["f"]) / max(abs(w["f"]), 1e-300))]
        assert dt <= POSE_TOL and dr <= POSE_TOL, (name, dt, dr)
        assert f_close(row["f"], w["f"], len(c["edges"])), (name, row["f"], w["f"])
        assert abs(row["step_rot"] - w["step_rot"]) <= POSE_TOL and abs(row["step_trans"] - w["step_trans"]) <= POSE_TOL
    dt, dr = ref.pose_error(got["R"], got["t"], want["R"], want["t"])
    print("%s (%d far edges): largest difference to the restatement over %d iterations: %.3g m, %.3g rad, f %.3g relative; final poses %.3g m, %.3g rad"
          % (name, got["n_far"], cases.ITERS, *worst, dt, dr))
    assert dt <= POSE_TOL and dr <= POSE_TOL
    R, t = split(got["trace_poses"][-1])
    assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t)
    fixed = np.flatnonzero(c["fixed"])
    assert np.array_equal(R[fixed], c["R"][fixed]) and np.array_equal(t[fixed], c["t"][fixed])
    pg.destroy()


# ---- 2. a wide graph of at most MH_PGO_FAR_MAX far edges has a plain graph's bits ------------------------------------------------
@pytest.mark.parametrize("name", cases.PLAIN)
def test_a_wide_graph_has_the_bits_of_a_plain_one(ctx, name):
    c = cases.case(name)
    runs = []
    for max_far in (None, 64, 512):
        pg = graph_of(ctx, c, max_far)
        runs.append(pg.optimise(iters=6, eps_rot=0.0, eps_trans=0.0, trace_poses=True))
        pg.destroy()
    a = runs[0]
    assert a["iters"] == 6 and all(q["flags"] == 0 for q in a["trace"])
    for b in runs[1:]:
        assert (b["iters"], b["n_far"]) == (a["iters"], a["n_far"]) and b["trace"] == a["trace"]
        assert np.array_equal(b["trace_poses"], a["trace_poses"]) and np.array_equal(b["R"], a["R"]) and np.array_equal(b["t"], a["t"])


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------------------
def test_bit_identical_on_a_repeat_and_across_check_every(ctx):
    c = cases.case("w120_far128")
    runs = []
    for check_every, max_far, slack in ((0, 128, 0), (0, 128, 0), (1, 128, 0), (3, 200, 7)):
        pg = graph_of(ctx, c, max_far, slack)
        runs.append(pg.optimise(iters=64, check_every=check_every, eps_rot=1e-6, eps_trans=1e-6, trace_poses=True))
        pg.destroy()
    a = runs[0]
    assert a["converged"] == 1 and a["iters"] < 64
    for b in runs[1:]:
        assert (b["iters"], b["converged"]) == (a["iters"], a["converged"]) and b["trace"] == a["trace"]
        assert np.array_equal(b["trace_poses"], a["trace_poses"]) and np.array_equal(b["R"], a["R"]) and np.array_equal(b["t"], a["t"])


# ---- 4. singular and robust cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.SINGULAR)
def test_singular_cases_take_no_step(ctx, name):
    c = cases.case(name)
    pg = graph_of(ctx, c, max(cases.n_far(c), 1))
    got = pg.optimise(iters=8, eps_rot=0.0, eps_trans=0.0, trace_poses=True)
    assert (got["iters"], got["converged"]) == (1, 0) and got["trace"][0]["flags"] == 4
    assert got["trace"][0]["step_rot"] == 0.0 and got["trace"][0]["step_trans"] == 0.0
    assert np.array_equal(got["R"], c["R"]) and np.array_equal(got["t"], c["t"])
    assert f_close(got["trace"][0]["f"], ref.residuals(c["R"], c["t"], c["edges"])[2], len(c["edges"]))
    pg.destroy()


def test_robust_case_against_the_restatement(ctx):
    c, want = cases.case(cases.ROBUST), cases.restated(cases.ROBUST)
    pg = graph_of(ctx, c, 70)
    got = pg.optimise(iters=cases.ITERS, eps_rot=0.0, eps_trans=0.0, trace_poses=True)
    assert got["iters"] == cases.ITERS and got["n_far"] == 70
    worst = [0.0, 0.0]
    for row, poses, w in zip(got["trace"], got["trace_poses"], want["trace"]):
        assert row["flags"] == 0
        dt, dr = ref.pose_error(*split(poses), w["R"], w["t"])
        worst = [max(worst[0], dt), max(worst[1], dr)]
        assert dt <= POSE_TOL and dr <= POSE_TOL and f_close(row["f"], w["f"], len(c["edges"])), (dt, dr, row["f"], w["f"])
    we, _, f = pg.weights()
    ww, _, wf = rref.weights(want["R"], want["t"], c["edges"], [], c["edge_loss"], None)
    dw = np.abs(we - ww).max()
    print("%s: largest difference to the restatement: %.3g m, %.3g rad, final weights %.3g; the false loop's weight %.3g" % (cases.ROBUST, *worst, dw, we[-1]))
    assert dw <= W_TOL and f_close(f, wf, len(c["edges"])) and we[-1] < 0.01
    pg.destroy()


# ---- 5. residuals and weights move nothing ----------------------------------------------------------------------------------------
def test_residuals_and_weights_move_nothing(ctx):
    c = cases.case("w80_far70")
    r, chi2, f = ref.residuals(c["R"], c["t"], c["edges"])
    pg = graph_of(ctx, c, 70)
    gr, gchi2, gf = pg.residuals()
    assert np.abs(gr - r).max() <= POSE_TOL and f_close(gf, f, len(chi2))
    we, _, wf = pg.weights()
    assert np.all(we == 1.0) and f_close(wf, gf, len(chi2))
    R, t = pg.poses()
    assert np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])
    again = pg.residuals()
    assert np.array_equal(again[0], gr) and np.array_equal(again[1], gchi2) and again[2] == gf
    assert pg.optimise(iters=1, eps_rot=0.0, eps_trans=0.0)["f_first"] == gf
    pg.destroy()


# ---- 6. covariances ---------------------------------------------------------------------------------------------------------------
def test_covariances_of_a_wide_graph(ctx):
    """holding at most MH_PGO_FAR_MAX far edges: a plain graph's bits; holding more: MH_ERR_UNSUPPORTED, nothing written"""
    from mimosa_amd import capi
    c = cases.case("n300_far32")
    pairs = [(0, 299), (10, 290), (148, 152)]
    plain, wide = graph_of(ctx, c, None), graph_of(ctx, c, 512)
    a, b = plain.covariances(0.0, pairs), wide.covariances(0.0, pairs)
    assert a[2] == b[2] and a[2]["flags"] == 0 and a[2]["n_far"] == 32
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.isfinite(a[0]).all()
    plain.destroy()
    wide.destroy()

    L = ctx.L
    L.mh_last_error.restype = C.c_char_p
    c = cases.case("w40_far33")
    pg = graph_of(ctx, c, 33)
    cov, info = np.full((40, 6, 6), np.nan), capi.PoseGraphCovInfo()
    assert L.mh_pose_graph_covariances(pg.h, 0.0, capi._p(cov), None, 0, None, C.byref(info)) == capi.MH_ERR_UNSUPPORTED
    assert b"MH_PGO_FAR_MAX" in L.mh_last_error(ctx.h) and np.isnan(cov).all()
    R, t = pg.poses()
    assert np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])
    pg.destroy()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_set_edges_past_max_far_is_refused(ctx):
    from mimosa_amd import capi
    L = ctx.L
    L.mh_last_error.restype = C.c_char_p
    c = cases.case("w40_far33")
    pg = graph_of(ctx, c, 33, slack=1)
    want = pg.residuals()
    a, b, ZR, Zt, Om = c["edges"][-1]
    edges = as_dicts(c["edges"]) + [{"a": 10, "b": 12, "Z": (ZR, Zt), "info": Om}]
    assert L.mh_pose_graph_set_edges(pg.h, capi.make_window_edge(edges), len(edges)) == capi.MH_ERR_UNSUPPORTED
    msg = L.mh_last_error(ctx.h)
    assert b"max_far" in msg and b"MH_PGO_FAR_MAX" not in msg
    got = pg.residuals()                                   # the graph keeps what it had
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert pg.optimise(iters=1, eps_rot=0.0, eps_trans=0.0)["n_far"] == 33
    pg.destroy()
    # a plain graph still refuses a 33rd far edge by its own name
    plain = capi.PoseGraph(ctx, 40, len(c["edges"]))
    plain.set_poses(c["R"], c["t"])
    assert L.mh_pose_graph_set_edges(plain.h, capi.make_window_edge(as_dicts(c["edges"])), len(c["edges"])) == capi.MH_ERR_UNSUPPORTED
    assert b"MH_PGO_FAR_MAX" in L.mh_last_error(ctx.h)
    plain.destroy()
    h = C.c_void_p()
    for far in (0, 513):
        assert L.mh_pose_graph_create_wide(ctx.h, 16, 16, far, C.byref(h)) == capi.MH_ERR_INVALID_ARG and b"max_far" in L.mh_last_error(ctx.h) and not h.value


def test_use_after_shutdown_is_refused():
    from mimosa_amd import capi
    L, p, INV = capi.load(), capi._p, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    h, pg = C.c_void_p(), C.c_void_p()
    assert L.mh_init(0, C.byref(h)) == capi.MH_OK
    assert L.mh_pose_graph_create_wide(h, 40, 80, 64, C.byref(pg)) == capi.MH_OK
    c = cases.case("w40_far33")
    R, t = c["R"].reshape(-1, 9).copy(), c["t"].copy()
    edges = capi.make_window_edge(as_dicts(c["edges"]))
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 40) == capi.MH_OK and L.mh_pose_graph_set_edges(pg, edges, len(c["edges"])) == capi.MH_OK
    L.mh_shutdown(h)
    cfg, res, f = capi.make_pose_graph_config(), capi.PoseGraphResult(), C.c_double()
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 40) == INV and b"shut down" in L.mh_last_error(None)
    assert L.mh_pose_graph_set_edges(pg, edges, len(c["edges"])) == INV
    assert L.mh_pose_graph_residuals(pg, None, None, C.byref(f)) == INV
    assert L.mh_pose_graph_optimise(pg, C.byref(cfg), C.byref(res), None) == INV and b"shut down" in L.mh_last_error(None)
    L.mh_pose_graph_destroy(pg)
