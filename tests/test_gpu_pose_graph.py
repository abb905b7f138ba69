"""-m gpu: the pose graph over all keyframes (mh_pose_graph_*) on the device, through the C ABI.  The graphs of
tests/pose_graph_cases.py against the numpy restatement (tests/pose_graph_ref.py) to the bars of tests/test_pose_graph_cpu.py,
which also asserts, on the restatement alone, the conditions these tests rest on; bit reproducibility on a repeat and across
check_every; residuals that move nothing; nothing else on the context moving; refusals; use after mh_shutdown."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_ref as ref
from pose_graph_cases import F_RTOL, POSE_TOL, STOP_CASES, f_close, f_floor

pytestmark = pytest.mark.gpu

LIN_KEYS = ("H_ss", "b_s", "f", "status_hist", "loc_trans_comp", "loc_rot_comp")


def as_dicts(edges):
    return [{"a": a, "b": b, "Z": (ZR, Zt), "info": Om} for a, b, ZR, Zt, Om in edges]


def graph_of(ctx, c, slack=0):
    """the case on the device, in a graph created for exactly its size (+ slack)"""
    from mimosa_amd import capi
    pg = capi.PoseGraph(ctx, len(c["R"]) + slack, len(c["edges"]) + slack)
    pg.set_poses(c["R"], c["t"])
    pg.set_fixed(c["fixed"])
    pg.set_edges(as_dicts(c["edges"]))
    return pg


def split(rows):
    rows = np.asarray(rows).reshape(-1, 12)
    return rows[:, :9].reshape(-1, 3, 3), rows[:, 9:]


# ---- 1. against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REGULAR)
def test_chain_against_the_restatement(ctx, name):
    c, want = cases.case(name), cases.restated(name)
    pg = graph_of(ctx, c)
    got = pg.optimise(iters=cases.ITERS, eps_rot=0.0, eps_trans=0.0, damping=c["damping"], trace_poses=True)
    assert (got["iters"], got["converged"], got["n_poses"]) == (cases.ITERS, 0, len(c["R"]))
    assert got["n_far"] == sum(1 for e in c["edges"] if e[1] - e[0] >= 2)
    worst = [0.0, 0.0, 0.0]
    for row, poses, w in zip(got["trace"], got["trace_poses"], want["trace"]):
        assert row["flags"] == 0
        dt, dr = ref.pose_error(*split(poses), w["R"], w["t"])
        worst = [max(worst[0], dt), max(worst[1], dr), max(worst[2], abs(row["f"] - w["f"]) / max(abs(w["f"]), 1e-300))]
        assert dt <= POSE_TOL and dr <= POSE_TOL, (name, dt, dr)
        assert f_close(row["f"], w["f"], len(c["edges"])), (name, row["f"], w["f"])
        assert abs(row["step_rot"] - w["step_rot"]) <= POSE_TOL and abs(row["step_trans"] - w["step_trans"]) <= POSE_TOL
    print("%s: largest difference to the restatement over %d iterations: %.3g m, %.3g rad, f %.3g relative" % (name, cases.ITERS, *worst))
    assert (got["f_first"], got["f_last"]) == (got["trace"][0]["f"], got["trace"][-1]["f"])
    # get_poses after optimise is the result: the last trace row, bit for bit; a fixed pose has not moved a bit
    R, t = split(got["trace_poses"][-1])
    assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t)
    fixed = np.flatnonzero(c["fixed"])
    assert np.array_equal(R[fixed], c["R"][fixed]) and np.array_equal(t[fixed], c["t"][fixed])
    pg.destroy()


@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_test_against_the_restatement(ctx, name):
    c, want = cases.case(name), cases.restated(name, 64, cases.STOP_EPS)
    pg = graph_of(ctx, c)
    got = pg.optimise(iters=64, eps_rot=cases.STOP_EPS, eps_trans=cases.STOP_EPS, trace_poses=True)
    assert (got["iters"], got["converged"]) == (want["iters"], 1) and len(got["trace_poses"]) == want["iters"]
    dt, dr = ref.pose_error(got["R"], got["t"], want["R"], want["t"])
    assert dt <= POSE_TOL and dr <= POSE_TOL
    pg.destroy()


@pytest.mark.parametrize("name", cases.SINGULAR)
def test_singular_cases_take_no_step(ctx, name):
    c = cases.case(name)
    pg = graph_of(ctx, c)
    got = pg.optimise(iters=8, eps_rot=0.0, eps_trans=0.0, trace_poses=True)
    assert (got["iters"], got["converged"]) == (1, 0) and got["trace"][0]["flags"] == 4
    assert got["trace"][0]["step_rot"] == 0.0 and got["trace"][0]["step_trans"] == 0.0
    assert np.array_equal(got["R"], c["R"]) and np.array_equal(got["t"], c["t"])
    assert f_close(got["trace"][0]["f"], ref.residuals(c["R"], c["t"], c["edges"])[2], len(c["edges"]))
    if name == "broken_chain":       # the documented way out: damping makes T positive definite
        want = ref.optimise(c["R"], c["t"], c["fixed"], c["edges"], 6, 1e-3)
        got = pg.optimise(iters=6, eps_rot=0.0, eps_trans=0.0, damping=1e-3)
        assert [q["flags"] for q in got["trace"]] == [0] * 6
        dt, dr = ref.pose_error(got["R"], got["t"], want["R"], want["t"])
        assert dt <= POSE_TOL and dr <= POSE_TOL
    pg.destroy()


# ---- 2. reproducibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("n3_far", "n65", "n300_far32"))
def test_bit_identical_on_a_repeat_and_across_check_every(ctx, name):
    c = cases.case(name)
    runs = []
    for check_every, slack in ((0, 0), (0, 0), (1, 0), (3, 7)):
        pg = graph_of(ctx, c, slack)
        runs.append(pg.optimise(iters=64, check_every=check_every, eps_rot=cases.STOP_EPS, eps_trans=cases.STOP_EPS, trace_poses=True))
        pg.destroy()
    a = runs[0]
    assert a["converged"] == 1 and a["iters"] < 64
    for b in runs[1:]:
        assert (b["iters"], b["converged"]) == (a["iters"], a["converged"]) and b["trace"] == a["trace"]
        assert np.array_equal(b["trace_poses"], a["trace_poses"]) and np.array_equal(b["R"], a["R"]) and np.array_equal(b["t"], a["t"])


def test_a_graph_is_reused(ctx):
    """set_poses again with the same n keeps edges and fixed flags and starts over: the same bits; another n drops them"""
    c = cases.case("n12_far_on_fixed")
    pg = graph_of(ctx, c, slack=5)
    a = pg.optimise(iters=5, eps_rot=0.0, eps_trans=0.0)
    pg.set_poses(c["R"], c["t"])
    b = pg.optimise(iters=5, eps_rot=0.0, eps_trans=0.0)
    assert a["trace"] == b["trace"] and np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])
    pg.set_poses(c["R"][:7], c["t"][:7])
    assert pg.residuals()[2] == 0.0 and pg.n_edges == 0
    got = pg.optimise(iters=2, eps_rot=0.0, eps_trans=0.0)           # no edge, no fixed pose, no damping: T is zero
    assert got["iters"] == 1 and got["trace"][0]["flags"] == 4 and np.array_equal(got["R"], c["R"][:7])
    pg.destroy()


# ---- 3. residuals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("n1", "n3_far", "n65", "n300_far32", "psd_info"))
def test_residuals_against_the_restatement(ctx, name):
    c = cases.case(name)
    r, chi2, f = ref.residuals(c["R"], c["t"], c["edges"])
    pg = graph_of(ctx, c)
    gr, gchi2, gf = pg.residuals()
    assert np.abs(gr - r).max(initial=0.0) <= POSE_TOL
    assert np.all(np.abs(gchi2 - chi2) <= F_RTOL * chi2 + f_floor(1)) and f_close(gf, f, len(chi2))
    R, t = pg.poses()
    assert np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])   # nothing moved
    again = pg.residuals()
    assert np.array_equal(again[0], gr) and np.array_equal(again[1], gchi2) and again[2] == gf
    if name in cases.REGULAR and len(c["edges"]):
        assert pg.optimise(iters=1, eps_rot=0.0, eps_trans=0.0)["f_first"] == gf     # the trace's f is this f, bit for bit
    pg.destroy()


# ---- 4. nothing else moves ------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(ctx, small_world):
    from mimosa_amd import capi
    gm = capi.VoxelMap(ctx)
    gm.insert(small_world["map_xyz"])
    f = capi.ICPFactor(ctx, gm, small_world["pts"], capi.make_reg_config(**small_world["cfg"]))

    def snapshot():
        lin = f.linearize(small_world["R"], small_world["t"])
        f.reset()
        return gm.stats(), {k: np.array(lin[k]) for k in LIN_KEYS}

    before = snapshot()
    c = cases.case("n65")
    pg = graph_of(ctx, c)
    pg.residuals()
    pg.optimise(iters=4, check_every=2, eps_rot=0.0, eps_trans=0.0, trace_poses=True)
    pg.poses()
    after = snapshot()
    assert before[0] == after[0]
    for k in LIN_KEYS:
        assert np.array_equal(before[1][k], after[1][k]), k
    pg.destroy()
    f.destroy()
    gm.release()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_graph_as_it_was(ctx):
    from mimosa_amd import capi
    L, p = ctx.L, capi._p
    L.mh_last_error.restype = C.c_char_p
    INV, UNS = capi.MH_ERR_INVALID_ARG, capi.MH_ERR_UNSUPPORTED
    c = cases.case("n12_far_on_fixed")
    fresh = capi.PoseGraph(ctx, 12, 12)
    cfg, res, f = capi.make_pose_graph_config(), capi.PoseGraphResult(), C.c_double()
    for call in (lambda: L.mh_pose_graph_optimise(fresh.h, C.byref(cfg), C.byref(res), None), lambda: L.mh_pose_graph_residuals(fresh.h, None, None, C.byref(f)),
                 lambda: L.mh_pose_graph_set_fixed(fresh.h, None), lambda: L.mh_pose_graph_set_edges(fresh.h, None, 0)):
        assert call() == INV and b"no poses have been set" in L.mh_last_error(ctx.h)
    fresh.destroy()

    pg = graph_of(ctx, c)
    want = pg.residuals()

    def unchanged():
        got = pg.residuals()
        R, t = pg.poses()
        return all(np.array_equal(x, y) for x, y in zip(got[:2], want[:2])) and got[2] == want[2] and np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])

    R, t = c["R"].reshape(-1, 9).copy(), c["t"].copy()
    assert L.mh_pose_graph_set_poses(pg.h, p(R), p(t), 0) == INV and L.mh_pose_graph_set_poses(pg.h, p(R), p(t), 13) == INV
    bad = R.copy()
    bad[11, 8] = np.nan
    assert L.mh_pose_graph_set_poses(pg.h, p(bad), p(t), 12) == INV and b"pose 11" in L.mh_last_error(ctx.h)
    bad = t.copy()
    bad[3, 1] = np.inf
    assert L.mh_pose_graph_set_poses(pg.h, p(R), p(bad), 12) == INV and b"pose 3" in L.mh_last_error(ctx.h)
    assert L.mh_pose_graph_set_poses(pg.h, None, p(t), 12) == INV
    assert unchanged()

    good = as_dicts(c["edges"])
    for change, code, msg in ((dict(a=-1), INV, b"pose_a < pose_b"), (dict(a=3, b=3), INV, b"pose_a < pose_b"), (dict(a=5, b=4), INV, b"pose_a < pose_b"),
                              (dict(b=12), INV, b"pose_a < pose_b"), (dict(Z=(np.eye(3), [0.0, np.nan, 0.0])), INV, b"not finite"),
                              (dict(Z=(np.full((3, 3), np.inf), [0.0, 0.0, 0.0])), INV, b"not finite"),
                              (dict(info=np.eye(6) * np.nan), INV, b"not finite"), (dict(info=np.eye(6) + np.eye(6, k=1) * 1e-9), INV, b"not symmetric")):
        edges = good[:-1] + [dict(good[-1], **change)]
        assert L.mh_pose_graph_set_edges(pg.h, capi.make_window_edge(edges), len(edges)) == code and msg in L.mh_last_error(ctx.h), change
    assert L.mh_pose_graph_set_edges(pg.h, capi.make_window_edge(good + good[:1]), len(good) + 1) == INV and b"more edges" in L.mh_last_error(ctx.h)
    assert L.mh_pose_graph_set_edges(pg.h, None, 3) == INV
    assert unchanged()
    Rb, tb, n = np.empty((12, 9)), np.empty((12, 3)), C.c_size_t()
    assert L.mh_pose_graph_get_poses(pg.h, p(Rb), p(tb), 11, C.byref(n)) == INV and b"capacity" in L.mh_last_error(ctx.h) and n.value == 12
    for change in (dict(iters=0), dict(iters=65), dict(check_every=-1), dict(damping=-1.0), dict(damping=np.nan), dict(eps_rot=-1e-9), dict(eps_trans=np.inf)):
        cfg = capi.make_pose_graph_config(**change)
        assert L.mh_pose_graph_optimise(pg.h, C.byref(cfg), C.byref(res), None) == INV, change
    cfg = capi.make_pose_graph_config()
    assert L.mh_pose_graph_optimise(pg.h, None, C.byref(res), None) == INV and L.mh_pose_graph_optimise(pg.h, C.byref(cfg), None, None) == INV
    assert unchanged()
    pg.destroy()

    # more than MH_PGO_FAR_MAX far edges; exactly that many pass (cases.n300_far32 runs them)
    c = cases.case("n300_far32")
    pg = graph_of(ctx, c, slack=1)
    want = pg.residuals()
    a, b, ZR, Zt, Om = c["edges"][-1]
    edges = as_dicts(c["edges"]) + [{"a": 100, "b": 102, "Z": (ZR, Zt), "info": Om}]
    assert L.mh_pose_graph_set_edges(pg.h, capi.make_window_edge(edges), len(edges)) == UNS and b"MH_PGO_FAR_MAX" in L.mh_last_error(ctx.h)
    got = pg.residuals()
    assert np.array_equal(got[0], want[0]) and got[2] == want[2]
    pg.destroy()


def test_use_after_shutdown_is_refused():
    """a graph is registered on its context: after mh_shutdown every call but destroy refuses it"""
    from mimosa_amd import capi
    L, p, INV = capi.load(), capi._p, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    h, pg = C.c_void_p(), C.c_void_p()
    assert L.mh_init(0, C.byref(h)) == capi.MH_OK
    assert L.mh_pose_graph_create(h, 4, 4, C.byref(pg)) == capi.MH_OK
    c = cases.case("n3_far")
    R, t = c["R"].reshape(-1, 9).copy(), c["t"].copy()
    edges = capi.make_window_edge(as_dicts(c["edges"]))
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 3) == capi.MH_OK and L.mh_pose_graph_set_edges(pg, edges, 3) == capi.MH_OK
    L.mh_shutdown(h)
    cfg, res, f, n = capi.make_pose_graph_config(), capi.PoseGraphResult(), C.c_double(), C.c_size_t()
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 3) == INV and b"shut down" in L.mh_last_error(None)
    assert L.mh_pose_graph_set_fixed(pg, None) == INV
    assert L.mh_pose_graph_set_edges(pg, edges, 3) == INV
    assert L.mh_pose_graph_get_poses(pg, p(R), p(t), 3, C.byref(n)) == INV
    assert L.mh_pose_graph_residuals(pg, None, None, C.byref(f)) == INV
    assert L.mh_pose_graph_optimise(pg, C.byref(cfg), C.byref(res), None) == INV and b"shut down" in L.mh_last_error(None)
    L.mh_pose_graph_destroy(pg)
