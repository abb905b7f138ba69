"""-m gpu: priors and losses of the pose graph (mh_pose_graph_set_priors, _set_loss, _prior_residuals, _weights) on the device,
through the C ABI.  The graphs of tests/pose_graph_robust_cases.py against the numpy restatement
(tests/pose_graph_robust_ref.py) to the bars of tests/test_pose_graph_robust_cpu.py, which also asserts, on the restatement
alone, the conditions these tests rest on; the bits of a graph that never saw the new calls; bit reproducibility on a repeat
and across check_every; evaluations that move nothing; what set_edges and set_poses drop; refusals; use after mh_shutdown."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cases as plain_cases
import pose_graph_ref as ref
import pose_graph_robust_cases as cases
import pose_graph_robust_ref as rref
from pose_graph_robust_cases import POSE_TOL, W_TOL, f_close

pytestmark = pytest.mark.gpu


def as_dicts(edges):
    return [{"a": a, "b": b, "Z": (ZR, Zt), "info": Om} for a, b, ZR, Zt, Om in edges]


def prior_dicts(priors):
    return [{"pose": i, "Z": (ZR, Zt), "info": Om} for i, ZR, Zt, Om in priors]


def graph_of(ctx, c, slack=0, new_calls=True):
    """the case on the device, in a graph created for exactly its size (+ slack)"""
    from mimosa_amd import capi
    pg = capi.PoseGraph(ctx, len(c["R"]) + slack, len(c["edges"]) + slack)
    pg.set_poses(c["R"], c["t"])
    pg.set_fixed(c["fixed"])
    pg.set_edges(as_dicts(c["edges"]))
    if new_calls:
        pg.set_priors(prior_dicts(c.get("priors", [])))
        pg.set_loss(c.get("edge_loss") if len(c["edges"]) else None, c.get("prior_loss"))
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
    worst = [0.0, 0.0, 0.0]
    for k, (row, poses, w) in enumerate(zip(got["trace"], got["trace_poses"], want["trace"])):
        assert row["flags"] == 0
        dt, dr = ref.pose_error(*split(poses), w["R"], w["t"])
        worst = [max(worst[0], dt), max(worst[1], dr), max(worst[2], abs(row["f"] - w["f"]) / max(abs(w["f"]), 1e-300))]
        print("%s iteration %d: %.3g m, %.3g rad, f %.17g against %.17g" % (name, k + 1, dt, dr, row["f"], w["f"]))
        assert dt <= POSE_TOL and dr <= POSE_TOL, (name, k, dt, dr)
        assert f_close(row["f"], w["f"], cases.n_terms(c)), (name, k, row["f"], w["f"])
        assert abs(row["step_rot"] - w["step_rot"]) <= POSE_TOL and abs(row["step_trans"] - w["step_trans"]) <= POSE_TOL
    print("%s: largest difference to the restatement over %d iterations: %.3g m, %.3g rad, f %.3g relative" % (name, cases.ITERS, *worst))
    R, t = split(got["trace_poses"][-1])
    assert np.array_equal(got["R"], R) and np.array_equal(got["t"], t)
    fixed = np.flatnonzero(c["fixed"])
    assert np.array_equal(R[fixed], c["R"][fixed]) and np.array_equal(t[fixed], c["t"][fixed])
    # the weights at the result, against the restatement's at ITS result: both have converged to the bar
    we, wp, f = pg.weights()
    rwe, rwp, rf = rref.weights(want["R"], want["t"], c["edges"], c["priors"], c["edge_loss"], c["prior_loss"])
    assert np.abs(we - rwe).max(initial=0.0) <= W_TOL and np.abs(wp - rwp).max(initial=0.0) <= W_TOL
    pg.destroy()


@pytest.mark.parametrize("name", cases.REGULAR)
def test_weights_and_prior_residuals_move_nothing(ctx, name):
    c = cases.case(name)
    rwe, rwp, rf = cases.restated_weights(name)
    rd, rchi2 = rref.prior_residuals(c["R"], c["t"], c["priors"])
    pg = graph_of(ctx, c)
    we, wp, f = pg.weights()
    d, chi2 = pg.prior_residuals()
    assert np.abs(we - rwe).max(initial=0.0) <= W_TOL and np.abs(wp - rwp).max(initial=0.0) <= W_TOL and f_close(f, rf, cases.n_terms(c))
    assert np.abs(d - rd).max(initial=0.0) <= POSE_TOL and np.all(np.abs(chi2 - rchi2) <= cases.F_RTOL * rchi2 + cases.base.f_floor(1))
    R, t = pg.poses()
    assert np.array_equal(R, c["R"]) and np.array_equal(t, c["t"])   # nothing moved
    again = pg.weights()
    assert np.array_equal(again[0], we) and np.array_equal(again[1], wp) and again[2] == f
    # s stays what mh_pose_graph_residuals reports, and its f stays the plain sum, whatever the losses
    r, s, fs = pg.residuals()
    want = ref.residuals(c["R"], c["t"], c["edges"])
    assert np.all(np.abs(s - want[1]) <= cases.F_RTOL * want[1] + cases.base.f_floor(1)) and f_close(fs, want[2], len(s))
    assert pg.optimise(iters=1, eps_rot=0.0, eps_trans=0.0)["f_first"] == f       # the trace's f is this f, bit for bit
    pg.destroy()


def test_no_anchor_takes_no_step(ctx):
    c = cases.case("no_anchor")
    pg = graph_of(ctx, c)
    got = pg.optimise(iters=8, eps_rot=0.0, eps_trans=0.0)
    assert (got["iters"], got["converged"]) == (1, 0) and got["trace"][0]["flags"] == 4
    assert np.array_equal(got["R"], c["R"]) and np.array_equal(got["t"], c["t"])
    # a prior is the anchor a fixed flag would be
    pg.set_priors([{"pose": 0, "Z": (c["truth_R"][0], c["truth_t"][0]), "info": np.eye(6) * 1e4}])
    got = pg.optimise(iters=8, eps_rot=0.0, eps_trans=0.0)
    assert got["iters"] == 8 and [q["flags"] for q in got["trace"]] == [0] * 8
    want = rref.optimise(c["R"], c["t"], c["fixed"], c["edges"], [(0, c["truth_R"][0], c["truth_t"][0], np.eye(6) * 1e4)], None, None, 8)
    dt, dr = ref.pose_error(got["R"], got["t"], want["R"], want["t"])
    assert dt <= POSE_TOL and dr <= POSE_TOL
    pg.destroy()


def test_a_prior_on_a_fixed_pose_acts_on_f_alone(ctx):
    c = cases.case("prior_on_fixed")
    a, b = graph_of(ctx, c), graph_of(ctx, dict(c, priors=[]))
    ga, gb = a.optimise(iters=4, eps_rot=0.0, eps_trans=0.0), b.optimise(iters=4, eps_rot=0.0, eps_trans=0.0)
    assert np.array_equal(ga["R"], gb["R"]) and np.array_equal(ga["t"], gb["t"])
    assert ga["trace"][0]["f"] > gb["trace"][0]["f"] + 1.0
    a.destroy()
    b.destroy()


def test_the_clamp_of_w_is_reached_and_no_pivot_fails(ctx):
    c = cases.case("huge_chi2")
    pg = graph_of(ctx, c)
    assert pg.weights()[0][-1] == rref.MIN_WEIGHT
    assert [q["flags"] for q in pg.optimise(iters=3, eps_rot=0.0, eps_trans=0.0)["trace"]] == [0, 0, 0]
    pg.destroy()


def test_the_false_loop_is_switched_off(ctx):
    """the conditions of test_pose_graph_robust_cpu.py on the device: plain bends, Cauchy and DCS do not"""
    c = cases.case("n64_false_loop_plain")
    err = lambda t: float(np.linalg.norm(t - c["truth_t"], axis=1)[c["fixed"] == 0].max())
    start = err(c["t"])
    pg = graph_of(ctx, c)
    plain = err(pg.optimise(iters=cases.ITERS, eps_rot=0.0, eps_trans=0.0)["t"])
    pg.destroy()
    assert plain > start
    for name in ("n64_false_loop_cauchy", "n64_false_loop_dcs"):
        pg = graph_of(ctx, cases.case(name))
        robust = err(pg.optimise(iters=cases.ITERS, eps_rot=0.0, eps_trans=0.0)["t"])
        w = pg.weights()[0][-4:]
        print("%s: %.3f m at the start, %.3f m plain, %.3f m robust, loop weights %s" % (name, start, plain, robust, w))
        assert robust < start and w[3] < 0.01 and np.all(w[:3] > 0.5)
        pg.destroy()


# ---- 2. the bits of a graph that never saw the new calls --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("n1", "n3_far", "n65", "n257_two_fixed", "n300_far32"))
def test_no_prior_and_kind_0_have_todays_bits(ctx, name):
    c = plain_cases.case(name)
    runs = []
    for how in ("never", "empty", "explicit"):
        pg = graph_of(ctx, c, new_calls=False)
        if how == "empty":
            pg.set_priors([])
            pg.set_loss(None, None)
        elif how == "explicit":
            pg.set_priors([])
            if len(c["edges"]):
                pg.set_loss([(0, 0.0)] * len(c["edges"]), None)
        runs.append(pg.optimise(iters=plain_cases.ITERS, eps_rot=0.0, eps_trans=0.0, trace_poses=True))
        pg.destroy()
    a = runs[0]
    want = plain_cases.restated(name)                      # and it still is the plain restatement's solution
    dt, dr = ref.pose_error(a["R"], a["t"], want["R"], want["t"])
    assert dt <= POSE_TOL and dr <= POSE_TOL
    for b in runs[1:]:
        assert b["trace"] == a["trace"] and (b["f_first"], b["f_last"]) == (a["f_first"], a["f_last"])
        assert np.array_equal(b["trace_poses"], a["trace_poses"]) and np.array_equal(b["R"], a["R"]) and np.array_equal(b["t"], a["t"])


@pytest.mark.parametrize("name", ("n3_far_cauchy", "n65_priors_no_fixed", "n257_mixed"))
def test_bit_identical_on_a_repeat_and_across_check_every(ctx, name):
    c = cases.case(name)
    runs = []
    for check_every, slack in ((0, 0), (0, 0), (1, 0), (3, 7)):
        pg = graph_of(ctx, c, slack)
        runs.append(pg.optimise(iters=64, check_every=check_every, eps_rot=plain_cases.STOP_EPS, eps_trans=plain_cases.STOP_EPS, trace_poses=True))
        pg.destroy()
    a = runs[0]
    assert a["converged"] == 1 and a["iters"] < 64
    for b in runs[1:]:
        assert (b["iters"], b["converged"]) == (a["iters"], a["converged"]) and b["trace"] == a["trace"]
        assert np.array_equal(b["trace_poses"], a["trace_poses"]) and np.array_equal(b["R"], a["R"]) and np.array_equal(b["t"], a["t"])


# ---- 3. what the setters drop -----------------------------------------------------------------------------------------------------
def test_set_edges_and_set_poses_drop_what_the_header_says(ctx):
    c = cases.case("n257_mixed")
    pg = graph_of(ctx, c, slack=3)
    we, wp, f = pg.weights()
    assert we.min() < 1.0 and wp.min() < 1.0
    pg.set_edges(as_dicts(c["edges"]))                     # the edges' losses go, the priors and theirs stay
    we2, wp2, f2 = pg.weights()
    assert np.all(we2 == 1.0) and np.array_equal(wp2, wp) and f2 > f
    pg.set_loss(c["edge_loss"], c["prior_loss"])
    assert pg.weights()[2] == f
    pg.set_priors(prior_dicts(c["priors"]))                # the priors' losses go, the edges' stay
    we3, wp3, _ = pg.weights()
    assert np.array_equal(we3, we) and np.all(wp3 == 1.0)
    pg.set_poses(c["R"], c["t"])                           # the same n: everything stays
    assert np.array_equal(pg.weights()[0], we)
    small = cases.case("n3_far_cauchy")
    pg.set_poses(small["R"], small["t"])                   # another n: edges, fixed flags, priors and losses go
    assert (pg.n_edges, pg.n_priors) == (0, 0)
    we4, wp4, f4 = pg.weights()
    assert len(we4) == 0 and len(wp4) == 0 and f4 == 0.0
    pg.set_fixed(small["fixed"])
    pg.set_edges(as_dicts(small["edges"]))
    assert np.all(pg.weights()[0] == 1.0)                  # the losses of the graph before are not these edges'
    plain = graph_of(ctx, dict(small, edge_loss=None), new_calls=False)
    a, b = pg.optimise(iters=5, eps_rot=0.0, eps_trans=0.0), plain.optimise(iters=5, eps_rot=0.0, eps_trans=0.0)
    assert a["trace"] == b["trace"] and np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])
    plain.destroy()
    pg.destroy()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_graph_as_it_was(ctx):
    from mimosa_amd import capi
    L = ctx.L
    L.mh_last_error.restype = C.c_char_p
    INV = capi.MH_ERR_INVALID_ARG
    c = cases.case("n257_mixed")
    fresh = capi.PoseGraph(ctx, 12, 12)
    f = C.c_double()
    one = capi.make_pose_prior(prior_dicts(c["priors"][:1]))
    for call in (lambda: L.mh_pose_graph_set_priors(fresh.h, one, 1), lambda: L.mh_pose_graph_set_loss(fresh.h, None, None),
                 lambda: L.mh_pose_graph_prior_residuals(fresh.h, None, None), lambda: L.mh_pose_graph_weights(fresh.h, None, None, C.byref(f))):
        assert call() == INV and b"no poses have been set" in L.mh_last_error(ctx.h)
    fresh.set_poses(c["R"][:12], c["t"][:12])
    loss1 = capi.make_pose_graph_loss([(2, 3.0)])
    assert L.mh_pose_graph_set_loss(fresh.h, loss1, None) == INV and b"no edges have been set" in L.mh_last_error(ctx.h)
    assert L.mh_pose_graph_set_loss(fresh.h, None, loss1) == capi.MH_OK      # no prior: a list of none
    fresh.destroy()

    pg = graph_of(ctx, c)                                  # created for exactly 257 poses
    want = pg.weights()
    want_d = pg.prior_residuals()

    def unchanged():
        got, d = pg.weights(), pg.prior_residuals()
        return all(np.array_equal(x, y) for x, y in zip(got[:2], want[:2])) and got[2] == want[2] and np.array_equal(d[0], want_d[0])

    good = prior_dicts(c["priors"])
    for change, msg in ((dict(pose=-1), b"0 <= pose < n"), (dict(pose=257), b"0 <= pose < n"), (dict(Z=(np.eye(3), [0.0, np.nan, 0.0])), b"not finite"),
                        (dict(Z=(np.full((3, 3), np.inf), [0.0, 0.0, 0.0])), b"not finite"), (dict(info=np.eye(6) * np.nan), b"not finite"),
                        (dict(info=np.eye(6) + np.eye(6, k=1) * 1e-9), b"not symmetric")):
        priors = good[:-1] + [dict(good[-1], **change)]
        assert L.mh_pose_graph_set_priors(pg.h, capi.make_pose_prior(priors), len(priors)) == INV and msg in L.mh_last_error(ctx.h), change
    many = [good[0]] * 258
    assert L.mh_pose_graph_set_priors(pg.h, capi.make_pose_prior(many), 258) == INV and b"more priors" in L.mh_last_error(ctx.h)
    assert L.mh_pose_graph_set_priors(pg.h, None, 2) == INV and b"NULL argument" in L.mh_last_error(ctx.h)
    assert unchanged()

    E, P = len(c["edges"]), len(c["priors"])
    for bad, msg in (((4, 1.0), b"kind outside"), ((-1, 1.0), b"kind outside"), ((1, 0.0), b"param > 0"), ((2, -3.0), b"param > 0"),
                     ((3, np.nan), b"param > 0"), ((2, np.inf), b"param > 0")):
        el, pl = list(c["edge_loss"]), list(c["prior_loss"])
        el[E - 1] = bad
        assert L.mh_pose_graph_set_loss(pg.h, capi.make_pose_graph_loss(el), capi.make_pose_graph_loss(pl)) == INV and msg in L.mh_last_error(ctx.h), bad
        el[E - 1], pl[P - 1] = c["edge_loss"][E - 1], bad
        assert L.mh_pose_graph_set_loss(pg.h, capi.make_pose_graph_loss(el), capi.make_pose_graph_loss(pl)) == INV and b"prior" in L.mh_last_error(ctx.h), bad
    assert unchanged()
    assert L.mh_pose_graph_set_loss(pg.h, capi.make_pose_graph_loss([(0, np.nan)] * E), None) == capi.MH_OK    # kind 0 reads no param
    assert np.all(pg.weights()[0] == 1.0) and np.all(pg.weights()[1] == 1.0)
    got = pg.optimise(iters=2, eps_rot=0.0, eps_trans=0.0)                  # and the graph is usable
    assert [q["flags"] for q in got["trace"]] == [0, 0]
    pg.destroy()


def test_use_after_shutdown_is_refused():
    from mimosa_amd import capi
    L, p, INV = capi.load(), capi._p, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    h, pg = C.c_void_p(), C.c_void_p()
    assert L.mh_init(0, C.byref(h)) == capi.MH_OK
    assert L.mh_pose_graph_create(h, 4, 4, C.byref(pg)) == capi.MH_OK
    c = cases.case("n3_far_cauchy")
    R, t = c["R"].reshape(-1, 9).copy(), c["t"].copy()
    edges = capi.make_window_edge(as_dicts(c["edges"]))
    prior = capi.make_pose_prior([{"pose": 1, "Z": (c["truth_R"][1], c["truth_t"][1]), "info": np.eye(6)}])
    loss = capi.make_pose_graph_loss(c["edge_loss"])
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 3) == capi.MH_OK and L.mh_pose_graph_set_edges(pg, edges, 3) == capi.MH_OK
    assert L.mh_pose_graph_set_priors(pg, prior, 1) == capi.MH_OK and L.mh_pose_graph_set_loss(pg, loss, None) == capi.MH_OK
    L.mh_shutdown(h)
    f = C.c_double()
    assert L.mh_pose_graph_set_priors(pg, prior, 1) == INV and b"shut down" in L.mh_last_error(None)
    assert L.mh_pose_graph_set_loss(pg, loss, None) == INV and b"shut down" in L.mh_last_error(None)
    assert L.mh_pose_graph_prior_residuals(pg, None, None) == INV
    assert L.mh_pose_graph_weights(pg, None, None, C.byref(f)) == INV and b"shut down" in L.mh_last_error(None)
    L.mh_pose_graph_destroy(pg)


# ---- 5. end to end in the hall ------------------------------------------------------------------------------------------------------
def test_end_to_end_in_the_hall_with_an_aliased_loop(ctx):
    """The scene and the measure of tests/test_gpu_map_rebuild.py::test_end_to_end_in_the_hall, the graph of
    pose_graph_robust_cases.hall_case(): ONE true loop (0, 35) and one aliased loop.  Optimise, rebuild at the result.  Without a
    loss the rebuilt map stays above half the drifted map's RMS distance to the true map; with Cauchy on the two far edges it
    comes below half of it (tests/test_pose_graph_robust_cpu.py asserts a quarter with the restatement and the oracle map), the
    aliased loop's weight below 0.01, the true loop's above 0.5."""
    from mimosa_amd import capi
    import map_rebuild_ref as mref
    from test_gpu_map_rebuild import store_of
    case = cases.hall_case()
    st = store_of(ctx, case["clouds"])
    got = {}
    for how in ("plain", "cauchy"):
        pg = capi.PoseGraph(ctx, 36, 37)
        pg.set_poses(*case["drifted"])
        pg.set_fixed(case["fixed"])
        pg.set_edges(as_dicts(case["edges"]))
        if how == "cauchy":
            pg.set_loss(case["edge_loss"], None)
        got[how] = pg.optimise(iters=cases.ITERS, eps_rot=0.0, eps_trans=0.0)
        got[how]["w"] = pg.weights()[0]
        pg.destroy()
    maps = {name: st.rebuild_map(poses, mode=27)[0] for name, poses in (("true", case["true"]), ("drifted", case["drifted"]),
                                                                        ("plain", (got["plain"]["R"], got["plain"]["t"])),
                                                                        ("cauchy", (got["cauchy"]["R"], got["cauchy"]["t"])))}

    def rms(m):
        cloud = m.get_cloud().astype(np.float64)
        _, sq, found = maps["true"].knn(cloud, 1)
        return mref.capped_rms(np.where(found > 0, np.sqrt(sq[:, 0]), mref.HALL_CAP))

    rms_d, rms_p, rms_r = rms(maps["drifted"]), rms(maps["plain"]), rms(maps["cauchy"])
    w = got["cauchy"]["w"]
    print("hall, device: RMS to the true map drifted %.4f m, plain %.4f m, Cauchy %.4f m; far weights %s" % (rms_d, rms_p, rms_r, w[-2:]))
    assert rms(maps["true"]) == 0.0
    assert rms_d > 0.1 and rms_p > 0.5 * rms_d and rms_r < 0.5 * rms_d
    assert w[-1] < 0.01 and w[-2] > 0.5 and np.all(w[:-2] == 1.0) and np.all(got["plain"]["w"] == 1.0)
    for m in maps.values():
        m.release()
    st.destroy()
