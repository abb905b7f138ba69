"""-m gpu: the pose graph's marginal covariances (mh_pose_graph_covariances, rule 10 in include/mimosa_hip.h) on the device,
through the C ABI.  The cases of tests/pose_graph_cov_cases.py against the dense restatement (tests/pose_graph_cov_ref.py) to
the bar measured per case there (16 x the error of numpy.linalg.inv); what holds to the bit (symmetry, zero blocks of fixed
poses, joint's diagonal blocks, a pair alone against the same pair among 64, repeats, cov without pairs); a call that moves
nothing; flags = 4 with the outputs untouched; refusals; use after mh_shutdown; one graph of 4 096 poses against a sparse LU;
the gate end to end on the 64-pose circuit with a false loop.  (The hall with an aliased loop stays out: on the restatement it
does not separate by a factor of 4 on both sides, see tests/test_pose_graph_cov_cpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cov_cases as cases
import pose_graph_cov_ref as cref
import pose_graph_robust_cases as robust
from test_gpu_pose_graph_robust import as_dicts, graph_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cases.CASES)
def test_covariances_against_the_restatement(ctx, name):
    c, want = cases.case(name), cases.restated(name)
    pg = graph_of(ctx, c)
    pairs = cases.pairs64(name)
    cov, joint, info = pg.covariances(c["damping"], pairs)
    assert info == {"n_poses": len(c["R"]), "n_far": sum(1 for e in c["edges"] if e[1] - e[0] >= 2), "n_pairs": len(pairs), "flags": 0}
    err = cases.compare(name, cov, joint)
    print("%s: relative error %.3g; numpy.linalg.inv %.3g; ratio %.2f; bar %.3g" % (name, err, want["err_np"], err / max(want["err_np"], 1e-300), want["bar"]))
    assert err <= want["bar"], (name, err, want["err_np"])
    cases.exact_properties(c, cov, pairs, joint)
    # the same bits on a repeat; cov without pairs; a pair alone
    cov2, joint2, _ = pg.covariances(c["damping"], pairs)
    assert np.array_equal(cov, cov2) and np.array_equal(joint, joint2)
    cov3, joint3, info3 = pg.covariances(c["damping"])
    assert np.array_equal(cov, cov3) and joint3.shape == (0, 12, 12) and info3["n_pairs"] == 0
    if pairs:
        _, joint1, _ = pg.covariances(c["damping"], pairs[:1])
        assert np.array_equal(joint1[0], joint[0])
        k = len(pairs) // 2
        _, jointk, _ = pg.covariances(c["damping"], [pairs[k], pairs[0]])
        assert np.array_equal(jointk[0], joint[k]) and np.array_equal(jointk[1], joint[0])
    pg.destroy()


@pytest.mark.parametrize("name", ("n64_false_loop_cauchy", "n257_mixed", "n3_far"))
def test_a_covariance_call_moves_nothing(ctx, name):
    c = cases.case(name)
    runs = []
    for with_cov in (False, True):
        pg = graph_of(ctx, c)
        if with_cov:
            pg.covariances(c["damping"], cases.pairs_of(name))
        before = (pg.poses(), pg.residuals(), pg.weights())
        if with_cov:
            pg.covariances(0.5, cases.pairs64(name))          # another damping: nothing of it stays either
        got = pg.optimise(iters=6, eps_rot=0.0, eps_trans=0.0, damping=c["damping"], trace_poses=True)
        runs.append((before, got))
        pg.destroy()
    (b0, g0), (b1, g1) = runs
    for x, y in zip(b0, b1):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    assert np.array_equal(b1[0][0], c["R"]) and np.array_equal(b1[0][1], c["t"])
    assert np.array_equal(g0["trace_poses"], g1["trace_poses"]) and g0["trace"] == g1["trace"]


@pytest.mark.parametrize("name", cases.SINGULAR)
def test_a_pivot_that_is_not_positive_writes_nothing(ctx, name):
    from mimosa_amd import capi
    c = cases.case(name)
    pg = graph_of(ctx, c)
    n = len(c["R"])
    cov, joint = np.full((n, 6, 6), -7.25), np.full((2, 12, 12), -7.25)
    pairs = np.array([[0, 1], [2, 9]], np.int32)
    info = capi.PoseGraphCovInfo()
    assert ctx.L.mh_pose_graph_covariances(pg.h, 0.0, capi._p(cov), capi._p(pairs), 2, capi._p(joint), C.byref(info)) == capi.MH_OK
    assert (info.flags, info.n_poses, info.n_pairs) == (4, n, 2)
    assert np.all(cov == -7.25) and np.all(joint == -7.25)
    # damping is the anchor the graph lacks
    cov2, _, info2 = pg.covariances(1e-3, [(0, 1)])
    assert info2["flags"] == 0 and np.isfinite(cov2).all()
    pg.destroy()


def test_refusals_enqueue_nothing(ctx):
    from mimosa_amd import capi
    L, p, INV = ctx.L, capi._p, capi.MH_ERR_INVALID_ARG
    L.mh_last_error.restype = C.c_char_p
    c = cases.case("n12_far_on_fixed")
    pg = graph_of(ctx, c)
    n = len(c["R"])
    cov, joint, info = np.full((n, 6, 6), -7.25), np.full((65, 12, 12), -7.25), capi.PoseGraphCovInfo()
    ok = np.array([[0, 1]], np.int32)
    many = np.ascontiguousarray(np.tile(ok, (65, 1)))
    call = lambda *a: L.mh_pose_graph_covariances(*a)
    bad = [("NULL argument", lambda: call(None, 0.0, p(cov), None, 0, None, C.byref(info))),
           ("NULL argument", lambda: call(pg.h, 0.0, p(cov), None, 0, None, None)),
           ("both NULL", lambda: call(pg.h, 0.0, None, None, 0, None, C.byref(info))),
           ("pairs and joint", lambda: call(pg.h, 0.0, p(cov), None, 1, p(joint), C.byref(info))),
           ("pairs and joint", lambda: call(pg.h, 0.0, p(cov), p(ok), 1, None, C.byref(info))),
           ("0..64", lambda: call(pg.h, 0.0, p(cov), p(many), 65, p(joint), C.byref(info))),
           ("damping", lambda: call(pg.h, -1.0, p(cov), None, 0, None, C.byref(info))),
           ("damping", lambda: call(pg.h, float("nan"), p(cov), None, 0, None, C.byref(info))),
           ("damping", lambda: call(pg.h, float("inf"), p(cov), None, 0, None, C.byref(info)))]
    for i, j in ((-1, 3), (3, 3), (5, 2), (0, n)):
        pr = np.array([[0, 1], [i, j]], np.int32)
        bad.append(("pair 1", lambda pr=pr: call(pg.h, 0.0, p(cov), p(pr), 2, p(joint), C.byref(info))))
    for text, f in bad:
        assert f() == INV and text.encode() in L.mh_last_error(ctx.h) + L.mh_last_error(None), text
    fresh = capi.PoseGraph(ctx, 4, 4)
    assert call(fresh.h, 0.0, p(cov), None, 0, None, C.byref(info)) == INV and b"no poses" in L.mh_last_error(ctx.h)
    fresh.destroy()
    assert np.all(cov == -7.25) and np.all(joint == -7.25)
    # more far edges than MH_PGO_FAR_MAX never reach a graph: set_edges refuses them, and the graph keeps what it had
    e = c["edges"][-1]
    too_many = as_dicts(list(c["edges"]) + [(0, 2 + k % 9, *e[2:]) for k in range(33)])
    bigger = capi.PoseGraph(ctx, n, len(too_many))
    bigger.set_poses(c["R"], c["t"])
    assert L.mh_pose_graph_set_edges(bigger.h, capi.make_window_edge(too_many), len(too_many)) == capi.MH_ERR_UNSUPPORTED
    bigger.destroy()
    got, _, _ = pg.covariances(c["damping"])
    assert cases.compare("n12_far_on_fixed", got, []) <= cases.restated("n12_far_on_fixed")["bar"]
    pg.destroy()


def test_use_after_shutdown_is_refused():
    from mimosa_amd import capi
    L, p = capi.load(), capi._p
    L.mh_last_error.restype = C.c_char_p
    h, pg = C.c_void_p(), C.c_void_p()
    assert L.mh_init(0, C.byref(h)) == capi.MH_OK
    assert L.mh_pose_graph_create(h, 4, 4, C.byref(pg)) == capi.MH_OK
    c = cases.case("n3_far")
    R, t = c["R"].reshape(-1, 9).copy(), c["t"].copy()
    assert L.mh_pose_graph_set_poses(pg, p(R), p(t), 3) == capi.MH_OK
    cov, info = np.full((3, 6, 6), -7.25), capi.PoseGraphCovInfo()
    assert L.mh_pose_graph_covariances(pg, 1.0, p(cov), None, 0, None, C.byref(info)) == capi.MH_OK and info.flags == 0
    assert np.array_equal(cov, np.broadcast_to(np.eye(6), (3, 6, 6)))     # no edge, damping 1: A is the identity
    L.mh_shutdown(h)
    cov[:] = -7.25
    assert L.mh_pose_graph_covariances(pg, 1.0, p(cov), None, 0, None, C.byref(info)) == capi.MH_ERR_INVALID_ARG
    assert b"shut down" in L.mh_last_error(None) and np.all(cov == -7.25)
    L.mh_pose_graph_destroy(pg)


def test_4096_poses_against_a_sparse_lu(ctx):
    c, want = cases.big_case(), cases.big_restated()
    pg = graph_of(ctx, c, new_calls=False)
    cov, joint, info = pg.covariances(0.0, cases.BIG_PAIRS)
    assert info["flags"] == 0 and info["n_far"] == 2
    err = max(np.abs(cov[i] - w).max() for i, w in want["cov"].items())
    err = max(err, max(np.abs(g - w).max() for g, w in zip(joint, want["joint"]))) / want["scale"]
    print("4096 poses: relative error %.3g; the unrefined sparse LU %.3g; bar %.3g; largest entry %.3g" % (err, want["err_np"], want["bar"], want["scale"]))
    assert err <= want["bar"]
    # The bits as everywhere.  The eigenvalues NOT to 1e-12: an entry may be off by bar x scale (the yardstick above), which moves
    # an eigenvalue of a 12 x 12 matrix by up to 12 times that, and the joint of the neighbours (2047, 2048) — both variances 2.8e3
    # m^2, their difference the odometry's 1e-5 — has eigenvalues far below it.  This is rule 10's limit at a condition number of
    # 1e10, not hidden: the bound asserted is the one the bar implies.
    cases.exact_properties(c, cov, cases.BIG_PAIRS, joint, eig_rel=12.0 * want["bar"])
    pg.destroy()


def test_the_gate_on_the_64_pose_circuit(ctx):
    """tests/test_pose_graph_cov_cpu.py asserts the scene's condition on the restatement; here the same figures through
    capi.PoseGraph.gate: d2 of the true loops below a quarter of the chi^2(6) 0.999 quantile, of the false loop above four times
    it, while the plain chi2 of every true loop is above the quantile"""
    g, cand = cases.held_out(cases.case("n64_false_loop_cauchy"))
    assert [q[:2] for q in cand] == robust.LOOPS64
    pg = graph_of(ctx, g)
    got = pg.gate(as_dicts(cand))
    _, joint = cref.covariances(g, [], [q[:2] for q in cand])
    r, chi2, d2 = cref.gate(g["R"], g["t"], cand, joint)
    print("gate: chi2 %s, d2 %s (the restatement: %s)" % (got["chi2"], got["d2"], d2))
    assert got["flags"] == 0 and np.allclose(got["r"], r, rtol=0, atol=1e-12) and np.allclose(got["chi2"], chi2, rtol=1e-9) and np.allclose(got["d2"], d2, rtol=1e-6)
    assert np.all(got["d2"][:3] < cref.CHI2_6_999 / 4.0) and got["d2"][3] > 4.0 * cref.CHI2_6_999 and np.all(got["chi2"][:3] > cref.CHI2_6_999)
    R, t = pg.poses()
    assert np.array_equal(R, g["R"]) and np.array_equal(t, g["t"])
    pg.destroy()
