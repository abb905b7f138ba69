"""-m gpu: mh_icp_score_poses / mh_icp_relocalise against the numpy restatement (tests/reloc_ref.py) fed with mh_map_knn(k = 1)
on the restated queries.

Scene: synth.small_world() — one 6 x 5 x 3 m room of ~5 k map points, a 16 x 64 scan cast from its ground-truth pose.
Bars: n_points, n_occupied, n_inliers equal; sum_sq to 1e-12 relative (the same d2 values — mh_map_knn's, bit for bit — added in
another order: 1 024 terms at most, 1e-16 each); determinism and "nothing else moves" bit for bit; the aligned poses of
mh_icp_relocalise within 1e-9 m / 1e-9 rad of mh_icp_align run by the caller from the same candidates.  Before any score is
compared the inputs are held off the gate edge: no restated d2 within 1e-9 relative of gate^2, where the last digit would decide
an inlier.

Poses: make_poses below; the seeded tail is the first seed tried (the gate-edge assertion held with it).

Relocalise: the box, the coarse configuration and the final gate were chosen with the host-driven version (restated scores,
numpy's top-K, one mh_icp_align per candidate, a restated re-score).  Measured with it, three boxes x strides 1 / 4 x four align
configurations: at a final gate of 0.3 m every aligned pose keeps all 1 024 points as inliers, the key falls to sum_sq, and the
alignment started AT the truth (which moves 0.5 mm) has the smaller sum (5.1496 against 5.151 .. 5.166) in every configuration
with a 0.5 m grid: sum_sq is not what the alignment minimises, so where it stops within its last millimetre is not ordered by
it.  At 0.1 m (955 inliers for the aligned truth) and at 0.05 m (254) the inlier count decides, and the best candidate's key was
not worse than the aligned truth's in all 24 configurations each.  FINAL_GATE = 0.1 with the first box tried.  Winner's distance
to the truth, printed by the test: see DESIGN.md."""
import numpy as np
import pytest

import reloc_ref

pytestmark = pytest.mark.gpu

G = np.array([0.0, 0.0, -1.0])
MODES = (7, 19, 27)


def rot_angle(Ra, Rb):
    M = Ra.T @ Rb
    return float(np.arctan2(np.linalg.norm(M - M.T) / (2.0 * np.sqrt(2.0)), (np.trace(M) - 1.0) / 2.0))


def about(R0, t0, yaw):
    """(R0, t0) turned by yaw about the vertical through the sensor"""
    from mimosa_amd import synth
    return synth.rot_z(yaw) @ R0, t0


def make_poses(aux):
    """37 poses: the truth, synth.query_pose, yaws of 90 and 180 degrees, translations of 0.3 / 1 / 3 m, one pose 1e7 m away
    (index 4), one with the whole cloud in free space (index 5: 40 m above the room), then seeded small and large perturbations"""
    from mimosa_amd import synth
    Rg, tg = aux["R_W_L"], aux["t_W_L"]
    poses = [(Rg, tg), synth.query_pose(Rg, tg), about(Rg, tg, np.pi / 2), about(Rg, tg, np.pi), (Rg, tg + np.array([1e7, 0.0, 0.0])),
             (Rg, tg + np.array([0.0, 0.0, 40.0]))]
    for d in (0.3, 1.0, 3.0):
        for ax in (np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0]), np.array([0.6, 0.8, 0.0])):
            poses.append((Rg, tg + d * ax))
    rng = np.random.default_rng(2024)
    while len(poses) < 37:
        big = len(poses) % 2 == 0
        w = rng.standard_normal(3) * (0.5 if big else 0.02)
        dt = rng.standard_normal(3) * (1.5 if big else 0.05)
        poses.append((Rg @ synth.so3_exp(w), tg + dt))
    return poses


FAR, FREE = 4, 5


@pytest.fixture(scope="module")
def world():
    from mimosa_amd import capi, synth
    ctx = capi.Context(0)
    m, pts, aux = synth.small_world()
    big_pts, _ = synth.make_scan(n_rows=64, seed=1234 + 1, n_cols=64, room=np.array([6.0, 5.0, 3.0]), sensor_local=np.array([2.3, 2.6, 1.2]))
    maps, occupied, factors = {}, {}, {}
    for mode in MODES:
        maps[mode] = capi.VoxelMap(ctx, mode=mode)
        maps[mode].insert(m)
        occupied[mode] = reloc_ref.occupied_set(maps[mode].get_cloud())
    maps["empty"] = capi.VoxelMap(ctx, mode=19)
    occupied["empty"] = set()
    reg = capi.make_reg_config(**synth.enwide_config())

    def factor(mode, n=None, cloud=None, binary=False, fresh=False):
        cloud = pts if cloud is None else cloud
        n = len(cloud) if n is None else n
        key = (mode, n, len(cloud), binary)
        if fresh:
            f = capi.ICPFactor(ctx, maps[mode], np.ascontiguousarray(cloud[:n]), reg, binary=binary)
            factors[(key, len(factors))] = f
            return f
        if key not in factors:
            factors[key] = capi.ICPFactor(ctx, maps[mode], np.ascontiguousarray(cloud[:n]), reg, binary=binary)
        return factors[key]

    def knn(mode):
        def f(q):
            _, sq, found = maps[mode].knn(q, 1)
            return found > 0, sq[:, 0]
        return f

    yield dict(ctx=ctx, maps=maps, occupied=occupied, factor=factor, knn=knn, pts=pts, big_pts=big_pts, aux=aux, poses=make_poses(aux), capi=capi, synth=synth)
    for f in factors.values():
        f.destroy()
    for gm in maps.values():
        gm.release()
    ctx.close()


def stack(poses):
    return np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])


def restate(world, mode, poses, cloud, gate, stride, check_edge=True):
    """the restated scores of the poses as a POSE_SCORE_DTYPE array; the gate-edge condition asserted on the way"""
    xyz = world["synth"].points_xyz(cloud)
    out = np.zeros(len(poses), world["capi"].POSE_SCORE_DTYPE)
    cache = {}
    for i, (R, t) in enumerate(poses):
        key = (R.tobytes(), t.tobytes())
        if key not in cache:
            r = reloc_ref.score_pose(R, t, xyz, gate, stride, world["knn"](mode), world["occupied"][mode])
            if check_edge:
                d2 = r["d2"][r["found"]]
                assert not (np.abs(d2 - gate * gate) <= 1e-9 * gate * gate).any(), "a restated d2 sits on the gate edge: choose another pose"
            cache[key] = (r["n_points"], r["n_occupied"], r["n_inliers"], 0, r["sum_sq"])
        out[i] = cache[key]
    return out


def assert_scores(got, ref, tag=""):
    for name in ("n_points", "n_occupied", "n_inliers"):
        assert np.array_equal(got[name], ref[name]), (tag, name, np.flatnonzero(got[name] != ref[name])[:8])
    assert not got["reserved"].any()
    err = np.abs(got["sum_sq"] - ref["sum_sq"])
    assert (err <= 1e-12 * ref["sum_sq"]).all(), (tag, float((err / np.maximum(ref["sum_sq"], 1e-300)).max()))


# ---- 1. score parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("gate", [0.3, 1.0])
@pytest.mark.parametrize("mode", MODES)
def test_score_parity(world, mode, gate, stride):
    poses = world["poses"]
    assert len(poses) == 37
    ref = restate(world, mode, poses, world["pts"], gate, stride)
    got, _ = world["factor"](mode).score_poses(*stack(poses), gate, stride=stride)
    print("mode %d gate %.1f stride %d: inliers of the truth %d / %d, of the 180-degree turn %d" %
          (mode, gate, stride, got["n_inliers"][0], got["n_points"][0], got["n_inliers"][3]))
    assert_scores(got, ref, (mode, gate, stride))
    assert got["n_points"][0] == -(-len(world["pts"]) // stride)
    assert (got["n_occupied"][FAR], got["n_inliers"][FAR], got["sum_sq"][FAR]) == (0, 0, 0.0)  # 1e7 m away: beyond 2^20 voxels, indexes nothing
    assert (got["n_occupied"][FREE], got["n_inliers"][FREE], got["sum_sq"][FREE]) == (0, 0, 0.0)
    assert got["n_inliers"][0] > got["n_points"][0] // 2  # the truth sees the room


# ---- 2. shapes where the fold can go wrong -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1024])
def test_factor_sizes(world, n):
    poses = world["poses"][:8]
    f = world["factor"](19, n=n)
    for stride in (1, n + 5):  # a stride larger than n: point 0 alone
        got, _ = f.score_poses(*stack(poses), 1.0, stride=stride)
        assert_scores(got, restate(world, 19, poses, world["pts"][:n], 1.0, stride), (n, stride))
        assert (got["n_points"] == (n if stride == 1 else 1)).all()


def test_cloud_spanning_several_chunks(world):
    """4 093 points: more than one workgroup per pose at stride 1 whatever the chunk (1 024 today), and at stride 3 (1 365 points)"""
    cloud = world["big_pts"][:4093]
    poses = world["poses"][:6] + world["poses"][10:14]
    f = world["factor"](19, cloud=cloud)
    for stride in (1, 3):
        got, _ = f.score_poses(*stack(poses), 1.0, stride=stride)
        assert_scores(got, restate(world, 19, poses, cloud, 1.0, stride), ("chunks", stride))


@pytest.mark.parametrize("n_poses", [1, 1025])
def test_batch_sizes(world, n_poses):
    base = world["poses"]
    poses = [base[(7 * j) % 37] for j in range(n_poses)]
    got, best = world["factor"](19).score_poses(*stack(poses), 1.0, stride=3, top_k=8)
    assert_scores(got, restate(world, 19, poses, world["pts"], 1.0, 3), n_poses)
    exp = list(reloc_ref.rank(got["n_inliers"], got["sum_sq"])[:8])
    assert list(best) == exp + [-1] * (8 - len(exp))


def test_empty_map(world):
    poses = world["poses"][:6]
    got, best = world["factor"]("empty").score_poses(*stack(poses), 1.0, top_k=3)
    assert (got["n_points"] == len(world["pts"])).all()
    assert not got["n_occupied"].any() and not got["n_inliers"].any() and not got["sum_sq"].any()
    assert list(best) == [0, 1, 2]  # all equal: the index decides


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloud_name", ["pts", "big_pts"])
def test_a_pose_scores_the_same_bits_anywhere(world, cloud_name):
    cloud = world[cloud_name] if cloud_name == "pts" else world["big_pts"][:4093]
    f = world["factor"](19, cloud=cloud)
    base = world["poses"]
    j = 1
    batch = [base[(5 * i + 2) % 37] for i in range(1025)]
    at0 = [base[j]] + batch[1:]
    at700 = batch[:700] + [base[j]] + batch[701:]
    alone = f.score_poses(*stack([base[j]]), 1.0)[0][0]
    rows = [alone, f.score_poses(*stack([base[j]]), 1.0)[0][0], f.score_poses(*stack(at0), 1.0)[0][0], f.score_poses(*stack(at700), 1.0)[0][700],
            f.score_poses(*stack(at700), 1.0)[0][700]]
    assert alone["n_inliers"] > 0 and alone["sum_sq"] > 0.0
    for r in rows[1:]:
        assert r.tobytes() == alone.tobytes()


# ---- 4. ranking --------------------------------------------------------------------------------------------------------------
def test_ranking_matches_numpy_sort(world):
    base = world["poses"]
    poses = [base[1 + i % 36] for i in range(200)]  # every pose several times over: equal keys that only the index separates
    poses[11] = poses[90] = poses[150] = base[0]    # the truth three times: it ranks first, lowest index first
    f = world["factor"](19)
    got, best = f.score_poses(*stack(poses), 1.0, stride=2, top_k=8)
    assert list(best) == list(reloc_ref.rank(got["n_inliers"], got["sum_sq"])[:8])
    assert list(best[:3]) == [11, 90, 150]
    # scores = NULL: the winners alone
    none, best2 = f.score_poses(*stack(poses), 1.0, stride=2, top_k=8, want_scores=False)
    assert none is None and list(best2) == list(best)
    for k in (1, 3):
        assert list(f.score_poses(*stack(poses), 1.0, stride=2, top_k=k, want_scores=False)[1]) == list(best[:k])
    # top_k above n_poses: -1 behind the last pose
    _, b3 = f.score_poses(*stack(poses[:3]), 1.0, top_k=8)
    assert sorted(b3[:3]) == [0, 1, 2] and list(b3[3:]) == [-1] * 5


# ---- 5. nothing else moves -----------------------------------------------------------------------------------------------------
def test_scoring_leaves_the_factor_alone(world):
    a, b = world["factor"](19, fresh=True), world["factor"](19, fresh=True)
    Rq, tq = world["poses"][1]
    ra, rb = a.linearize(Rq, tq, G), b.linearize(Rq, tq, G)
    before = a.state()
    poses = [world["poses"][(5 * i) % 37] for i in range(1025)]
    a.score_poses(*stack(poses), 1.0, top_k=8)
    for x, y, z in zip(a.state(), before, b.state()):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    R2, t2 = world["poses"][0]
    ra2, rb2 = a.linearize(R2, t2, G), b.linearize(R2, t2, G)
    assert ra2["linearize_count"] == rb2["linearize_count"] == ra["linearize_count"] + 1
    for k in ra2:
        if k.startswith("gpu_ms"):
            continue
        assert np.asarray(ra2[k]).tobytes() == np.asarray(rb2[k]).tobytes(), k
    for x, z in zip(a.state(), b.state()):
        assert x.tobytes() == z.tobytes()


# ---- 6. async ----------------------------------------------------------------------------------------------------------------
def test_async_equals_sync_and_holds_the_factor(world):
    capi = world["capi"]
    f = world["factor"](19)
    poses = [world["poses"][(2 * i) % 37] for i in range(300)]
    R, t = stack(poses)
    sync, best = f.score_poses(R, t, 1.0, stride=2, top_k=8)
    scores, b = f.score_poses_async(R, t, 1.0, stride=2, top_k=8)
    with pytest.raises(capi.MhError) as e:
        f.score_poses(R, t, 1.0)
    assert e.value.code == capi.MH_ERR_INVALID_ARG and "in flight" in str(e.value)
    with pytest.raises(capi.MhError) as e:
        f.relocalise(R, t, capi.make_reloc_config())
    assert e.value.code == capi.MH_ERR_INVALID_ARG
    f.wait()
    assert scores.tobytes() == sync.tobytes() and list(b) == list(best)
    again, _ = f.score_poses(R, t, 1.0, stride=2)  # free again
    assert again.tobytes() == sync.tobytes()


# ---- 7. relocalise -------------------------------------------------------------------------------------------------------------
GUESS_OFF = np.array([1.2, -0.9, 0.0])   # 1.5 m: more than the 1 m gate
GUESS_YAW = np.deg2rad(20.0)
GRID = dict(half_xy=2.0, step_xy=0.5, half_yaw=np.deg2rad(30.0), step_yaw=np.deg2rad(7.5))
COARSE = dict(gate=1.0, stride=4, top_k=4)
FINAL_GATE = 0.1


def reloc_align_cfg(capi):
    return capi.make_align_config(max_iters=30, eps_rot=1e-9, eps_trans=1e-9, damping=1e-9)


def test_relocalise_recovers_the_pose(world):
    """The grid is centred on a guess 1.5 m and 20 degrees off; the true pose is no node of it (offsets of 1.2 / 0.9 m on a 0.5 m
    grid, 20 degrees on a 7.5-degree one).  The image of the truth under the room's half turn lies a half turn away in yaw: outside
    the +-30 degrees searched."""
    capi, synth = world["capi"], world["synth"]
    Rg, tg = world["aux"]["R_W_L"], world["aux"]["t_W_L"]
    R0, t0 = synth.rot_z(GUESS_YAW) @ Rg, tg + GUESS_OFF
    Rs, ts = capi.pose_grid(R0, t0, **GRID)
    n = len(Rs)
    d_t, d_r = np.linalg.norm(ts - tg, axis=1), np.array([rot_angle(R, Rg) for R in Rs])
    assert (d_t + d_r > 1e-3).all() and d_t.min() < 0.36  # no node is the truth; one is near it
    cfg = capi.make_reloc_config(align=reloc_align_cfg(capi), final_gate=FINAL_GATE, **COARSE)
    f, twin = world["factor"](19, fresh=True), world["factor"](19, fresh=True)

    # the host-driven version: restated scores, numpy's top-K, one mh_icp_align per candidate, a restated re-score
    poses = [(Rs[i], ts[i]) for i in range(n)]
    coarse = restate(world, 19, poses, world["pts"], COARSE["gate"], COARSE["stride"], check_edge=False)
    order = [int(i) for i in reloc_ref.rank(coarse["n_inliers"], coarse["sum_sq"])[: COARSE["top_k"]]]
    aligned = []
    for i in order:
        twin.reset()
        aligned.append(twin.align(Rs[i], ts[i], cfg.align, G))
    fine = restate(world, 19, [(a["R"], a["t"]) for a in aligned], world["pts"], FINAL_GATE, 1, check_edge=False)
    host_best = int(reloc_ref.rank(fine["n_inliers"], fine["sum_sq"])[0])
    twin.reset()
    true_aligned = twin.align(Rg, tg, cfg.align, G)
    true_fine = restate(world, 19, [(true_aligned["R"], true_aligned["t"])], world["pts"], FINAL_GATE, 1, check_edge=False)[0]
    print("host-driven: candidates", order, "fine", [(int(s["n_inliers"]), float(s["sum_sq"])) for s in fine], "best", host_best,
          "aligned truth", (int(true_fine["n_inliers"]), float(true_fine["sum_sq"])))
    assert reloc_ref.key_not_worse(fine[host_best], true_fine)  # the host-driven version alone recovers the pose

    before = f.linearize(*world["poses"][1], G)["linearize_count"]
    out = f.relocalise(Rs, ts, cfg, G)
    assert out["n_candidates"] == COARSE["top_k"]
    assert [c["index"] for c in out["cand"]] == order
    fine_dev = restate(world, 19, [(c["R"], c["t"]) for c in out["cand"]], world["pts"], FINAL_GATE, 1, check_edge=False)
    for c, a, s_c, s_f in zip(out["cand"], aligned, coarse[order], fine_dev):
        dt, dr = float(np.linalg.norm(c["t"] - a["t"])), rot_angle(c["R"], a["R"])
        print("candidate %d: iters %d / %d, aligned pose differs by %.3e m %.3e rad" % (c["index"], c["iters"], a["iters"], dt, dr))
        assert dt <= 1e-9 and dr <= 1e-9
        assert (c["iters"], c["converged"]) == (a["iters"], a["converged"])
        for name in ("n_points", "n_occupied", "n_inliers"):
            assert c["coarse"][name] == s_c[name] and c["fine"][name] == s_f[name]
        assert abs(c["coarse"]["sum_sq"] - s_c["sum_sq"]) <= 1e-12 * s_c["sum_sq"]
        assert abs(c["fine"]["sum_sq"] - s_f["sum_sq"]) <= 1e-12 * s_f["sum_sq"]  # restated at the pose the device reports
    assert out["best"] == host_best
    w = out["cand"][out["best"]]
    assert np.array_equal(out["R"], w["R"]) and np.array_equal(out["t"], w["t"])
    assert reloc_ref.key_not_worse(w["fine"], true_fine)
    print("winner: candidate %d, %.4f m / %.4f deg from the truth (start node: %.3f m / %.2f deg)" %
          (w["index"], np.linalg.norm(out["t"] - tg), np.rad2deg(rot_angle(out["R"], Rg)), d_t[w["index"]], np.rad2deg(d_r[w["index"]])))
    # the factor is left reset: its state is a fresh factor's, its count advanced by the iterations run
    fresh = world["factor"](19, fresh=True)
    for x, y in zip(f.state(), fresh.state()):
        assert x.tobytes() == y.tobytes()
    after = f.linearize(*world["poses"][1], G)
    assert after["linearize_count"] == before + sum(c["iters"] for c in out["cand"]) + 1
    cold = fresh.linearize(*world["poses"][1], G)
    for k in ("H_ss", "b_s", "f", "n_knn"):
        assert np.asarray(after[k]).tobytes() == np.asarray(cold[k]).tobytes(), k


# ---- 8. refusals that need a device --------------------------------------------------------------------------------------------
def test_refusals(world):
    capi = world["capi"]
    L = world["ctx"].L
    f = world["factor"](19)
    R, t = stack(world["poses"][:4])

    def refused(code, call, *words):
        with pytest.raises(capi.MhError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    rcfg = capi.make_reloc_config()
    binary = world["factor"](19, binary=True)
    refused(capi.MH_ERR_UNSUPPORTED, lambda: binary.score_poses(R, t, 1.0), "unary")
    refused(capi.MH_ERR_UNSUPPORTED, lambda: binary.relocalise(R, t, rcfg))
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.relocalise(R, t, capi.make_reloc_config(top_k=0)), "top_k")
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.relocalise(R, t, capi.make_reloc_config(final_gate=float("nan"))), "final_gate")
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.score_poses(R[:0], t[:0], 1.0), "n_poses")
    for gate in (0.0, -1.0, float("inf"), float("nan")):
        refused(capi.MH_ERR_INVALID_ARG, lambda: f.score_poses(R, t, gate), "gate")
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.score_poses(R, t, 1.0, stride=0), "stride")
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.score_poses(R, t, 1.0, top_k=9), "top_k")
    bad = t.copy()
    bad[2, 1] = np.nan
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.score_poses(R, bad, 1.0), "pose 2")
    badR = R.copy()
    badR[3, 0, 0] = np.inf
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.score_poses(badR, t, 1.0), "pose 3")
    empty = capi.ICPFactor(world["ctx"], world["maps"][19], np.zeros(0, world["pts"].dtype), capi.make_reg_config(**world["synth"].enwide_config()))
    refused(capi.MH_ERR_INVALID_ARG, lambda: empty.score_poses(R, t, 1.0), "no points")
    empty.destroy()
    # best == NULL with top_k > 0
    Rc, tc = np.ascontiguousarray(R.reshape(-1, 9)), np.ascontiguousarray(t)
    cfg = capi.ScoreConfig(1.0, 1, 2)
    import ctypes as C
    assert L.mh_icp_score_poses(f.h, capi._p(Rc), capi._p(tc), len(Rc), C.byref(cfg), None, None) == capi.MH_ERR_INVALID_ARG
    # a call in flight: a linearize nobody waited for
    keep = f.linearize_async(*world["poses"][1], G)
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.score_poses(R, t, 1.0), "in flight")
    refused(capi.MH_ERR_INVALID_ARG, lambda: f.relocalise(R, t, rcfg), "in flight")
    f.wait()
    assert keep.linearize_count >= 1
    f.score_poses(R, t, 1.0)  # and accepted again
