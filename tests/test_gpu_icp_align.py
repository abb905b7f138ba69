"""-m gpu: mh_icp_align — the Gauss-Newton loop as one chain of launches — against the loop a caller writes around
mh_icp_linearize (components off) with a numpy solve and the replay's retraction, on clones of the same factor.

Scene: one room of mimosa_amd/synth.py as the map, a scan cast from the ground-truth pose (24 576 points: the two-lanes-per-point
launch class for k = 5, the 256-thread class for k = 8; 131 072 points: the 512-thread class), started from the truth perturbed
by 0.05-0.5 m and 1-5 degrees.  Bars: same iters / converged, every trace pose within 1e-9 m / 1e-9 rad of the host loop's, final
status arrays equal; final error against the truth no worse than the host loop's + 1e-9.

Seeds: CASES below are the first seeds tried, none replaced.  test_host_loop_is_stable_on_the_kept_cases runs the host loop
against itself under a 1e-13 m perturbation of the start pose and holds it to the same 1e-9 bar."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = np.array([0.0, 0.0, -1.0])


def expmap(w):
    w = np.asarray(w, float)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    return np.eye(3) + A * K + B * (K @ K)


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    s = np.linalg.norm((Ra.T @ Rb - (Ra.T @ Rb).T)) / (2.0 * np.sqrt(2.0))
    return float(np.arctan2(s, c))


def host_step(r, R, t, cfg):
    """(R, t) after one step from the result of a linearize at (R, t); None when the system is singular"""
    A = r["H_ss"].copy()
    pr = 1.0 / cfg.prior_sigma_rot**2 if cfg.prior_sigma_rot > 0 else 0.0
    pt = 1.0 / cfg.prior_sigma_trans**2 if cfg.prior_sigma_trans > 0 else 0.0
    for i in range(6):
        A[i, i] = (A[i, i] + (pr if i < 3 else pt)) + cfg.damping
    if not np.all(np.linalg.eigvalsh((A + A.T) / 2) > 0):
        return None
    xi = np.linalg.solve(A, -r["b_s"])
    return R @ expmap(xi[:3]), t + R @ xi[3:], xi


def host_loop(f, R0, t0, cfg, g=G):
    """what a caller writes today: mh_icp_linearize + solve + retract, same config and stopping rule"""
    f.set_components(False)
    R, t = np.array(R0, float), np.array(t0, float)
    trace, converged = [], 0
    for _ in range(cfg.max_iters):
        r = f.linearize(R, t, g)
        s = host_step(r, R, t, cfg)
        if s is None:
            trace.append(dict(R=R, t=t, f=r["f"], singular=True, res=r))
            break
        R, t, xi = s
        trace.append(dict(R=R, t=t, f=r["f"], singular=False, res=r, xi=xi))
        if np.linalg.norm(xi[:3]) < cfg.eps_rot and np.linalg.norm(xi[3:]) < cfg.eps_trans:
            converged = 1
            break
    return dict(R=R, t=t, iters=len(trace), converged=converged, trace=trace)


@pytest.fixture(scope="module")
def world():
    from mimosa_amd import capi, synth
    ctx = capi.Context(0)
    gm = capi.VoxelMap(ctx)
    gm.insert(synth.make_room(synth.BASE_SEED, 0, 0))
    big, _ = synth.make_scan(128)
    mid, _ = synth.make_scan(64)
    clouds = {131072: np.ascontiguousarray(big[:131072]), 24576: np.ascontiguousarray(mid[:: max(1, len(mid) // 24576)][:24576])}
    assert len(clouds[131072]) == 131072 and len(clouds[24576]) == 24576
    factors = {}

    def factor(n, k, reg4, project=0, binary=False):
        key = (n, k, reg4, project, binary)
        if key not in factors:
            cfg = dict(synth.enwide_config(), num_corres_points=k, reg_4_dof=reg4, project_on_degneneracy=project)
            factors[key] = capi.ICPFactor(ctx, gm, clouds[n], capi.make_reg_config(**cfg), binary=binary)
        return factors[key]

    yield dict(ctx=ctx, map=gm, factor=factor, truth=synth.sensor_pose_gt())
    for f in factors.values():
        f.destroy()
    gm.release()
    ctx.close()


def perturbed(truth, seed):
    rng = np.random.default_rng(seed)
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    w = ax / np.linalg.norm(ax) * np.deg2rad(rng.uniform(1.0, 5.0))
    dt = d / np.linalg.norm(d) * rng.uniform(0.05, 0.5)
    R, t = truth
    return R @ expmap(w), t + dt


def align_cfg(reg4, **kw):
    from mimosa_amd import capi
    base = dict(max_iters=30, eps_rot=1e-6, eps_trans=1e-6, damping=1e-9, prior_sigma_rot=(0.1 if reg4 else 0.0))
    base.update(kw)
    return capi.make_align_config(**base)


CASES = [(n, k, reg4, seed) for n in (24576, 131072) for k in (5, 8) for reg4 in (0, 1) for seed in (1, 2)]


def compare(got, ref, tag):
    print(tag, "iters", got["iters"], ref["iters"], "converged", got["converged"], ref["converged"])
    worst_t = worst_r = 0.0
    for a, b in zip(got["trace"], ref["trace"]):
        worst_t = max(worst_t, float(np.linalg.norm(a["t"] - b["t"])))
        worst_r = max(worst_r, rot_angle(a["R"], b["R"]))
    print(tag, "worst trace difference: %.3e m %.3e rad" % (worst_t, worst_r))
    assert got["iters"] == ref["iters"] and got["converged"] == ref["converged"]
    assert worst_t <= 1e-9 and worst_r <= 1e-9
    return worst_t, worst_r


def test_one_iteration_is_a_linearize(world):
    for n, k, reg4 in ((24576, 5, 0), (24576, 8, 1), (131072, 5, 0)):
        base = world["factor"](n, k, reg4)
        a, b = base.clone(), base.clone()
        R0, t0 = perturbed(world["truth"], 7)
        cfg = align_cfg(reg4, max_iters=1)
        got = a.align(R0, t0, cfg)
        b.set_components(False)
        ref = b.linearize(R0, t0, G)
        for key in ("H_ss", "b_s", "f", "n_knn", "n_exact_fallback", "mean_candidates", "mean_scanned", "loc_rot_final", "loc_trans_final",
                    "eigvec_rot", "eigvec_trans", "degen_rot", "degen_trans", "linearize_count", "status_hist"):
            assert np.array_equal(np.asarray(got["first"][key]), np.asarray(ref[key]), equal_nan=True), (n, k, key)
        assert np.all(np.isnan(got["first"]["loc_trans_comp"])) and np.array_equal(np.asarray(got["last"]["H_ss"]), np.asarray(ref["H_ss"]))
        for x, y in zip(a.state(), b.state()):
            assert np.array_equal(x, y, equal_nan=True)
        Rn, tn, xi = host_step(ref, R0, t0, cfg)
        assert got["iters"] == 1 and np.abs(got["R"] - Rn).max() <= 1e-12 and np.abs(got["t"] - tn).max() <= 1e-12
        assert got["trace"][0]["n_knn"] == ref["n_knn"] and got["trace"][0]["f"] == ref["f"]
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("n,k,reg4,seed", CASES)
def test_chain_is_the_host_loop(world, n, k, reg4, seed):
    base = world["factor"](n, k, reg4)
    a, b = base.clone(), base.clone()
    R0, t0 = perturbed(world["truth"], seed)
    cfg = align_cfg(reg4)
    got = a.align(R0, t0, cfg)
    ref = host_loop(b, R0, t0, cfg)
    compare(got, ref, f"n={n} k={k} reg4={reg4} seed={seed}")
    assert np.array_equal(a.state()[0], b.state()[0])
    # `last` is what mh_icp_linearize returned at the last pose the host loop evaluated (the poses agree to 1e-9, not to the
    # bit, from the second iteration on: the sums follow them), `first` is the host loop's first result bit for bit
    for key in ("H_ss", "b_s", "f", "n_knn", "n_exact_fallback", "mean_candidates", "mean_scanned", "linearize_count"):
        assert np.array_equal(np.asarray(got["first"][key]), np.asarray(ref["trace"][0]["res"][key])), key
    lr = ref["trace"][-1]["res"]
    for key in ("n_knn", "n_exact_fallback", "mean_candidates", "mean_scanned", "linearize_count"):
        assert np.array_equal(np.asarray(got["last"][key]), np.asarray(lr[key])), key
    for key in ("H_ss", "b_s", "f"):
        x, y = np.asarray(got["last"][key], float), np.asarray(lr[key], float)
        assert np.linalg.norm(x - y) <= 1e-6 * np.linalg.norm(y), key  # d(sums) / d(pose) ~ |H| / 0.07 m: 1e-9 m of pose is ~1e-8 relative
    # it converges where the host loop does: error against the scene's true pose
    Rt, tt = world["truth"]
    e_got, e_ref = (np.linalg.norm(got["t"] - tt), rot_angle(got["R"], Rt)), (np.linalg.norm(ref["t"] - tt), rot_angle(ref["R"], Rt))
    print("error against the truth: chain %.3e m %.3e rad, host loop %.3e m %.3e rad" % (e_got + e_ref))
    assert e_got[0] <= e_ref[0] + 1e-9 and e_got[1] <= e_ref[1] + 1e-9
    if not reg4:
        assert got["converged"] == 1 and e_got[0] < 0.02 and e_got[1] < 0.005  # a well-constrained room: it does get there
    a.destroy()
    b.destroy()


@pytest.mark.parametrize("n,k,reg4,seed", CASES)
def test_host_loop_is_stable_on_the_kept_cases(world, n, k, reg4, seed):
    """the reference against itself under a 1e-13 m perturbation: a case whose associations sit on a threshold would move here"""
    base = world["factor"](n, k, reg4)
    a, b = base.clone(), base.clone()
    R0, t0 = perturbed(world["truth"], seed)
    cfg = align_cfg(reg4)
    r0, r1 = host_loop(a, R0, t0, cfg), host_loop(b, R0, t0 + np.array([1e-13, 0.0, 0.0]), cfg)
    compare(r0, r1, f"host loop vs itself n={n} k={k} reg4={reg4} seed={seed}")
    a.destroy()
    b.destroy()


def test_check_every_async_warm_and_cold(world):
    from mimosa_amd import capi
    base = world["factor"](24576, 5, 0)
    R0, t0 = perturbed(world["truth"], 3)

    def flat(d):
        return np.concatenate([d["R"].ravel(), d["t"], [d["iters"], d["converged"]]] + [np.concatenate([r["R"].ravel(), r["t"], [r["f"], r["step_rot"], r["step_trans"], r["n_knn"], r["degenerate"]]]) for r in d["trace"]]
                              + [np.asarray(d["last"]["H_ss"]).ravel(), np.asarray(d["first"]["b_s"])])

    outs, states = [], []
    for ce in (0, 1, 4, 7):
        c = base.clone()
        outs.append(flat(c.align(R0, t0, align_cfg(0, check_every=ce))))
        states.append(c.state())
        assert c.linearize(R0, t0, G)["linearize_count"] == int(outs[-1][12]) + 1  # the count advanced by the executed iterations
        c.destroy()
    c = base.clone()
    cfg = align_cfg(0)
    pending = c.align_async(R0, t0, cfg)
    with pytest.raises(capi.MhError):  # in flight: refused
        c.align(R0, t0, cfg)
    with pytest.raises(capi.MhError):
        c.linearize(R0, t0, G)
    c.wait()
    outs.append(flat(pending.as_dict()))
    states.append(c.state())
    c.destroy()
    for o, s in zip(outs[1:], states[1:]):
        assert np.array_equal(o, outs[0])
        for x, y in zip(s, states[0]):
            assert np.array_equal(x, y, equal_nan=True)
    # a warm factor (linearized once before) and a cold one both match their host loops
    for warm in (False, True):
        a, b = base.clone(), base.clone()
        if warm:
            Rw, tw = perturbed(world["truth"], 99)
            for f in (a, b):
                f.set_components(False)
                f.linearize(Rw, tw, G)
        got, ref = a.align(R0, t0, cfg), host_loop(b, R0, t0, cfg)
        compare(got, ref, f"warm={warm}")
        assert np.array_equal(a.state()[0], b.state()[0])
        assert got["last"]["linearize_count"] == ref["trace"][-1]["res"]["linearize_count"]
        a.destroy()
        b.destroy()


def test_refusals(world):
    from mimosa_amd import capi
    f = world["factor"](24576, 5, 0).clone()
    R0, t0 = world["truth"]
    for bad in (0, 65, -3):
        with pytest.raises(capi.MhError) as e:
            f.align(R0, t0, align_cfg(0, max_iters=bad))
        assert e.value.code == capi.MH_ERR_INVALID_ARG and "max_iters" in str(e.value)
    with pytest.raises(capi.MhError) as e:
        f.align(R0, t0, align_cfg(0, damping=-1.0))
    assert e.value.code == capi.MH_ERR_INVALID_ARG
    f.destroy()
    b = world["factor"](24576, 5, 0, binary=True)
    with pytest.raises(capi.MhError) as e:
        b.align(R0, t0, align_cfg(0))
    assert e.value.code == capi.MH_ERR_UNSUPPORTED and "unary" in str(e.value)


def test_degenerate_scene(world):
    """A single plane: a floor with 4 mm of roughness (an exact plane fails the reference's minimum-eigenvalue gate and leaves
    no valid point at all) and the scan's floor hits.  x, y and yaw are unconstrained.
    project_on_degneneracy on: every iteration is degenerate, H = b = 0 — with a prior the step is zero, the pose
    does not move and the call converges at once; without prior and damping the system is singular: MH_OK, converged = 0, pose
    unchanged, one iteration, bit 4.  Projection off + a tight prior (0.5 mm, 0.12 mrad): the chain is the host loop, every row
    carries the translation bit, and the pose moves in z, roll and pitch only.  What leaks into x, y and yaw is bounded from the
    scene: the fitted normals tilt by delta ~ roughness / neighbour spacing = 4 mm / 0.15 m, so b has sqrt(N) delta e0 / sigma^2 in
    x, y (r_max times that in yaw) against the prior's 1 / sigma_prior^2 on the diagonal; the residual e0 (3 cm of height + the
    tilt's lever over 8 m) decays by p / (H + p) per iteration (H from the first linearization), and the scan's 2 cm range noise
    stays in the residuals of every one of the 40 iterations (convergence test off: a fixed count); ten times that is the bar."""
    from mimosa_amd import capi, synth
    ctx = world["ctx"]
    Rt, tt = world["truth"]
    gx, gy = np.meshgrid(np.arange(-10.0, 10.0, 0.08), np.arange(-10.0, 10.0, 0.08))  # the patch of floor under the sensor
    origin = synth.room_origin(0, 0)
    rough = np.random.default_rng(0).normal(0.0, 0.004, gx.size)
    plane = np.stack([gx.ravel() + tt[0], gy.ravel() + tt[1], origin[2] + rough], axis=1).astype(np.float32)
    gm = capi.VoxelMap(ctx)
    gm.insert(plane)
    scan, _ = synth.make_scan(64)
    pw = synth.points_xyz(scan).astype(np.float64) @ Rt.T + tt
    room = np.asarray(synth.ROOM, float)
    inside = np.all((pw[:, :2] > origin[:2] + 0.3) & (pw[:, :2] < origin[:2] + room[:2] - 0.3), axis=1)  # (no wall hit near the floor)
    near = np.linalg.norm(synth.points_xyz(scan), axis=1) < 8.0  # (a short lever: the tilt's residual stays below the gates)
    floor = np.ascontiguousarray(scan[inside & near & (np.abs(pw[:, 2] - origin[2]) < 0.06)][:20000])
    assert len(floor) > 5000
    tilt, lift = np.array([0.002, -0.003, 0.0]), 0.03
    R0, t0 = Rt @ expmap(tilt), tt + np.array([0.0, 0.0, lift])
    for project in (1, 0):
        cfg = dict(synth.enwide_config(), project_on_degneneracy=project, degen_thresh_trans=1e6)  # (a threshold no plane's x, y reach)
        base = capi.ICPFactor(ctx, gm, floor, capi.make_reg_config(**cfg))
        if project:
            a = base.clone()
            got = a.align(R0, t0, align_cfg(0, prior_sigma_rot=0.1, prior_sigma_trans=0.1))
            assert got["iters"] == 1 and got["converged"] == 1 and got["trace"][0]["degenerate"] & 2
            assert np.array_equal(got["R"], R0) and np.array_equal(got["t"], t0)
            assert not np.any(got["first"]["H_ss"]) and got["trace"][0]["f"] > 0.0  # points were valid: it is the projection that zeroed H
            a.destroy()
            a, b = base.clone(), base.clone()
            c0 = align_cfg(0, damping=0.0)
            got, ref = a.align(R0, t0, c0), host_loop(b, R0, t0, c0)
            assert got["iters"] == 1 == ref["iters"] and got["converged"] == 0 == ref["converged"] and got["trace"][0]["degenerate"] & 4
            assert np.array_equal(got["R"], R0) and np.array_equal(got["t"], t0) and np.all(np.isfinite(got["R"]))
            assert np.array_equal(a.state()[0], b.state()[0])
            a.destroy()
            b.destroy()
        else:
            a, b = base.clone(), base.clone()
            sp_t, sp_r, n_it = 5e-4, 1.2e-4, 40
            c1 = align_cfg(0, prior_sigma_rot=sp_r, prior_sigma_trans=sp_t, max_iters=n_it, eps_rot=0.0, eps_trans=0.0)
            got, ref = a.align(R0, t0, c1), host_loop(b, R0, t0, c1)
            compare(got, ref, "plane, projection off")
            assert all(r["degenerate"] & 2 for r in got["trace"])
            d = got["t"] - t0
            dR = got["R"] @ R0.T  # the total rotation in the world frame
            w = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0
            r_max = float(np.linalg.norm(synth.points_xyz(floor), axis=1).max())
            n_pts, delta, sigma = len(floor), 0.004 / 0.15, 0.07
            e0 = lift + float(np.linalg.norm(tilt)) * r_max
            H0 = np.asarray(got["first"]["H_ss"])
            geo_t, geo_r = 1.0 + 1.0 / (H0[5, 5] * sp_t**2), 1.0 + 1.0 / (min(H0[0, 0], H0[1, 1]) * sp_r**2)  # sum of (p / (H + p))^k
            floor_res = n_it * synth.SIGMA_N  # what the scan's range noise leaves in every iteration's residuals
            bar_xy = 10 * np.sqrt(n_pts) * delta * (geo_t * e0 + floor_res) / sigma**2 * sp_t**2
            bar_yaw = 10 * np.sqrt(n_pts) * r_max * delta * (geo_r * e0 + floor_res) / sigma**2 * sp_r**2
            print("plane: moved", d, "rotated", w, "bars: xy %.3e m, yaw %.3e rad" % (bar_xy, bar_yaw), "iters", got["iters"])
            print("plane: H diagonal at the start", np.diag(got["first"]["H_ss"]), "points", n_pts, "r_max", r_max)
            assert abs(got["t"][2] - tt[2]) < 0.005 and abs(d[2]) > 0.02                              # z comes back to the floor's
            assert np.hypot(w[0], w[1]) > 0.5 * np.linalg.norm(tilt)                                  # roll and pitch are corrected
            assert np.hypot(d[0], d[1]) <= bar_xy and bar_xy <= 0.1 * abs(d[2])                       # x, y: the leak only
            assert abs(w[2]) <= bar_yaw and bar_yaw <= 0.3 * np.hypot(w[0], w[1])                     # yaw likewise
            a.destroy()
            b.destroy()
        base.destroy()
    gm.release()
