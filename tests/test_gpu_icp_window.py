"""-m gpu: mh_icp_window_optimise — the fixed-lag Gauss-Newton loop as one chain of launches — against the loop a caller writes
today: mh_icp_linearize_batch (components off), a numpy assembly of the window's system with a refined solve, the replay's
retraction; on clones of the same factors.

Scene: synth.small_world() (a map of ~5 k points, a 1 024-point scan cloned W times), every pose the truth perturbed by up to
0.2 m and 3 degrees with its own seed, Z from the unperturbed relative poses (identity) with the replay's sigmas.  One case of
nine 8 192-point scans in the big room (73 728 points: the 512-thread launch class), one with an empty factor, one with
project_on_degneneracy.

Bars.  First iteration: per-point state and counters bit-identical to mh_icp_linearize_batch, the sums too (both choose the
launch class the same way).  Every iteration: every pose within 1e-9 m and 1e-9 rad of the host loop's; same iters and
converged; final status arrays equal.  W = 1 against mh_icp_align under the equivalent config: 1e-12.  The result does not
depend on check_every nor on sync / async, bit for bit.  Refusals leave the handles usable.

Seeds: the poses' seeds are 100 * case seed + pose index, case seeds as listed in KEPT (the parametrised CASES and the four
single cases) — the first tried, none replaced.  test_host_loop_is_stable_on_the_kept_cases runs the host loop of every one of
them against itself under a 1e-13 m perturbation of every start pose and holds it to the same 1e-9 bar."""
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


def so3log(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    th = np.arccos(c)
    s = 0.5 if th < 1e-9 else th / (2.0 * np.sin(th))
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * s


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def adjoint(R, t):
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    s = np.linalg.norm((Ra.T @ Rb - (Ra.T @ Rb).T)) / (2.0 * np.sqrt(2.0))
    return float(np.arctan2(s, c))


def solve_refined(A, rhs):
    x = np.linalg.solve(A, rhs)
    Al, rl = A.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(4):
        r = (rl - Al @ x.astype(np.longdouble)).astype(np.float64)
        x = x + np.linalg.solve(A, r)
    return x


def host_system(res, poses, Z, has_Z, cfg):
    """one iteration of WindowSmootherT::optimise without the photometric terms, from the batch's results"""
    W = len(poses)
    A, g, cost = np.zeros((6 * W, 6 * W)), np.zeros(6 * W), 0.0
    for i, r in enumerate(res):
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += r["H_ss"]
        g[6 * i:6 * i + 6] += r["b_s"]
        cost += r["f"]
    Wb = np.diag(np.array(cfg.between_info))
    for i in range(1, W):
        if not has_Z[i]:
            continue
        (Ra, ta), (Rb, tb), (ZR, Zt) = poses[i - 1], poses[i], Z[i]
        abR, abt = Ra.T @ Rb, Ra.T @ (tb - ta)
        r = np.concatenate([so3log(ZR.T @ abR), ZR.T @ (abt - Zt)])
        Ja = -adjoint(abR.T, abR.T @ (-abt))
        a, b = slice(6 * (i - 1), 6 * i), slice(6 * i, 6 * i + 6)
        A[a, a] += Ja.T @ Wb @ Ja
        A[a, b] += Ja.T @ Wb
        A[b, a] += Wb @ Ja
        A[b, b] += Wb
        g[a] += Ja.T @ Wb @ r
        g[b] += Wb @ r
        cost += r @ Wb @ r
    A[:6, :6] += np.diag(np.array(cfg.prior_info))
    A += cfg.damping * np.eye(6 * W)
    return A, g, cost


def host_loop(factors, poses, Z, has_Z, cfg):
    """what a caller writes today: mh_icp_linearize_batch + assembly + solve + retract, same config and stopping rule"""
    from mimosa_amd import capi
    for f in factors:
        f.set_components(False)
    poses = [(np.array(R, float), np.array(t, float)) for R, t in poses]
    W = len(poses)
    trace, converged = [], 0
    for _ in range(cfg.iters):
        res = capi.linearize_batch(factors, [p[0] for p in poses], [p[1] for p in poses])
        A, g, cost = host_system(res, poses, Z, has_Z, cfg)
        if not np.all(np.linalg.eigvalsh((A + A.T) / 2) > 0):
            trace.append(dict(poses=poses, f=cost, res=res, singular=True))
            break
        xi = solve_refined(A, -g).reshape(W, 6)
        poses = [(R @ expmap(x[:3]), t + R @ x[3:]) for (R, t), x in zip(poses, xi)]
        trace.append(dict(poses=poses, f=cost, res=res, singular=False, xi=xi))
        if np.all(np.linalg.norm(xi[:, :3], axis=1) < cfg.eps_rot) and np.all(np.linalg.norm(xi[:, 3:], axis=1) < cfg.eps_trans):
            converged = 1
            break
    return dict(poses=poses, iters=len(trace), converged=converged, trace=trace)


class World:
    def __init__(self):
        from mimosa_amd import capi, synth
        self.capi, self.synth = capi, synth
        self.ctx = capi.Context(0)
        m, pts, aux = synth.small_world()
        self.small_map = capi.VoxelMap(self.ctx)
        self.small_map.insert(m)
        self.small_scan = np.ascontiguousarray(pts)
        self.small_truth = (np.array(aux["R_W_L"]), np.array(aux["t_W_L"]))
        self.big_map = None
        self.bases = {}
        assert len(self.small_scan) == 1024

    def base(self, k=5, reg4=0, project=0, big=False, empty=False, binary=False):
        key = (k, reg4, project, big, empty, binary)
        if key not in self.bases:
            capi, synth = self.capi, self.synth
            cfg = dict(synth.enwide_config(), num_corres_points=k, reg_4_dof=reg4, project_on_degneneracy=project)
            if project:
                cfg["degen_thresh_trans"] = 1e6  # a threshold no direction reaches: every iteration is degenerate
            if big and self.big_map is None:
                self.big_map = capi.VoxelMap(self.ctx)
                self.big_map.insert(synth.make_room(synth.BASE_SEED, 0, 0))
                self.big_scan = np.ascontiguousarray(synth.make_scan(64, n_cols=128)[0])
                assert len(self.big_scan) == 8192
            pts = self.big_scan if big else (self.small_scan[:0] if empty else self.small_scan)
            self.bases[key] = capi.ICPFactor(self.ctx, self.big_map if big else self.small_map, pts, capi.make_reg_config(**cfg), binary=binary)
        return self.bases[key]

    def truth(self, big=False):
        return self.synth.sensor_pose_gt() if big else self.small_truth

    def close(self):
        for f in self.bases.values():
            f.destroy()
        self.small_map.release()
        if self.big_map is not None:
            self.big_map.release()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def perturbed(truth, seed):
    rng = np.random.default_rng(seed)
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    w = ax / np.linalg.norm(ax) * np.deg2rad(rng.uniform(0.0, 3.0))
    dt = d / np.linalg.norm(d) * rng.uniform(0.0, 0.2)
    R, t = truth
    return R @ expmap(w), t + dt


def scene(world, W, seed, big=False):
    """start poses, between measurements (the unperturbed relative poses: every scan was cast from the same pose) and has_Z"""
    poses = [perturbed(world.truth(big), 100 * seed + i) for i in range(W)]
    Z = [(np.eye(3), np.zeros(3)) for _ in range(W)]
    return poses, Z, [0] + [1] * (W - 1)


def window_cfg(tight=False, **kw):
    from mimosa_amd import capi
    base = dict(iters=10, eps_rot=1e-6, eps_trans=1e-6, damping=1e-9)
    if not tight:  # the replay's loose prior: the oldest pose was never optimised
        base.update(prior_sigma_rot=0.017453292519943295, prior_sigma_trans=0.1)
    base.update(kw)
    return capi.make_window_config(**base)


def compare(got, ref, tag):
    print(tag, "iters", got["iters"], ref["iters"], "converged", got["converged"], ref["converged"])
    worst_t = worst_r = 0.0
    for it in range(min(got["iters"], ref["iters"])):
        for i, (R, t) in enumerate(ref["trace"][it]["poses"]):
            p = got["poses"][it, i]
            worst_t = max(worst_t, float(np.linalg.norm(p[9:] - t)))
            worst_r = max(worst_r, rot_angle(p[:9].reshape(3, 3), R))
    print(tag, "worst pose difference over the iterations: %.3e m %.3e rad" % (worst_t, worst_r))
    assert got["iters"] == ref["iters"] and got["converged"] == ref["converged"]
    assert worst_t <= 1e-9 and worst_r <= 1e-9


COUNTERS = ("n_knn", "n_exact_fallback", "mean_candidates", "mean_scanned", "linearize_count")


def run_case(world, W, k, reg4, seed, tight=False, project=0, big=False, empty_at=None, **cfg_kw):
    capi = world.capi
    base = world.base(k, reg4, project, big)
    mk = lambda i: (world.base(k, reg4, project, empty=True) if i == empty_at else base).clone()  # noqa: E731
    a, b = [mk(i) for i in range(W)], [mk(i) for i in range(W)]
    poses, Z, has_Z = scene(world, W, seed, big)
    cfg = window_cfg(tight, **cfg_kw)
    got = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True)
    ref = host_loop(b, poses, Z, has_Z, cfg)
    tag = f"W={W} k={k} reg4={reg4} seed={seed} tight={tight} project={project} big={big} empty_at={empty_at}"
    # the first iteration is a batch linearize at the start poses, bit for bit
    for i in range(W):
        r0 = ref["trace"][0]["res"][i]
        for key in ("H_ss", "b_s", "f") + COUNTERS:
            assert np.array_equal(np.asarray(got["first"][i][key]), np.asarray(r0[key]), equal_nan=True), (tag, i, key)
    compare(got, ref, tag)
    for i in range(W):
        assert np.array_equal(a[i].state()[0], b[i].state()[0]), (tag, i)
        lr = ref["trace"][-1]["res"][i]
        for key in COUNTERS:
            assert np.array_equal(np.asarray(got["last"][i][key]), np.asarray(lr[key]), equal_nan=True), (tag, i, key)
        assert np.abs(got["R"][i] - got["poses"][-1, i, :9].reshape(3, 3)).max() == 0.0 and np.array_equal(got["t"][i], got["poses"][-1, i, 9:])
    for it in range(got["iters"]):
        assert abs(got["trace"][it]["f"] - ref["trace"][it]["f"]) <= 1e-6 * max(1.0, abs(ref["trace"][it]["f"]))  # (the sums follow poses 1e-9 apart)
    for f in a + b:
        f.destroy()
    return got, ref


CASES = [(W, k, reg4, 1) for W in (1, 2, 5, 16) for k in (5, 8) for reg4 in (0, 1)]


@pytest.mark.parametrize("W,k,reg4,seed", CASES)
def test_chain_is_the_host_loop(world, W, k, reg4, seed):
    run_case(world, W, k, reg4, seed, tight=(W == 5))


def test_fixed_iteration_count_of_the_replay(world):
    got, _ = run_case(world, 5, 5, 0, 2, tight=True, iters=6, eps_rot=0.0, eps_trans=0.0)
    assert got["iters"] == 6 and got["converged"] == 0


def test_project_on_degeneracy(world):
    """every factor degenerate in every iteration: H = b = 0, the between factors and the prior alone move the poses"""
    got, _ = run_case(world, 3, 5, 0, 3, project=1)
    assert all(r["degenerate"] & 0b101010 == 0b101010 for r in got["trace"])
    assert not np.any(got["first"][1]["H_ss"])


def test_more_than_65536_points_runs_the_512_thread_class(world):
    run_case(world, 9, 5, 0, 4, big=True, iters=6)


def test_an_empty_factor_contributes_nothing(world):
    got, _ = run_case(world, 4, 5, 0, 5, empty_at=2)
    assert not np.any(got["first"][2]["H_ss"]) and got["first"][2]["f"] == 0.0


def test_first_iteration_state_is_the_batch_linearize(world):
    capi = world.capi
    for W, k in ((5, 5), (3, 8), (16, 5)):
        base = world.base(k)
        a, b = [base.clone() for _ in range(W)], [base.clone() for _ in range(W)]
        poses, Z, has_Z = scene(world, W, 6)
        capi.optimise_window(a, poses, window_cfg(iters=1), has_Z=has_Z, Z=Z)
        for f in b:
            f.set_components(False)
        capi.linearize_batch(b, [p[0] for p in poses], [p[1] for p in poses])
        for x, y in zip(a, b):
            for u, v in zip(x.state(), y.state()):
                assert np.array_equal(u, v, equal_nan=True)
        for f in a + b:
            f.destroy()


# every case held to the 1e-9 bar against the host loop above: run_case's arguments
KEPT = [dict(W=W, k=k, reg4=reg4, seed=seed, tight=(W == 5)) for W, k, reg4, seed in CASES] + [
    dict(W=5, k=5, reg4=0, seed=2, tight=True, iters=6, eps_rot=0.0, eps_trans=0.0),  # test_fixed_iteration_count_of_the_replay
    dict(W=3, k=5, reg4=0, seed=3, project=1),                                         # test_project_on_degeneracy
    dict(W=9, k=5, reg4=0, seed=4, big=True, iters=6),                                 # test_more_than_65536_points_...
    dict(W=4, k=5, reg4=0, seed=5, empty_at=2),                                        # test_an_empty_factor_contributes_nothing
]


@pytest.mark.parametrize("case", KEPT, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k in ("W", "k", "reg4", "seed")))
def test_host_loop_is_stable_on_the_kept_cases(world, case):
    """the reference against itself under a 1e-13 m perturbation: a case whose associations sit on a threshold would move here"""
    c = dict(case)
    W, k, reg4, seed = c.pop("W"), c.pop("k"), c.pop("reg4"), c.pop("seed")
    tight, project, big, empty_at = c.pop("tight", False), c.pop("project", 0), c.pop("big", False), c.pop("empty_at", None)
    base = world.base(k, reg4, project, big)
    mk = lambda i: (world.base(k, reg4, project, empty=True) if i == empty_at else base).clone()  # noqa: E731
    a, b = [mk(i) for i in range(W)], [mk(i) for i in range(W)]
    poses, Z, has_Z = scene(world, W, seed, big)
    cfg = window_cfg(tight, **c)
    r0 = host_loop(a, poses, Z, has_Z, cfg)
    r1 = host_loop(b, [(R, t + np.array([1e-13, 0.0, 0.0])) for R, t in poses], Z, has_Z, cfg)
    r1["poses"] = np.array([[np.concatenate([R.ravel(), t]) for R, t in tr["poses"]] for tr in r1["trace"]])
    compare(r1, r0, f"host loop vs itself {case}")
    for f in a + b:
        f.destroy()


def test_one_pose_window_is_mh_icp_align(world):
    capi = world.capi
    for k, reg4 in ((5, 0), (8, 1)):
        base = world.base(k, reg4)
        a, b = base.clone(), base.clone()
        (R0, t0), = scene(world, 1, 7)[0]
        wc = window_cfg(iters=8, prior_sigma_rot=0.1, prior_sigma_trans=0.0)
        ac = capi.make_align_config(max_iters=8, eps_rot=1e-6, eps_trans=1e-6, damping=1e-9, prior_sigma_rot=0.1, prior_sigma_trans=0.0)
        got, ref = capi.optimise_window([a], [(R0, t0)], wc, trace_poses=True), b.align(R0, t0, ac)
        assert got["iters"] == ref["iters"] and got["converged"] == ref["converged"]
        for it in range(got["iters"]):
            assert np.abs(got["poses"][it, 0, :9].reshape(3, 3) - ref["trace"][it]["R"]).max() <= 1e-12
            assert np.abs(got["poses"][it, 0, 9:] - ref["trace"][it]["t"]).max() <= 1e-12
        assert np.array_equal(a.state()[0], b.state()[0])
        a.destroy()
        b.destroy()


def flat(d):
    return np.concatenate([d["R"].ravel(), d["t"].ravel(), [d["iters"], d["converged"]], np.nan_to_num(d["poses"]).ravel()]
                          + [[r["f"], r["step_rot"], r["step_trans"], r["flags"], r["degenerate"]] for r in d["trace"]]
                          + [np.asarray(r["H_ss"]).ravel() for r in d["last"]] + [np.asarray(r["b_s"]) for r in d["first"]])


def test_check_every_and_async_do_not_change_the_result(world):
    capi = world.capi
    W = 5
    base = world.base(5)
    poses, Z, has_Z = scene(world, W, 8)
    outs, states = [], []
    for ce in (0, 1, 4, 7):
        fs = [base.clone() for _ in range(W)]
        outs.append(flat(capi.optimise_window(fs, poses, window_cfg(check_every=ce), has_Z=has_Z, Z=Z, trace_poses=True)))
        states.append([f.state() for f in fs])
        iters = int(outs[-1][12 * W])
        assert fs[0].linearize(*poses[0], G)["linearize_count"] == iters + 1  # the count advanced by the executed iterations
        for f in fs:
            f.destroy()
    fs = [base.clone() for _ in range(W)]
    cfg = window_cfg()
    call = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, wait=False)
    for op in (lambda: fs[1].reset(), lambda: fs[1].linearize(*poses[1], G), lambda: fs[1].align(*poses[1], capi.make_align_config()),
               lambda: fs[1].wait(), lambda: capi.linearize_batch(fs, [p[0] for p in poses], [p[1] for p in poses]),
               lambda: capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z)):
        with pytest.raises(capi.MhError):  # in flight: refused
            op()
    outs.append(flat(call.wait()))
    states.append([f.state() for f in fs])
    for f in fs:
        f.destroy()
    for o, s in zip(outs[1:], states[1:]):
        assert np.array_equal(o, outs[0])
        for fa, fb in zip(s, states[0]):
            for x, y in zip(fa, fb):
                assert np.array_equal(x, y, equal_nan=True)


def test_refusals_leave_the_handles_usable(world):
    capi = world.capi
    base = world.base(5)
    fs = [base.clone() for _ in range(3)]
    poses, Z, has_Z = scene(world, 3, 9)

    def refused(code, factors, p=poses, z=Z, hz=has_Z, **kw):
        with pytest.raises(capi.MhError) as e:
            capi.optimise_window(factors, p, window_cfg(**kw), has_Z=hz[:len(factors)], Z=None if z is None else z[:len(factors)])
        assert e.value.code == code, str(e.value)
        return str(e.value)

    for bad in (0, 65, -3):
        assert "iters" in refused(capi.MH_ERR_INVALID_ARG, fs, iters=bad)
    refused(capi.MH_ERR_INVALID_ARG, fs, damping=-1.0)
    refused(capi.MH_ERR_INVALID_ARG, fs, z=None)                      # has_Z set, no measurements
    assert "twice" in refused(capi.MH_ERR_INVALID_ARG, [fs[0], fs[1], fs[0]])
    many = [fs[0]] * 17
    assert "16" in refused(capi.MH_ERR_UNSUPPORTED, many, p=[poses[0]] * 17, z=[Z[0]] * 17, hz=[0] * 17)
    bin_f = world.base(5, binary=True)
    assert "unary" in refused(capi.MH_ERR_UNSUPPORTED, [fs[0], bin_f, fs[2]])
    fs[2].set_components(False)
    pending = fs[2].linearize_async(*poses[2], G)
    assert "in flight" in refused(capi.MH_ERR_INVALID_ARG, fs)
    fs[2].wait()
    assert pending.as_dict()["linearize_count"] == 1
    with pytest.raises(capi.MhError):
        world.ctx.check(world.ctx.L.mh_icp_window_wait(world.ctx.h))  # nothing in flight
    # nothing was enqueued, no count moved: the handles work, and the call itself does
    assert fs[0].linearize(*poses[0], G)["linearize_count"] == 1
    fresh = [base.clone() for _ in range(3)]
    a = capi.optimise_window(fs, poses, window_cfg(iters=3, eps_rot=0.0, eps_trans=0.0), has_Z=has_Z, Z=Z)
    assert a["iters"] == 3 and [r["linearize_count"] for r in a["last"]] == [4, 3, 4]
    for f in fs + fresh:
        f.destroy()
