"""-m gpu: mh_icp_window_optimise_relin — the fixed-lag chain that evaluates a factor again only once its pose has moved past
ISAM2's relinearization thresholds from the pose of its last evaluation.

Scene: that of tests/test_gpu_icp_window.py (synth.small_world(): a map of ~5 k points, a 1 024-point scan cloned W times).

1.  Thresholds 0: result, traced poses and every factor's state bit-identical to mh_icp_window_optimise, sync and async,
    check_every 0 and 1, W = 1, 5, 16; the mask all ones for every executed iteration.
2.  The reference's thresholds (1.75e-2 rad, 5e-3 m) against a host-driven loop written here: mh_icp_linearize on the factors
    the rule selects, the kept model carried in numpy, the assembly and refined solve of tests/test_gpu_icp_window.py, the
    retraction.  Every pose within 1e-9 m and 1e-9 rad per iteration (the bar of that file, for its reason: the two loops feed
    K3 poses that differ in the last digits), the masks equal.  A decision closer than 1e-9 to its threshold could flip between
    the two; the host loop's smallest margin | |d[k]| - threshold | is asserted to stay above 1e-7 for every case.  Seeds: the
    scenarios that share a start function take 0, 1, 2 in the order listed; "drift" takes the first of 0, 1, 2, ... whose masks
    show a factor kept and evaluated again later (seed 0 shows none).  They were tried with this file's host loop over the CPU
    oracle's factor (oracle/ref_cpu.py) before any device run — margins there 6e-5 .. 2.7e-3 — and none was replaced for missing
    the pose bar.  Inputs: one pose 5 cm / 2 degrees off and the rest at their optimum; the newest pose 20 cm / 6 degrees off,
    whose neighbour is kept, carried on and evaluated again; a window of reg_4_dof factors; an empty factor; a chain that stops
    on eps.
3.  Thresholds of 1e9: only iteration 0 evaluates — counts advance by 1, the per-point state is that of one
    mh_icp_linearize_batch at the start poses, last == first.
4.  Bad arguments and the in-flight refusals through the new entry points; the handles stay usable.
5.  The reference's thresholds, blocking with check_every 0 and 1 and async + wait: the same bits in every field."""
import numpy as np
import pytest

import test_gpu_icp_window as base
from test_gpu_icp_window import world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G = base.G
RELIN = (1.75e-2, 5.0e-3)  # relinearize_threshold_rotation / _translation of the reference's configuration


# ---- the host loop ---------------------------------------------------------------------------------------------------------
def jrinv(phi):
    th2 = float(phi @ phi)
    th = np.sqrt(th2)
    K = base.hat(phi)
    c = 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0 if th < 1e-2 else 1.0 / th2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) + 0.5 * K + c * (K @ K)


def local(L, T):
    return np.concatenate([base.so3log(L[0].T @ T[0]), L[0].T @ (T[1] - L[1])])


def transported(H, b, f, d):
    if not np.any(d):
        return H, b, f
    M = np.zeros((6, 6))
    M[:3, :3], M[3:, 3:] = jrinv(d[:3]), base.expmap(d[:3])
    return M.T @ H @ M, M.T @ (b + H @ d), f + 2.0 * b @ d + d @ H @ d


def host_relin_loop(linearize, have, poses, Z, has_Z, cfg, relin):
    """linearize(i, R, t) -> dict with H_ss, b_s, f of factor i (components off).  Returns per iteration the poses, the mask and
    the smallest margin of a decision."""
    poses = [(np.array(R, float), np.array(t, float)) for R, t in poses]
    W = len(poses)
    kept = [None] * W  # (L, H, b, f)
    trace, masks, converged, margin = [], [], 0, np.inf
    zero = dict(H_ss=np.zeros((6, 6)), b_s=np.zeros(6), f=0.0)
    for it in range(cfg.iters):
        mask, res = 0, []
        for i in range(W):
            if not have[i]:
                res.append(zero)
                continue
            d = None if it == 0 else local(kept[i][0], poses[i])
            if it:
                thr = np.array([relin[0]] * 3 + [relin[1]] * 3)
                margin = min(margin, float(np.abs(np.abs(d) - thr).min()))
            if it == 0 or bool(np.any(np.abs(d[:3]) > relin[0]) or np.any(np.abs(d[3:]) > relin[1])):
                r = linearize(i, *poses[i])
                H, b, f = np.array(r["H_ss"], float).reshape(6, 6), np.array(r["b_s"], float), float(r["f"])
                kept[i] = (poses[i], H, b, f)
                mask |= 1 << i
            else:
                H, b, f = transported(kept[i][1], kept[i][2], kept[i][3], d)
            res.append(dict(H_ss=H, b_s=b, f=f))
        A, g, cost = base.host_system(res, poses, Z, has_Z, cfg)
        masks.append(mask)
        if not np.all(np.linalg.eigvalsh((A + A.T) / 2) > 0):
            break
        xi = base.solve_refined(A, -g).reshape(W, 6)
        poses = [(R @ base.expmap(x[:3]), t + R @ x[3:]) for (R, t), x in zip(poses, xi)]
        trace.append(dict(poses=poses, f=cost))
        if np.all(np.linalg.norm(xi[:, :3], axis=1) < cfg.eps_rot) and np.all(np.linalg.norm(xi[:, 3:], axis=1) < cfg.eps_trans):
            converged = 1
            break
    return dict(poses=poses, iters=len(trace), converged=converged, trace=trace, masks=masks, margin=margin)


# ---- scenarios: start poses around the window's optimum -------------------------------------------------------------------------
def offset(R, t, seed, rot_deg, trans):
    rng = np.random.default_rng(seed)
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    return R @ base.expmap(ax / np.linalg.norm(ax) * np.deg2rad(rot_deg)), t + d / np.linalg.norm(d) * trans


def one_off(opt, seed, who=2):
    """pose `who` 5 cm / 2 degrees off, the others at their optimum"""
    return [offset(R, t, seed, 2.0, 0.05) if i == who else (R, t) for i, (R, t) in enumerate(opt)]


def all_near(opt, seed):
    """every pose off by about a threshold (0.3 .. 1.2 degrees, 2 .. 9 mm), each its own direction: first steps on either side of
    the thresholds, and poses carried over them later by their neighbours' re-evaluations"""
    rng = np.random.default_rng(1000 + seed)
    return [offset(R, t, 100 * seed + i, rng.uniform(0.3, 1.2), rng.uniform(0.002, 0.009)) for i, (R, t) in enumerate(opt)]


def far_off(opt, seed, who=4):
    """the newest pose 20 cm / 6 degrees off: its factor needs several evaluations, and what they do to it reaches its neighbours
    through the between factors over more than one step"""
    return [offset(R, t, seed, 6.0, 0.2) if i == who else (R, t) for i, (R, t) in enumerate(opt)]


# name -> (start poses, seed, reg_4_dof, empty_at, tight prior, config)
FIXED = dict(eps_rot=0.0, eps_trans=0.0)
SCENARIOS = {
    "one_off": (one_off, 0, 0, None, True, dict(iters=6, **FIXED)),
    "drift": (far_off, 1, 0, None, True, dict(iters=8, **FIXED)),  # a pose kept, carried on by the others' steps, evaluated again
    "reg_4_dof": (all_near, 0, 1, None, True, dict(iters=6, **FIXED)),
    "empty": (one_off, 1, 0, 3, True, dict(iters=6, **FIXED)),
    # (under the tight prior, which is centred on the step's own pose, the oldest pose creeps for ever: the loose one converges)
    "eps": (one_off, 2, 0, None, False, dict(iters=12, eps_rot=1e-6, eps_trans=1e-6)),
}
W_REF = 5


def evaluated_later_again(masks, W):
    """a factor kept in some iteration and evaluated in a later one"""
    return any(not (masks[a] >> i) & 1 and (masks[b] >> i) & 1 for i in range(W) for a in range(1, len(masks)) for b in range(a + 1, len(masks)))


@pytest.fixture(scope="module")
def optima(world):
    """per reg_4_dof the optimum of a window of W_REF clones, found once with the plain chain"""
    capi = world.capi
    out = {}
    for reg4 in (0, 1):
        fs = [world.base(5, reg4).clone() for _ in range(W_REF)]
        Z = [(np.eye(3), np.zeros(3)) for _ in range(W_REF)]
        r = capi.optimise_window(fs, [world.truth()] * W_REF, base.window_cfg(True, iters=12, eps_rot=0.0, eps_trans=0.0), has_Z=[0] + [1] * (W_REF - 1), Z=Z)
        out[reg4] = [(r["R"][i].copy(), r["t"][i].copy()) for i in range(W_REF)]
        for f in fs:
            f.destroy()
    return out


def rows(d):
    return np.array([[np.concatenate([R.ravel(), t]) for R, t in tr["poses"]] for tr in d["trace"]])


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_reference_thresholds_against_the_host_loop(world, optima, name):
    capi = world.capi
    start, seed, reg4, empty_at, tight, kw = SCENARIOS[name]
    mk = lambda i: (world.base(5, reg4, empty=True) if i == empty_at else world.base(5, reg4)).clone()  # noqa: E731
    a, b = [mk(i) for i in range(W_REF)], [mk(i) for i in range(W_REF)]
    for f in b:
        f.set_components(False)
    poses = start(optima[reg4], seed)
    Z, has_Z = [(np.eye(3), np.zeros(3)) for _ in range(W_REF)], [0] + [1] * (W_REF - 1)
    cfg = base.window_cfg(tight, **kw)
    count0 = 0
    got = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=RELIN)
    ref = host_relin_loop(lambda i, R, t: b[i].linearize(R, t, G), [i != empty_at for i in range(W_REF)], poses, Z, has_Z, cfg, RELIN)
    print(name, "masks", [bin(m) for m in ref["masks"]], "device", [bin(int(m)) for m in got["evaluated"]], "margin %.3e" % ref["margin"],
          "iters", got["iters"], ref["iters"], "converged", got["converged"], ref["converged"])
    assert ref["margin"] > 1e-7
    base.compare(got, ref, name)
    assert [int(m) for m in got["evaluated"]] == ref["masks"][:ref["iters"]]
    masks = ref["masks"]
    # what the scenario is for
    if name == "one_off":
        assert len(set(masks)) > 1 and any(bin(m).count("1") not in (0, W_REF) for m in masks)  # differ across factors and iterations
    if name == "drift":
        assert evaluated_later_again(masks, W_REF)
    if name == "empty":
        assert all(not (m >> empty_at) & 1 for m in masks)
    if name == "eps":
        assert got["converged"] == 1 and got["iters"] < cfg.iters
    # books: counts by the evaluations, first / last the factor's first and last evaluation, the state its last evaluation's
    for i in range(W_REF):
        n_eval = sum((m >> i) & 1 for m in masks[:ref["iters"]])
        want = count0 + (got["iters"] if i == empty_at else n_eval)
        assert got["last"][i]["linearize_count"] == want and got["first"][i]["linearize_count"] == 1
        assert np.array_equal(a[i].state()[0], b[i].state()[0]), (name, i)
        if i != empty_at:
            assert a[i].linearize(*poses[i], G)["linearize_count"] == n_eval + 1
    for f in a + b:
        f.destroy()


# ---- thresholds 0: the existing chain, bit for bit ---------------------------------------------------------------------------
def flat(d):
    return np.concatenate([base.flat(d)] + [np.asarray(r[k], float).ravel() for r in d["first"] + d["last"]
                                            for k in ("H_ss", "b_s", "f", "loc_rot_final", "loc_trans_final", "degen_rot", "degen_trans") + base.COUNTERS])


@pytest.mark.parametrize("W", [1, 5, 16])
def test_thresholds_zero_are_the_existing_chain_bit_for_bit(world, W):
    capi = world.capi
    base_f = world.base(5)
    poses, Z, has_Z = base.scene(world, W, 11)
    for ce in (0, 1):
        cfg = base.window_cfg(W == 5, check_every=ce)
        fs = [base_f.clone() for _ in range(W)]
        ref = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True)
        ref_state = [f.state() for f in fs]
        for f in fs:
            f.destroy()
        for wait in (True, False):
            fs = [base_f.clone() for _ in range(W)]
            got = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=(0.0, 0.0), wait=wait)
            if not wait:
                got = got.wait()
            assert np.array_equal(flat(got), flat(ref), equal_nan=True), (W, ce, wait)
            assert got["iters"] >= 2 and list(got["evaluated"]) == [(1 << W) - 1] * got["iters"]
            for f, s in zip(fs, ref_state):
                for x, y in zip(f.state(), s):
                    assert np.array_equal(x, y, equal_nan=True)
            for f in fs:
                f.destroy()


def test_thresholds_zero_with_an_empty_factor(world):
    capi = world.capi
    W = 4
    mk = lambda i: (world.base(5, empty=True) if i == 2 else world.base(5)).clone()  # noqa: E731
    poses, Z, has_Z = base.scene(world, W, 5)
    cfg = base.window_cfg()
    a, b = [mk(i) for i in range(W)], [mk(i) for i in range(W)]
    ref = capi.optimise_window(a, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True)
    got = capi.optimise_window(b, poses, cfg, has_Z=has_Z, Z=Z, trace_poses=True, relin=(0.0, 0.0))
    assert np.array_equal(flat(got), flat(ref), equal_nan=True)
    assert list(got["evaluated"]) == [0b1011] * got["iters"]
    for f in a + b:
        f.destroy()


# ---- how the host drives the chain does not show in the result ------------------------------------------------------------------
def same_bits(a, b, where="result"):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same_bits(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{where}[{i}]")
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), where


def test_check_every_and_async_do_not_change_the_relin_result(world, optima):
    """The reference's thresholds on the smallest scenario (one_off), W = 3 with an empty factor, 6 iterations: blocking with
    check_every 0 and 1 and _async + mh_icp_window_wait give the same bits in every field — poses, trace, first, last, masks —
    and leave every factor's linearize_count the same."""
    capi = world.capi
    W, empty_at = 3, 1
    mk = lambda i: (world.base(5, empty=True) if i == empty_at else world.base(5)).clone()  # noqa: E731
    poses = one_off(optima[0][:W], 0, who=2)
    Z, has_Z = [(np.eye(3), np.zeros(3)) for _ in range(W)], [0] + [1] * (W - 1)
    runs, counts = [], []
    for ce, wait in ((0, True), (1, True), (0, False)):
        fs = [mk(i) for i in range(W)]
        got = capi.optimise_window(fs, poses, base.window_cfg(True, iters=6, check_every=ce, **FIXED), has_Z=has_Z, Z=Z, trace_poses=True, relin=RELIN, wait=wait)
        runs.append(got if wait else got.wait())
        counts.append([f.linearize(*poses[i], G)["linearize_count"] - 1 for i, f in enumerate(fs)])  # (the next call's number, less one)
        for f in fs:
            f.destroy()
    print("masks", [bin(int(m)) for m in runs[0]["evaluated"]], "counts", counts[0])
    assert runs[0]["iters"] == 6 and len(runs[0]["evaluated"]) == 6 and runs[0]["poses"].shape == (6, W, 12)
    assert all(not (int(m) >> empty_at) & 1 for m in runs[0]["evaluated"])
    for r, c in zip(runs[1:], counts[1:]):
        same_bits(r, runs[0])
        assert c == counts[0]


# ---- thresholds nothing reaches ------------------------------------------------------------------------------------------------
def test_huge_thresholds_evaluate_iteration_zero_only(world):
    capi = world.capi
    W = 5
    base_f = world.base(5)
    a, b = [base_f.clone() for _ in range(W)], [base_f.clone() for _ in range(W)]
    poses, Z, has_Z = base.scene(world, W, 12)
    got = capi.optimise_window(a, poses, base.window_cfg(True, iters=6, eps_rot=0.0, eps_trans=0.0), has_Z=has_Z, Z=Z, relin=(1e9, 1e9))
    assert got["iters"] == 6 and list(got["evaluated"]) == [(1 << W) - 1] + [0] * 5
    for f in b:
        f.set_components(False)
    res = capi.linearize_batch(b, [p[0] for p in poses], [p[1] for p in poses])
    for i in range(W):
        for x, y in zip(a[i].state(), b[i].state()):
            assert np.array_equal(x, y, equal_nan=True)
        for key in ("H_ss", "b_s", "f") + base.COUNTERS:
            assert np.array_equal(np.asarray(got["first"][i][key]), np.asarray(res[i][key]), equal_nan=True), (i, key)
            assert np.array_equal(np.asarray(got["last"][i][key]), np.asarray(got["first"][i][key]), equal_nan=True), (i, key)
        assert got["last"][i]["linearize_count"] == 1
        assert a[i].linearize(*poses[i], G)["linearize_count"] == 2
    for f in a + b:
        f.destroy()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handles_usable(world):
    capi = world.capi
    base_f = world.base(5)
    fs = [base_f.clone() for _ in range(3)]
    poses, Z, has_Z = base.scene(world, 3, 9)

    def refused(code, factors, p=poses, z=Z, hz=has_Z, relin=RELIN, **kw):
        with pytest.raises(capi.MhError) as e:
            capi.optimise_window(factors, p, base.window_cfg(**kw), has_Z=hz[:len(factors)], Z=None if z is None else z[:len(factors)], relin=relin)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    for bad in ((-1e-3, 5e-3), (1e-2, -1.0), (float("nan"), 5e-3), (1e-2, float("inf")), (float("-inf"), 0.0)):
        assert "relin" in refused(capi.MH_ERR_INVALID_ARG, fs, relin=bad)
    for bad in (0, 65, -3):
        assert "iters" in refused(capi.MH_ERR_INVALID_ARG, fs, iters=bad)
    refused(capi.MH_ERR_INVALID_ARG, fs, damping=-1.0)
    refused(capi.MH_ERR_INVALID_ARG, fs, z=None)
    assert "twice" in refused(capi.MH_ERR_INVALID_ARG, [fs[0], fs[1], fs[0]])
    assert "16" in refused(capi.MH_ERR_UNSUPPORTED, [fs[0]] * 17, p=[poses[0]] * 17, z=[Z[0]] * 17, hz=[0] * 17)
    assert "unary" in refused(capi.MH_ERR_UNSUPPORTED, [fs[0], world.base(5, binary=True), fs[2]])
    fs[2].set_components(False)
    pending = fs[2].linearize_async(*poses[2], G)
    assert "in flight" in refused(capi.MH_ERR_INVALID_ARG, fs)
    fs[2].wait()
    assert pending.as_dict()["linearize_count"] == 1
    # in flight through the new entry point: everything else on its factors is refused, mh_icp_window_wait collects it
    cfg = base.window_cfg(iters=3, eps_rot=0.0, eps_trans=0.0)
    call = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, wait=False, relin=RELIN)
    for op in (lambda: fs[1].reset(), lambda: fs[1].linearize(*poses[1], G), lambda: fs[1].align(*poses[1], capi.make_align_config()),
               lambda: fs[1].wait(), lambda: capi.linearize_batch(fs, [p[0] for p in poses], [p[1] for p in poses]),
               lambda: capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z), lambda: capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, relin=RELIN)):
        with pytest.raises(capi.MhError):
            op()
    r = call.wait()
    assert r["iters"] == 3 and int(r["evaluated"][0]) == 0b111
    with pytest.raises(capi.MhError):
        world.ctx.check(world.ctx.L.mh_icp_window_wait(world.ctx.h))  # nothing in flight
    n2 = sum((int(m) >> 2) & 1 for m in r["evaluated"])
    assert fs[2].linearize(*poses[2], G)["linearize_count"] == 1 + n2 + 1
    for f in fs:
        f.destroy()
