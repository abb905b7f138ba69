"""Shared arithmetic of tests/test_icp_derivatives_cpu.py (oracle.ref_cpu.ICP) and tests/test_gpu_icp_derivatives.py
(capi.ICPFactor): the ICP factor held to finite differences of the cost it reports itself.  No oracle takes part.

The factor reports f = sum e^2 over its Valid points.  A point keeps its cached plane (mean, normal) until its query has moved
more than min_dist_in_voxel / 4 = 3.75 cm from the query of its last k-NN, so around the pose of a cold call, with Huber off,
f(T (+) xi) is a smooth function evaluated by the very code under test, and its derivatives fix what H and b must be:

    grad f = 2 b                               (e(xi) = e + J xi + ..., b = J^T e)
    1/2 hess f = H + sum_valid e_i d2e_i       (H = J^T J; the cost is not quadratic in rotation)

under the chart  retract(R, t, xi) = (R Exp(xi[:3]), t + R xi[3:])  — rotation first, the chart align_device.hpp and
window_device.hpp step in, GTSAM's Pose3::retract to first order.  In that chart only the rotation-rotation block has a second
term, `curvature()` below: THE ONLY FORMULA OF THE FACTOR THIS MODULE RESTATES (the Jacobian, the whitening, the adjoint of the
target block, the 4-DoF projector are all taken from derivatives of f or from exact identities between the factor's outputs).

Every evaluation of f asserts the preconditions of the identity (`cost_probe`): no point ran k-NN again, and no point changed
its status.  A violated precondition is an error of the test's inputs and fails the test; no evaluation is ever left out.

Works on any object with linearize(R, t, g_unit, R_tgt=, t_tgt=) -> dict and state() -> (status, mean, normal, ...).

Out of scope, on purpose (do not extend this harness there by reflex):
  * Huber-on gradient: the reported f is GTSAM's weighted error, h |w| per outlier, while 2 b is the gradient of the Huber loss
    2 h |w| - h^2; the two cannot be related from the totals alone.  (Huber on appears below only in exact identities.)
  * Photometric factor: its Jacobian uses the Sobel images, not the derivative of the bilinear interpolant, so grad f != 2 b by
    construction in the reference.
  * The window chains' between factors (window_between[_dense]): J_b = I, J_a = -Ad(between^-1) with the residual (Log R, t) is
    first order in the residual by design, as in replay.hpp; a check of it needs its own bar in |r|.
  * Radar: the restatement has its finite-difference test already (tests/test_radar_cpu.py).
"""
import numpy as np
import pytest

from mimosa_amd import synth

VALID = 8
D_GRAD = 1e-5   # rad and m alike.  Not above 1e-4: 1e-3 moves a point of the k = 8 case across the MaxError gate
D_HESS = 1e-4
BAR_GRAD = 1e-7   # central difference: O(d^2) truncation + cancellation in f; the oracle shows 6e-11 .. 3e-9
BAR_HESS = 1e-6   # second differences at 1e-4; the oracle shows 1e-10 .. 5e-9.  The smallest wrong term is the curvature, 7e-3
BAR_EXACT = 1e-12  # identities that hold to rounding
G_UNIT = np.array([0.02, -0.01, -1.0]) / np.linalg.norm([0.02, -0.01, -1.0])
UNARY_CASES = [(5, 19), (8, 27), (4, 7), (6, 1)]   # (k, neighbour mode); k = 3 is unusable: 3 neighbours are always coplanar
HESSIAN_CASES = [(5, 19), (8, 27)]
R_TGT = synth.so3_exp(np.array([0.2, 0.1, -0.3]))
T_TGT = np.array([0.5, -0.3, 0.2])
TILES = 65  # 65 x 1024 = 66 560 points: past 65 536, the 512-thread launch class


def config(k=5, **changes):
    return dict(synth.enwide_config(), num_corres_points=k, **changes)


def sigma_of(cfg):
    return float(np.float32(cfg["lidar_point_noise_std_dev"]))


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def retract(R, t, xi):
    xi = np.asarray(xi, float)
    return R @ synth.so3_exp(xi[:3]), t + R @ xi[3:]


def adjoint(R, t):
    """6 x 6 adjoint of the pose (R, t), (rotation, translation) order."""
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, :3] = skew(t) @ R
    A[3:, 3:] = R
    return A


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, float) - np.asarray(b, float)) / np.linalg.norm(np.asarray(b, float)))


def cost_probe(factor, base_status, R, t, xi, g_unit=G_UNIT, R_tgt=None, t_tgt=None, xi_tgt=None, case=""):
    """f at the retracted pose(s), with the preconditions of the identities asserted on this very evaluation."""
    Rs, ts = retract(R, t, xi)
    if R_tgt is not None:
        Rt, tt = retract(R_tgt, t_tgt, np.zeros(6) if xi_tgt is None else xi_tgt)
        out = factor.linearize(Rs, ts, g_unit, R_tgt=Rt, t_tgt=tt)
    else:
        out = factor.linearize(Rs, ts, g_unit)
    if int(out["n_knn"]) != 0:
        pytest.fail(f"{case}: test-input error: {int(out['n_knn'])} points re-associated at xi = {xi}, xi_tgt = {xi_tgt}")
    status = factor.state()[0]
    if not np.array_equal(status, base_status):
        pytest.fail(f"{case}: test-input error: {int((status != base_status).sum())} points changed status at xi = {xi}, xi_tgt = {xi_tgt}")
    return float(out["f"])


class Cost:
    """The cold call of a fresh factor at its base pose(s), then f as a function of the tangent (6 unary, 12 binary:
    source first, then target)."""

    def __init__(self, factor, R, t, R_tgt=None, t_tgt=None, g_unit=G_UNIT, case=""):
        self.factor, self.R, self.t, self.R_tgt, self.t_tgt, self.g, self.case = factor, R, t, R_tgt, t_tgt, g_unit, case
        self.dim = 6 if R_tgt is None else 12
        self.base = factor.linearize(R, t, g_unit) if R_tgt is None else factor.linearize(R, t, g_unit, R_tgt=R_tgt, t_tgt=t_tgt)
        self.state = tuple(np.array(a) for a in factor.state()[:3])
        self.f0 = float(self.base["f"])
        self.calls = 1
        n = len(self.state[0])
        assert int(self.base["n_knn"]) == n, (case, "the base call must be the cold one")
        # the identity must not hold vacuously
        assert int(self.base["status_hist"][VALID]) >= 300 * (n // 1024), (case, self.base["status_hist"])

    def __call__(self, xi):
        xi = np.asarray(xi, float)
        self.calls += 1
        return cost_probe(self.factor, self.state[0], self.R, self.t, xi[:6], self.g, self.R_tgt, self.t_tgt,
                          xi[6:] if self.dim == 12 else None, self.case)


def _e(n, i, d):
    v = np.zeros(n)
    v[i] = d
    return v


def fd_gradient(cost, delta=D_GRAD):
    n = cost.dim
    return np.array([(cost(_e(n, i, delta)) - cost(_e(n, i, -delta))) / (2 * delta) for i in range(n)])


def fd_half_hessian(cost, idx=range(6), delta=D_HESS):
    """1/2 hess f over the coordinates `idx`: diagonal and mixed central second differences."""
    idx, n = list(idx), cost.dim
    m = len(idx)
    Hf = np.zeros((m, m))
    for a, i in enumerate(idx):
        Hf[a, a] = (cost(_e(n, i, delta)) - 2 * cost.f0 + cost(_e(n, i, -delta))) / delta**2
        for b in range(a + 1, m):
            j = idx[b]
            pp, pm = _e(n, i, delta) + _e(n, j, delta), _e(n, i, delta) - _e(n, j, delta)
            Hf[a, b] = Hf[b, a] = (cost(pp) - cost(pm) - cost(-pm) + cost(-pp)) / (4 * delta**2)
    return 0.5 * Hf


def curvature(state, P, R, t, sigma):
    """C = sum_valid (e_i / sigma^2) d2e_i / d(rotation)^2, the one formula restated here.
    e_i = n_i . (m_i - (R Exp(w) p_i + t)) and d^2/ds^2 Exp(s d) p = d x (d x p) give, with ns_i = R^T n_i,
    d2e_i = (ns_i . p_i) I - 1/2 (ns_i p_i^T + p_i ns_i^T).  m_i, n_i and the status are the factor's own state()."""
    st, mean, nrm = state[:3]
    v = st == VALID
    p, ns = P[v], nrm[v] @ R
    e = np.einsum("ij,ij->i", nrm[v], mean[v] - (p @ R.T + t))
    w = e / sigma**2
    nsp = np.einsum("i,ij,ik->jk", w, ns, p)
    return np.sum(w * np.einsum("ij,ij->i", ns, p)) * np.eye(3) - 0.5 * (nsp + nsp.T)


class Report:
    """Prints every measured deviation as it comes, asserts them all at the end."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def at_most(self, name, value, bar):
        print(f"[icp-derivatives] {self.case}: {name} = {value:.3e}  (bar {bar:g})")
        self.rows.append((name, float(value), bar, float(value) <= bar))

    def more_than(self, name, value, bar):
        print(f"[icp-derivatives] {self.case}: {name} = {value:.3e}  (must exceed {bar:g})")
        self.rows.append((name, float(value), bar, float(value) > bar))

    def check(self):
        bad = [(n, v, b) for n, v, b, ok in self.rows if not ok]
        assert not bad, (self.case, bad)
        return {n: v for n, v, _, _ in self.rows}


def points_of(pts):
    return synth.points_xyz(pts).astype(np.float64)


def _blocks(rep, what, got, want, scale, bar):
    for name, (r, c) in (("rot-rot", (0, 0)), ("rot-trans", (0, 3)), ("trans-rot", (3, 0)), ("trans-trans", (3, 3))):
        d = np.linalg.norm(got[r:r + 3, c:c + 3] - want[r:r + 3, c:c + 3]) / scale
        rep.at_most(f"{what} {name}", d, bar)


# ---- the identities.  `make(k, mode, binary=False, pts=None, **config_changes)` returns a fresh factor of the small world ----

def check_unary_gradient(make, world, k, mode, pts=None, case=None):
    """1.  grad f = 2 b_s, Huber off."""
    rep = Report(case or f"unary gradient k={k} mode={mode}")
    cost = Cost(make(k, mode, pts=pts, use_huber=0), world["R"], world["t"], case=rep.case)
    g = fd_gradient(cost)
    rep.at_most("|g/2 - b_s| / |b_s|", rel(g / 2, cost.base["b_s"]), BAR_GRAD)
    assert cost.calls == 13
    return rep.check(), cost.base


def check_unary_hessian(make, world, k, mode):
    """2.  1/2 hess f - C = H_ss, Huber off, the full 6 x 6."""
    rep = Report(f"unary Hessian k={k} mode={mode}")
    cfg = config(k, use_huber=0)
    cost = Cost(make(k, mode, use_huber=0), world["R"], world["t"], case=rep.case)
    half = fd_half_hessian(cost)
    assert cost.calls == 73
    H = cost.base["H_ss"]
    scale = np.linalg.norm(H)
    corrected = half.copy()
    corrected[:3, :3] -= curvature(cost.state, points_of(world["pts"]), world["R"], world["t"], sigma_of(cfg))
    _blocks(rep, "1/2 hess f - C against H_ss,", corrected, H, scale, BAR_HESS)
    # the correction is exercised, and the test can tell the two apart
    rep.more_than("uncorrected 1/2 hess f against H_ss", np.linalg.norm(half - H) / scale, 1e-3)
    return rep.check()


def check_four_dof(make, world, k=5, mode=19):
    """3.  reg_4_dof: the same f, the factor projected with Pi = l l^T, l = R^T (-g_unit), on its rotation part."""
    rep = Report(f"4-DoF k={k} mode={mode}")
    cfg = config(k, use_huber=0, reg_4_dof=1)
    cost = Cost(make(k, mode, use_huber=0, reg_4_dof=1), world["R"], world["t"], case=rep.case)
    plain = make(k, mode, use_huber=0).linearize(world["R"], world["t"], G_UNIT)
    rep.at_most("|f(4-DoF) - f| / f", abs(cost.f0 - plain["f"]) / plain["f"], 0.0)
    l = world["R"].T @ (-G_UNIT)
    Pi = np.outer(l, l)
    P6 = np.eye(6)
    P6[:3, :3] = Pi
    g = fd_gradient(cost)
    rep.at_most("|P g/2 - b_s| / |b_s|", rel(P6 @ (g / 2), cost.base["b_s"]), BAR_GRAD)
    half = fd_half_hessian(cost)
    half[:3, :3] -= curvature(cost.state, points_of(world["pts"]), world["R"], world["t"], sigma_of(cfg))
    want = P6 @ half
    want[:, :3] = want[:, :3] @ Pi
    H = cost.base["H_ss"]
    _blocks(rep, "P (1/2 hess f - C) P against H_ss,", want, H, np.linalg.norm(H), BAR_HESS)
    rep.more_than("unprojected 1/2 hess f - C against H_ss", np.linalg.norm(half - H) / np.linalg.norm(H), 1e-3)  # a rank-1 projector: O(1)
    return rep.check()


def binary_pose(world):
    """source pose = target o base pose: the relative pose is the usual query pose"""
    return R_TGT @ world["R"], R_TGT @ world["t"] + T_TGT


def joint_hessian(out):
    return np.block([[out["H_ss"], out["H_st"]], [out["H_st"].T, out["H_tt"]]])


def check_binary_gradient(make, world, k=5, mode=19):
    """4.  grad f = 2 [b_s; b_t] over all twelve coordinates; in the six translation coordinates f is exactly quadratic."""
    rep = Report(f"binary gradient k={k} mode={mode}")
    Rs, ts = binary_pose(world)
    cost = Cost(make(k, mode, binary=True, use_huber=0), Rs, ts, R_TGT, T_TGT, case=rep.case)
    g = fd_gradient(cost)
    assert cost.calls == 25
    b = np.concatenate([cost.base["b_s"], cost.base["b_t"]])
    rep.at_most("|g/2 - [b_s; b_t]| / |b|", rel(g / 2, b), BAR_GRAD)
    rep.at_most("|g_s/2 - b_s| / |b_s|", rel(g[:6] / 2, b[:6]), BAR_GRAD)
    rep.at_most("|g_t/2 - b_t| / |b_t|", rel(g[6:] / 2, b[6:]), BAR_GRAD)
    idx = [3, 4, 5, 9, 10, 11]
    half = fd_half_hessian(cost, idx)
    rep.at_most("translation sub-block of 1/2 hess f against [[H_ss, H_st], [H_st^T, H_tt]]",
                rel(half, joint_hessian(cost.base)[np.ix_(idx, idx)]), BAR_HESS)
    return rep.check()


def check_binary_adjoint(make, world, k=5, mode=19):
    """5.  The target block is the source block carried by A = Ad(T_rel^-1); a unary factor at T_rel gives the source block.
    Huber on (plain enwide).  Exact to rounding."""
    rep = Report(f"binary adjoint k={k} mode={mode}")
    Rs, ts = binary_pose(world)
    out = make(k, mode, binary=True).linearize(Rs, ts, G_UNIT, R_tgt=R_TGT, t_tgt=T_TGT)
    assert int(out["status_hist"][VALID]) >= 300
    R_rel, t_rel = R_TGT.T @ Rs, R_TGT.T @ (ts - T_TGT)
    A = adjoint(R_rel.T, -R_rel.T @ t_rel)
    rep.at_most("|b_t + A^T b_s| / |b_t|", rel(-A.T @ out["b_s"], out["b_t"]), BAR_EXACT)
    rep.at_most("|H_st + H_ss A| / |H_st|", rel(-out["H_ss"] @ A, out["H_st"]), BAR_EXACT)
    rep.at_most("|H_tt - A^T H_ss A| / |H_tt|", rel(A.T @ out["H_ss"] @ A, out["H_tt"]), BAR_EXACT)
    un = make(k, mode).linearize(R_rel, t_rel, G_UNIT)
    assert np.array_equal(un["status_hist"], out["status_hist"])
    rep.at_most("unary at T_rel: H_ss", rel(un["H_ss"], out["H_ss"]), BAR_EXACT)
    rep.at_most("unary at T_rel: b_s", rel(un["b_s"], out["b_s"]), BAR_EXACT)
    rep.at_most("unary at T_rel: f", abs(un["f"] - out["f"]) / out["f"], BAR_EXACT)
    return rep.check()


def check_whitening_and_huber(make, world, k=5, mode=19):
    """6.  Powers of two commute with every rounding: all bit for bit."""
    R, t = world["R"], world["t"]
    a = make(k, mode, use_huber=0, lidar_point_noise_std_dev=0.0625).linearize(R, t, G_UNIT)
    b = make(k, mode, use_huber=0, lidar_point_noise_std_dev=0.03125).linearize(R, t, G_UNIT)
    assert int(a["status_hist"][VALID]) >= 300 and np.array_equal(a["status_hist"], b["status_hist"])
    for key in ("H_ss", "b_s", "f"):
        print(f"[icp-derivatives] whitening: max |{key}(sigma/2) - 4 {key}(sigma)| = {np.abs(np.asarray(b[key]) - 4 * np.asarray(a[key])).max():.3e}  (bit for bit)")
    for key in ("H_ss", "b_s", "f"):
        assert np.array_equal(np.asarray(b[key]), 4 * np.asarray(a[key])), key
    c = make(k, mode, use_huber=1, huber_threshold=1e6, lidar_point_noise_std_dev=0.0625).linearize(R, t, G_UNIT)
    for key in ("H_ss", "b_s", "f", "status_hist"):
        print(f"[icp-derivatives] Huber at 1e6 against off: max |d {key}| = {np.abs(np.asarray(c[key], float) - np.asarray(a[key], float)).max():.3e}  (bit for bit)")
    for key in ("H_ss", "b_s", "f", "status_hist"):
        assert np.array_equal(np.asarray(c[key]), np.asarray(a[key])), key
    on, off = make(k, mode).linearize(R, t, G_UNIT), make(k, mode, use_huber=0).linearize(R, t, G_UNIT)
    print(f"[icp-derivatives] plain enwide: f(Huber on) = {on['f']!r}, f(Huber off) = {off['f']!r}")
    assert np.array_equal(on["status_hist"], off["status_hist"]) and int(on["status_hist"][VALID]) >= 300
    assert on["f"] <= off["f"]


def check_tiled(make, world, k=5, mode=19, sums=True):
    """7.  The source cloud 65 times over: gradient identity, and (sums) 65 x the 1024-point factor."""
    pts = np.tile(world["pts"], TILES)
    assert len(pts) == 66560
    dev, big = check_unary_gradient(make, world, k, mode, pts=pts, case=f"tiled x{TILES} gradient k={k} mode={mode}")
    if sums:
        rep = Report(f"tiled x{TILES} k={k} mode={mode}")
        one = make(k, mode, use_huber=0).linearize(world["R"], world["t"], G_UNIT)
        assert np.array_equal(big["status_hist"], TILES * one["status_hist"])
        for key in ("H_ss", "b_s"):
            rep.at_most(f"|{key} - {TILES} {key}(1024)| / |.|", rel(big[key], TILES * one[key]), BAR_EXACT)
        rep.at_most(f"|f - {TILES} f(1024)| / f", abs(big["f"] - TILES * one["f"]) / (TILES * one["f"]), BAR_EXACT)
        dev.update(rep.check())
    return dev
