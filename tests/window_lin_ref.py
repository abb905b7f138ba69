"""A numpy restatement of one Gauss-Newton iteration of the fixed-lag window with linear (host-linearized Hessian) factors,
written from the contract in include/mimosa_hip.h and not from mimosa_amd/csrc/window_device.hpp: its own Exp, Log and
Jr^-1 (closed forms, series near zero), a dense 6W x 6W assembly and numpy.linalg.solve.  Shared by
tests/test_icp_window_lin_cpu.py and tests/test_gpu_icp_window_lin.py.

Conventions: a pose is (R, t); the retraction is R <- R Exp(xi_r), t <- t + R xi_t; a factor on one pose is the model
f + 2 b^T x + x^T H x in that pose's tangent, so it adds H to the system, b to the gradient and f to the cost."""
import numpy as np


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, float)
    th = float(np.sqrt(w @ w))
    K = skew(w)
    if th < 1e-6:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def log_so3(R):
    """through atan2 of the antisymmetric part's norm and the trace (angles far below pi, as a window's offsets are)"""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0  # sin(th) * axis
    s, c = float(np.sqrt(v @ v)), (np.trace(R) - 1.0) / 2.0
    th = np.arctan2(s, c)
    if s < 1e-9:
        return v * (1.0 + s * s / 6.0)
    return v * (th / s)


def jr_inv(phi):
    phi = np.asarray(phi, float)
    th = float(np.sqrt(phi @ phi))
    K = skew(phi)
    if th < 1e-3:
        c = 1.0 / 12.0 + th * th / 720.0
    else:
        c = 1.0 / (th * th) - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) + 0.5 * K + c * (K @ K)


def retract(T, xi):
    R, t = T
    return R @ exp_so3(xi[:3]), t + R @ xi[3:]


def local(L, T):
    return np.concatenate([log_so3(L[0].T @ T[0]), L[0].T @ (T[1] - L[1])])


def transport(H, b, f, L, T):
    """the model (H, b, f) around L as seen from T: a step xi at T is x = d + M xi to first order"""
    d = local(L, T)
    M = np.zeros((6, 6))
    M[:3, :3] = jr_inv(d[:3])
    M[3:, 3:] = exp_so3(d[:3])
    return M.T @ H @ M, M.T @ (b + H @ d), f + 2.0 * b @ d + d @ H @ d


def adjoint(R, t):
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = skew(t) @ R
    return A


def iteration(poses, icp, has_Z, Z, Wb, prior, damping, linear, solve=np.linalg.solve):
    """poses: [(R, t)] * W; icp: per pose (H, b, f) at the current pose, or None; Z[i]: the measured T_{i-1}^-1 T_i where has_Z[i];
    linear: dicts pose / at / H / b / f; solve: numpy.linalg.solve, or a caller's refinement around it.  Returns the new poses, xi (W, 6) and the cost at `poses`."""
    W = len(poses)
    A, g, cost = np.zeros((6 * W, 6 * W)), np.zeros(6 * W), 0.0
    for i in range(W):
        if icp[i] is not None:
            H, b, f = icp[i]
            A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += np.asarray(H, float).reshape(6, 6)
            g[6 * i:6 * i + 6] += b
            cost += f
    for l in linear:
        i = l["pose"]
        H, b, f = transport(np.asarray(l["H"], float).reshape(6, 6), np.asarray(l["b"], float), float(l["f"]), l["at"], poses[i])
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += H
        g[6 * i:6 * i + 6] += b
        cost += f
    Wm = np.diag(Wb)
    for i in range(1, W):
        if not has_Z[i]:
            continue
        (Ra, ta), (Rb, tb) = poses[i - 1], poses[i]
        abR, abt = Ra.T @ Rb, Ra.T @ (tb - ta)
        r = np.concatenate([log_so3(Z[i][0].T @ abR), Z[i][0].T @ (abt - Z[i][1])])
        Ja = -adjoint(abR.T, -abR.T @ abt)
        a, b = slice(6 * i - 6, 6 * i), slice(6 * i, 6 * i + 6)
        A[a, a] += Ja.T @ Wm @ Ja
        A[a, b] += Ja.T @ Wm
        A[b, a] += Wm @ Ja
        A[b, b] += Wm
        g[a] += Ja.T @ Wm @ r
        g[b] += Wm @ r
        cost += r @ Wm @ r
    A[:6, :6] += np.diag(prior)
    A += damping * np.eye(6 * W)
    xi = solve(A, -g).reshape(W, 6)
    return [retract(poses[i], xi[i]) for i in range(W)], xi, cost


def pose_error(Ta, Tb):
    """(rad, m) between two poses"""
    return float(np.linalg.norm(log_so3(Ta[0].T @ Tb[0]))), float(np.linalg.norm(Ta[1] - Tb[1]))


def random_spd(rng, scale, cond=1e2):
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    lam = scale * np.logspace(0, np.log10(cond), 6)[rng.permutation(6)]
    H = (Q * lam) @ Q.T
    return (H + H.T) / 2.0


def random_linear(rng, pose, T, rot=3e-2, trans=2e-2, scale=1e3):
    """a linear factor on `pose`, linearized up to rot rad / trans m away from T, whose minimum lies a few mrad / mm from L"""
    ax = rng.standard_normal(3)
    d = np.concatenate([ax / np.linalg.norm(ax) * rng.uniform(0.2, 1.0) * rot, rng.uniform(-1.0, 1.0, 3) / np.sqrt(3.0) * trans])
    L = retract(T, d)
    H = random_spd(rng, scale * 10.0 ** rng.uniform(-1, 1))
    b = H @ (rng.standard_normal(6) * 5e-3)
    return dict(pose=int(pose), at=L, H=H, b=b, f=float(rng.uniform(0.5, 5.0)))
