"""The pose graph of mh_pose_graph_* restated in numpy: the rule of include/mimosa_hip.h ("pose graph over all keyframes") with the
system assembled dense and solved by numpy.linalg.solve — the same residual, Jacobians, fixed-pose rule, damping, retraction and
stop test as mimosa_amd/csrc/pose_graph_device.hpp, none of its structure (no near / far split, no block sweeps, no refinement)."""
import numpy as np


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(w):
    w = np.asarray(w, np.float64)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    K = hat(w)
    if th < 1e-10:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    return np.eye(3) + A * K + B * (K @ K)


def so3_log(R):
    c = min(1.0, max(-1.0, (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) / 2.0))
    th = np.arccos(c)
    s = 0.5 if th < 1e-9 else th / (2.0 * np.sin(th))
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * s


def adjoint(R, t):
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[3:, 3:] = R
    Ad[3:, :3] = hat(t) @ R
    return Ad


def edge_terms(Ra, ta, Rb, tb, ZR, Zt):
    """the residual [Log(Z.R^T R_ab), Z.R^T (t_ab - Z.t)] and J_a = -Ad(T_ab^-1)  (J_b = I)"""
    abR = Ra.T @ Rb
    abt = Ra.T @ (tb - ta)
    r = np.concatenate([so3_log(ZR.T @ abR), ZR.T @ (abt - Zt)])
    return r, -adjoint(abR.T, -(abR.T @ abt))


def residuals(R, t, edges):
    """r (E x 6), chi2 (E), f = sum chi2"""
    r = np.zeros((len(edges), 6))
    chi2 = np.zeros(len(edges))
    for e, (a, b, ZR, Zt, Om) in enumerate(edges):
        r[e], _ = edge_terms(R[a], t[a], R[b], t[b], ZR, Zt)
        chi2[e] = r[e] @ Om @ r[e]
    return r, chi2, float(chi2.sum())


def system(R, t, fixed, edges, damping):
    """A, -g, f of one iteration, dense"""
    n = len(R)
    A = np.zeros((6 * n, 6 * n))
    g = np.zeros(6 * n)
    f = 0.0
    for a, b, ZR, Zt, Om in edges:
        r, Ja = edge_terms(R[a], t[a], R[b], t[b], ZR, Zt)
        f += r @ Om @ r
        sa, sb = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
        if not fixed[a]:
            A[sa, sa] += Ja.T @ Om @ Ja
            g[sa] += Ja.T @ Om @ r
        if not fixed[b]:
            A[sb, sb] += Om
            g[sb] += Om @ r
        if not fixed[a] and not fixed[b]:
            A[sb, sa] += Om @ Ja
            A[sa, sb] += (Om @ Ja).T
    for i in range(n):
        s = slice(6 * i, 6 * i + 6)
        A[s, s] += np.eye(6) if fixed[i] else damping * np.eye(6)
    return A, -g, float(f)


def optimise(R, t, fixed, edges, iters, damping=0.0, eps_rot=0.0, eps_trans=0.0, solve=np.linalg.solve):
    """dict(iters, converged, trace = [dict(f, step_rot, step_trans, R, t)], R, t): Gauss-Newton as the device chain runs it"""
    R = [np.array(x, np.float64).reshape(3, 3) for x in R]
    t = [np.array(x, np.float64).reshape(3) for x in t]
    fixed = [bool(x) for x in fixed] if fixed is not None else [False] * len(R)
    trace, converged = [], False
    for _ in range(iters):
        A, rhs, f = system(R, t, fixed, edges, damping)
        xi = np.asarray(solve(A, rhs)).reshape(-1, 6)
        for i in range(len(R)):
            if fixed[i]:
                xi[i] = 0.0
                continue
            t[i] = t[i] + R[i] @ xi[i, 3:]
            R[i] = R[i] @ so3_exp(xi[i, :3])
        sr = float(np.linalg.norm(xi[:, :3], axis=1).max())
        st = float(np.linalg.norm(xi[:, 3:], axis=1).max())
        trace.append(dict(f=f, step_rot=sr, step_trans=st, R=np.array(R), t=np.array(t)))
        converged = sr < eps_rot and st < eps_trans
        if converged:
            break
    return dict(iters=len(trace), converged=converged, trace=trace, R=np.array(R), t=np.array(t))


def rot_angle(Ra, Rb):
    """the angle of Ra^T Rb, rad (accurate for small angles: from the skew part)"""
    D = Ra.T @ Rb
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.arctan2(s, (np.trace(D) - 1.0) / 2.0))


def pose_error(R, t, R2, t2):
    """largest translation distance (m) and rotation angle (rad) between two sets of poses"""
    R, t, R2, t2 = np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3), np.asarray(R2).reshape(-1, 3, 3), np.asarray(t2).reshape(-1, 3)
    return float(np.linalg.norm(t - t2, axis=1).max()), max(rot_angle(a, b) for a, b in zip(R, R2))
