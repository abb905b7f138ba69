"""Priors and losses of the pose graph (rules 7 - 9 of "pose graph over all keyframes" in include/mimosa_hip.h) restated in numpy,
dense, on top of tests/pose_graph_ref.py: the prior's residual and Jacobian, the three losses, the weighted system solved by
numpy.linalg.solve and refined (solve_refined).  None of the device's structure (no near / far split, no sweeps, no refinement, no per-entry weighting: a
term's whole block is scaled by its weight).

priors: [(pose, Z_R, Z_t, info)]; losses: one (kind, param) per edge / per prior, or None for no loss on any of them."""
import numpy as np

from pose_graph_ref import edge_terms, hat, so3_exp, so3_log

NONE, HUBER, CAUCHY, DCS = 0, 1, 2, 3
MIN_WEIGHT = 1e-12


def local(ZR, Zt, R, t):
    """the pose (R, t) in the tangent of Z: [Log(Z.R^T R), Z.R^T (t - Z.t)]"""
    return np.concatenate([so3_log(ZR.T @ R), ZR.T @ (t - Zt)])


def jr_inv(phi):
    """the inverse right Jacobian of SO(3)"""
    phi = np.asarray(phi, np.float64)
    th2 = float(phi @ phi)
    th = np.sqrt(th2)
    K = hat(phi)
    c = 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0 if th < 1e-2 else 1.0 / th2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) + 0.5 * K + c * (K @ K)


def prior_terms(R, t, ZR, Zt):
    """d and M = blockdiag(Jr^-1(d_r), Exp(d_r))"""
    d = local(ZR, Zt, R, t)
    M = np.zeros((6, 6))
    M[:3, :3] = jr_inv(d[:3])
    M[3:, 3:] = so3_exp(d[:3])
    return d, M


def loss(kind, param, s):
    """(w, rho) of a term whose chi^2 is s"""
    if kind == NONE:
        return 1.0, s
    s = max(s, 0.0)
    if kind == HUBER:
        w, rho = (1.0, s) if s <= param * param else (param / np.sqrt(s), 2.0 * param * np.sqrt(s) - param * param)
    elif kind == CAUCHY:
        w, rho = 1.0 / (1.0 + s / param ** 2), param ** 2 * np.log(1.0 + s / param ** 2)
    elif kind == DCS:
        c = min(1.0, 2.0 * param / (param + s))
        w, rho = c * c, c * c * s + param * (1.0 - c) ** 2
    else:
        raise ValueError(kind)
    return max(w, MIN_WEIGHT), rho


def solve_refined(A, rhs):
    """numpy.linalg.solve with two refinement steps against a longdouble residual (the window chains' tests take four): the
    device refines its step twice against a residual in twice the working precision, so the reference has to carry the system's
    own digits too.  A 300-pose chain whose loops a loss has down-weighted has a condition number of 5e7; a step shrinks the
    error by cond * 1.1e-16 = 5e-9, two are more than enough."""
    x = np.linalg.solve(A, rhs)
    Al, rl = A.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(2):
        r = (rl - Al @ x.astype(np.longdouble)).astype(np.float64)
        x = x + np.linalg.solve(A, r)
    return x


def _loss_of(losses, k):
    return (NONE, 0.0) if losses is None else losses[k]


def system(R, t, fixed, edges, priors, edge_loss, prior_loss, damping):
    """A, -g, f (the sum of rho), (w per edge, w per prior) of one iteration, dense"""
    n = len(R)
    A = np.zeros((6 * n, 6 * n))
    g = np.zeros(6 * n)
    f = 0.0
    we, wp = np.ones(len(edges)), np.ones(len(priors))
    for e, (a, b, ZR, Zt, Om) in enumerate(edges):
        r, Ja = edge_terms(R[a], t[a], R[b], t[b], ZR, Zt)
        we[e], rho = loss(*_loss_of(edge_loss, e), float(r @ Om @ r))
        f += rho
        W = we[e] * Om
        sa, sb = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
        if not fixed[a]:
            A[sa, sa] += Ja.T @ W @ Ja
            g[sa] += Ja.T @ W @ r
        if not fixed[b]:
            A[sb, sb] += W
            g[sb] += W @ r
        if not fixed[a] and not fixed[b]:
            A[sb, sa] += W @ Ja
            A[sa, sb] += (W @ Ja).T
    for p, (i, ZR, Zt, Om) in enumerate(priors):
        d, M = prior_terms(R[i], t[i], ZR, Zt)
        wp[p], rho = loss(*_loss_of(prior_loss, p), float(d @ Om @ d))
        f += rho
        if not fixed[i]:
            s = slice(6 * i, 6 * i + 6)
            A[s, s] += wp[p] * (M.T @ Om @ M)
            g[s] += wp[p] * (M.T @ Om @ d)
    for i in range(n):
        s = slice(6 * i, 6 * i + 6)
        A[s, s] += np.eye(6) if fixed[i] else damping * np.eye(6)
    return A, -g, float(f), (we, wp)


def weights(R, t, edges, priors, edge_loss=None, prior_loss=None):
    """(w per edge, w per prior, f = the sum of rho) at the given poses"""
    R, t = np.asarray(R).reshape(-1, 3, 3), np.asarray(t).reshape(-1, 3)
    _, _, f, (we, wp) = system(R, t, [True] * len(R), edges, priors, edge_loss, prior_loss, 0.0)
    return we, wp, f


def prior_residuals(R, t, priors):
    """d (P x 6), chi2 (P)"""
    d = np.array([local(ZR, Zt, R[i], t[i]) for i, ZR, Zt, _ in priors]).reshape(-1, 6)
    return d, np.array([q @ p[3] @ q for q, p in zip(d, priors)])


def optimise(R, t, fixed, edges, priors, edge_loss, prior_loss, iters, damping=0.0, eps_rot=0.0, eps_trans=0.0):
    """dict(iters, converged, trace = [dict(f, step_rot, step_trans, R, t, w_edges, w_priors)], R, t): as pose_graph_ref.optimise"""
    R = [np.array(x, np.float64).reshape(3, 3) for x in R]
    t = [np.array(x, np.float64).reshape(3) for x in t]
    fixed = [bool(x) for x in fixed] if fixed is not None else [False] * len(R)
    trace, converged = [], False
    for _ in range(iters):
        A, rhs, f, (we, wp) = system(R, t, fixed, edges, priors, edge_loss, prior_loss, damping)
        xi = solve_refined(A, rhs).reshape(-1, 6)
        for i in range(len(R)):
            if fixed[i]:
                xi[i] = 0.0
                continue
            t[i] = t[i] + R[i] @ xi[i, 3:]
            R[i] = R[i] @ so3_exp(xi[i, :3])
        sr = float(np.linalg.norm(xi[:, :3], axis=1).max())
        st = float(np.linalg.norm(xi[:, 3:], axis=1).max())
        trace.append(dict(f=f, step_rot=sr, step_trans=st, R=np.array(R), t=np.array(t), w_edges=we, w_priors=wp))
        converged = sr < eps_rot and st < eps_trans
        if converged:
            break
    return dict(iters=len(trace), converged=converged, trace=trace, R=np.array(R), t=np.array(t))
