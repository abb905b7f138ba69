"""A numpy restatement of one Gauss-Newton iteration of the fixed-lag window with edges (between factors on any pair of poses,
each with a dense information matrix), written from the contract in include/mimosa_hip.h and not from
mimosa_amd/csrc/window_device.hpp: a dense 6W x 6W assembly and numpy.linalg.solve, no profile, no block sweep.  Exp, Log,
the adjoint and the carried linear factors are those of tests/window_lin_ref.py.  Shared by tests/test_icp_window_edges_cpu.py
and tests/test_gpu_icp_window_edges.py.

An edge is a dict {"a": i, "b": j, "Z": (R, t) the measured T_a^-1 T_b, "info": 6 x 6}."""
import numpy as np

import window_lin_ref as lin_ref


def edge_terms(Ta, Tb, Z, Om):
    """r, J_a and what the edge adds: J_a^T Om J_a, Om J_a, J_a^T Om r, Om r, r^T Om r  (J_b = I)"""
    (Ra, ta), (Rb, tb) = Ta, Tb
    abR, abt = Ra.T @ Rb, Ra.T @ (tb - ta)
    r = np.concatenate([lin_ref.log_so3(Z[0].T @ abR), Z[0].T @ (abt - Z[1])])
    Ja = -lin_ref.adjoint(abR.T, -abR.T @ abt)  # -Ad(T_ab^-1)
    Om = np.asarray(Om, float).reshape(6, 6)
    return r, Ja, Ja.T @ Om @ Ja, Om @ Ja, Ja.T @ Om @ r, Om @ r, float(r @ Om @ r)


def system(poses, icp, has_Z, Z, Wb, prior, damping, linear, edges):
    """the dense system A, the gradient g (before the sign flip) and the cost at `poses`"""
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
        H, b, f = lin_ref.transport(np.asarray(l["H"], float).reshape(6, 6), np.asarray(l["b"], float), float(l["f"]), l["at"], poses[i])
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += H
        g[6 * i:6 * i + 6] += b
        cost += f
    ties = [dict(a=i - 1, b=i, Z=Z[i], info=np.diag(Wb)) for i in range(1, W) if has_Z[i]]
    for e in ties + list(edges):
        _, _, Baa, Eba, ga, gb, c = edge_terms(poses[e["a"]], poses[e["b"]], e["Z"], e["info"])
        a, b = slice(6 * e["a"], 6 * e["a"] + 6), slice(6 * e["b"], 6 * e["b"] + 6)
        A[a, a] += Baa
        A[b, a] += Eba
        A[a, b] += Eba.T
        A[b, b] += np.asarray(e["info"], float).reshape(6, 6)
        g[a] += ga
        g[b] += gb
        cost += c
    A[:6, :6] += np.diag(prior)
    A += damping * np.eye(6 * W)
    return A, g, cost


def iteration(poses, icp, has_Z, Z, Wb, prior, damping, linear, edges, solve=np.linalg.solve):
    """as window_lin_ref.iteration, with the edges.  Returns the new poses, xi (W, 6) and the cost at `poses`."""
    A, g, cost = system(poses, icp, has_Z, Z, Wb, prior, damping, linear, edges)
    xi = solve(A, -g).reshape(len(poses), 6)
    return [lin_ref.retract(poses[i], xi[i]) for i in range(len(poses))], xi, cost


def random_info(rng, lo=1e2, hi=1e6):
    """a dense symmetric positive definite information matrix with eigenvalues between lo and hi (both attained)"""
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    lam = np.logspace(np.log10(lo), np.log10(hi), 6)[rng.permutation(6)]
    Om = (Q * lam) @ Q.T
    return (Om + Om.T) / 2.0


def random_edge(rng, a, b, poses, rot=0.02, trans=0.03, info=None):
    """an edge of the poses a < b whose measurement lies a few degrees / centimetres off the poses' own relative pose"""
    (Ra, ta), (Rb, tb) = poses[a], poses[b]
    nR, nt = lin_ref.exp_so3(rng.standard_normal(3) * rot), rng.standard_normal(3) * trans
    return dict(a=int(a), b=int(b), Z=(Ra.T @ Rb @ nR, Ra.T @ (tb - ta) + nt), info=random_info(rng) if info is None else np.asarray(info, float))
