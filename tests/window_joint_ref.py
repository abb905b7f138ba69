"""A numpy restatement of the joint factor of mh_icp_window_optimise_joint and of mh_icp_window_marginalise_joint, written from
the contract in include/mimosa_hip.h and not from mimosa_amd/csrc/window_device.hpp: dense matrices over the whole window (or
over pose 0 and its separator) and numpy.linalg.solve — no blocks, no profile, no mirrored triangle.  The members' offsets and
Jacobians come from tests/window_lin_ref.py's transport, member by member; the between terms are tests/window_edge_ref.py's.
Shared by tests/test_icp_window_joint_cpu.py, tests/test_gpu_icp_window_joint.py and the replay test.

A joint factor is a dict {"poses": ascending indices, "at": [(R, t)] per member, "H": 6n x 6n, "b": 6n, "f": float}: the model
f + 2 b^T x + x^T H x, x the stacked tangents of the members at their "at" (rotation first, R <- R Exp(x_r), t <- t + R x_t)."""
import numpy as np

import window_edge_ref as edge_ref
import window_lin_ref as lin_ref


def member_jacobian(L, T):
    """d and M of one member: a step xi at T is x = d + M xi in L's tangent.  M is read off window_lin_ref.transport, which
    carries a gradient e_k to M^T e_k."""
    Z = np.zeros((6, 6))
    Mt = np.column_stack([lin_ref.transport(Z, np.eye(6)[k], 0.0, L, T)[1] for k in range(6)])
    return lin_ref.local(L, T), Mt.T


def carry(joint, poses):
    """the joint factor as seen from the current poses of its members: (H', b', f')"""
    n = len(joint["poses"])
    H, b, f = np.asarray(joint["H"], float).reshape(6 * n, 6 * n), np.asarray(joint["b"], float).reshape(6 * n), float(joint["f"])
    d, M = np.zeros(6 * n), np.zeros((6 * n, 6 * n))
    for m, i in enumerate(joint["poses"]):
        d[6 * m:6 * m + 6], M[6 * m:6 * m + 6, 6 * m:6 * m + 6] = member_jacobian(joint["at"][m], poses[i])
    return M.T @ H @ M, M.T @ (b + H @ d), f + 2.0 * b @ d + d @ H @ d


def scatter(A, g, joint, carried, slot_of):
    """add the carried factor into a dense system whose 6 x 6 slot of pose i is slot_of(i)"""
    H, b, _ = carried
    for m, i in enumerate(joint["poses"]):
        si = slot_of(i)
        g[6 * si:6 * si + 6] += b[6 * m:6 * m + 6]
        for k, j in enumerate(joint["poses"]):
            sj = slot_of(j)
            A[6 * si:6 * si + 6, 6 * sj:6 * sj + 6] += H[6 * m:6 * m + 6, 6 * k:6 * k + 6]


def system(poses, icp, has_Z, Z, Wb, prior, damping, linear, edges, joint):
    A, g, cost = edge_ref.system(poses, icp, has_Z, Z, Wb, prior, damping, linear, edges)
    if joint is not None:
        carried = carry(joint, poses)
        scatter(A, g, joint, carried, lambda i: i)
        cost += carried[2]
    return A, g, cost


def iteration(poses, icp, has_Z, Z, Wb, prior, damping, linear, edges, joint, solve=np.linalg.solve):
    """as window_edge_ref.iteration, with the joint factor (None: none).  Returns the new poses, xi (W, 6) and the cost at `poses`."""
    A, g, cost = system(poses, icp, has_Z, Z, Wb, prior, damping, linear, edges, joint)
    xi = solve(A, -g).reshape(len(poses), 6)
    return [lin_ref.retract(poses[i], xi[i]) for i in range(len(poses))], xi, cost


def separator(edges, joint):
    S = {1} | {e["b"] for e in edges if e["a"] == 0}
    if joint is not None:
        S |= {i for i in joint["poses"] if i != 0}
    return sorted(S)


def marginal(poses, icp0, has_Z1, Z1, Wb, prior, damping, linear, edges, joint):
    """what eliminating pose 0 leaves on its separator.  icp0: (H, b, f) of the oldest factor at pose 0, or None.  Returns a dict:
    sep, H, b, f (the model on the separator poses as given), valid, n_ties and the accumulated A00, AS0, ASS, g0, gS, c."""
    assert joint is None or joint["poses"][0] == 0
    sep = separator(edges, joint)
    ns = len(sep)
    slot = {0: 0, **{i: 1 + k for k, i in enumerate(sep)}}
    A, g, c = np.zeros((6 + 6 * ns, 6 + 6 * ns)), np.zeros(6 + 6 * ns), 0.0
    if icp0 is not None:
        A[:6, :6] += np.asarray(icp0[0], float).reshape(6, 6)
        g[:6] += np.asarray(icp0[1], float)
        c += float(icp0[2])
    for l in linear:
        if l["pose"] != 0:
            continue
        H, b, f = lin_ref.transport(np.asarray(l["H"], float).reshape(6, 6), np.asarray(l["b"], float), float(l["f"]), l["at"], poses[0])
        A[:6, :6] += H
        g[:6] += b
        c += f
    if joint is not None:
        carried = carry(joint, poses)
        scatter(A, g, joint, carried, lambda i: slot[i])
        c += carried[2]
    ties = ([dict(a=0, b=1, Z=Z1, info=np.diag(Wb))] if has_Z1 else []) + [e for e in edges if e["a"] == 0]
    for e in ties:
        _, _, Baa, Eba, ga, gb, cz = edge_ref.edge_terms(poses[0], poses[e["b"]], e["Z"], e["info"])
        s = slice(6 * slot[e["b"]], 6 * slot[e["b"]] + 6)
        A[:6, :6] += Baa
        A[s, :6] += Eba
        A[:6, s] += Eba.T
        A[s, s] += np.asarray(e["info"], float).reshape(6, 6)
        g[:6] += ga
        g[s] += gb
        c += cz
    A[:6, :6] += np.diag(prior) + damping * np.eye(6)
    A00, AS0, ASS, g0, gS = A[:6, :6], A[6:, :6], A[6:, 6:], g[:6], g[6:]
    out = dict(sep=sep, A00=A00, AS0=AS0, ASS=ASS, g0=g0, gS=gS, c=c, n_ties=len(ties))
    try:
        np.linalg.cholesky(A00)
    except np.linalg.LinAlgError:
        return dict(out, H=np.zeros((6 * ns, 6 * ns)), b=np.zeros(6 * ns), f=0.0, valid=0)
    X = np.linalg.solve(A00, np.column_stack([AS0.T, g0]))
    H = ASS - AS0 @ X[:, :-1]
    return dict(out, H=(H + H.T) / 2.0, b=gS - AS0 @ X[:, -1], f=c - g0 @ X[:, -1], valid=1)


def deviation(got, want):
    """(H, b, f): ||H_m - H_ref||_F relative to ||A_SS'||_F, b_m relative to ||g_S'||, f_m relative to |c| — the uncancelled scales.
    Without anything on the separator A_SS' and g_S' are zero and so must the differences be: they are then reported as they are."""
    n = 6 * len(want["sep"])
    nH, nb, nf = np.linalg.norm(want["ASS"]), np.linalg.norm(want["gS"]), abs(want["c"])
    dH = np.linalg.norm(np.asarray(got["H"], float).reshape(n, n) - want["H"])
    db = np.linalg.norm(np.asarray(got["b"], float).reshape(n) - want["b"])
    df = abs(float(got["f"]) - want["f"])
    return dH / nH if nH > 0 else dH, db / nb if nb > 0 else db, df / nf if nf > 0 else df


def as_joint(m, poses, shift=1):
    """a marginal (the restatement's or a driver's dict with sep, H, b, f) as the joint factor of the window without its oldest pose"""
    n = 6 * len(m["sep"])
    return dict(poses=[int(i) - shift for i in m["sep"]], at=[poses[i] for i in m["sep"]], H=np.asarray(m["H"], float).reshape(n, n),
                b=np.asarray(m["b"], float).reshape(n), f=float(m["f"]))


def random_joint(rng, members, poses, rot=3e-2, trans=2e-2, scale=1e3, cond=1e2):
    """a joint factor on `members` (ascending), each linearized up to rot rad / trans m away from its pose, H symmetric positive
    definite with correlations between the members, its minimum a few mrad / mm from L"""
    n = len(members)
    at = []
    for i in members:
        ax = rng.standard_normal(3)
        d = np.concatenate([ax / np.linalg.norm(ax) * rng.uniform(0.2, 1.0) * rot, rng.uniform(-1.0, 1.0, 3) / np.sqrt(3.0) * trans])
        at.append(lin_ref.retract(poses[i], d))
    Q = np.linalg.qr(rng.standard_normal((6 * n, 6 * n)))[0]
    lam = scale * np.logspace(0, np.log10(cond), 6 * n)[rng.permutation(6 * n)]
    H = (Q * lam) @ Q.T
    H = (H + H.T) / 2.0
    return dict(poses=[int(i) for i in members], at=at, H=H, b=H @ (rng.standard_normal(6 * n) * 5e-3), f=float(rng.uniform(0.5, 5.0)))
