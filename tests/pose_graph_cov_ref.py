"""Marginal covariances of the pose graph (rule 10 of "pose graph over all keyframes" in include/mimosa_hip.h) restated in numpy,
dense: A from pose_graph_robust_ref.system, every needed column of A^-1 from solve_refined (numpy.linalg.solve with two
refinement steps against a longdouble residual), the blocks of fixed poses zeroed.  None of the device's structure: no
tridiagonal factor, no recursion, no Woodbury correction.  The gate (capi.PoseGraph.gate) restated on top of it.  For graphs
of at most 12 poses an mpmath inverse at 40 digits as a second reference.

A case is a dict as tests/pose_graph_cases.py / tests/pose_graph_robust_cases.py make them (the plain ones have no "priors",
"edge_loss", "prior_loss": read as none)."""
import numpy as np

import pose_graph_ref as ref
import pose_graph_robust_ref as rref

CHI2_6_999 = 22.46      # the 0.999 quantile of chi^2 with 6 degrees of freedom


def system_of(c, R=None, t=None):
    R = c["R"] if R is None else R
    t = c["t"] if t is None else t
    return rref.system(R, t, [bool(x) for x in c["fixed"]], c["edges"], c.get("priors") or [], c.get("edge_loss"), c.get("prior_loss"), c["damping"])[0]


def columns(A, idx):
    """the columns `idx` of A^-1, refined"""
    E = np.zeros((A.shape[0], len(idx)))
    E[np.asarray(idx), np.arange(len(idx))] = 1.0
    return rref.solve_refined(A, E)


def _zero_fixed(c, S, rows, cols):
    fixed = np.asarray(c["fixed"]) != 0
    return S * np.outer(~np.repeat(fixed[rows], 6), ~np.repeat(fixed[cols], 6))


def covariances(c, poses=None, pairs=(), A=None, solve=columns):
    """({i: cov block (i, i)} for i in `poses` (None: all), [12 x 12 joint of each pair]) of a case: the needed columns of A^-1,
    refined, the blocks of fixed poses zero.  `solve(A, idx)`: the columns idx of A^-1."""
    A = system_of(c) if A is None else A
    n = A.shape[0] // 6
    poses = sorted(set(range(n) if poses is None else poses) | {q for pr in pairs for q in pr})
    at = {q: k for k, q in enumerate(poses)}
    S = solve(A, [6 * q + k for q in poses for k in range(6)])                     # 6 n x 6 len(poses)
    blk = lambda i, j: _zero_fixed(c, S[6 * i:6 * i + 6, 6 * at[j]:6 * at[j] + 6], [i], [j])
    cov = {q: (blk(q, q) + blk(q, q).T) / 2.0 for q in poses}
    joint = [np.block([[cov[i], blk(i, j)], [blk(i, j).T, cov[j]]]) for i, j in pairs]
    return cov, joint


def sparse_system(c):
    """A of a case without priors and losses as a scipy.sparse matrix: pose_graph_ref.system block by block (for graphs whose
    dense A does not fit)"""
    import scipy.sparse as sp
    assert not c.get("priors") and not c.get("edge_loss")
    R, t, fixed = c["R"], c["t"], c["fixed"]
    rows, cols, vals = [], [], []

    def add(i, j, B):
        rr, cc = np.meshgrid(np.arange(6 * i, 6 * i + 6), np.arange(6 * j, 6 * j + 6), indexing="ij")
        rows.append(rr.ravel()), cols.append(cc.ravel()), vals.append(np.asarray(B).ravel())
    for a, b, ZR, Zt, Om in c["edges"]:
        _, Ja = ref.edge_terms(R[a], t[a], R[b], t[b], ZR, Zt)
        if not fixed[a]:
            add(a, a, Ja.T @ Om @ Ja)
        if not fixed[b]:
            add(b, b, Om)
        if not fixed[a] and not fixed[b]:
            add(b, a, Om @ Ja)
            add(a, b, (Om @ Ja).T)
    for i in range(len(R)):
        add(i, i, np.eye(6) if fixed[i] else c["damping"] * np.eye(6))
    n = 6 * len(R)
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()


def sparse_columns(A, idx, refine=1):
    """the columns idx of A^-1 by a sparse LU, refined `refine` times against a longdouble residual"""
    import scipy.sparse.linalg as spl
    lu = spl.splu(A)
    E = np.zeros((A.shape[0], len(idx)))
    E[np.asarray(idx), np.arange(len(idx))] = 1.0
    x = lu.solve(E)
    Ac = A.tocoo()
    vl = Ac.data.astype(np.longdouble)
    for _ in range(refine):
        r = E.astype(np.longdouble)
        np.subtract.at(r, Ac.row, vl[:, None] * x[Ac.col].astype(np.longdouble))
        x = x + lu.solve(r.astype(np.float64))
    return x


def plain_inverse(c, poses=None, A=None):
    """{i: cov block} by numpy.linalg.inv alone: the yardstick the tests measure the reference's neighbourhood with"""
    A = system_of(c) if A is None else A
    S = np.linalg.inv(A)
    poses = range(A.shape[0] // 6) if poses is None else poses
    return {i: _zero_fixed(c, S[6 * i:6 * i + 6, 6 * i:6 * i + 6], [i], [i]) for i in poses}


def mp_covariances(c, digits=40):
    """{i: cov block} by an mpmath inverse (graphs of at most 12 poses: a 64-pose inverse takes minutes)"""
    import mpmath
    A = system_of(c)
    n = A.shape[0] // 6
    assert n <= 12
    with mpmath.workdps(digits):
        Ai = mpmath.matrix(A.tolist()) ** -1
        S = np.array([[float(Ai[r, q]) for q in range(6 * n)] for r in range(6 * n)])
    return {i: _zero_fixed(c, S[6 * i:6 * i + 6, 6 * i:6 * i + 6], [i], [i]) for i in range(n)}


def gate(R, t, candidates, joint):
    """per candidate edge (a, b, Z_R, Z_t, info) NOT in the graph and its pair's joint covariance: r, the plain chi2 = r^T Om r,
    and d2 = r^T (J S J^T + Om^-1)^-1 r with J = [J_a | I]"""
    r, chi2, d2 = [], [], []
    for (a, b, ZR, Zt, Om), S in zip(candidates, joint):
        rr, Ja = ref.edge_terms(R[a], t[a], R[b], t[b], ZR, Zt)
        J = np.hstack([Ja, np.eye(6)])
        r.append(rr)
        chi2.append(float(rr @ Om @ rr))
        d2.append(float(rr @ np.linalg.solve(J @ S @ J.T + np.linalg.inv(Om), rr)))
    return np.array(r).reshape(-1, 6), np.array(chi2), np.array(d2)
