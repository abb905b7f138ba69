"""The graphs tests/test_pose_graph_cpu.py and tests/test_gpu_pose_graph.py share: seeded keyframe trajectories on a closed
circuit.  Odometry edges (i, i + 1) carry noise of 2 mrad / 1 cm, loop edges twice that; information matrices are dense (rotated,
so not diagonal) and exactly symmetric; the start is integrated odometry.  Sizes are chosen where the code can go wrong: one
pose, no far edge, a far edge on the fixed pose, the 64-lane boundary, several workgroups of the per-pose kernels, the far-edge
limit, and two graphs whose T or Om is singular.  The restatement's run of every case is computed once and shared."""
import functools

import numpy as np

import pose_graph_ref as ref

ITERS = 12            # queued for the comparisons, convergence off: every regular case has converged by then (asserted on the restatement)
STOP_EPS = 1e-6       # the stop test's case: rad and m
POSE_TOL = 1e-9       # m and rad: the project's standing bar for poses (the numpy prototype of this solver stayed below 2e-14)
F_RTOL = 1e-12
STOP_CASES = ("n12_far_on_fixed", "n65")


def f_floor(n_edges):
    """what a cost that is zero in exact arithmetic may come out as: a residual entry carries roundings of 1e-16 times a pose
    magnitude of up to 100 m, 1e-14, and the largest information entry is 1 / (2 mrad)^2 = 2.5e5; 36 E such products"""
    return 36 * max(n_edges, 1) * 2.5e5 * 1e-28


def f_close(got, want, n_edges):
    return abs(got - want) <= F_RTOL * abs(want) + f_floor(n_edges)


SIGMA_ODO = (2e-3, 1e-2)
SIGMA_LOOP = (4e-3, 2e-2)


def _info(rng, sigma):
    """Q diag(1 / sigma^2) Q^T with Q a rotation of the 6-space near the identity, symmetrised exactly"""
    w = np.array([1.0 / sigma[0] ** 2] * 3 + [1.0 / sigma[1] ** 2] * 3)
    S = rng.standard_normal((6, 6)) * 0.2
    Q, _ = np.linalg.qr(np.eye(6) + (S - S.T))
    M = Q @ np.diag(w) @ Q.T
    return (M + M.T) / 2.0


def _truth(n):
    """n poses on a closed circuit of 0.5 m steps: heading along the tangent, with a roll / pitch / height wave"""
    radius = max(1.0, 0.5 * n / (2.0 * np.pi))
    R, t = [], []
    for i in range(n):
        a = 2.0 * np.pi * i / max(n, 2)
        R.append(ref.so3_exp([0.0, 0.0, a + np.pi / 2.0]) @ ref.so3_exp([0.05 * np.sin(3.0 * a), 0.04 * np.cos(2.0 * a), 0.0]))
        t.append(np.array([radius * np.cos(a), radius * np.sin(a), 0.3 * np.sin(2.0 * a)]))
    return np.array(R), np.array(t)


def _measure(rng, R, t, a, b, sigma):
    abR = R[a].T @ R[b]
    abt = R[a].T @ (t[b] - t[a])
    return a, b, abR @ ref.so3_exp(rng.standard_normal(3) * sigma[0]), abt + rng.standard_normal(3) * sigma[1], _info(rng, sigma)


def circuit(n, seed, loops=(), fixed=(0,), twice_near=(), skip_near=(), damping=0.0):
    """dict(R, t (the start), fixed, edges [(a, b, Z_R, Z_t, info)], truth_R, truth_t, damping); edges in list order: the odometry
    chain (a pair of `twice_near` twice, a pair of `skip_near` not at all), then the loops"""
    rng = np.random.default_rng(seed)
    Rt, tt = _truth(n)
    edges = []
    for i in range(n - 1):
        if i in skip_near:
            continue
        edges.append(_measure(rng, Rt, tt, i, i + 1, SIGMA_ODO))
        if i in twice_near:
            edges.append(_measure(rng, Rt, tt, i, i + 1, SIGMA_ODO))
    odo = {e[0]: e for e in edges}
    for a, b in loops:
        edges.append(_measure(rng, Rt, tt, a, b, SIGMA_LOOP))
    R, t = [Rt[0]], [tt[0]]
    for i in range(n - 1):
        if i in odo:
            _, _, ZR, Zt, _ = odo[i]
        else:  # the chain is broken here: the start carries on from the truth's relative pose
            ZR, Zt = Rt[i].T @ Rt[i + 1], Rt[i].T @ (tt[i + 1] - tt[i])
        t.append(t[i] + R[i] @ Zt)
        R.append(R[i] @ ZR)
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    return dict(R=np.array(R), t=np.array(t), fixed=fx, edges=edges, truth_R=Rt, truth_t=tt, damping=damping)


def _loops32():
    """exactly 32 far edges over 300 poses: every span from 2 to 290, several on one pose, one on the fixed pose"""
    out = [(0, 299), (0, 150), (1, 3), (297, 299), (10, 290), (10, 12), (148, 152), (149, 151)]
    k = 0
    while len(out) < 32:
        a = 7 + 9 * k
        out.append((a, min(299, a + 40 + 5 * k)))
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "n1":
        return circuit(1, 1)
    if name == "n2":
        return circuit(2, 2)
    if name == "n3_far":
        return circuit(3, 3, loops=[(0, 2)])
    if name == "n12_far_on_fixed":
        return circuit(12, 4, loops=[(0, 11)])
    if name == "n64":
        return circuit(64, 5, loops=[(3, 60), (3, 60), (10, 50)], twice_near=(5,))
    if name == "n65":
        return circuit(65, 6, loops=[(0, 64), (20, 44), (20, 44)], twice_near=(63,))
    if name == "n257_two_fixed":
        return circuit(257, 7, loops=[(2, 250), (50, 200), (100, 180), (99, 101)], fixed=(100, 256))
    if name == "n300_far32":
        return circuit(300, 8, loops=_loops32())
    if name == "broken_chain":  # no near edge (5, 6): A is regular through the far edge (4, 7), T is not
        return circuit(12, 9, loops=[(4, 7)], skip_near=(5,))
    if name == "psd_info":      # the far edge's info has a zero row and column: positive semi-definite, Om^-1 does not exist
        c = circuit(12, 10, loops=[(2, 9)])
        a, b, ZR, Zt, Om = c["edges"][-1]
        Om = Om.copy()
        Om[2, :] = 0.0
        Om[:, 2] = 0.0
        c["edges"][-1] = (a, b, ZR, Zt, Om)
        return c
    raise KeyError(name)


REGULAR = ("n1", "n2", "n3_far", "n12_far_on_fixed", "n64", "n65", "n257_two_fixed", "n300_far32")
SINGULAR = ("broken_chain", "psd_info")
CIRCUITS = ("n12_far_on_fixed", "n64", "n65", "n257_two_fixed", "n300_far32")   # long enough for the loops to matter


@functools.lru_cache(maxsize=None)
def restated(name, iters=ITERS, eps=0.0):
    """the restatement's run of a regular case (shared, never changed)"""
    c = case(name)
    return ref.optimise(c["R"], c["t"], c["fixed"], c["edges"], iters, c["damping"], eps, eps)


@functools.lru_cache(maxsize=None)
def restated_residuals(name):
    c = case(name)
    return ref.residuals(c["R"], c["t"], c["edges"])
