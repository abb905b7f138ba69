"""The graphs with more than MH_PGO_FAR_MAX far edges that tests/test_pose_graph_wide_cpu.py and tests/test_gpu_pose_graph_wide.py
share, built on the seeded circuits of tests/pose_graph_cases.py.  Random loops come from one seeded helper (wide_loops): it starts
with (0, n - 1), (0, 2), (n - 3, n - 1), then draws a in [0, n - 2) and b in [a + 2, n) and keeps duplicates.  Sizes where the
blocked phases of C can go wrong: one edge past the old limit, a skip edge on every pose, far edges on a fixed pose in the middle
(a zeroed block column of W), more far slots than the 64 lanes of the factor kernel, and two sizes tied to the panel width NB = 64
of pose_graph_device.hpp (kPgoWideNB): 6 F an exact multiple of NB, and 6 F the nearest value above a multiple of NB.  A case is
a circuit's dict plus edge_loss (one (kind, param) per edge, or None).  The restatement's run of every case is computed once and
shared."""
import copy
import functools

import numpy as np

import pose_graph_cases as base
import pose_graph_ref as ref
import pose_graph_robust_cases as robust
import pose_graph_robust_ref as rref

ITERS = base.ITERS
POSE_TOL = base.POSE_TOL
F_RTOL = base.F_RTOL
W_TOL = robust.W_TOL
f_close = base.f_close
NB = 64               # kPgoWideNB
CAUCHY_K = 3.0


def wide_loops(n, count, seed):
    rng = np.random.default_rng(seed)
    out = [(0, n - 1), (0, 2), (n - 3, n - 1)]
    while len(out) < count:
        a = int(rng.integers(0, n - 2))
        out.append((a, int(rng.integers(a + 2, n))))
    return out


def _plain(c):
    c = dict(c)
    c["edge_loss"] = None
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "w40_far33":              # one edge past the old limit
        return _plain(base.circuit(40, 21, loops=wide_loops(40, 33, 121)))
    if name == "w60_skip2":              # a skip edge on every pose: 59 far edges
        return _plain(base.circuit(60, 22, loops=[(i, i + 2) for i in range(58)] + [(0, 59)]))
    if name == "w80_far70":
        return _plain(base.circuit(80, 23, loops=wide_loops(80, 70, 123)))
    if name == "w80_far70_fixed41":      # the same loops; pose 41 fixed too: far edges on a fixed pose, the zeroed block column
        return _plain(base.circuit(80, 23, loops=wide_loops(80, 70, 123), fixed=(0, 41)))
    if name == "w120_far128":
        return _plain(base.circuit(120, 24, loops=wide_loops(120, 128, 124)))
    if name == "w90_far64":              # NB = 64: 6 F = 384 = 6 NB, every block full
        return _plain(base.circuit(90, 25, loops=wide_loops(90, 64, 125)))
    if name == "w90_far43":              # NB = 64: 6 F = 258 = 4 NB + 2, a last block of two rows
        return _plain(base.circuit(90, 26, loops=wide_loops(90, 43, 126)))
    if name == "w80_psd_last":           # the LAST far edge's info positive semi-definite, as psd_info makes it: far slot 69
        c = copy.deepcopy(case("w80_far70"))
        a, b, ZR, Zt, Om = c["edges"][-1]
        Om = Om.copy()
        Om[2, :] = 0.0
        Om[:, 2] = 0.0
        c["edges"][-1] = (a, b, ZR, Zt, Om)
        return c
    if name == "broken_chain":
        return _plain(copy.deepcopy(base.case("broken_chain")))
    if name == "w80_far70_cauchy":       # Cauchy k = 3 on every loop, the last loop falsified
        c = copy.deepcopy(case("w80_far70"))
        robust._falsify(c, len(c["edges"]) - 1)
        c["edge_loss"] = [((rref.CAUCHY, CAUCHY_K) if b - a >= 2 else (rref.NONE, 0.0)) for a, b, *_ in c["edges"]]
        return c
    if name in ("n300_far32", "n64", "n3_far", "n1"):
        return _plain(copy.deepcopy(base.case(name)))
    raise KeyError(name)


REGULAR = ("w40_far33", "w60_skip2", "w80_far70", "w80_far70_fixed41", "w120_far128", "w90_far64", "w90_far43")
SINGULAR = ("w80_psd_last", "broken_chain")
ROBUST = "w80_far70_cauchy"
PLAIN = ("n300_far32", "n64", "n3_far", "n1")    # cases of at most MH_PGO_FAR_MAX far edges, run on wide graphs


def n_far(c):
    return sum(1 for e in c["edges"] if e[1] - e[0] >= 2)


@functools.lru_cache(maxsize=None)
def restated(name, iters=ITERS):
    """the dense restatement's run of a case (shared, never changed)"""
    c = case(name)
    if c["edge_loss"] is None:
        return ref.optimise(c["R"], c["t"], c["fixed"], c["edges"], iters, c["damping"], 0.0, 0.0)
    return rref.optimise(c["R"], c["t"], c["fixed"], c["edges"], [], c["edge_loss"], None, iters, c["damping"])
