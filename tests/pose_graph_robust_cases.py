"""The graphs with priors and losses that tests/test_pose_graph_robust_cpu.py and tests/test_gpu_pose_graph_robust.py share, built
from the seeded circuits of tests/pose_graph_cases.py.  A case is a circuit's dict plus priors [(pose, Z_R, Z_t, info)],
edge_loss and prior_loss (one (kind, param) per edge / prior, or None).  Sizes as there — one pose, a far edge on three poses, a
far edge on the fixed pose, the 64-lane boundary, several workgroups, the far-edge limit — each with what this rule adds: a
prior alone, two priors on one pose, a prior whose info has no rotation part, priors instead of a fixed pose, every loss on near
and far edges and on priors.  The restatement's run of every case is computed once and shared."""
import copy
import functools

import numpy as np

import pose_graph_cases as base
import pose_graph_ref as ref
import pose_graph_robust_ref as rref
from pose_graph_robust_ref import CAUCHY, DCS, HUBER, NONE

ITERS = 20            # queued for the comparisons, convergence off
POSE_TOL = base.POSE_TOL
F_RTOL = base.F_RTOL
W_TOL = 1e-9
SIGMA_PRIOR = (4e-3, 2e-2)
FALSE_LOOP = (np.array([0.1, -0.05, 0.6]), np.array([3.0, -2.0, 0.5]))
LOOPS64 = [(3, 60), (10, 50), (5, 55), (20, 44)]


def f_close(got, want, n_terms):
    return abs(got - want) <= F_RTOL * abs(want) + base.f_floor(n_terms)


def _prior(rng, c, pose, sigma=SIGMA_PRIOR, offset=None):
    """a measurement of the pose's true value with noise (or a given offset in its tangent) and a dense info"""
    off = np.concatenate([rng.standard_normal(3) * sigma[0], rng.standard_normal(3) * sigma[1]]) if offset is None else np.asarray(offset, np.float64)
    info = base._info(rng, sigma)
    return pose, c["truth_R"][pose] @ ref.so3_exp(off[:3]), c["truth_t"][pose] + off[3:], info


def _with(c, priors=(), edge_loss=None, prior_loss=None):
    c = dict(copy.deepcopy(c))
    c.update(priors=list(priors), edge_loss=edge_loss, prior_loss=prior_loss)
    return c


def _loss_where(c, far=None, near=None):
    return [((far if b - a >= 2 else near) or (NONE, 0.0)) for a, b, *_ in c["edges"]]


def _falsify(c, e):
    a, b, ZR, Zt, Om = c["edges"][e]
    c["edges"][e] = (a, b, ZR @ ref.so3_exp(FALSE_LOOP[0]), Zt + FALSE_LOOP[1], Om)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "n1_prior_only":          # the start is the truth; the prior sits 0.3 rad and 0.6 m away: M is far from the identity
        c = base.circuit(1, 1, fixed=())
        return _with(c, [_prior(rng, c, 0, offset=[0.2, -0.15, 0.1, 0.4, -0.3, 0.35])])
    if name == "n2_two_priors_one_pose":
        c = base.circuit(2, 2, fixed=())
        return _with(c, [_prior(rng, c, 1, offset=[0.02, 0.01, -0.03, 0.1, 0.05, -0.08]), _prior(rng, c, 1)])
    if name == "n3_far_cauchy":
        c = base.circuit(3, 3, loops=[(0, 2)])
        return _with(c, edge_loss=_loss_where(c, far=(CAUCHY, 3.0)))
    if name == "n12_far_on_fixed_dcs":
        c = copy.deepcopy(base.case("n12_far_on_fixed"))
        return _with(c, edge_loss=_loss_where(c, far=(DCS, 9.0)))
    if name.startswith("n64_false_loop"):
        c = base.circuit(64, 5, loops=LOOPS64)
        _falsify(c, len(c["edges"]) - 1)
        far = {"n64_false_loop_plain": None, "n64_false_loop_huber": (HUBER, 3.0), "n64_false_loop_cauchy": (CAUCHY, 3.0), "n64_false_loop_dcs": (DCS, 9.0)}[name]
        return _with(c, edge_loss=_loss_where(c, far=far) if far else None)
    if name == "n65_priors_no_fixed":
        c = base.circuit(65, 6, loops=[(0, 64), (20, 44)], fixed=())
        p0, p64 = _prior(rng, c, 0), _prior(rng, c, 64)
        info = p64[3].copy()
        info[:3, :] = 0.0
        info[:, :3] = 0.0
        return _with(c, [p0, p64[:3] + (info,)])
    if name == "n257_mixed":
        c = base.circuit(257, 7, loops=[(2, 250), (50, 200), (100, 180), (99, 101)], fixed=(100, 256))
        priors = [_prior(rng, c, 200), _prior(rng, c, 0), _prior(rng, c, 128), _prior(rng, c, 255, offset=[0.05, 0.0, -0.04, 0.5, -0.4, 0.1]), _prior(rng, c, 128)]
        return _with(c, priors, _loss_where(c, far=(CAUCHY, 3.0), near=(HUBER, 3.0)), [(NONE, 0.0), (HUBER, 2.0), (DCS, 9.0), (CAUCHY, 3.0), (NONE, 0.0)])
    if name == "n300_far32_cauchy":
        # k = 300, chosen from the RESTATEMENT'S own error, before any run of the code under test.  The first step of this graph is
        # 1.2 m and f of the second iteration is taken far from a minimum, where it follows the poses to first order.  A rounding
        # of 1.1e-16 on the entries of the restatement's first system (six seeds) moves that f by up to, relative:
        #   no loss 7.2e-13 | k = 3: 3.4e-12 | 10: 4.5e-12 | 30: 3.4e-12 | 100: 1.5e-12 | 300: 8.6e-13
        # (with k = 3 the start's chi^2 of 1e3 .. 4e4 all but switches the loops off, w down to 2e-4, and the first system is an
        # open chain of 300 poses whose step moves by 1.4e-11 m under the same rounding).  Only k = 300 leaves the reference inside
        # F_RTOL; the 32 weights are then 0.70 .. 1.0 at the start, still 32 different factors on the far-edge path.  Small weights
        # are the business of n3_far_cauchy, n64_false_loop_*, n257_mixed and huge_chi2.
        c = copy.deepcopy(base.case("n300_far32"))
        return _with(c, edge_loss=_loss_where(c, far=(CAUCHY, 300.0)))
    if name == "prior_on_fixed":         # acts on f alone
        c = copy.deepcopy(base.case("n12_far_on_fixed"))
        return _with(c, [_prior(rng, c, 0, offset=[0.01, 0.02, -0.01, 0.1, -0.2, 0.05])])
    if name == "no_anchor":              # T is singular: flag 4
        return _with(base.circuit(12, 4, loops=[(0, 11)], fixed=()))
    if name == "huge_chi2":              # the far edge is 1e6 m off: its Cauchy weight falls below the clamp
        c = copy.deepcopy(base.case("n12_far_on_fixed"))
        a, b, ZR, Zt, Om = c["edges"][-1]
        c["edges"][-1] = (a, b, ZR, Zt + np.array([1e6, 0.0, 0.0]), Om)
        return _with(c, edge_loss=_loss_where(c, far=(CAUCHY, 1.0)))
    raise KeyError(name)


FALSE_LOOP_CASES = ("n64_false_loop_huber", "n64_false_loop_cauchy", "n64_false_loop_dcs")
REGULAR = ("n1_prior_only", "n2_two_priors_one_pose", "n3_far_cauchy", "n12_far_on_fixed_dcs") + FALSE_LOOP_CASES + (
    "n65_priors_no_fixed", "n257_mixed", "n300_far32_cauchy", "prior_on_fixed", "huge_chi2")
SINGULAR = ("no_anchor",)


def n_terms(c):
    return len(c["edges"]) + len(c["priors"])


@functools.lru_cache(maxsize=None)
def restated(name, iters=ITERS):
    """the restatement's run of a case (shared, never changed)"""
    c = case(name)
    return rref.optimise(c["R"], c["t"], c["fixed"], c["edges"], c["priors"], c["edge_loss"], c["prior_loss"], iters, c["damping"])


@functools.lru_cache(maxsize=None)
def restated_weights(name):
    c = case(name)
    return rref.weights(c["R"], c["t"], c["edges"], c["priors"], c["edge_loss"], c["prior_loss"])


# ---- the hall with an aliased loop ------------------------------------------------------------------------------------------------
HALL_ALIAS = ((10, 28), (8, 26))      # the loop (10, 28), measured as the true relative pose of the pair (8, 26): two aisles alike
HALL_CAUCHY = 3.0


@functools.lru_cache(maxsize=None)
def hall_case():
    """tests/map_rebuild_ref.hall_case() — 36 keyframes, a drift of (3, 2, 0) cm per keyframe, pose 0 fixed, the true loop (0, 35) —
    plus one aliased loop.  ONE true loop: it carries the restatement into the right basin (asserted in
    tests/test_pose_graph_robust_cpu.py), so (1, 34) and (2, 33) are not added.  Returns the case with "edges" extended and
    "edge_loss": Cauchy on the two far edges."""
    import map_rebuild_ref
    case = dict(map_rebuild_ref.hall_case())
    Rt, tt = case["true"]
    (a, b), (a2, b2) = HALL_ALIAS
    info = case["edges"][0][4]
    case["edges"] = list(case["edges"]) + [(a, b, Rt[a2].T @ Rt[b2], Rt[a2].T @ (tt[b2] - tt[a2]), info)]
    case["edge_loss"] = [((CAUCHY, HALL_CAUCHY) if q[1] - q[0] >= 2 else (NONE, 0.0)) for q in case["edges"]]
    return case
