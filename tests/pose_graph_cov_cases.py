"""What tests/test_pose_graph_cov_cpu.py and tests/test_gpu_pose_graph_cov.py share: the cases (graphs of
tests/pose_graph_cases.py and tests/pose_graph_robust_cases.py), the pairs asked of each, the restatement's covariances
(tests/pose_graph_cov_ref.py), computed once per case and never changed, and the bar.

THE BAR is measured per case, never fixed: err_np is the error of plain numpy.linalg.inv(A) against the refined reference
over the checked free blocks, relative to the largest entry of those blocks; the code under test must stay within
16 x err_np, not below 1e-13.  (The structured route does not pivot and goes through the Woodbury subtraction; an unrefined
numpy prototype of it stayed within 4.4 x err_np against mpmath.)

Blocks checked: every pose of a graph of at most 65 poses; of a longer one the poses of CHECKED (ends, middle, the fixed poses
and their neighbours, the ends of the first far edges) and of the pairs, since every checked pose costs the reference six
refined columns of a dense system."""
import functools

import numpy as np

import pose_graph_cases as base
import pose_graph_cov_ref as cref
import pose_graph_robust_cases as robust

CASES = ("n1_prior_only", "n2_two_priors_one_pose", "n3_far", "n12_far_on_fixed", "n12_far_on_fixed_dcs", "n64", "n64_false_loop_cauchy",
         "n65_priors_no_fixed", "n257_two_fixed", "n257_mixed", "n300_far32")
SINGULAR = ("no_anchor", "broken_chain")
MARGIN, FLOOR = 16.0, 1e-13


@functools.lru_cache(maxsize=None)
def case(name):
    try:
        return robust.case(name)
    except KeyError:
        return dict(base.case(name), priors=[], edge_loss=None, prior_loss=None)


def pairs_of(name):
    """the pairs whose joint is compared with the restatement: adjacent, far apart, one with a fixed end (where there is one)"""
    c = case(name)
    n = len(c["R"])
    if n == 1:
        return []
    if n <= 3:
        return [(0, 1)] + ([(0, 2), (1, 2)] if n == 3 else [])
    fixed = np.flatnonzero(c["fixed"])
    out = [(n // 3, n // 3 + 1), (1, n - 2), (n // 4, (3 * n) // 4)]
    if len(fixed):
        f = int(fixed[0])
        out.append((f, f + 5) if f + 5 < n else (f - 5, f))
    return out


def pairs64(name):
    """64 pairs that begin with pairs_of(name): the rest run through the graph (repeats where it has fewer pairs)"""
    n = len(case(name)["R"])
    out = list(pairs_of(name))
    k = 0
    while out and len(out) < 64:
        i = (7 * k) % (n - 1)
        out.append((i, min(n - 1, i + 1 + k % 5)))
        k += 1
    return out


def checked(name):
    c = case(name)
    n = len(c["R"])
    if n <= 65:
        return list(range(n))
    fixed = [int(v) for v in np.flatnonzero(c["fixed"])]
    far = [q for e in c["edges"] if e[1] - e[0] >= 2 for q in e[:2]][:8]
    want = {0, 1, n // 2, n - 2, n - 1, *fixed, *[f - 1 for f in fixed if f > 0], *[f + 1 for f in fixed if f + 1 < n], *far}
    return sorted(want | {q for pr in pairs_of(name) for q in pr})


@functools.lru_cache(maxsize=None)
def restated(name):
    """dict(cov {i: 6 x 6}, joint [12 x 12 per pair of pairs_of], err_np, scale, bar): shared, never changed"""
    c = case(name)
    A = cref.system_of(c)
    poses = checked(name)
    cov, joint = cref.covariances(c, poses, pairs_of(name), A)
    plain = cref.plain_inverse(c, poses, A)
    free = [i for i in poses if not c["fixed"][i]]
    scale = max(np.abs(cov[i]).max() for i in free)
    err_np = max(np.abs(plain[i] - cov[i]).max() for i in free) / scale
    return dict(cov=cov, joint=joint, err_np=err_np, scale=scale, bar=max(MARGIN * err_np, FLOOR))


def compare(name, cov, joint):
    """largest error of the blocks under test against the restatement, relative to `scale`"""
    want = restated(name)
    err = max(np.abs(cov[i] - want["cov"][i]).max() for i in want["cov"])
    for got, w in zip(joint, want["joint"]):
        err = max(err, np.abs(got - w).max())
    return err / want["scale"]


def held_out(c):
    """the case without its far edges (and their losses), and the far edges as the gate's candidates"""
    near = [e for e in c["edges"] if e[1] - e[0] < 2]
    return dict(c, edges=near, edge_loss=None), [e for e in c["edges"] if e[1] - e[0] >= 2]


def exact_properties(c, cov, pairs, joint, eig_rel=1e-12):
    """what holds to the bit, and the joint's eigenvalues: the smallest not below -eig_rel x the largest"""
    for i in range(len(cov)):
        assert np.array_equal(cov[i], cov[i].T), i
        if c["fixed"][i]:
            assert not cov[i].any(), i
    for (i, j), S in zip(pairs, joint):
        assert np.array_equal(S[:6, :6], cov[i]) and np.array_equal(S[6:, 6:], cov[j]) and np.array_equal(S[:6, 6:], S[6:, :6].T), (i, j)
        if c["fixed"][i] or c["fixed"][j]:
            assert not S[:6, 6:].any(), (i, j)
        w = np.linalg.eigvalsh(S)
        assert w[0] >= -eig_rel * w[-1], (i, j, w[0], w[-1])


# ---- the largest graph the library takes ------------------------------------------------------------------------------------------
BIG_N, BIG_LOOPS = 4096, [(5, 4000), (1000, 3000)]
BIG_POSES = (1, 2048, 4000, 4095)        # first free, middle, a loop end, last
BIG_PAIRS = [(5, 4000), (2047, 2048)]


@functools.lru_cache(maxsize=None)
def big_case():
    return dict(base.circuit(BIG_N, 11, loops=BIG_LOOPS), priors=[], edge_loss=None, prior_loss=None)


@functools.lru_cache(maxsize=None)
def big_restated():
    """As restated(), with the restatement's A assembled sparse and its columns from a sparse LU refined once against a longdouble
    residual (no dense 24 576^2 inverse).  The yardstick of the bar is the UNREFINED sparse LU's error against the refined
    columns — what a backward-stable direct solve leaves at this condition number, as numpy.linalg.inv's is for the dense cases —
    with the same margin and floor."""
    c = big_case()
    A = cref.sparse_system(c)
    cov, joint = cref.covariances(c, BIG_POSES, BIG_PAIRS, A, solve=cref.sparse_columns)
    plain, _ = cref.covariances(c, BIG_POSES, BIG_PAIRS, A, solve=lambda A_, idx: cref.sparse_columns(A_, idx, refine=0))
    scale = max(np.abs(v).max() for v in cov.values())
    err_sp = max(np.abs(plain[i] - cov[i]).max() for i in cov) / scale
    return dict(cov=cov, joint=joint, err_np=err_sp, scale=scale, bar=max(MARGIN * err_sp, FLOOR))
