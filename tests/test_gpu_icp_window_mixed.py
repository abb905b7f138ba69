"""-m gpu: the three fixed-lag window chains (mh_icp_window_optimise, _relin, _lin and their _async forms) on windows whose
factors differ — in k, in the neighbour mode of their map, in size, in reg_4_dof and project_on_degneneracy — so that an
iteration makes several K3 launches and the step kernels reach the argument blocks through a permuted slot[].

Reference: a host-driven loop written here.  Per iteration ONE SEPARATE mh_icp_linearize per factor (components off, window
order, on clones) — not mh_icp_linearize_batch, which shares its grouping with the chains — then tests/window_lin_ref.py's
iteration (numpy, written from the header's contract: general Z, has_Z with gaps, linear factors) with the refined solve of
tests/test_gpu_icp_window.py.  With thresholds: evaluate when any(|d| > thr), strictly, otherwise transport the kept H, b, f.

Scene: synth.small_world() (a map of ~5 k points, a 1 024-point scan), the same map points under neighbour modes 7, 19 and 27;
a factor of n points takes every (1024 // n)-th point of the scan, the first n of them.  Start poses perturbed(truth, 100 * seed
+ i); Z[i] the true relative pose (identity) composed with an offset of up to 1 degree and 0.05 m of seed 100 * seed + 50 + i,
so Z_R != Z_R^T, Z_t != 0 and the between residuals do not vanish at the optimum.  The replay's loose prior on pose 0,
damping 1e-9, iters = 6 and eps = 0 unless the case says otherwise.  Every pose is held by the prior, a between factor or a
factor of >= 300 points that does not project; a has_Z gap lies only between two poses with a full factor each.

Launch groups (window_launch_groups' rule, restated in launch_groups() below and checked against the lists given here): the
non-empty factors in window order; key = (workgroup class, k == 5 or the generic path, neighbour mode); class = 128 threads
for a k = 5 factor when the window has at most 8 factors and at most 32 768 points in all, else 256 (windows above 65 536
points: out of scope); groups in order of first appearance, slots handed out group by group.

  A  W = 5, k = [5, 8, 5, 8, 5], mode 19, 1 024 points each, has_Z = [0, 1, 1, 1, 1].
     groups (128, 5, 19): poses 0 2 4 | (256, 8, 19): poses 1 3.  slot = [0, 3, 1, 4, 2].
  B  W = 6, k = 5, modes [7, 19, 27, 19, 7, 27], 1 024 points each, has_Z = [0, 1, 1, 0, 1, 1] (the gap at pose 3).
     groups (128, 5, 7): 0 4 | (128, 5, 19): 1 3 | (128, 5, 27): 2 5.  slot = [0, 2, 4, 3, 1, 5].
  C  W = 8, k = [5, 8, 3, 5, 8, 5, 8, 5], modes [19, 19, 7, 27, 27, 19, 7, 19], sizes [1024, 512, 300, 1, 1024, 63, 0, 65],
     reg_4_dof = [0, 1, 0, 0, 1, 0, 0, 1], project = [0, 0, 0, 0, 1, 0, 0, 0], has_Z = [0, 1, 1, 1, 1, 1, 1, 1].
     groups (128, 5, 19): 0 5 7 (ragged: 1 024, 63, 65 points) | (256, 8, 19): 1 | (256, 8, 7): 2 (k = 3 takes the generic path) |
     (128, 5, 27): 3 | (256, 8, 27): 4; pose 6 is empty and has no slot.  slot = [0, 3, 4, 5, 6, 1, -1, 2].
  D  W = 16 (the staged launch form, the window limit), 256 points each, k = 5, 8, 5, 8, ..., modes 19, 7, 27, 19, ...,
     has_Z = [0] + [1] * 15.  W > 8: every class is 256; the key (k, mode) of pose i depends on i mod 6: six groups,
     poses {g, g + 6, g + 12}.  slot = [0, 3, 6, 9, 12, 14, 1, 4, 7, 10, 13, 15, 2, 5, 8, 11].
  E  case A with iters = 10, eps_rot = eps_trans = 1e-6: the chain stops early and the iterations queued behind the stop get
     n = 0 through the permuted slots.

What each run asserts.  Poses: every pose of every iteration within 1e-9 m and 1e-9 rad of the reference loop's, the same iters
and converged (the bar of the three window modules, through their compare()); each iteration's cost within 1e-6 relative.
first[i]: bit-identical to mh_icp_linearize_batch on a third set of clones at the start poses (H_ss, b_s, f, counters).  After
the call: every status array equals the reference factor's, last[i]'s counters those of the reference's last evaluation of
factor i, every handle's linearize count moved by its evaluations (an empty factor's by the executed iterations, as the
header says).  Relin: (0, 0) is the plain call bit for bit; at (1.75e-2, 5e-3) the masks equal the reference's, whose smallest
decision margin stays above 1e-7, and some iteration keeps a factor of one launch group while it evaluates one of another.
Lin: one random_linear factor per non-empty pose and two on pose 1; linear=[] is the call without it bit for bit, and the
factors move the final poses by more than 1e-6.  Case C: sync, async + mh_icp_window_wait and check_every = 1 give the same
bits.  test_reference_loop_is_stable runs every reference used here against itself with every start translation moved by
1e-13 m in x and holds it to the same 1e-9 bar.

Seeds: A 1, B 2, C 3, D 4, E 1 (it is case A) — the first tried; the linear factors' generator takes the case's seed.
None was replaced: every reference holds the 1e-9 bar against itself (worst 5.4e-15 m, 1.1e-15 rad, case A with linear factors).

Measured (MI355X): the worst pose difference of a chain from its reference loop over the module is 5.0e-16 m, 1.1e-16 rad (case C
with thresholds / case C plain).  Masks at the reference's thresholds, equal on both sides: A 11111, 11111, 00001, 0, 0, 0;
C 10111111, 10111111, 10110001, 0, 0, 0 (with linear factors 10100001 in iteration 2); smallest decision margin 1.0e-5 (C).

What the cases notice, tried once on deliberately wrong builds: next[] indexed by pose instead of by slot[] in the step kernels
(the poses of the plain kernel: A .. E; n = 0 of a kept factor: C in both threshold forms — not A, whose kept poses 1 .. 4
occupy slots 1 .. 4); reg_4_dof or project_on_degeneracy shifted by one pose, thresh_trans[] taken from the neighbour: C;
Z_R transposed, Z_t read one double early: every case.  The modules of like factors notice the first only through their empty
factor, the two mask shifts, and none of the last three."""
import numpy as np
import pytest

import test_gpu_icp_window as base
import test_gpu_icp_window_relin as relin_base
import window_lin_ref as ref
from test_gpu_icp_window import world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G = base.G
RELIN = relin_base.RELIN

_A = dict(seed=1, k=[5, 8, 5, 8, 5], mode=[19] * 5, n=[1024] * 5, reg4=[0] * 5, project=[0] * 5, has_Z=[0, 1, 1, 1, 1])
CASES = {
    "A": _A,
    "B": dict(seed=2, k=[5] * 6, mode=[7, 19, 27, 19, 7, 27], n=[1024] * 6, reg4=[0] * 6, project=[0] * 6, has_Z=[0, 1, 1, 0, 1, 1]),
    "C": dict(seed=3, k=[5, 8, 3, 5, 8, 5, 8, 5], mode=[19, 19, 7, 27, 27, 19, 7, 19], n=[1024, 512, 300, 1, 1024, 63, 0, 65],
              reg4=[0, 1, 0, 0, 1, 0, 0, 1], project=[0, 0, 0, 0, 1, 0, 0, 0], has_Z=[0] + [1] * 7),
    "D": dict(seed=4, k=[5, 8] * 8, mode=[(19, 7, 27)[i % 3] for i in range(16)], n=[256] * 16, reg4=[0] * 16, project=[0] * 16, has_Z=[0] + [1] * 15),
    "E": dict(_A, cfg=dict(iters=10, eps_rot=1e-6, eps_trans=1e-6)),
}
# what the module docstring states per case: the groups' keys and the slot of every pose
LAYOUT = {
    "A": ([(128, 5, 19), (256, 8, 19)], [0, 3, 1, 4, 2]),
    "B": ([(128, 5, 7), (128, 5, 19), (128, 5, 27)], [0, 2, 4, 3, 1, 5]),
    "C": ([(128, 5, 19), (256, 8, 19), (256, 8, 7), (128, 5, 27), (256, 8, 27)], [0, 3, 4, 5, 6, 1, -1, 2]),
    "D": ([(256, 5, 19), (256, 8, 7), (256, 5, 27), (256, 8, 19), (256, 5, 7), (256, 8, 27)], [0, 3, 6, 9, 12, 14, 1, 4, 7, 10, 13, 15, 2, 5, 8, 11]),
    "E": ([(128, 5, 19), (256, 8, 19)], [0, 3, 1, 4, 2]),
}
RUN_MODES = {"plain": (None, False), "relin": (RELIN, False), "lin": (None, True), "lin_relin": (RELIN, True)}  # mode -> (thresholds, linear factors)
# every reference loop this module compares a chain with
REFERENCES = [(name, "plain") for name in CASES] + [(name, mode) for name in ("A", "C") for mode in ("relin", "lin", "lin_relin")]


def launch_groups(case):
    """the rule of window_launch_groups from its contract (the ABI does not report the grouping): keys in order of first
    appearance, the group of every pose (-1: empty) and its slot"""
    W, total = len(case["n"]), sum(case["n"])
    keys, group = [], []
    for i in range(W):
        if case["n"][i] == 0:
            group.append(-1)
            continue
        k5 = case["k"][i] == 5
        key = (128 if k5 and W <= 8 and total <= 32768 else 256, 5 if k5 else 8, case["mode"][i])
        if key not in keys:
            keys.append(key)
        group.append(keys.index(key))
    order = [i for g in range(len(keys)) for i in range(W) if group[i] == g]
    return keys, group, [order.index(i) if group[i] >= 0 else -1 for i in range(W)]


def subsample(scan, n):
    return scan[:0] if n == 0 else np.ascontiguousarray(scan[::len(scan) // n][:n])


def z_offset(seed):
    """the true relative pose (identity) composed with an offset of up to 1 degree and 0.05 m"""
    rng = np.random.default_rng(seed)
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    return base.expmap(ax / np.linalg.norm(ax) * np.deg2rad(rng.uniform(0.0, 1.0))), d / np.linalg.norm(d) * rng.uniform(0.0, 0.05)


def scene(truth, case):
    W, seed = len(case["n"]), case["seed"]
    poses = [base.perturbed(truth, 100 * seed + i) for i in range(W)]
    Z = [z_offset(100 * seed + 50 + i) for i in range(W)]
    return poses, Z, list(case["has_Z"])


def case_cfg(case, **kw):
    return base.window_cfg(False, **dict(dict(iters=6, eps_rot=0.0, eps_trans=0.0), **case.get("cfg", {}), **kw))


def linear_factors(case, poses):
    """one per non-empty pose, then a second one on pose 1"""
    rng = np.random.default_rng(case["seed"])
    lin = [ref.random_linear(rng, i, poses[i]) for i in range(len(poses)) if case["n"][i]]
    return lin + [ref.random_linear(rng, 1, poses[1])]


def reference_loop(linearize, have, poses, Z, has_Z, cfg, linear=(), relin=None):
    """linearize(i, R, t) -> the result of a separate, components-off linearize of factor i.  Per iteration the poses, the cost
    and the mask of the evaluated factors; per factor its last evaluation's result and how many it had; the smallest margin of
    a threshold decision."""
    poses = [(np.array(R, float), np.array(t, float)) for R, t in poses]
    W = len(poses)
    Wb, prior = np.array(cfg.between_info), np.array(cfg.prior_info)
    thr = None if relin is None else np.array([relin[0]] * 3 + [relin[1]] * 3)
    kept, last, n_eval = [None] * W, [None] * W, [0] * W
    trace, masks, margin, converged = [], [], np.inf, 0
    for it in range(cfg.iters):
        icp, mask = [], 0
        for i in range(W):
            evaluate = True
            if thr is not None and it and have[i]:
                d = ref.local(kept[i][0], poses[i])
                margin = min(margin, float(np.abs(np.abs(d) - thr).min()))
                evaluate = bool(np.any(np.abs(d) > thr))
            if evaluate:  # (an empty factor's call launches nothing: its books move with the iterations, as the chain's do)
                last[i] = linearize(i, *poses[i])
                n_eval[i] += 1
                if have[i]:
                    kept[i] = (poses[i], np.array(last[i]["H_ss"], float).reshape(6, 6), np.array(last[i]["b_s"], float), float(last[i]["f"]))
                    mask |= 1 << i
                icp.append(kept[i][1:] if have[i] else None)
            else:
                icp.append(ref.transport(kept[i][1], kept[i][2], kept[i][3], kept[i][0], poses[i]))
        poses, xi, cost = ref.iteration(poses, icp, has_Z, Z, Wb, prior, cfg.damping, list(linear), solve=base.solve_refined)
        trace.append(dict(poses=poses, f=cost))
        masks.append(mask)
        if np.all(np.linalg.norm(xi[:, :3], axis=1) < cfg.eps_rot) and np.all(np.linalg.norm(xi[:, 3:], axis=1) < cfg.eps_trans):
            converged = 1
            break
    return dict(poses=poses, iters=len(trace), converged=converged, trace=trace, masks=masks, margin=margin, last=last, n_eval=n_eval)


class Mixed:
    """the maps of the three neighbour modes over the same points, the base factors of the cases, and every reference loop's
    result, computed once and left unchanged"""

    def __init__(self, world):
        capi = world.capi
        self.world, self.capi = world, capi
        points = world.synth.small_world()[0]
        self.maps = {19: world.small_map}
        for mode in (7, 27):
            self.maps[mode] = capi.VoxelMap(world.ctx, mode=mode)
            self.maps[mode].insert(points)
        self.bases, self.refs, self.batches = {}, {}, {}

    def base(self, k, mode, reg4, project, n):
        key = (k, mode, reg4, project, n)
        if key not in self.bases:
            cfg = dict(self.world.synth.enwide_config(), num_corres_points=k, reg_4_dof=reg4, project_on_degneneracy=project)
            if project:
                cfg["degen_thresh_trans"] = 1e6  # a threshold no direction reaches: every iteration is degenerate
            f = self.capi.ICPFactor(self.world.ctx, self.maps[mode], subsample(self.world.small_scan, n), self.capi.make_reg_config(**cfg))
            assert f.n == n
            self.bases[key] = f
        return self.bases[key]

    def clones(self, case):
        return [self.base(case["k"][i], case["mode"][i], case["reg4"][i], case["project"][i], case["n"][i]).clone() for i in range(len(case["n"]))]

    def run_reference(self, name, mode, shift=0.0):
        case = CASES[name]
        relin, with_linear = RUN_MODES[mode]
        poses, Z, has_Z = scene(self.world.truth(), case)
        linear = linear_factors(case, poses) if with_linear else []
        b = self.clones(case)
        for f in b:
            f.set_components(False)
        out = reference_loop(lambda i, R, t: b[i].linearize(R, t, G), [n > 0 for n in case["n"]], [(R, t + np.array([shift, 0.0, 0.0])) for R, t in poses],
                             Z, has_Z, case_cfg(case), linear, relin)
        out["status"] = [f.state()[0].copy() for f in b]
        for f in b:
            f.destroy()
        return out

    def reference(self, name, mode):
        if (name, mode) not in self.refs:
            self.refs[name, mode] = self.run_reference(name, mode)
        return self.refs[name, mode]

    def batch(self, name):
        """mh_icp_linearize_batch on clones of the case's factors at the start poses"""
        if CASES[name]["seed"] not in self.batches:
            case = CASES[name]
            poses = scene(self.world.truth(), case)[0]
            c = self.clones(case)
            for f in c:
                f.set_components(False)
            self.batches[case["seed"]] = self.capi.linearize_batch(c, [p[0] for p in poses], [p[1] for p in poses])
            for f in c:
                f.destroy()
        return self.batches[CASES[name]["seed"]]

    def chain(self, name, relin=None, linear=None, wait=True, **cfg_kw):
        """the call on fresh clones: its result, every factor's status array afterwards and by how much every handle's count moved"""
        case = CASES[name]
        poses, Z, has_Z = scene(self.world.truth(), case)
        a = self.clones(case)
        got = self.capi.optimise_window(a, poses, case_cfg(case, **cfg_kw), has_Z=has_Z, Z=Z, trace_poses=True, relin=relin, linear=linear, wait=wait)
        if not wait:
            got = got.wait()
        status = [f.state()[0].copy() for f in a]
        moved = [f.linearize(*poses[i], G)["linearize_count"] - 1 for i, f in enumerate(a)]  # (the next call's number, less one)
        for f in a:
            f.destroy()
        return got, status, moved

    def close(self):
        for f in self.bases.values():
            f.destroy()
        for mode in (7, 27):
            self.maps[mode].release()


@pytest.fixture(scope="module")
def mixed(world):
    m = Mixed(world)
    yield m
    m.close()


def against_the_reference(mixed, name, mode):
    """one chain call of the case in that mode against its reference loop: everything a run asserts"""
    case = CASES[name]
    W, have = len(case["n"]), [n > 0 for n in case["n"]]
    relin, with_linear = RUN_MODES[mode]
    linear = linear_factors(case, scene(mixed.world.truth(), case)[0]) if with_linear else None
    want = mixed.reference(name, mode)
    got, status, moved = mixed.chain(name, relin=relin, linear=linear)
    tag = f"case {name} {mode}"
    base.compare(got, want, tag)
    for it in range(got["iters"]):
        print(tag, "iteration", it, "cost", got["trace"][it]["f"], want["trace"][it]["f"])
        assert abs(got["trace"][it]["f"] - want["trace"][it]["f"]) <= 1e-6 * max(1.0, abs(want["trace"][it]["f"]))
    if relin is not None:
        print(tag, "masks", [bin(m) for m in want["masks"]], "device", [bin(int(m)) for m in got["evaluated"]], "margin %.3e" % want["margin"])
        assert want["margin"] > 1e-7  # no decision so close to its threshold that poses 1e-9 apart could take it differently
        assert [int(m) for m in got["evaluated"]] == want["masks"]
    first = mixed.batch(name)
    for i in range(W):
        for key in ("H_ss", "b_s", "f") + base.COUNTERS:
            assert np.array_equal(np.asarray(got["first"][i][key]), np.asarray(first[i][key]), equal_nan=True), (tag, "first", i, key)
        assert np.array_equal(status[i], want["status"][i]), (tag, "status", i)
        print(tag, "pose", i, "last", {k: got["last"][i][k] for k in base.COUNTERS}, "reference", {k: want["last"][i][k] for k in base.COUNTERS})
        for key in base.COUNTERS:
            assert np.array_equal(np.asarray(got["last"][i][key]), np.asarray(want["last"][i][key]), equal_nan=True), (tag, "last", i, key)
        evaluations = sum((m >> i) & 1 for m in want["masks"]) if have[i] else got["iters"]
        assert moved[i] == evaluations == want["n_eval"][i], (tag, "count", i)
        assert np.array_equal(got["R"][i].ravel(), got["poses"][-1, i, :9]) and np.array_equal(got["t"][i], got["poses"][-1, i, 9:])
    return got, want


def test_the_cases_span_the_launch_groups_the_docstring_states():
    for name, case in CASES.items():
        keys, group, slot = launch_groups(case)
        assert (keys, slot) == LAYOUT[name], name
        assert len(keys) >= 2 and slot != sorted(slot)  # several K3 launches per iteration, and slot[i] != i
    assert [len(launch_groups(CASES[n])[0]) for n in "ABCD"] == [2, 3, 5, 6]


@pytest.mark.parametrize("name", list(CASES))
def test_chain_is_the_reference_loop(mixed, name):
    got, want = against_the_reference(mixed, name, "plain")
    if name == "C":
        assert not np.any(got["first"][4]["H_ss"]) and not np.any(got["first"][6]["H_ss"])  # the projecting and the empty factor
        assert all((r["degenerate"] >> 8) & 2 for r in got["trace"])  # pose 4, a translation direction: every iteration projects
    if name == "E":  # what the case is for: the stop, with iterations queued behind it
        assert want["converged"] == 1 and want["iters"] < CASES["E"]["cfg"]["iters"]
    else:
        assert got["iters"] == 6 and got["converged"] == 0


def without_masks(d):
    return {k: v for k, v in d.items() if k != "evaluated"}


@pytest.mark.parametrize("name", ["A", "C"])
def test_relin_thresholds_zero_are_the_plain_chain_bit_for_bit(mixed, name):
    have = sum(1 << i for i, n in enumerate(CASES[name]["n"]) if n)
    plain, status, moved = mixed.chain(name)
    got, status0, moved0 = mixed.chain(name, relin=(0.0, 0.0))
    relin_base.same_bits(without_masks(got), plain)
    assert [int(m) for m in got["evaluated"]] == [have] * got["iters"]
    assert moved0 == moved and all(np.array_equal(x, y) for x, y in zip(status0, status))


@pytest.mark.parametrize("name", ["A", "C"])
def test_relin_thresholds_against_the_reference_loop(mixed, name):
    case = CASES[name]
    _, want = against_the_reference(mixed, name, "relin")
    have = sum(1 << i for i, n in enumerate(case["n"]) if n)
    group = launch_groups(case)[1]
    masks = want["masks"]
    assert any(m not in (0, have) for m in masks)
    # an iteration that keeps a factor of one launch group while it evaluates a factor of another
    assert any((have & ~m) >> i & 1 and (m >> j) & 1 and group[i] != group[j] for m in masks for i in range(len(group)) for j in range(len(group)))


@pytest.mark.parametrize("thresholds", [None, RELIN], ids=["all", "relin"])
@pytest.mark.parametrize("name", ["A", "C"])
def test_linear_factors_against_the_reference_loop(mixed, name, thresholds):
    got, _ = against_the_reference(mixed, name, "lin" if thresholds is None else "lin_relin")
    bare = mixed.chain(name, relin=thresholds)[0]
    empty = mixed.chain(name, relin=thresholds, linear=[])[0]
    relin_base.same_bits(empty, bare)
    moved = float(np.abs(got["poses"][-1] - bare["poses"][-1]).max())
    print("case", name, "final poses moved by the linear factors: %.3e" % moved)
    assert moved > 1e-6


@pytest.mark.parametrize("mode", ["plain", "relin", "lin_relin"])
def test_how_the_chain_is_driven_does_not_show(mixed, mode):
    relin, with_linear = RUN_MODES[mode]
    linear = linear_factors(CASES["C"], scene(mixed.world.truth(), CASES["C"])[0]) if with_linear else None
    runs = [mixed.chain("C", relin=relin, linear=linear, wait=wait, check_every=ce) for ce, wait in ((0, True), (1, True), (0, False))]
    assert runs[0][0]["iters"] == 6
    for got, status, moved in runs[1:]:
        relin_base.same_bits(got, runs[0][0])
        assert moved == runs[0][2] and all(np.array_equal(x, y) for x, y in zip(status, runs[0][1]))


@pytest.mark.parametrize("name,mode", REFERENCES)
def test_reference_loop_is_stable(mixed, name, mode):
    """the reference against itself with every start translation moved by 1e-13 m in x: a case whose associations or threshold
    decisions sit on an edge would move here"""
    r0, r1 = mixed.reference(name, mode), mixed.run_reference(name, mode, shift=1e-13)
    r1["poses"] = relin_base.rows(r1)
    base.compare(r1, r0, f"reference loop vs itself, case {name} {mode}")
    assert r1["masks"] == r0["masks"]
