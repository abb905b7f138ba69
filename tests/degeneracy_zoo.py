"""A "degenerate-geometry zoo" for what every consumer of the ICP factor decides on: loc_*_final (square roots of the eigenvalues of
the 3 x 3 rotation and translation blocks of H_ss), eigvec_* (their eigenvectors), the component sums projected on those bases
(K4), and the test "is a localizability above degen_thresh_*" (finish_result's project_on_degneneracy on the host,
align_block_degenerate on the device: mh_icp_align, the batch chain, every window chain).  Pure numpy + mpmath: the same checks
run on the CPU oracle and the host branches of math3.hpp (test_degeneracy_zoo_cpu.py), on the device (test_gpu_degeneracy_zoo.py)
and in the two tests that used to look away at degenerate blocks (test_gpu_fuzz.py, test_gpu_lane_classes.py).

Scenes.  A scene is a set of planes around a sensor at the origin of a local frame; every source point has a map cluster of
its own: five points c + a n, c +- su u - b n, c +- sv v - b n (a = 4 b = 1/64, su = 1/8, sv = 5/32 m) around a centre c on
the plane with unit normal n and in-plane axes u, v.  The cluster's mean is c and its covariance is diagonal in (n, u, v) with
eigenvalues 5 b^2 = 7.6e-5 < su^2 / 2 < sv^2 / 2 (every gate of the plane stage passes), so the fitted normal is n up to the
float32 rounding of the map coordinates; centres sit 0.625 m apart, so the five nearest map points of a query within 2 cm of c
are its own cluster (build() asserts it, with 0.1 m to spare) and a 0.5 m voxel holds at most 20 points.  The query is
c + e n + jitter, |e| <= 3 cm (below the Huber threshold).  All lengths are dyadic: in the axis pose (R = I, t = 0) the map is
exact in float32, the normals are exact axis vectors and the Hessian blocks carry exact zeros (the n == 0 and p <= 1e-8 branches
of the solvers, exactly repeated and exactly vanishing eigenvalues); in the generic pose (rotation exp([0.4, -0.7, 0.9]), offset
(100, -50, 20) m) the float32 rounding at 100 m tilts every normal by ~1e-4 and the same spectra come out perturbed: vanishing
eigenvalues at 1e-8 .. 1e-10 of the largest, repeated ones split by as much.  The scenes aim their spectra only approximately:
every reference is computed from the blocks the call REPORTED.  The map holds five points per source point (2 000 - 5 000
points), not the few ten thousand of a sampled room: the k-NN stage is not under test here (tests/plane_zoo.py).
Families (FAMILIES):
  floor          one plane: translation block of rank 1, yaw unobservable
  slab           floor and ceiling
  tunnel         four walls of a 4.6 x 4 m section, no ends: the translation eigenvalue along the axis vanishes
  tunnel_end_m   the tunnel and an end patch of m = 1, 8, 64 points: a small eigenvalue that is decided
  pipe           planes tangent to a cylinder around the x axis, twelve of sixteen azimuths (22.5 (j + 0.37) degrees: no
                 direction component near 0.5): one rotation and one translation eigenvalue vanish
  square_tunnel  a square section with equal walls: two equal translation eigenvalues
  cube_centre    six equal faces around the sensor: three equal translation eigenvalues
  near_parallel_e  a floor and two walls whose normals differ by e = 1e-2, 1e-4, 1e-6: smallest eigenvalue ~ N e^2 / 2
  few_m          200 source points of which m = 1, 2, 3, 5 have a map cluster (the others see nothing: status 1)
TILED: the floor's cloud (1 024 points) 65 times over, 66 560 points: the 512-thread launch class.

Reference.  A block A is read as exact numbers and decomposed with mp.eigsy at 60 digits.  |A| is its largest entry in
magnitude, lambda the reference eigenvalues (ascending).

Bars.
  eigenvalues   |loc_i^2 - lambda_i| <= 4e-13 |A|.  sym_eigen3 accepts a residual of 1e-13 |A| per component, at most
                sqrt(3) e-13 in the 2-norm, the Jacobi path is tighter; the error of a Rayleigh quotient is bounded by its
                residual.  A NaN localizability is accepted only where lambda_i <= 4e-13 |A| (the root of a rounding-level
                negative number, which Eigen produces too).
  eigenvectors  |V'V - I| <= 2e-10 (the code accepts dot products up to 1e-10); |A v - (v'A v) v|_inf <= 4e-13 |A|; reference
                eigenvalues whose gap is at most 1e-6 |A| form a cluster, and for every cluster that is not all three the
                projector on its span obeys |P_got - P_ref|_F <= 4e-13 / sep + 4e-10, sep = distance of the cluster to the other
                eigenvalues over |A| (Davis-Kahan with the residual bar, plus the orthogonality slack).  Single vectors inside a
                cluster are never compared.
  components    the sums recomputed in fp64 from state() and the REPORTED bases: |delta| <= 0.5 nb + 1e-9 N, nb = the number
                of valid points with a component within 1e-12 of 0.5 (asserted <= 4 per case), N the valid points.
  decisions     thresholds (float32, as the config holds them) are placed at the smallest DECIDED eigenvalue lambda_p of a
                block — the smallest one whose float32 neighbours below are decidable —: the two float32 values on either
                side of sqrt(lambda_p), and float32(sqrt(lambda_p) (1 +- 1e-3)).  A threshold t is used only where it is
                decidable: |t^2 - lambda_i| >= 16 * 4e-13 |A| for every i.  Expected: degenerate iff lambda_min > t^2 is
                false, lambda_min the block's smallest reference eigenvalue (what the code compares; below lambda_p it is
                rounding-level and every placed threshold must come out degenerate, NaN root included).  Exact.
  reg_4_dof     H_ss, b_s of a reg_4_dof call against Pi H Pi, Pi H_rt, H_tr Pi, Pi b computed in mpmath from the unprojected
                call (Pi = l l', l = R' (-g_unit)): 8 eps (eps = 2^-52) of the unprojected block's largest entry.
The Schur degeneracy info (degen_*, degen_eigvec_*) is out of scope: its error grows with cond(H)^2 and it is host code the
oracle restates line by line.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
from mpmath import matrix, mp, mpf

from mimosa_amd import synth

DPS = 60
EPS = 2.0 ** -52
BAR = 4e-13            # eigenvalues, residuals: times |A|
BAR_ORTHO = 2e-10
BAR_PROJ_FLOOR = 4e-10
CLUSTER_GAP = 1e-6     # times |A|
DECIDABLE = 16.0 * BAR  # times |A|
NB_MAX = 4
NEAR_HALF = 1e-12
BAR_REG4 = 8.0 * EPS
VALID = 8

A_OUT, B_IN, SU, SV = 1.0 / 64.0, 1.0 / 256.0, 1.0 / 8.0, 5.0 / 32.0
PITCH = 0.625
MAP_KW = dict(leaf=0.5, min_dist=0.0, mode=27)
R_GENERIC = synth.so3_exp(np.array([0.4, -0.7, 0.9]))
T_GENERIC = np.array([100.0, -50.0, 20.0])
POSES = ("axis", "generic")
FAMILIES = ("floor", "slab", "tunnel", "tunnel_end_1", "tunnel_end_8", "tunnel_end_64", "pipe", "square_tunnel", "cube_centre",
            "near_parallel_1e-2", "near_parallel_1e-4", "near_parallel_1e-6", "few_1", "few_2", "few_3", "few_5")
CASES = tuple((fam, pose) for fam in FAMILIES for pose in POSES)
BINARY_FAMILIES = ("tunnel", "cube_centre", "near_parallel_1e-4")
EXEMPT = ("floor", "pipe", "few")      # families that need not keep all four thresholds
TILED = ("floor", "generic")
TILES = 65
# binary factors: a target pose whose inverse composes exactly with dyadic translations (entries 0 / +-1)
R_TGT = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
T_TGT = np.array([0.5, -0.25, 1.0])
G_UNIT = np.array([0.02, -0.01, -1.0]) / np.linalg.norm([0.02, -0.01, -1.0])
X, Y, Z_ = np.eye(3)


def family_of(name):
    return name.rsplit("_", 1)[0] if name.startswith(("tunnel_end", "near_parallel", "few")) else name


def config(**changes):
    """enwide's scan_to_map block with the map's own min_dist 0 (every call re-associates); thresholds 0, projections off"""
    cfg = dict(synth.enwide_config(), target_ivox_map_min_dist_in_voxel=0.0, degen_thresh_rot=0.0, degen_thresh_trans=0.0)
    cfg.update(changes)
    return cfg


# ---- scenes ----

def _patch(origin, n, u, v, nu, nv):
    """cluster frames (c, n, u, v) on the plane through `origin`: an nu x nv grid of centres, PITCH apart, centred on it"""
    return [(origin + PITCH * (i - (nu - 1) / 2.0) * u + PITCH * (j - (nv - 1) / 2.0) * v, n, u, v) for i in range(nu) for j in range(nv)]


def _tunnel(half_y, lo_z, hi_z, nx=21, na=5):
    return (_patch(np.array([0.0, -half_y, 0.1875]), Y, X, Z_, nx, na) + _patch(np.array([0.0, half_y, 0.1875]), -Y, X, Z_, nx, na)
            + _patch(np.array([0.0, 0.0, lo_z]), Z_, X, Y, nx, na) + _patch(np.array([0.0, 0.0, hi_z]), -Z_, X, Y, nx, na))


def _frames(name):
    fam = family_of(name)
    if fam == "floor":
        return _patch(np.array([0.3125, 0.3125, -1.8125]), Z_, X, Y, 32, 32)
    if fam == "slab":
        return _patch(np.array([0.0, 0.0, -1.8125]), Z_, X, Y, 15, 15) + _patch(np.array([0.0, 0.0, 2.1875]), -Z_, X, Y, 15, 15)
    if fam == "tunnel":
        return _tunnel(2.3125, -1.8125, 2.1875)
    if fam == "tunnel_end":
        m = int(name.rsplit("_", 1)[1])
        side = {1: 1, 8: (2, 4), 64: 8}[m]
        nu, nv = (side, side) if isinstance(side, int) else side
        return _tunnel(2.3125, -1.8125, 2.1875) + _patch(np.array([7.3125, 0.0625, 0.1875]), -X, Y, Z_, nu, nv)
    if fam == "square_tunnel":
        return (_patch(np.array([0.0, -2.3125, 0.0]), Y, X, Z_, 21, 5) + _patch(np.array([0.0, 2.3125, 0.0]), -Y, X, Z_, 21, 5)
                + _patch(np.array([0.0, 0.0, -2.3125]), Z_, X, Y, 21, 5) + _patch(np.array([0.0, 0.0, 2.3125]), -Z_, X, Y, 21, 5))
    if fam == "cube_centre":
        out = []
        for ax, (u, v) in ((X, (Y, Z_)), (Y, (Z_, X)), (Z_, (X, Y))):
            out += _patch(-2.3125 * ax, ax, u, v, 7, 7) + _patch(2.3125 * ax, -ax, u, v, 7, 7)
        return out
    if fam == "pipe":
        out = []
        for j in range(16):
            if j in (3, 4, 11, 12):  # fewer normals along z: the two transverse eigenvalues differ
                continue
            th = 2.0 * np.pi * (j + 0.37) / 16.0
            rad, tan = np.array([0.0, np.cos(th), np.sin(th)]), np.array([0.0, -np.sin(th), np.cos(th)])
            out += _patch(2.5 * rad, -rad, X, tan, 21, 1)
        return out
    if fam == "near_parallel":
        e = float(name.rsplit("_", 1)[1])
        n2, u2 = -np.array([np.cos(e), np.sin(e), 0.0]), np.array([-np.sin(e), np.cos(e), 0.0])
        return (_patch(np.array([0.0, 0.0, -1.8125]), Z_, X, Y, 15, 15) + _patch(np.array([-2.3125, 0.0, 0.1875]), X, Y, Z_, 9, 5)
                + _patch(np.array([2.3125, 0.0, 0.1875]), n2, u2, Z_, 9, 5))
    if fam == "few":
        m = int(name.rsplit("_", 1)[1])
        d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
        u = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
        five = [(np.array([0.625, 0.0, -1.8125]), Z_, X, Y), (np.array([2.3125, 0.625, 0.0]), -X, Y, Z_), (np.array([0.0, 2.3125, 0.625]), -Y, Z_, X),
                (np.array([-1.25, 1.25, -1.8125]), Z_, X, Y), (1.5 * np.sqrt(3.0) * d, -d, u, np.cross(d, u))]
        return five[:m]
    raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def build(name, pose):
    """-> map_xyz float32 (5 n, 3), pts (POINT_DTYPE, sensor frame), R, t (the sensor's pose in the map), n_designed."""
    frames = _frames(name)
    rng = np.random.default_rng([20262, FAMILIES.index(name)])
    Rg, tg = (np.eye(3), np.zeros(3)) if pose == "axis" else (R_GENERIC, T_GENERIC)
    local, query = [], []
    for c, n, u, v in frames:
        assert n @ (-c) > 0  # the plane faces the sensor
        local += [c + A_OUT * n, c + SU * u - B_IN * n, c - SU * u - B_IN * n, c + SV * v - B_IN * n, c - SV * v - B_IN * n]
        jv = rng.uniform(-0.02, 0.02) * (0.0 if family_of(name) == "pipe" else 1.0)  # (pipe: no lever about the axis)
        query.append(c + rng.uniform(-0.03, 0.03) * n + rng.uniform(-0.02, 0.02) * u + jv * v)
    local, query = np.array(local), np.array(query)
    map_xyz = (local @ Rg.T + tg).astype(np.float32)
    src = query.astype(np.float32)
    n_designed = len(src)
    if family_of(name) == "few":  # the rest of the cloud sees nothing
        far = np.stack([40.0 + 0.25 * np.arange(200 - n_designed), np.full(200 - n_designed, 40.0), np.full(200 - n_designed, 40.0)], 1)
        src = np.concatenate([src, far.astype(np.float32)])
    # the five nearest map points of every designed query are its own cluster, with room to spare
    q = src[:n_designed].astype(np.float64) @ Rg.T + tg
    m64 = map_xyz.astype(np.float64)
    d = np.sqrt(np.maximum((q * q).sum(1)[:, None] + (m64 * m64).sum(1)[None, :] - 2.0 * q @ m64.T, 0.0))  # (good to 1e-6 m at 100 m)
    order = np.argsort(d, axis=1)[:, :6]
    assert np.array_equal(np.sort(order[:, :5], axis=1), 5 * np.arange(n_designed)[:, None] + np.arange(5)[None, :])
    if d.shape[1] > 5:
        assert np.all(np.take_along_axis(d, order[:, 5:6], 1) - np.take_along_axis(d, order[:, 4:5], 1) >= 0.1)
    if n_designed < len(src):
        qf = src[n_designed:].astype(np.float64) @ Rg.T + tg
        assert np.linalg.norm(m64[None] - qf[:, None], axis=2).min() > 10.0
    vox = np.floor(map_xyz.astype(np.float64) / MAP_KW["leaf"]).astype(np.int64)
    assert np.unique(vox, axis=0, return_counts=True)[1].max() <= synth.MAX_PTS_PER_VOXEL
    if pose == "axis":
        assert np.array_equal(map_xyz.astype(np.float64), local) or family_of(name) in ("pipe", "near_parallel", "few")
    pts = np.zeros(len(src), synth.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = src[:, 0], src[:, 1], src[:, 2]
    pts["intensity"] = 100.0
    pts["idx"] = np.arange(len(src), dtype=np.uint32)
    pts["range"] = np.sqrt(src[:, 0] ** 2 + src[:, 1] ** 2 + src[:, 2] ** 2)
    for a in (map_xyz, pts):
        a.setflags(write=False)
    return SimpleNamespace(name=name, pose=pose, family=family_of(name), map_xyz=map_xyz, pts=pts, R=Rg.copy(), t=tg.copy(), n_designed=n_designed)


def binary_poses(scene):
    """(R_src, t_src, R_tgt, t_tgt) with T_tgt^-1 T_src == (scene.R, scene.t) exactly."""
    R_src, t_src = R_TGT @ scene.R, R_TGT @ scene.t + T_TGT
    assert np.array_equal(R_TGT.T @ R_src, scene.R) and np.array_equal(R_TGT.T @ (t_src - T_TGT), scene.t)
    return R_src, t_src, R_TGT, T_TGT


def tiled_points(scene):
    pts = np.tile(scene.pts, TILES)
    pts["idx"] = np.arange(len(pts), dtype=np.uint32)
    assert len(pts) > 65536
    return pts


# ---- reference ----

_REF = {}


def blocks_of(res):
    H = np.asarray(res["H_ss"], np.float64).reshape(6, 6)
    return {"rot": H[:3, :3].copy(), "trans": H[3:, 3:].copy()}


def reference(A):
    """mp.eigsy of the block read as exact numbers -> lam (mpf, ascending), vec (mp matrix, columns), scale |A| (float),
    rel (float lam / |A|), clusters (lists of indices)."""
    A = np.ascontiguousarray(A, np.float64).reshape(3, 3)
    key = A.tobytes()
    if key in _REF:
        return _REF[key]
    assert np.all(np.isfinite(A)) and np.array_equal(A, A.T), A
    scale = float(np.abs(A).max())
    with mp.workdps(DPS):
        M = matrix(3, 3)
        for r in range(3):
            for c in range(3):
                M[r, c] = mpf(float(A[r, c]))
        if scale == 0.0:
            lam, vec = [mpf(0)] * 3, mp.eye(3)
        else:
            ev, V = mp.eigsy(M)
            idx = sorted(range(3), key=lambda a: ev[a])
            lam = [ev[a] for a in idx]
            vec = matrix(3, 3)
            for k, a in enumerate(idx):
                nn = mp.sqrt(sum(V[r, a] ** 2 for r in range(3)))
                for r in range(3):
                    vec[r, k] = V[r, a] / nn
        clusters, cur = [], [0]
        for i in (1, 2):
            if lam[i] - lam[i - 1] <= mpf(CLUSTER_GAP) * mpf(scale):
                cur.append(i)
            else:
                clusters.append(cur)
                cur = [i]
        clusters.append(cur)
        rel = [float(x / mpf(scale)) if scale > 0 else 0.0 for x in lam]
    ref = SimpleNamespace(A=A, M=M, lam=lam, vec=vec, scale=scale, rel=rel, clusters=clusters)
    _REF[key] = ref
    return ref


def rank_of(ref):
    """number of eigenvalues above the decidability bar"""
    return sum(1 for r in ref.rel if r > DECIDABLE)


# ---- checks ----

class Ratios(dict):
    """worst measured value / bar per check"""

    def add(self, name, value):
        self[name] = max(self.get(name, 0.0), float(value))

    def merge(self, other):
        for k, v in other.items():
            self.add(k, v)
        return self

    def line(self, title):
        return title + ": " + ", ".join(f"{k} {v:.2g}" for k, v in sorted(self.items()))


def check_block(A, loc, V, label="", ratios=None, eigenvalues=True):
    """Hold a reported (localizabilities, eigenvectors in columns) pair to the reference of the block A."""
    ratios = Ratios() if ratios is None else ratios
    ref = reference(A)
    loc, V = np.asarray(loc, np.float64).reshape(3), np.asarray(V, np.float64).reshape(3, 3)
    bad, s = [], ref.scale
    with mp.workdps(DPS):
        sc = mpf(s)
        if eigenvalues:
            for i in range(3):
                if np.isnan(loc[i]):
                    if not ref.lam[i] <= mpf(BAR) * sc:
                        bad.append(("NaN localizability of a decided eigenvalue", i, ref.rel[i]))
                    continue
                err = abs(mpf(float(loc[i])) ** 2 - ref.lam[i])
                if s > 0:
                    ratios.add("eigenvalue", err / (mpf(BAR) * sc))
                if not err <= mpf(BAR) * sc:
                    bad.append(("eigenvalue", i, float(err / sc) if s > 0 else float(err), ref.rel))
        if not np.all(np.isfinite(V)):
            bad.append(("eigenvectors not finite", V.tolist()))
        else:
            ortho = float(np.abs(V.T @ V - np.eye(3)).max())
            ratios.add("orthonormal", ortho / BAR_ORTHO)
            if not ortho <= BAR_ORTHO:
                bad.append(("orthonormal", ortho))
            Vm = matrix(3, 3)
            for r in range(3):
                for c in range(3):
                    Vm[r, c] = mpf(float(V[r, c]))
            for k in range(3):
                v = [Vm[r, k] for r in range(3)]
                Av = [sum(ref.M[r, c] * v[c] for c in range(3)) for r in range(3)]
                rq = sum(v[r] * Av[r] for r in range(3))
                res = max(abs(Av[r] - rq * v[r]) for r in range(3))
                if s > 0:
                    ratios.add("residual", res / (mpf(BAR) * sc))
                if not res <= mpf(BAR) * sc:
                    bad.append(("residual", k, float(res / sc) if s > 0 else float(res), ref.rel))
            for cl in ref.clusters:
                if len(cl) == 3:
                    continue
                others = [j for j in range(3) if j not in cl]
                sep = min(abs(ref.lam[i] - ref.lam[j]) for i in cl for j in others) / sc
                bound = mpf(BAR) / sep + mpf(BAR_PROJ_FLOOR)
                d2 = mpf(0)
                for r in range(3):
                    for c in range(3):
                        d2 += (sum(Vm[r, k] * Vm[c, k] for k in cl) - sum(ref.vec[r, k] * ref.vec[c, k] for k in cl)) ** 2
                d = mp.sqrt(d2)
                ratios.add("projector", d / bound)
                if not d <= bound:
                    bad.append(("projector", cl, float(d), float(bound), ref.rel))
    assert not bad, (label, bad)
    return ratios


def check_result(res, label="", ratios=None, blocks=("rot", "trans")):
    """loc_*_final and eigvec_* of a result against the reference of its own reported H_ss blocks (reg_4_dof and
    project_on_degneneracy off, or blocks they leave alone)."""
    ratios = Ratios() if ratios is None else ratios
    B = blocks_of(res)
    for name in blocks:
        check_block(B[name], res[f"loc_{name}_final"], res[f"eigvec_{name}"], f"{label} {name}", ratios)
    return ratios


def component_sums(pts, R, state, E_t, E_r):
    """The component localizabilities (geometric_factor.hpp:434-457) in fp64 from the per-point state and the given bases.
    -> (trans sums, rot sums, valid points, points with a component within NEAR_HALF of 0.5)"""
    st, _, nrm = state[:3]
    P = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64)
    v = np.asarray(st) == VALID
    ns = np.asarray(nrm)[v] @ np.asarray(R, np.float64)
    lt = -ns
    lr = np.cross(ns, P[v])
    nr = np.linalg.norm(lr, axis=1, keepdims=True)
    lr = np.where(nr > 0, lr / np.where(nr > 0, nr, 1.0), lr)
    ct, cr = np.abs(lt @ E_t), np.abs(lr @ E_r)
    near = (np.abs(ct - 0.5) <= NEAR_HALF).any(1) | (np.abs(cr - 0.5) <= NEAR_HALF).any(1)
    return np.where(ct >= 0.5, ct, 0.0).sum(0), np.where(cr >= 0.5, cr, 0.0).sum(0), int(v.sum()), int(near.sum())


def check_components(res, pts, R, state, label="", ratios=None):
    """loc_*_comp of a result against the sums recomputed from state() and the bases the result reports."""
    ratios = Ratios() if ratios is None else ratios
    ct, cr, n, nb = component_sums(pts, R, state, np.asarray(res["eigvec_trans"], float).reshape(3, 3), np.asarray(res["eigvec_rot"], float).reshape(3, 3))
    assert nb <= NB_MAX, (label, "points with a component at 0.5", nb)
    bound = 0.5 * nb + 1e-9 * n
    for name, want in (("trans", ct), ("rot", cr)):
        d = float(np.abs(want - np.asarray(res[f"loc_{name}_comp"], float)).max()) if n else float(np.abs(np.asarray(res[f"loc_{name}_comp"], float)).max())
        if n:
            ratios.add("components", d / bound)
        assert d <= bound, (label, name, want.tolist(), np.asarray(res[f"loc_{name}_comp"]).tolist(), nb, n)
    return ratios


def _f32_sides(s):
    """the float32 values on either side of the mpf s: (largest <= s, smallest > s)"""
    f = np.float32(float(s))
    if mpf(float(f)) > s:
        return float(np.nextafter(f, np.float32(-np.inf))), float(f)
    return float(f), float(np.nextafter(f, np.float32(np.inf)))


def thresholds(A):
    """-> (kept, dropped, placed_at): kept = [(threshold as float32 value, expected degenerate)], placed at the block's smallest
    decided eigenvalue (its index, or None where no eigenvalue is decided); expectation and decidability from the reference alone."""
    ref = reference(A)
    with mp.workdps(DPS):
        bar = mpf(DECIDABLE) * mpf(ref.scale)
        for p in range(3):
            if ref.lam[p] <= 0:
                continue
            s = mp.sqrt(ref.lam[p])
            lo, hi = _f32_sides(s)
            if lo > 0 and all(abs(mpf(t) ** 2 - ref.lam[p]) >= bar for t in (lo, hi)):
                break
        else:
            return [], 4, None
        cands = [lo, hi, float(np.float32(float(s * (1 - mpf(1e-3))))), float(np.float32(float(s * (1 + mpf(1e-3)))))]
        kept = [(t, not ref.lam[0] > mpf(t) ** 2) for t in cands if all(abs(mpf(t) ** 2 - l) >= bar for l in ref.lam)]
    return kept, 4 - len(kept), p


def decision(A, t):
    """-> (decidable, degenerate) of the block A at the threshold t, from the reference alone"""
    ref = reference(A)
    with mp.workdps(DPS):
        bar = mpf(DECIDABLE) * mpf(ref.scale)
        return all(abs(mpf(t) ** 2 - l) >= bar for l in ref.lam), not ref.lam[0] > mpf(t) ** 2


def never_degenerate(A):
    """True where the block compares as not degenerate at the threshold -1 (no localizability may be NaN), False where it may
    compare either way (a rounding-level eigenvalue)."""
    ref = reference(A)
    return ref.scale > 0 and ref.rel[0] > BAR


def check_reg4(plain, reg, R, g_unit, label="", ratios=None):
    """H_ss, b_s of a reg_4_dof call against the projection of the unprojected call's, computed in mpmath."""
    ratios = Ratios() if ratios is None else ratios
    H, b = np.asarray(plain["H_ss"], float).reshape(6, 6), np.asarray(plain["b_s"], float)
    Hg, bg = np.asarray(reg["H_ss"], float).reshape(6, 6), np.asarray(reg["b_s"], float)
    R, g = np.asarray(R, float).reshape(3, 3), np.asarray(g_unit, float)
    with mp.workdps(DPS):
        lz = [sum(mpf(float(R[j, i])) * mpf(float(-g[j])) for j in range(3)) for i in range(3)]
        Pi = [[lz[r] * lz[c] for c in range(3)] for r in range(3)]
        Hm = [[mpf(float(H[r, c])) for c in range(6)] for r in range(6)]
        mul = lambda A_, B_: [[sum(A_[r][k] * B_[k][c] for k in range(3)) for c in range(3)] for r in range(3)]  # noqa: E731
        blk = lambda r0, c0: [[Hm[r0 + r][c0 + c] for c in range(3)] for r in range(3)]  # noqa: E731
        want = {(0, 0): mul(mul(Pi, blk(0, 0)), Pi), (0, 3): mul(Pi, blk(0, 3)), (3, 0): mul(blk(3, 0), Pi), (3, 3): blk(3, 3)}
        bad = []
        for (r0, c0), W in want.items():
            scale = float(np.abs(H[r0:r0 + 3, c0:c0 + 3]).max())
            err = max(abs(mpf(float(Hg[r0 + r, c0 + c])) - W[r][c]) for r in range(3) for c in range(3))
            if scale > 0:
                ratios.add("reg_4_dof", err / (mpf(BAR_REG4) * mpf(scale)))
            if not err <= mpf(BAR_REG4) * mpf(scale):
                bad.append(("H", r0, c0, float(err), scale))
        bw = [sum(Pi[r][c] * mpf(float(b[c])) for c in range(3)) for r in range(3)] + [mpf(float(x)) for x in b[3:]]
        scale = float(np.abs(b[:3]).max())
        err = max(abs(mpf(float(bg[r])) - bw[r]) for r in range(3))
        if scale > 0:
            ratios.add("reg_4_dof", err / (mpf(BAR_REG4) * mpf(scale)))
        if not err <= mpf(BAR_REG4) * mpf(scale) or not np.array_equal(bg[3:], b[3:]):
            bad.append(("b", float(err), scale))
    assert not bad, (label, bad)
    # the localizabilities and bases are those of the unprojected sums
    for k in ("loc_rot_final", "loc_trans_final", "eigvec_rot", "eigvec_trans"):
        assert np.array_equal(np.asarray(reg[k]), np.asarray(plain[k]), equal_nan=True), (label, k)
    return ratios


def is_zero_result(res):
    return not np.any(np.asarray(res["H_ss"])) and not np.any(np.asarray(res["b_s"]))


def check_zero_localizabilities(res, label=""):
    """after the degeneracy projection zeroed H: the localizabilities and bases are those of the zero matrix"""
    for name in ("rot", "trans"):
        assert np.array_equal(np.asarray(res[f"loc_{name}_final"], float), np.zeros(3)), (label, name, res[f"loc_{name}_final"])
        check_block(np.zeros((3, 3)), res[f"loc_{name}_final"], res[f"eigvec_{name}"], f"{label} {name} zero")


def describe(name, pose, res):
    """one line per case: spectrum, clusters, thresholds kept, for the test output"""
    out = []
    for blk, A in blocks_of(res).items():
        ref = reference(A)
        kept, dropped, p = thresholds(A)
        out.append(f"{blk}: |A| {ref.scale:.3g} lambda/|A| [{', '.join(f'{r:.3g}' for r in ref.rel)}] clusters {ref.clusters} rank {rank_of(ref)} "
                   f"thresholds kept {len(kept)} at {p} ({sum(1 for _, d in kept if d)} degenerate)")
    return f"[degeneracy-zoo] {name} {pose}: " + "; ".join(out)


# what a family is built to show: (rank of the translation block, rank of the rotation block) by the decidability bar, None where
# the float32 rounding of the scene decides it
INTENDED_RANK_AXIS = {"floor": (1, 2), "slab": (1, 2), "tunnel": (2, 3), "tunnel_end": (3, 3), "pipe": (2, 2), "square_tunnel": (2, 3),
                      "cube_centre": (3, 3)}
