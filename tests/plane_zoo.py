"""A "neighbourhood zoo" for the per-point plane stage of ICPFactor::linearize (K3 in icp_kernels.hip: k-NN selection, mean and
covariance of the k neighbours, plane_eigen / null_vector3, the gates, the normal's sign), and its multi-precision reference.

A zoo is a map of isolated, designed clusters on a 2 m lattice (leaf 0.5, inserted with min_dist 0) and one scan point per
cluster.  Every point's status, mean and normal is held to a reference computed with mpmath at 60 digits from the exact float32
coordinates that went into the map and the cloud: candidates by voxel offset, the k nearest by exact squared distance, mean,
covariance / (k - 1), mp.eigsy, the gates in the order of geometric_factor.hpp:176-229, 319-328, the sign from n.(t - mean).
Pure numpy + mpmath: the same checks run on the CPU oracle (test_plane_zoo_cpu.py) and on the device (test_gpu_plane_zoo.py).

One zoo = (k, neighbour mode, coordinate offset): 176 cases; the nine k = 5 zoos (modes 7 / 19 / 27 x offsets 0 / 100 / 1000 m)
hold 1584 cases, the k = 8 (mode 27) and k = 4 (mode 7) zoos 528 each.  A cluster is a zero-mean k x 3 design Z with
Z'Z / (k - 1) = I, scaled by sqrt(w), rotated by a random Q, moved to its centre and rounded to float32; the reference
recomputes the true spectrum from the rounded points, the design only aims it (families that sit next to a gate are re-scaled
a few times and nudged by single float32 ulps towards their target).  Families (FAMILIES), each with the cluster centred in a
voxel, on a face, on an edge and on a corner (neighbours from up to eight voxels; a cluster that spills into a voxel the mode
does not visit must come out as the reference says, status 1 included):
  valid       w0 2e-6..5e-4, w1 3e-3..3e-2, w2/w1 1.05..2.8; eight further cases with w1 1e-2..3e-2, w2/w1 1.05..1.6, whose normal
              is known to 1e-12 at offset 0 (rows of the sums test)
  pair        w0 = w1 (1 - 10^u), u -6..-0.5, every third case with w1 = 1.3..1.5 w0 (just outside the kernel's 25 % trigger);
              sixteen further cases with w2 = 1.0..1.1 w1 as well, eight at w1 = 1.335..1.375 w0 and eight at 1.3..1.5 w0: three
              eigenvalues of one size with the pair just past the trigger is where Newton on the cubic is slowest among the
              lanes that get no refinement (eight steps from 0 ended up to 6e-8 |A| short there: normals up to 18 nb off in
              17 of these cases, by a host emulation of the kernel as it was; fixed in plane_eigen)
  iso         three eigenvalues within 10^u of each other, u -9..-3
  low         w0 = 1e-6 (1 +- 10^u), u -7..-1
  line        w2 = 3 w1 (1 +- 10^u), u -6..-1
  gate        largest |X_j.n| = plane_validity_distance (1 +- 10^u), u -7..-1.5
  maxerr      range 0.5..2 m, the query displaced along the normal to 9 |e| = sqrt(range) (1 +- 10^u), u -4..-1
  flat        points on an exact float32 plane (w0 = 0); collinear: on a line; duplicates: k identical points
  few         k - 1 points (status 1)
  far         own config, max_corres_distance 0.3: the k-th squared distance at 0.09 (1 +- 10^u), u -6..-1
  crowd       8 / 12 / 20 points (12 / 16 / 20 for k = 8): the k nearest a designed cluster, the others on a shell whose squared
              distance exceeds the k-th by >= 1e-3 relative (survivor / member mask, the 20-point cap)
pair and iso are sized so that every neighbour is nearer to the mean than plane_validity_distance: their status does not hang
on a normal that the data do not determine.

Ambiguity.  delta = 16 eps (|mean|_inf sqrt(w2) + w2), eps = 2^-53: the first-order size of the float64 centring and covariance
round-off on float32 inputs.  nb = 4 delta / (w1 - w0) + 8 eps is the normal's bound (eigenvector perturbation,
|dv| <= |dA| / gap, a backward-stable solver allowed a few eps |A|).  A case is ambiguous when, on the way the reference takes
through the gates, a quantity lies within its margin of the threshold: |w0 - 1e-6| <= delta; |w2 - 3 w1| <= 4 delta (both sides
move); the k-th squared distance within 16 eps (|q|_inf d + d^2) of max_corres_distance^2; | |X_j.n| - pvd | <= 1e-9 pvd +
|X_j| nb; | 9 |e| - sqrt(range) | <= 1e-6 sqrt(range) + 9 |mean - q| nb (the |.| nb terms: the quantity moves with the normal,
which is only known to nb; where nb > 1e-3 the normal is not determined and the gate counts as decided only if it comes out
the same for every unit normal); |n.(t - mean)| < 1e-9 + |t - mean| nb.  Ambiguous cases are dropped from the status, normal and
sign checks and from no other.  At most 1 % of a zoo may be ambiguous and none in valid, pair or iso: build() asserts it.
These margins are wider than the bare "within delta of the threshold": 4 delta at the line gate, the |.| nb terms, and the margin
at the k-th distance.  No zoo has an ambiguous case, so they drop nothing today.  At a moved pose (the warm test) a query may
come within the face margin, or the k-th place may tie; such a case (knn_open) leaves every check at that pose, and reference()
asserts that they are at most 1 % of the zoo.

Bounds.  Status: exact.  Mean: |mean - ref| <= 4 eps |mean|_inf (a sum of k <= 8 float32 values in double is exact; 1 / k and
the product round).  Normal, status >= 6: |n - ref|_inf <= nb; where nb > 1e-3 only status and mean are checked (a fixed rule of
the zoo).  On a cold factor statuses 1, 2, 4 and 5 leave a zero normal, 1 and 2 a zero mean as well.

Measured worst error / bound per family (k = 5, all nine zoos; normal | mean), oracle (oracle/ref_cpu.hpp, float64 Jacobi):
  valid 0.0019|0.5, pair 8.5e-05|0.5, iso 0.00033|0.47, low 0.0011|0.5, line 0.00019|0.48, gate 0.0013|0.4, maxerr 0.00015|0.33,
  flat -|0.47, collinear -|0.5, far 0.00014|0.47, crowd 0.00029|0.4 (k = 8: normal <= 0.0015, k = 4: <= 0.0016; their means are exact:
  1 / k is a power of two).  The factor 4 in nb leaves three orders of magnitude of room; the mean's 4 eps is tight (two roundings).
The device's figures are in DESIGN.md ("Plane stage against a multi-precision reference").
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
from mpmath import matrix, mp, mpf

from mimosa_amd import synth

DPS = 60
LEAF = 0.5
PITCH = 2.0
SIDE = 6                      # lattice sites per axis: 216 sites, 176 used
EPS = 2.0 ** -53
FACE_MARGIN = 1e-4
KNN_MARGIN = 1e-9             # relative gap between the k-th and the (k+1)-th squared distance below which the set is not decided
NORMAL_DETERMINED = 1e-3
PVD = float(np.float32(0.07))                          # plane_validity_distance as the factor reads it
MAX_D2 = {False: float(np.float32(1.0) * np.float32(1.0)), True: float(np.float32(0.3) * np.float32(0.3))}  # float product, then double
FAMILIES = ("valid", "pair", "iso", "low", "line", "gate", "maxerr", "flat", "collinear", "duplicates", "few", "far", "crowd")
PLACEMENTS = ("centre", "face", "edge", "corner")
REPS = 3
EXTRA_REPS = {"pair": 4, "valid": 2}                   # further cases of a family, appended to the zoo (see the docstring)
N_CASES = (len(FAMILIES) * REPS - 1) * len(PLACEMENTS) + sum(EXTRA_REPS.values()) * len(PLACEMENTS)  # maxerr has two repetitions
OFFSETS_M = (0.0, 100.0, 1000.0)
K5_ZOOS = tuple((5, mode, off) for mode in (7, 19, 27) for off in OFFSETS_M)
K8_ZOOS = tuple((8, 27, off) for off in OFFSETS_M)
K4_ZOOS = tuple((4, 7, off) for off in OFFSETS_M)
R_ZOO = synth.so3_exp(np.array([0.4, -0.7, 0.9]))
POSE_STEP = np.array([0.6, -0.64, 0.48])               # unit vector: poses 1 / 2 move t by 0.01 / 0.1 m along it
POSE_MOVES = (0.0, 0.01, 0.1)
# binary factor: a target pose whose composition with (R_ZOO, t) and back is exact in float64 (entries 0 / +-1, dyadic translations)
R_TGT = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
T_TGT = np.array([0.5, -0.25, 1.0])


def neighbour_offsets(mode):
    o = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    if mode == 7:
        return [c for c in o if abs(c[0]) + abs(c[1]) + abs(c[2]) <= 1]
    if mode == 19:
        return [c for c in o if abs(c[0]) + abs(c[1]) + abs(c[2]) <= 2]
    assert mode == 27
    return o


def config(k, far=False, warm=False, huber=1):
    """enwide's scan_to_map block; the factor's own min_dist 0 (every call re-associates) unless `warm` (0.15: threshold 0.0375 m)."""
    return dict(synth.enwide_config(), num_corres_points=k, max_corres_distance=0.3 if far else 1.0,
                target_ivox_map_min_dist_in_voxel=0.15 if warm else 0.0, use_huber=huber)


def pose(zoo, which=0):
    return zoo.R, zoo.t + POSE_MOVES[which] * POSE_STEP


def binary_poses(zoo, which=0):
    """(R_src, t_src, R_tgt, t_tgt) with T_tgt^-1 T_src == pose(zoo, 0) exactly."""
    assert which == 0
    R_src, t_src = R_TGT @ zoo.R, R_TGT @ zoo.t + T_TGT
    assert np.array_equal(R_TGT.T @ R_src, zoo.R) and np.array_equal(R_TGT.T @ (t_src - T_TGT), zoo.t)
    return R_src, t_src, R_TGT, T_TGT


def _face_ok(x):
    u = np.asarray(x, np.float64) / LEAF
    return bool(np.all(np.abs(u - np.round(u)) * LEAF >= FACE_MARGIN))


def _design(rng, k):
    A = rng.standard_normal((k, 3))
    A -= A.mean(0)
    U, _ = np.linalg.qr(A)
    return U * np.sqrt(k - 1.0)


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    return Q


def _spectrum(P32):
    X = P32.astype(np.float64)
    m = X.mean(0)
    Xc = X - m
    w, V = np.linalg.eigh(Xc.T @ Xc / (len(X) - 1.0))
    return m, w, V, Xc


def _cluster(centre, Z, w, Q):
    return (centre + (Z * np.sqrt(w)) @ Q.T).astype(np.float32)


def _aim(rng, centre, Z, w, Q, axis, measure, goal, power):
    """Re-scale w[axis] until measure(points) ~ goal, then take single-ulp moves of single coordinates that bring it nearer."""
    w = np.array(w, np.float64)
    for _ in range(6):
        w[axis] *= (goal / measure(_cluster(centre, Z, w, Q))) ** power
    P = _cluster(centre, Z, w, Q)
    best = abs(measure(P) / goal - 1.0)
    for _ in range(48):
        T = P.copy()
        i, c = rng.integers(len(P)), rng.integers(3)
        T[i, c] = np.nextafter(T[i, c], np.float32(np.inf if rng.random() < 0.5 else -np.inf))
        e = abs(measure(T) / goal - 1.0)
        if e < best:
            P, best = T, e
    return P


def _logu(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _near(rng, lo, hi):
    """1 +- 10^u, u uniform in lo..hi."""
    return 1.0 + (1.0 if rng.random() < 0.5 else -1.0) * 10.0 ** rng.uniform(lo, hi)


def _source(q, R, t):
    """float32 source point whose image R p + t is (nearly) q, and that image in float64."""
    p = (R.T @ (q - t)).astype(np.float32)
    return p, R @ p.astype(np.float64) + t


def _make_case(rng, fam, rep, k, centre, R, t):
    """-> (map points float32 (n, 3), source point float32 (3,)) of one case, or None where a draw has to be repeated."""
    Z, Q = _design(rng, k), _rotation(rng)
    w2max = 4e-3 / (k - 1.0)  # every |X_j| <= sqrt(w2 (k - 1)) < 0.0633 < plane_validity_distance: pair, iso
    qn, qr = 0.005 * rng.uniform(-1, 1), 0.02  # the query's offset from the centre: along the normal, in the plane
    if fam == "valid" and rep % 3 == 1:
        qn = rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 0.14)  # |e| / sigma > the Huber threshold, 9 |e| still below sqrt(range >= 2.5 m)
    n_map = k
    if fam == "valid" or fam == "maxerr" or fam == "few":
        w = [_logu(rng, 2e-6, 5e-4), _logu(rng, 3e-3, 3e-2), 0.0]
        if fam == "maxerr":
            w = [_logu(rng, 2e-6, 5e-5), _logu(rng, 3e-4, 1e-3), 0.0]  # a small cluster: the displaced query keeps it in reach
        w[2] = w[1] * rng.uniform(1.05, 2.8)
        if fam == "valid" and rep >= REPS:  # well-conditioned: the normal known to 1e-12 at offset 0 (the rows of the sums test)
            w[1] = _logu(rng, 1e-2, 3e-2)
            w[2] = w[1] * rng.uniform(1.05, 1.6)
        P = _cluster(centre, Z, w, Q)
        if fam == "few":
            P = P[: k - 1]
    elif fam == "pair":
        w1 = _logu(rng, w2max / 2.8 / 30.0, w2max / 2.8)
        w0 = w1 / rng.uniform(1.3, 1.5) if rep % 3 == 2 else w1 * (1.0 - 10.0 ** rng.uniform(-6.0, -0.5))
        w2 = w1 * rng.uniform(1.05, 2.8)
        if rep >= REPS:  # the band past the trigger with w2 next to w1 as well, where Newton on the cubic is slowest outside it
            w0 = w1 / (rng.uniform(1.335, 1.375) if rep < REPS + 2 else rng.uniform(1.3, 1.5))
            w2 = w1 * rng.uniform(1.0, 1.1)
        P = _cluster(centre, Z, [w0, w1, w2], Q)
    elif fam == "iso":
        w0, r = _logu(rng, w2max / 30.0, w2max / 1.01), 10.0 ** rng.uniform(-9.0, -3.0)
        P = _cluster(centre, Z, [w0, w0 * (1.0 + 0.5 * r), w0 * (1.0 + r)], Q)
    elif fam == "low":
        w1 = _logu(rng, 3e-3, 3e-2)
        P = _aim(rng, centre, Z, [1e-6, w1, w1 * rng.uniform(1.05, 2.8)], Q, 0, lambda T: _spectrum(T)[1][0], 1e-6 * _near(rng, -7.0, -1.0), 1.0)
    elif fam == "line":
        w1 = _logu(rng, 1e-3, 5e-3)

        def ratio(T):
            s = _spectrum(T)[1]
            return s[2] / (3.0 * s[1])
        P = _aim(rng, centre, Z, [_logu(rng, 2e-6, 2e-4), w1, 3.0 * w1], Q, 2, ratio, _near(rng, -6.0, -1.0), 1.0)
    elif fam == "gate":
        w1 = _logu(rng, 1e-2, 3e-2)

        def reach(T):
            _, _, V, Xc = _spectrum(T)
            return np.abs(Xc @ V[:, 0]).max()
        P = _aim(rng, centre, Z, [(PVD / np.abs(Z[:, 0]).max()) ** 2, w1, w1 * rng.uniform(1.05, 2.8)], Q, 0, reach, PVD * _near(rng, -7.0, -1.5), 2.0)
    elif fam == "flat" or fam == "collinear":
        c = np.round(centre * 1024.0) + np.array([3.0, 5.0, 7.0])
        if fam == "flat":
            a, b = rng.integers(-200, 201, k).astype(np.float64), rng.integers(-200, 201, k).astype(np.float64)
            G = [np.stack([a, b, 0 * a], 1), np.stack([a, -a, b], 1), np.stack([a, b, -a - b], 1)][rep % 3]  # z = c, x + y = c, x + y + z = c
            P = ((c + G) / 1024.0).astype(np.float32)
            assert np.array_equal(P.astype(np.float64) * 1024.0, c + G)  # exactly on the plane
            if np.linalg.matrix_rank(G - G.mean(0)) < 2:
                return None
        elif rep % 2 == 0:
            s = rng.permutation(np.arange(-60, 61))[:k].astype(np.float64)
            G = s[:, None] * np.array([3.0, -2.0, 1.0])
            P = ((c + G) / 1024.0).astype(np.float32)
            assert np.array_equal(P.astype(np.float64) * 1024.0, c + G)  # exactly on the line
        else:
            P = (centre + rng.uniform(-0.25, 0.25, k)[:, None] * Q[:, 1]).astype(np.float32)  # on a line up to float32 rounding
    elif fam == "duplicates":
        P = np.repeat((centre + 0.01 * rng.uniform(-1, 1, 3)).astype(np.float32)[None], k, 0)
    elif fam == "far" or fam == "crowd":
        w = [_logu(rng, 2e-6, 2e-5), _logu(rng, 2e-4, 6e-4), 0.0]
        w[2] = w[1] * rng.uniform(1.05, 2.8)
        P = _cluster(centre, Z, w, Q)
    else:
        raise AssertionError(fam)

    m, _, V, _ = _spectrum(P) if len(P) >= 4 and fam not in ("duplicates",) else (P.astype(np.float64).mean(0), None, Q, None)
    a = rng.uniform(0, 2 * np.pi)
    inplane = np.cos(a) * V[:, 1] + np.sin(a) * V[:, 2]
    q = m + qn * V[:, 0] + qr * rng.uniform(0.2, 1.0) * inplane
    p, qa = _source(q, R, t)
    if fam == "maxerr":
        goal, side = _near(rng, -4.0, -1.0), (1.0 if rng.random() < 0.5 else -1.0)
        d = 0.12
        for _ in range(8):  # 9 |e| = sqrt(|p|) * goal, |p| moving with the query
            p, qa = _source(m + side * d * V[:, 0] + 0.01 * inplane, R, t)
            e = abs(V[:, 0] @ (m - qa))
            d *= np.sqrt(np.linalg.norm(p.astype(np.float64))) * goal / (9.0 * e)
        if not 0.5 <= np.linalg.norm(p.astype(np.float64)) <= 2.0:
            return None
    if fam == "far":
        goal, d = MAX_D2[True] * _near(rng, -6.0, -1.0), 0.3
        for _ in range(8):  # the k-th squared distance = goal
            p, qa = _source(m + qn * V[:, 0] + d * inplane, R, t)
            dk = np.sort(((P.astype(np.float64) - qa) ** 2).sum(1))[k - 1]
            d += (goal - dk) / (2.0 * np.sqrt(dk))
    if fam == "crowd":
        total = ((8, 12, 20) if k <= 5 else (12, 16, 20))[rep % 3]
        dk = np.sort(((P.astype(np.float64) - qa) ** 2).sum(1))[k - 1]
        extra = []
        while len(extra) < total - k:
            u = rng.standard_normal(3)
            u /= np.linalg.norm(u)
            grow = 1.0 + 1e-3 + 10.0 ** rng.uniform(-3.0, 0.0)
            while True:
                x = (qa + np.sqrt(dk * grow) * u).astype(np.float32)
                if ((x.astype(np.float64) - qa) ** 2).sum() >= dk * (1.0 + 1.5e-3):
                    break
                grow *= 1.0 + 1e-3
            extra.append(x)
        P = np.concatenate([P, np.array(extra, np.float32)])
        P = P[rng.permutation(len(P))]
    if not (_face_ok(P) and _face_ok(qa)):
        return None
    return P, p


@functools.lru_cache(maxsize=None)
def build(k, mode, offset):
    """The zoo of (k, mode, offset): map, cloud, cases.  Asserts the layout rules (face margins, isolation, ambiguity cap)."""
    rng = np.random.default_rng([20261, k, mode, int(offset)])
    base = np.array([-6.0 + offset, -4.0 - offset, 2.0 + offset])
    t = np.round((base + np.array([5.13, 4.79, 5.17])) * 1024.0) / 1024.0  # inside the lattice; dyadic (binary_poses)
    R = R_ZOO
    sites = base + PITCH * np.array([(i, j, l) for i in range(SIDE) for j in range(SIDE) for l in range(SIDE)], np.float64)
    order = np.argsort(np.linalg.norm(sites - t, axis=1), kind="stable")
    near, rest = list(order[:8]), list(rng.permutation(order[8:]))
    shifts = {"centre": (0.25, 0.25, 0.25), "face": (0.0, 0.25, 0.25), "edge": (0.0, 0.0, 0.25), "corner": (0.0, 0.0, 0.0)}
    fam_i, place_i, far, src, owner, chunks, centres = [], [], [], [], [], [], []
    specs = [(fam, place, rep) for fam in FAMILIES for place in PLACEMENTS for rep in range(2 if fam == "maxerr" else REPS)]
    specs += [(fam, place, REPS + rep) for fam, extra in EXTRA_REPS.items() for place in PLACEMENTS for rep in range(extra)]
    for fam, place, rep in specs:
        fi, pi = FAMILIES.index(fam), PLACEMENTS.index(place)
        site = sites[near.pop() if fam == "maxerr" else rest.pop()]
        for _ in range(400):
            sh = np.array(shifts[place])[rng.permutation(3)]
            sh = sh * (np.sign(t - site) if fam == "maxerr" else rng.choice([-1.0, 1.0], 3))  # maxerr: towards the sensor (range <= 2 m)
            made = _make_case(rng, fam, rep, k, site + sh, R, t)
            if made is not None:
                break
        else:
            raise AssertionError(("no admissible draw", fam, place, rep))
        owner += [len(src)] * len(made[0])
        chunks.append(made[0])
        centres.append(site + sh)
        src.append(made[1])
        fam_i.append(fi)
        place_i.append(pi)
        far.append(fam == "far")
    assert len(src) == N_CASES
    map_xyz = np.concatenate(chunks).astype(np.float32)
    src = np.array(src, np.float32)
    n = len(src)
    pts = np.zeros(n, synth.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = src[:, 0], src[:, 1], src[:, 2]
    pts["intensity"] = 100.0
    pts["idx"] = np.arange(n, dtype=np.uint32)
    pts["range"] = np.sqrt(src[:, 0] ** 2 + src[:, 1] ** 2 + src[:, 2] ** 2)
    zoo = SimpleNamespace(k=k, mode=mode, offset=offset, R=R, t=t, map_xyz=map_xyz, src=src, pts=pts, n=n, owner=np.array(owner),
                          family=np.array(fam_i), placement=np.array(place_i), far=np.array(far), centres=np.array(centres))
    zoo.clouds = {name: np.flatnonzero(zoo.far == f) for name, f in (("main", False), ("far", True))}
    # layout rules: face margins, and no map point in the 27-voxel neighbourhood of another cluster's query (at any of the three poses)
    assert _face_ok(map_xyz)
    vox = np.floor(map_xyz.astype(np.float64) / LEAF).astype(np.int64)
    for which in range(3):
        Rw, tw = pose(zoo, which)
        q = src.astype(np.float64) @ Rw.T + tw
        assert which > 0 or _face_ok(q)
        qv = np.floor(q / LEAF).astype(np.int64)
        cheb = np.abs(vox[:, None, :] - qv[None, :, :]).max(2)
        cheb[np.arange(len(vox)), zoo.owner] = 9
        assert cheb.min() >= 2, "clusters are not isolated"
        assert np.all(np.abs(q).max(1) > 1.0)  # no query at the zero a fresh factor's cached pose reads as
    # per-voxel cap: every map point must survive the insert
    _, counts = np.unique(vox, axis=0, return_counts=True)
    assert counts.max() <= synth.MAX_PTS_PER_VOXEL
    with mp.workdps(DPS):
        ref = zoo.ref0 = _freeze(_reference(zoo, 0))
    assert not ref.knn_open.any()
    amb = ref.ambiguous
    assert amb.sum() <= 0.01 * n, ("more than 1 % ambiguous", int(amb.sum()), n)
    for fam in ("valid", "pair", "iso"):
        assert not amb[zoo.family == FAMILIES.index(fam)].any(), fam
    return zoo


def _mpv(a):
    return [mpf(float(x)) for x in a]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _freeze(ref):
    for a in vars(ref).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(k, mode, offset, which=0):
    """The multi-precision answer for every case of the zoo at pose `which`: status, mean, normal (float64 arrays, and the mp values
    in mp_mean / mp_normal), eigenvalues w, delta, the normal's bound nb, `ambiguous`, `knn_open` (the k nearest are not decided: a
    query within the face margin at a moved pose, or a tie at the k-th place), e and range of the max-error gate."""
    zoo = build(k, mode, offset)
    if which == 0:
        return zoo.ref0
    with mp.workdps(DPS):
        ref = _freeze(_reference(zoo, which))
    # a moved pose may put a query within the face margin (about one in a thousand does): such cases leave every check there
    assert ref.knn_open.sum() <= 0.01 * zoo.n, ("more than 1 % of the cases are open at a moved pose", int(ref.knn_open.sum()), zoo.n)
    return ref


def _reference(zoo, which):
    k, n = zoo.k, zoo.n
    Rw, tw = pose(zoo, which)
    Rm, tm = [_mpv(r) for r in Rw], _mpv(tw)
    X = [_mpv(x) for x in zoo.map_xyz]
    cells = {}
    for j, c in enumerate(np.floor(zoo.map_xyz.astype(np.float64) / LEAF).astype(np.int64)):
        cells.setdefault(tuple(c), []).append(j)
    offs = neighbour_offsets(zoo.mode)
    status = np.zeros(n, np.int32)
    mean, normal, w = np.zeros((n, 3)), np.zeros((n, 3)), np.full((n, 3), np.nan)
    delta, nb = np.full(n, np.nan), np.full(n, np.nan)
    ambiguous, knn_open = np.zeros(n, bool), np.zeros(n, bool)
    e_out, range_out = np.full(n, np.nan), np.zeros(n)
    mp_mean, mp_normal, mp_q = [None] * n, [None] * n, [None] * n
    pvd, eps = mpf(PVD), mpf(EPS)
    for i in range(n):
        p = _mpv(zoo.src[i])
        q = [_dot(Rm[r], p) + tm[r] for r in range(3)]
        mp_q[i] = q
        qf = np.array([float(x) for x in q])
        rng_ = mp.sqrt(_dot(p, p))
        range_out[i] = float(rng_)
        if not _face_ok(qf):
            knn_open[i] = True
            continue
        c = np.floor(qf / LEAF).astype(np.int64)
        cand = [j for o in offs for j in cells.get((c[0] + o[0], c[1] + o[1], c[2] + o[2]), ())]
        d2 = sorted(((sum((X[j][a] - q[a]) ** 2 for a in range(3)), j) for j in cand), key=lambda v: v[0])
        if len(d2) < k:
            status[i] = 1
            continue
        if len(d2) > k and d2[k][0] - d2[k - 1][0] <= KNN_MARGIN * d2[k - 1][0] and X[d2[k][1]] != X[d2[k - 1][1]]:
            knn_open[i] = True
            continue
        dk = d2[k - 1][0]
        max_d2 = mpf(MAX_D2[bool(zoo.far[i])])
        qinf = max(abs(x) for x in q)
        if abs(dk - max_d2) <= 16 * eps * (qinf * mp.sqrt(dk) + dk):
            ambiguous[i] = True
        sel = [X[j] for _, j in d2[:k]]
        m = [sum(x[a] for x in sel) / k for a in range(3)]
        if dk > max_d2:
            status[i] = 2
            if ambiguous[i]:
                mean[i] = [float(x) for x in m]  # what the device holds if it decides the other way
                mp_mean[i] = m
            continue
        Xc = [[x[a] - m[a] for a in range(3)] for x in sel]
        A = matrix(3, 3)
        for r in range(3):
            for s in range(3):
                A[r, s] = sum(x[r] * x[s] for x in Xc) / (k - 1)
        ev, V = mp.eigsy(A)
        idx = sorted(range(3), key=lambda a: ev[a])
        w0, w1, w2 = (ev[a] for a in idx)
        nrm = [V[r, idx[0]] for r in range(3)]
        nn = mp.sqrt(_dot(nrm, nrm))
        nrm = [x / nn for x in nrm]
        mean[i] = [float(x) for x in m]
        mp_mean[i] = m
        w[i] = [float(w0), float(w1), float(w2)]
        minf = max(abs(x) for x in m)
        dl = 16 * eps * (minf * mp.sqrt(w2) + w2)
        delta[i] = float(dl)
        gap = w1 - w0
        b = 4 * dl / gap + 8 * eps if gap > 0 else mpf(2)
        nb[i] = float(min(b, mpf(2)))
        determined = b <= NORMAL_DETERMINED
        if ambiguous[i]:
            status[i] = 0  # not decided (the far gate): never compared
            continue
        if abs(w0 - mpf(1e-6)) <= dl:
            ambiguous[i] = True
        if w0 < mpf(1e-6):
            status[i] = 4
            continue
        if ambiguous[i]:
            continue
        if abs(w2 - 3 * w1) <= 4 * dl:
            ambiguous[i] = True
        if w2 > 3 * w1:
            status[i] = 5
            continue
        if ambiguous[i]:
            continue
        tmm = [tm[a] - m[a] for a in range(3)]
        s = _dot(nrm, tmm)
        if s < 0:
            nrm = [-x for x in nrm]
        normal[i] = [float(x) for x in nrm]
        mp_normal[i] = nrm
        if determined and abs(s) < mpf(1e-9) + mp.sqrt(_dot(tmm, tmm)) * b:
            ambiguous[i] = True
        invalid = False
        for x in Xc:
            dj, xn = abs(_dot(x, nrm)), mp.sqrt(_dot(x, x))
            if determined:
                if abs(dj - pvd) <= pvd * mpf(1e-9) + xn * b:
                    ambiguous[i] = True
            elif xn >= pvd * (1 - mpf(1e-9)):
                ambiguous[i] = True  # some unit normal puts this neighbour past the gate
            if dj > pvd:
                invalid = True
        if invalid:
            status[i] = 6
            continue
        if ambiguous[i]:
            status[i] = 8
            continue
        mq = [m[a] - q[a] for a in range(3)]
        e = _dot(nrm, mq)
        e_out[i] = float(e)
        sr, mqn = mp.sqrt(rng_), mp.sqrt(_dot(mq, mq))
        if determined:
            if abs(9 * abs(e) - sr) <= mpf(1e-6) * sr + 9 * mqn * b:
                ambiguous[i] = True
        elif 9 * mqn >= sr * (1 - mpf(1e-6)):
            ambiguous[i] = True
        status[i] = 7 if 9 * abs(e) > sr else 8
    return SimpleNamespace(status=status, mean=mean, normal=normal, w=w, delta=delta, nb=nb, ambiguous=ambiguous, knn_open=knn_open,
                           e=e_out, range=range_out, mp_mean=mp_mean, mp_normal=mp_normal, mp_q=mp_q)


def expected_cached(zoo, ref0):
    """Pose 1 (t moved by 0.01 m, inside the factor's 0.0375 m re-association threshold) on a factor linearized at pose 0: every
    point keeps its plane; statuses <= 6 stay, 7 / 8 re-run the max-error gate at the new query.  -> (status, undecided)."""
    _, tw = pose(zoo, 1)
    status, undecided = ref0.status.copy(), ref0.ambiguous | ref0.knn_open
    with mp.workdps(DPS):
        Rm, tm = [_mpv(r) for r in zoo.R], _mpv(tw)
        for i in np.flatnonzero((ref0.status >= 7) & ~undecided):
            p = _mpv(zoo.src[i])
            q = [_dot(Rm[r], p) + tm[r] for r in range(3)]
            mq = [ref0.mp_mean[i][a] - q[a] for a in range(3)]
            e, sr = _dot(ref0.mp_normal[i], mq), mp.sqrt(mp.sqrt(_dot(p, p)))
            b = mpf(ref0.nb[i])
            if b > NORMAL_DETERMINED:
                undecided[i] = 9 * mp.sqrt(_dot(mq, mq)) >= sr * (1 - mpf(1e-6))
            else:
                undecided[i] = abs(9 * abs(e) - sr) <= mpf(1e-6) * sr + 9 * mp.sqrt(_dot(mq, mq)) * b
            status[i] = 7 if 9 * abs(e) > sr else 8
    return status, undecided


def check_state(zoo, ref, idx, state, cold=True, label=""):
    """Hold (status, mean, normal) of the factor over the zoo's cases `idx` to the reference.  -> {family: (normal ratio, mean ratio)}."""
    st, mean, nrm = (np.asarray(a) for a in state[:3])
    assert len(st) == len(idx)
    bad, ratios = [], {}
    for j, i in enumerate(idx):
        fam = FAMILIES[zoo.family[i]]
        tag = (label, zoo.k, zoo.mode, zoo.offset, fam, PLACEMENTS[zoo.placement[i]], int(i))
        if ref.knn_open[i]:
            continue
        rs = int(ref.status[i])
        decided = not ref.ambiguous[i]
        if decided and st[j] != rs:
            bad.append((tag, "status", int(st[j]), rs))
            continue
        has_mean = rs >= 3 if decided else st[j] >= 3
        r_n = r_m = 0.0
        if has_mean:
            tol = 4.0 * EPS * np.abs(ref.mean[i]).max()
            err = np.abs(mean[j] - ref.mean[i]).max()
            r_m = err / tol
            if not err <= tol:
                bad.append((tag, "mean", err, tol))
        elif cold and not np.all(mean[j] == 0.0):
            bad.append((tag, "mean not zero", mean[j].tolist(), rs))
        if decided and rs >= 6:
            if ref.nb[i] <= NORMAL_DETERMINED:
                err = np.abs(nrm[j] - ref.normal[i]).max()
                r_n = err / ref.nb[i]
                if not err <= ref.nb[i]:
                    bad.append((tag, "normal", err, float(ref.nb[i]), ref.w[i].tolist()))
        elif decided and cold and not np.all(nrm[j] == 0.0):
            bad.append((tag, "normal not zero", nrm[j].tolist(), rs))
        a, b = ratios.get(fam, (0.0, 0.0))
        ratios[fam] = (max(a, r_n), max(b, r_m))
    assert not bad, (len(bad), bad[:12])
    return ratios


def merge_ratios(total, part):
    for fam, (a, b) in part.items():
        c, d = total.get(fam, (0.0, 0.0))
        total[fam] = (max(a, c), max(b, d))
    return total


def format_ratios(ratios, title):
    return title + ": " + ", ".join(f"{fam} {ratios[fam][0]:.2g}|{ratios[fam][1]:.2g}" for fam in FAMILIES if fam in ratios)


def check_cold(make, key, binary=False, batch=None, label=""):
    """One cold linearize of the zoo's two factors (main / far config) at pose 0, held to the reference.  make(zoo, idx, far=...,
    binary=...) -> a factor with linearize() and state(); batch: a function linearizing a list of factors instead.  -> ratios."""
    zoo, ref = build(*key), reference(*key, 0)
    ratios = {}
    for name, idx in zoo.clouds.items():
        f = make(zoo, idx, far=name == "far", binary=binary)
        if binary:
            R, t, Rt, tt = binary_poses(zoo)
            f.linearize(R, t, R_tgt=Rt, t_tgt=tt)
        elif batch is not None:
            batch([f], [zoo.R], [zoo.t])
        else:
            f.linearize(zoo.R, zoo.t)
        merge_ratios(ratios, check_state(zoo, ref, idx, f.state(), True, label + name))
    print(format_ratios(ratios, f"{label}k {zoo.k} mode {zoo.mode} offset {zoo.offset:g}"))
    return ratios


def check_warm(make, key, label="warm "):
    """A factor with the config's own min_dist 0.15 (re-association threshold 0.0375 m): cold at pose 0; pose 1 (0.01 m) leaves every
    point cached: mean and normal keep their bits, statuses 7 / 8 follow the max-error gate at the new query, the others stay;
    pose 2 (0.1 m) re-associates every point and is held to the reference recomputed there."""
    zoo, ref0, ref2 = build(*key), reference(*key, 0), reference(*key, 2)
    ratios = {}
    for name, idx in zoo.clouds.items():
        f = make(zoo, idx, far=name == "far", warm=True)
        f.linearize(*pose(zoo, 0))
        s0 = [np.array(a) for a in f.state()[:3]]
        merge_ratios(ratios, check_state(zoo, ref0, idx, s0, True, label + "pose 0 " + name))
        f.linearize(*pose(zoo, 1))
        s1 = [np.array(a) for a in f.state()[:3]]
        assert np.array_equal(s1[1].view(np.uint64), s0[1].view(np.uint64)) and np.array_equal(s1[2].view(np.uint64), s0[2].view(np.uint64)), \
            "a cached point's mean / normal changed its bits"
        exp, undecided = expected_cached(zoo, ref0)
        ok = ~undecided[idx]
        assert np.array_equal(s1[0][ok], exp[idx][ok]), (label, name, np.flatnonzero(s1[0][ok] != exp[idx][ok])[:8].tolist())
        low = s0[0] <= 6
        assert np.array_equal(s1[0][low], s0[0][low])  # (ambiguous ones included: no gate below 7 is run again)
        f.linearize(*pose(zoo, 2))
        merge_ratios(ratios, check_state(zoo, ref2, idx, f.state(), False, label + "pose 2 " + name))
    print(format_ratios(ratios, f"{label}k {zoo.k} mode {zoo.mode} offset {zoo.offset:g}"))
    return ratios


def check_tiled(make, key, label="tiled "):
    """The zoo's main cloud repeated past 65 536 points (the device's 512-thread class): the first copy is held to the reference,
    every further copy must equal it bit for bit."""
    zoo, ref = build(*key), reference(*key, 0)
    idx = zoo.clouds["main"]
    copies = 65536 // len(idx) + 1
    pts = np.tile(zoo.pts[idx], copies)
    pts["idx"] = np.arange(len(pts), dtype=np.uint32)
    assert len(pts) > 65536
    f = make(zoo, idx, pts=pts)
    f.linearize(zoo.R, zoo.t)
    st, mean, nrm = (np.asarray(a) for a in f.state()[:3])
    n = len(idx)
    ratios = check_state(zoo, ref, idx, (st[:n], mean[:n], nrm[:n]), True, label)
    assert np.array_equal(st.reshape(copies, n), np.tile(st[:n], (copies, 1)))
    for a in (mean, nrm):
        bits = np.ascontiguousarray(a).view(np.uint64).reshape(copies, n * 3)
        assert np.array_equal(bits, np.tile(bits[0], (copies, 1)))
    print(format_ratios(ratios, f"{label}k {zoo.k} mode {zoo.mode} offset {zoo.offset:g} ({len(pts)} points)"))
    return ratios


SUMS_BAR = 1e-11  # the issue's ceiling for the sums' bound (4 max nb + 256 eps stays below it: nb <= 1e-12 by selection)


def check_sums(make, key, huber, label="sums "):
    """H_ss, b_s and f of a factor over the Valid cases whose normal is known to 1e-12 against the sums built in mpmath from the
    reference planes: relative norm error <= 4 max nb + 256 eps (rows are linear in the normal, H quadratic)."""
    zoo, ref = build(*key), reference(*key, 0)
    sel, H, b, f, n_huber = sums_reference(zoo, ref, huber)
    assert len(sel) >= 8 and (n_huber >= 2 if huber else n_huber == 0), (len(sel), n_huber)
    bound = 4.0 * float(ref.nb[sel].max()) + 256.0 * EPS
    assert bound <= SUMS_BAR
    fac = make(zoo, sel, huber=huber)
    got = fac.linearize(zoo.R, zoo.t)
    assert got["status_hist"][8] == len(sel)
    errs = {}
    for name, want in (("H_ss", H), ("b_s", b), ("f", np.array([f]))):
        have = np.asarray(got[name], np.float64).reshape(want.shape)
        errs[name] = float(np.linalg.norm(have - want) / np.linalg.norm(want))
    print(f"{label}k {zoo.k} mode {zoo.mode} offset {zoo.offset:g} huber {huber}: {len(sel)} rows, bound {bound:.2g}, " +
          ", ".join(f"{n} {e:.2g}" for n, e in errs.items()))
    assert all(e <= bound for e in errs.values()), (errs, bound)
    return errs


def sums_reference(zoo, ref, huber):
    """H_ss, b_s, f of a unary factor over the zoo's Valid cases whose normal is known to 1e-12, summed in mpmath from the
    reference planes.  -> (case indices, H (6, 6), b (6,), f, number of rows the Huber weight changes)."""
    sel = np.flatnonzero((ref.status == 8) & ~ref.ambiguous & ~ref.knn_open & (ref.nb <= 1e-12) & ~zoo.far)
    cfg = synth.enwide_config()
    with mp.workdps(DPS):
        sigma, hub = mpf(float(np.float32(cfg["lidar_point_noise_std_dev"]))), mpf(float(np.float32(cfg["huber_threshold"])))
        Rm = [_mpv(r) for r in zoo.R]
        H = [[mpf(0)] * 6 for _ in range(6)]
        b, f, n_huber = [mpf(0)] * 6, mpf(0), 0
        for i in sel:
            p, nrm = _mpv(zoo.src[i]), ref.mp_normal[i]
            e = _dot(nrm, [ref.mp_mean[i][a] - ref.mp_q[i][a] for a in range(3)])
            sw = mpf(1)
            if huber and abs(e / sigma) > hub:
                sw = mp.sqrt(hub / abs(e / sigma))
                n_huber += 1
            wgt = sw / sigma
            ns = [Rm[0][c] * nrm[0] + Rm[1][c] * nrm[1] + Rm[2][c] * nrm[2] for c in range(3)]
            J = [ns[1] * p[2] - ns[2] * p[1], ns[2] * p[0] - ns[0] * p[2], ns[0] * p[1] - ns[1] * p[0], -ns[0], -ns[1], -ns[2]]
            J = [x * wgt for x in J]
            e = e * wgt
            for r in range(6):
                for c in range(6):
                    H[r][c] += J[r] * J[c]
                b[r] += J[r] * e
            f += e * e
        return sel, np.array([[float(x) for x in r] for r in H]), np.array([float(x) for x in b]), float(f), n_huber
