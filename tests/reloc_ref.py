"""numpy restatement of the score of mh_icp_score_poses (include/mimosa_hip.h, mimosa_amd/csrc/reloc_device.hpp), for the CPU and
GPU relocalisation tests.  Nothing of the library is called here: the nearest map point comes from a pluggable knn(q), the
occupancy from a pluggable set of occupied voxels.

Score of a pose (R, t), gate g, stride s over the points i with i % s == 0 in the caller's order:
  q_a = ((R[3a] x + R[3a+1] y) + R[3a+2] z) + t[a]     x, y, z the point's floats widened to double, each operation rounded
  u = q * inv_leaf; a point with any |u_a| not below 2^20 (or not finite) is looked up nowhere: not occupied, no inlier
  occupied: floor(u) is a voxel that holds a point
  inlier: knn finds a nearest point and its d2 <= g * g;  sum_sq adds d2 over the inliers
The ranking key: n_inliers descending, sum_sq ascending, pose index ascending."""
import math

import numpy as np

COORD_LIMIT = float(2 ** 20)
NEIGHBOR_OFFSETS = {
    1: [(0, 0, 0)],
    7: [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
    19: [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if not (i and j and k)],
    27: [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)],
}


def transform(R, t, xyz):
    """q [m, 3] of the float32 points xyz [m, 3]: written out element by element in the stated order (numpy rounds every
    product and every sum on its own: no contraction)"""
    R = np.asarray(R, np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    x, y, z = (np.asarray(xyz[:, a], np.float32).astype(np.float64) for a in range(3))
    q = np.empty((len(x), 3))
    for a in range(3):
        q[:, a] = ((R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z) + t[a]
    return q


def in_range(u):
    with np.errstate(invalid="ignore"):
        return np.all(np.abs(u) < COORD_LIMIT, axis=1)  # False for NaN and inf as well


def voxel_of(u):
    return np.floor(u).astype(np.int64)


def occupied_set(map_xyz, inv_leaf=2.0):
    """the voxels that hold a point of the float32 cloud map_xyz, as the maps file them: floor(double(p) * inv_leaf)"""
    c = np.floor(np.asarray(map_xyz, np.float32).astype(np.float64) * inv_leaf).astype(np.int64)
    return set(map(tuple, c))


def score_pose(R, t, xyz, gate, stride, knn, occupied, inv_leaf=2.0):
    """xyz: the factor's float32 points [n, 3] in the caller's order.  knn(q [m, 3]) -> (found [m] bool, d2 [m]) for k = 1.
    Returns dict(n_points, n_occupied, n_inliers, sum_sq, q, d2, found, looked) — the last four per looked-at point, for the
    callers that check the gate edge (d2 is inf where nothing was found or looked up)."""
    sub = np.asarray(xyz)[::stride]
    q = transform(R, t, sub)
    u = q * inv_leaf
    ok = in_range(u)
    found = np.zeros(len(sub), bool)
    d2 = np.full(len(sub), np.inf)
    occ = np.zeros(len(sub), bool)
    if ok.any():
        f, d = knn(q[ok])
        found[ok] = np.asarray(f, bool)
        d2[ok] = np.where(np.asarray(f, bool), np.asarray(d, np.float64), np.inf)
        occ[ok] = [tuple(c) in occupied for c in voxel_of(u[ok])]
    inl = found & (d2 <= gate * gate)
    return dict(n_points=len(sub), n_occupied=int(occ.sum()), n_inliers=int(inl.sum()), sum_sq=math.fsum(d2[inl]), q=q, d2=d2, found=found,
                looked=ok)


def brute_knn(map_xyz, mode, inv_leaf=2.0):
    """knn(q) by brute force: the nearest point of the float32 cloud map_xyz among those filed under the neighbour voxels
    (NEIGHBOR_OFFSETS[mode]) of q's voxel; d2 = (dx dx + dz dz) + dy dy, d = point - q, the expression mh_map_knn reports"""
    P = np.asarray(map_xyz, np.float32).astype(np.float64)
    cells = {}
    for i, c in enumerate(map(tuple, np.floor(P * inv_leaf).astype(np.int64))):
        cells.setdefault(c, []).append(i)

    def knn(q):
        found = np.zeros(len(q), bool)
        d2 = np.full(len(q), np.inf)
        for n, (qq, c) in enumerate(zip(q, voxel_of(q * inv_leaf))):
            idx = [i for o in NEIGHBOR_OFFSETS[mode] for i in cells.get((c[0] + o[0], c[1] + o[1], c[2] + o[2]), ())]
            if idx:
                d = P[idx] - qq
                dd = (d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]) + d[:, 1] * d[:, 1]
                found[n], d2[n] = True, dd.min()
        return found, d2
    return knn


def rank(n_inliers, sum_sq):
    """pose indices in rank order"""
    n_inliers = np.asarray(n_inliers, np.int64)
    return np.lexsort((np.arange(len(n_inliers)), np.asarray(sum_sq, np.float64), -n_inliers))


def key_not_worse(a, b):
    """a, b: dicts with n_inliers, sum_sq — a's key (index aside) is not behind b's"""
    return (-a["n_inliers"], a["sum_sq"]) <= (-b["n_inliers"], b["sum_sq"])
