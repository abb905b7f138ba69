"""The numpy restatement of map carving (include/mimosa_hip.h, mh_map_carve*): the observation image, the decision for every map
point and the six counters.  Every expression is fp64 in the written order; numpy evaluates each operation on its own (no FMA),
and fp64 divide and square root are correctly rounded on both sides, so the device's decisions are matched exactly.

It works on mh_map_get_cloud's output (points in voxel order) plus per-voxel counts: voxel_counts(cloud, leaf) recovers them,
because a voxel's points are contiguous in the cloud and no two consecutive voxels share coordinates."""
import numpy as np

UNTESTED, KEPT, SEEN_THROUGH = 0, 1, 2
COUNTERS = ("n_obs_used", "n_cells_hit", "n_tested", "n_removed", "n_voxels_touched", "n_voxels_emptied")


def cells(s, N):
    """(cell, face, i, j) of the vectors s (n, 3); cell = -1 where there is none"""
    s = np.asarray(s, np.float64).reshape(-1, 3)
    a = np.abs(s)
    f = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    k = np.arange(len(s))
    m = a[k, f]
    ok = (m > 0.0) & np.isfinite(s).all(axis=1)
    ms = np.where(ok, m, 1.0)
    face = 2 * f + (s[k, f] < 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.where(ok, s[k, (f + 1) % 3] / ms, 0.0)
        v = np.where(ok, s[k, (f + 2) % 3] / ms, 0.0)
    half = 0.5 * float(N)
    i = np.minimum(N - 1, np.floor((u + 1.0) * half).astype(np.int64))
    j = np.minimum(N - 1, np.floor((v + 1.0) * half).astype(np.int64))
    cell = np.where(ok, (face * N + j) * N + i, -1)
    return cell, face, i, j


def r2_of(s):
    return (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]


def image(obs, origin, cfg):
    """(6 N^2 doubles with +inf = not hit, n_obs_used)"""
    N = int(cfg["grid"])
    img = np.full(6 * N * N, np.inf)
    obs = np.asarray(obs, np.float32).reshape(-1, 3)
    p = obs.astype(np.float64)
    fin = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p - np.asarray(origin, np.float64)
        r2 = r2_of(s)
        cell, _, _, _ = cells(np.where(fin[:, None], s, 0.0), N)
        use = fin & (r2 >= float(cfg["range_min"]) * float(cfg["range_min"])) & (cell >= 0)
    np.minimum.at(img, cell[use], r2[use])
    return img, int(use.sum())


def map_vectors(points, R, t, origin):
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    R, t, o = np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3), np.asarray(origin, np.float64).reshape(3)
    d0, d1, d2 = p[:, 0] - t[0], p[:, 1] - t[1], p[:, 2] - t[2]
    return np.stack([((R[a] * d0 + R[3 + a] * d1) + R[6 + a] * d2) - o[a] for a in range(3)], axis=1)


def decide(points, img, origin, R, t, cfg):
    """UNTESTED / KEPT / SEEN_THROUGH per map point"""
    N, ring = int(cfg["grid"]), int(cfg["ring"])
    s = map_vectors(points, R, t, origin)
    r2 = r2_of(s)
    rmin2, rmax2 = float(cfg["range_min"]) * float(cfg["range_min"]), float(cfg["range_max"]) * float(cfg["range_max"])
    cell, face, ci, cj = cells(s, N)
    tested = (r2 >= rmin2) & (r2 <= rmax2) & (cell >= 0)
    r = np.sqrt(r2)
    q = np.full(len(s), np.inf)
    all_hit = np.ones(len(s), bool)
    for dj in range(-ring, ring + 1):
        for di in range(-ring, ring + 1):
            i, j = ci + di, cj + dj
            inside = (i >= 0) & (i < N) & (j >= 0) & (j < N)
            c = img[np.where(inside, (face * N + j) * N + i, 0)]
            all_hit &= ~inside | (c < np.inf)
            q = np.where(inside, np.minimum(q, c), q)
    lim = r + (float(cfg["margin_abs"]) + float(cfg["margin_rel"]) * r)
    seen = tested & all_hit & (lim * lim < q)
    return np.where(seen, SEEN_THROUGH, np.where(tested, KEPT, UNTESTED)).astype(np.int32)


def voxel_counts(cloud, leaf):
    """points per voxel of a get_cloud() output, in voxel order"""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    if len(cloud) == 0:
        return np.zeros(0, np.int64)
    c = np.floor(cloud.astype(np.float64) * (1.0 / leaf)).astype(np.int64)
    start = np.concatenate([[True], (c[1:] != c[:-1]).any(axis=1)])
    return np.diff(np.concatenate([np.flatnonzero(start), [len(cloud)]]))


def carve(cloud, counts, obs, origin, R, t, cfg):
    """(counters, removed mask over the cloud's points): what mh_map_carve* reports and removes on a map whose get_cloud() is `cloud`
    with `counts` points per voxel"""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
    obs = np.asarray(obs, np.float32).reshape(-1, 3)
    if len(obs) == 0:
        return dict.fromkeys(COUNTERS, 0), np.zeros(len(cloud), bool)
    img, n_used = image(obs, origin, cfg)
    dec = decide(cloud, img, origin, R, t, cfg)
    removed = dec == SEEN_THROUGH
    vox = np.repeat(np.arange(len(counts)), counts)
    gone = np.bincount(vox[removed], minlength=len(counts)) if len(counts) else np.zeros(0, np.int64)
    counters = dict(n_obs_used=n_used, n_cells_hit=int(np.isfinite(img).sum()), n_tested=int((dec != UNTESTED).sum()), n_removed=int(removed.sum()),
                    n_voxels_touched=int((gone > 0).sum()), n_voxels_emptied=int(((gone > 0) & (gone == np.asarray(counts))).sum()))
    return counters, removed
