"""numpy restatement of the place-recognition rule as include/mimosa_hip.h states it: the ring x sector height image of a cloud
and the distance of two images over every column shift.  Its own copy of the sector table; numpy rounds every elementwise
product and sum on its own (no FMA), and every sum below is written as a loop over its terms in the stated order, so the
descriptor matches the library bit for bit and the distance to the last few bits."""
import numpy as np

RINGS, SECTORS, MAX_HITS = 20, 60, 16
CELLS = RINGS * SECTORS
NO_MATCH = 2.0

# cos and sin of 6 degrees * j, j = 0 .. 14
COS = np.array([1.0, 0.9945218953682733, 0.9781476007338057, 0.9510565162951535, 0.9135454576426009, 0.8660254037844386, 0.8090169943749475,
                0.7431448254773942, 0.6691306063588582, 0.5877852522924731, 0.5, 0.4067366430758002, 0.30901699437494745, 0.20791169081775934,
                0.10452846326765347])
SIN = np.array([0.0, 0.10452846326765347, 0.20791169081775934, 0.30901699437494745, 0.4067366430758002, 0.5, 0.5877852522924731,
                0.6691306063588582, 0.7431448254773942, 0.8090169943749475, 0.8660254037844386, 0.9135454576426009, 0.9510565162951535,
                0.9781476007338057, 0.9945218953682733])


def ring_table(r_max):
    w = np.float64(r_max) / np.float64(RINGS)
    e = np.arange(RINGS + 1, dtype=np.float64) * w
    return e * e


def cells(xyz, R, cfg):
    """per point (cell or -1, value as f32)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(9)
    b2 = ring_table(cfg["r_max"])
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        q3 = [(R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z for a in range(3)]
        xp, yp, zp = q3
        r2 = xp * xp + yp * yp
        counts = (r2 >= np.float64(cfg["r_min"]) * np.float64(cfg["r_min"])) & (r2 < b2[RINGS]) & (zp > cfg["z_min"]) & (zp < cfg["z_max"])
        ring = np.zeros(len(p), np.int64)
        for i in range(1, RINGS):
            ring += r2 >= b2[i]
        q = np.where((xp > 0) & (yp >= 0), 0, np.where((xp <= 0) & (yp > 0), 1, np.where((xp < 0) & (yp <= 0), 2, 3)))
        u = np.choose(q, [xp, yp, -xp, -yp])
        v = np.choose(q, [yp, -xp, -yp, xp])
        m = np.zeros(len(p), np.int64)
        for j in range(1, 15):
            m += (v * COS[j]) >= (u * SIN[j])
        value = (zp - np.float64(cfg["z_min"])).astype(np.float32)
    cell = np.where(counts, ring * SECTORS + 15 * q + m, -1)
    return cell, value


def describe(xyz, R, cfg):
    cell, value = cells(xyz, R, cfg)
    desc = np.zeros(CELLS, np.float32)
    ok = cell >= 0
    np.maximum.at(desc, cell[ok], value[ok])
    return desc


def norms(desc):
    """column norms of descriptors [..., 1200] -> [..., 60]"""
    X = np.asarray(desc, np.float32).reshape(-1, RINGS, SECTORS).astype(np.float64)
    s = np.zeros((X.shape[0], SECTORS))
    for i in range(RINGS):
        s = s + X[:, i, :] * X[:, i, :]
    return np.sqrt(s).reshape(np.shape(desc)[:-1] + (SECTORS,))


def shift_distances(q, cands, min_overlap):
    """d(s) of query q [1200] against candidates [M, 1200]: [M, 60]"""
    Q = np.asarray(q, np.float32).reshape(RINGS, SECTORS).astype(np.float64)
    Cd = np.asarray(cands, np.float32).reshape(-1, RINGS, SECTORS).astype(np.float64)
    nq, nc = norms(q), norms(np.asarray(cands, np.float32).reshape(-1, CELLS))
    M = Cd.shape[0]
    d = np.empty((M, SECTORS))
    for s in range(SECTORS):
        Cs = np.roll(Cd, -s, axis=2)                     # column j holds C's column (j + s) % 60
        ncs = np.roll(nc, -s, axis=1)
        dot = np.zeros((M, SECTORS))
        for i in range(RINGS):
            dot = dot + Q[i][None, :] * Cs[:, i, :]
        valid = (nq[None, :] > 0) & (ncs > 0)
        with np.errstate(all="ignore"):
            c = dot / (nq[None, :] * ncs)
        acc = np.zeros(M)
        for j in range(SECTORS):                         # valid j ascending
            acc = np.where(valid[:, j], acc + c[:, j], acc)
        n = valid.sum(axis=1)
        with np.errstate(all="ignore"):
            d[:, s] = np.where(n >= min_overlap, 1.0 - acc / n, NO_MATCH)
    return d


def distances(q, cands, min_overlap):
    """(D [M], shift [M], gap [M]): gap = second-best minus best d(s) (inf where fewer than two shifts are admissible)"""
    d = shift_distances(q, cands, min_overlap)
    shift = d.argmin(axis=1)                             # the smallest s that attains the minimum
    D = d.min(axis=1)
    shift = np.where(D < NO_MATCH, shift, 0)
    srt = np.sort(d, axis=1)
    gap = np.where(srt[:, 1] < NO_MATCH, srt[:, 1] - srt[:, 0], np.inf) if SECTORS > 1 else np.full(len(D), np.inf)
    return D, shift.astype(np.int32), gap


def rank(D, top_k):
    """the hits: indices in rank order (D ascending, index ascending; D == 2.0 never), -1 behind the last"""
    D = np.asarray(D)
    order = np.lexsort((np.arange(len(D)), D))
    order = [int(i) for i in order if D[i] < NO_MATCH][:top_k]
    return np.array(order + [-1] * (top_k - len(order)), np.int32)


def rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
