"""Inputs of the place-recognition tests (tests/test_place_cpu.py, tests/test_gpu_place.py), built on the CPU so that what each
one is for can be checked against the restatement (tests/place_ref.py) before a device sees it."""
import functools

import numpy as np

import place_ref as ref

# ---- the designed cloud of the descriptor tests ---------------------------------------------------------------------------------
# exact in f32 wherever a gate is meant to be hit exactly: r_min = 0.5, r_max = 40 (w = 2), z in (-2, 30)
DESIGNED_CFG = dict(r_min=0.5, r_max=40.0, z_min=-2.0, z_max=30.0, min_overlap=30, capacity=8)
# a rotation that is not the identity and is exact in fp64: a quarter turn about z after a half turn about x
DESIGNED_R = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])


def f32_next(v, toward):
    return float(np.nextafter(np.float32(v), np.float32(toward)))


def designed_levelled():
    """points in the levelled frame G (the tests hand DESIGNED_R^T p to the library, which is exact for this R)"""
    p = []
    for r in (0.5, 40.0):                                # the range gates, just below, at and just above, on an axis
        p += [[f32_next(r, 0.0), 0.0, 1.0], [r, 0.0, 1.0], [f32_next(r, 99.0), 0.0, 1.0], [0.0, -f32_next(r, 0.0), 1.0], [0.0, -r, 1.0]]
    for z in (-2.0, 30.0):                               # the height gates likewise
        p += [[3.0, 4.0, f32_next(z, -99.0)], [3.0, 4.0, z], [3.0, 4.0, f32_next(z, 99.0)]]
    for i in range(1, 21):                               # exactly on every ring boundary (2 i), and just inside it
        p += [[2.0 * i, 0.0, 0.5], [0.0, f32_next(2.0 * i, 0.0), 0.25], [-2.0 * i, 0.0, 0.5]]
    for s in (1.0, 7.0, 39.0):                           # the four axes and the four diagonals
        p += [[s, 0.0, 2.0], [0.0, s, 2.0], [-s, 0.0, 2.0], [0.0, -s, 2.0], [s, s, 2.0], [-s, s, 2.0], [-s, -s, 2.0], [s, -s, 2.0]]
    p += [[0.0, 0.0, 1.0], [0.0, -0.0, 5.0]]             # x = y = 0: inside r_min
    p += [[np.nan, 1.0, 1.0], [1.0, np.nan, 1.0], [1.0, 1.0, np.nan], [np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0], [1.0, 1.0, np.inf], [np.inf, np.inf, -np.inf]]
    for j in range(60):                                  # a direction on every sector edge (to f32 rounding) and in every sector
        for a in (np.deg2rad(6.0 * j), np.deg2rad(6.0 * j + 2.5)):
            p += [[11.0 * np.cos(a), 11.0 * np.sin(a), 1.5 + 0.01 * j]]
    p += [[5.0, 5.0, 3.0], [5.0, 5.0, 7.5], [5.0, 5.0, 7.25]]  # three in one cell: the maximum wins, whatever the order
    return np.array(p, np.float32)


def designed_cloud(n):
    """n points in F: the designed list, then seeded random ones spread over every gate; (xyz f32 [n, 3], R_G_F)"""
    base = designed_levelled()
    rng = np.random.default_rng(5)
    extra = np.empty((max(n - len(base), 0), 3))
    extra[:, :2] = rng.uniform(-45.0, 45.0, (len(extra), 2))
    extra[:, 2] = rng.uniform(-4.0, 33.0, len(extra))
    g = np.concatenate([base, extra.astype(np.float32)])[:n]
    # F = R^T G.  R permutes and negates axes, so this is exact and R (R^T g) == g bit for bit; written as the permutation it is, so
    # that an infinite coordinate stays one (0 * inf in a matrix product would make its neighbours NaN)
    return np.ascontiguousarray(np.stack([g[:, 1], g[:, 0], -g[:, 2]], axis=1)), DESIGNED_R.copy()


DESIGNED_SIZES = (0, 1, 64, 65, 1025, 2049)             # 1 025 and 2 049: one past one and two of the kernel's 1 024-point chunks


# ---- seeded sparse descriptors of the query tests ----------------------------------------------------------------------------
QUERY_MIN_OVERLAP = 20
QUERY_SIZES = (1, 2, 65, 300)
ROTATED = {5: 7, 9: 59, 40: 1, 41: 30}                  # entry -> the shift it must answer with: (nearly) copies of the query rolled by that much


@functools.lru_cache(maxsize=None)
def query_set():
    """(query [1200], entries [300, 1200]).  Entry 0 is all zero; entry 1 has fewer than min_overlap occupied columns; entries 3
    and 17 are an exact duplicate pair near the query; the ROTATED entries are column-rotated copies of the query, each with a few cells
    raised by an amount of its own."""
    rng = np.random.default_rng(77)

    def sparse(n_cols):
        d = np.zeros((ref.RINGS, ref.SECTORS), np.float32)
        cols = rng.choice(ref.SECTORS, n_cols, replace=False)
        for c in cols:
            rows = rng.choice(ref.RINGS, rng.integers(1, 8), replace=False)
            d[rows, c] = rng.uniform(0.1, 6.0, len(rows)).astype(np.float32)
        return d

    q = sparse(48)
    E = np.stack([sparse(int(rng.integers(30, 61))) for _ in range(300)])
    E[0] = 0.0
    E[1] = sparse(QUERY_MIN_OVERLAP - 1)
    near = q.copy()
    near[rng.integers(0, ref.RINGS, 40), rng.integers(0, ref.SECTORS, 40)] += rng.uniform(0.2, 1.0, 40).astype(np.float32)
    E[3] = near
    E[17] = near
    for n, (e, s) in enumerate(ROTATED.items()):
        E[e] = np.roll(q, s, axis=1)                     # its column (j + s) % 60 is the query's column j
        E[e][rng.integers(0, ref.RINGS, 6), rng.integers(0, ref.SECTORS, 6)] += np.float32(0.25 * (n + 1))  # (no two of them at the same distance)
    return q.reshape(-1), E.reshape(300, -1)


# ---- the end-to-end scene: a cluttered hall, keyframes on a lattice, queries off it --------------------------------------------
HALL_LO, HALL_HI = np.array([0.0, 0.0, 0.0]), np.array([40.0, 30.0, 6.0])
# five boxes: they break the point symmetry of an empty hall, where the mirrored place scores the same
BOXES = [(np.array([9.2, 3.2, 0.0]), np.array([11.6, 6.0, 3.0])), (np.array([13.9, 18.8, 0.0]), np.array([16.5, 21.6, 4.5])),
         (np.array([23.6, 8.4, 0.0]), np.array([26.0, 11.2, 6.0])), (np.array([28.4, 13.6, 0.0]), np.array([30.8, 16.4, 2.0])),
         (np.array([18.8, 23.9, 0.0]), np.array([21.2, 26.8, 2.5]))]
SENSOR_Z = 1.2
SCENE_CFG = dict(r_min=0.5, r_max=40.0, z_min=-2.0, z_max=30.0, min_overlap=30, capacity=64)
KEYFRAME_XY = [(8.0 + 4.8 * i, 2.0 + 5.2 * j) for i in range(6) for j in range(6)]   # 36 keyframes; the boxes stand between the lattice lines, more than 1 m from every keyframe


def _hit_inside(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf)).min(axis=1)


def _hit_outside(o, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    return np.where((near <= far) & (near > 0), near, np.inf)


def cast(xy, yaw, rows=32, cols=256, half_fov=0.39):
    """a level scan from (xy, SENSOR_Z) with heading yaw: points in the sensor frame, f32 [rows * cols, 3]"""
    alt = np.linspace(-half_fov, half_fov, rows)
    az = np.arange(cols) * (2.0 * np.pi / cols)
    a, z = np.meshgrid(alt, az, indexing="ij")
    d_s = np.stack([np.cos(a) * np.cos(z), np.cos(a) * np.sin(z), np.sin(a)], axis=-1).reshape(-1, 3)
    R = ref.rz(yaw)
    d = d_s @ R.T
    o = np.broadcast_to(np.array([xy[0], xy[1], SENSOR_Z]), d.shape)
    r = _hit_inside(o, d, HALL_LO, HALL_HI)
    for lo, hi in BOXES:
        r = np.minimum(r, _hit_outside(o, d, lo, hi))
    return (r[:, None] * d_s).astype(np.float32)


def pose_of(xy, yaw):
    return ref.rz(yaw), np.array([xy[0], xy[1], SENSOR_Z])


@functools.lru_cache(maxsize=None)
def keyframes():
    """[(xy, yaw, cloud)]: the keyframes' headings vary, so a hit's shift is not the query's yaw alone"""
    rng = np.random.default_rng(3)
    return [(xy, float(yaw), cast(xy, float(yaw))) for xy, yaw in zip(KEYFRAME_XY, rng.uniform(-np.pi, np.pi, len(KEYFRAME_XY)))]


@functools.lru_cache(maxsize=None)
def keyframe_descriptors():
    return np.stack([ref.describe(c, np.eye(3), SCENE_CFG) for _, _, c in keyframes()])


@functools.lru_cache(maxsize=None)
def candidates(n=40, seed=9):
    """n candidate queries: up to 1 m off a keyframe, any heading.  Per candidate a dict with the restatement's answers."""
    rng = np.random.default_rng(seed)
    K = keyframe_descriptors()
    out = []
    for _ in range(n):
        k = int(rng.integers(0, len(KEYFRAME_XY)))
        off = rng.uniform(-1.0, 1.0, 2)
        off *= min(1.0, 1.0 / np.linalg.norm(off))
        xy = (KEYFRAME_XY[k][0] + off[0], KEYFRAME_XY[k][1] + off[1])
        yaw = float(rng.uniform(-np.pi, np.pi))
        cloud = cast(xy, yaw)
        desc = ref.describe(cloud, np.eye(3), SCENE_CFG)
        D, shift, gap = ref.distances(desc, K, SCENE_CFG["min_overlap"])
        top = ref.rank(D, 5)
        nearest = int(np.argmin([np.hypot(xy[0] - x, xy[1] - y) for x, y in KEYFRAME_XY]))
        out.append(dict(xy=xy, yaw=yaw, cloud=cloud, desc=desc, D=D, shift=shift, gap=gap, top=top, nearest=nearest))
    return out


def qualifies(c):
    """the scene conditions of the end-to-end test: the nearest keyframe among the restatement's top 4, consecutive distances among
    its top 5 more than 1e-9 apart (and, so that the shifts can be compared as well, every top-4 shift decided by more than 1e-9)"""
    top = c["top"]
    if (top < 0).any() or c["nearest"] not in top[:4].tolist():
        return False
    return bool((np.diff(c["D"][top]) > 1e-9).all() and (c["gap"][top[:4]] > 1e-9).all())


@functools.lru_cache(maxsize=None)
def queries():
    """the first six candidates that qualify"""
    q = [c for c in candidates() if qualifies(c)][:6]
    assert len(q) == 6, len(q)
    return q
