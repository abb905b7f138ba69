"""numpy restatement of mh_map_rebuild_from_keyframes (include/mimosa_hip.h): the chunk plan of csrc/rebuild_plan.hpp, and a
chunked build on oracle.numpy_ref.VoxelMap — the concatenation of a chunk's clouds inserted as one batch, every touched voxel
stamped with the counter of the last keyframe of the chunk that put a point into it, the LRU purge at the chunk ends that land
on the cycle.  Plus the corridor scene the CPU and the GPU test share."""
from __future__ import annotations

import numpy as np

from oracle import numpy_ref

DEFAULT_CHUNK_POINTS = 4 << 20


def plan(sizes, counter0, cycle, budget):
    """[(k0, k1, points, counter_start, purge_after)]: rebuild_plan.hpp's rule.  A chunk ends behind the keyframe whose insert makes
    the counter a multiple of `cycle`, and in front of the keyframe with which its point total would pass `budget`."""
    out, k, n = [], 0, len(sizes)
    while k < n:
        k0, pts, purge = k, 0, False
        while k < n:
            if k > k0 and pts + int(sizes[k]) > budget:
                break
            pts += int(sizes[k])
            k += 1
            if (counter0 + k) % cycle == 0:
                purge = True
                break
        out.append((k0, k, pts, counter0 + k0, purge))
    return out


def world_f32(xyz, R, t):
    """map_assign_kernel's transform: f32, (r0 x + (r1 y + r2 z)) + t, no FMA."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    R = np.asarray(R, np.float32).reshape(3, 3)
    t = np.asarray(t, np.float32).reshape(3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(R[a, 0] * x + (R[a, 1] * y + R[a, 2] * z)) + t[a] for a in range(3)], axis=1).astype(np.float32)


def _purge(vm):
    keep = [c for c in vm.order if not (vm.cells[c][1] + vm.lru_horizon < vm.lru_counter)]
    removed = [c for c in vm.order if c not in set(keep)] if len(keep) != len(vm.order) else []
    vm.cells = {c: vm.cells[c] for c in keep}
    vm.order = keep
    return removed


def sequential_build(vm, clouds_world, events=None):
    """One VoxelMap.insert per keyframe: the twin.  events (a dict) receives 'removed' (per purge: the voxels it erased) and
    'created' (per keyframe: the voxels it created)."""
    for cloud in clouds_world:
        before, order_before = set(vm.cells), list(vm.order)
        vm.insert(cloud)
        if events is not None:
            events.setdefault("created", []).append([c for c in vm.order if c not in before])
            if vm.lru_counter % vm.lru_clear_cycle == 0:
                events.setdefault("removed", []).append([c for c in order_before if c not in vm.cells])
    return vm


def chunked_build(vm, clouds_world, budget=DEFAULT_CHUNK_POINTS, stats=None):
    """The rebuild's route on the oracle map.  stats (a dict) receives chunks, purges and full_in_chunk (voxels that reached the cap
    while a chunk was being inserted)."""
    sizes = [len(c) for c in clouds_world]
    chunks = plan(sizes, vm.lru_counter, vm.lru_clear_cycle, budget)
    n_purges, full = 0, 0
    for k0, k1, _, counter_start, purge in chunks:
        assert counter_start == vm.lru_counter
        last = {}  # voxel -> ordinal of the last keyframe of the chunk with a point in it
        for j, cloud in enumerate(clouds_world[k0:k1]):
            for p in np.asarray(cloud, np.float32).reshape(-1, 3):
                pd = p.astype(np.float64)
                c = vm.coord(pd)
                cell = vm.cells.get(c)
                if cell is None:
                    cell = [[], counter_start]
                    vm.cells[c] = cell
                    vm.order.append(c)
                last[c] = j
                pts = cell[0]
                if len(pts) >= vm.max_pts:
                    continue
                if any(float(np.sum((q - pd) ** 2)) < vm.min_sq for q in pts):
                    continue
                pts.append(pd)
                full += len(pts) == vm.max_pts
        for c, j in last.items():
            vm.cells[c][1] = counter_start + j
        vm.lru_counter += k1 - k0
        if purge:
            _purge(vm)
            n_purges += 1
    if stats is not None:
        stats.update(chunks=len(chunks), purges=n_purges, full_in_chunk=full)
    return vm


def map_signature(vm):
    """Everything of an oracle map that can be compared: voxel order, points, stamps, counter."""
    return (list(vm.order), [np.array(vm.cells[c][0]).reshape(-1, 3) for c in vm.order], [vm.cells[c][1] for c in vm.order], vm.lru_counter)


def assert_same_map(a, b):
    sa, sb = map_signature(a), map_signature(b)
    assert sa[0] == sb[0], "voxel order differs"
    for c, pa, pb in zip(sa[0], sa[1], sb[1]):
        assert pa.shape == pb.shape and np.array_equal(pa, pb), f"points of voxel {c} differ"
    assert sa[2] == sb[2], "LRU stamps differ"
    assert sa[3] == sb[3], "lru_counter differs"


# ---- the corridor ----------------------------------------------------------------------------------------------------------
CORRIDOR_MAP = dict(leaf=0.5, min_dist=0.05, max_pts=20, mode=19, lru_horizon=3, lru_clear_cycle=5)


def rot_z(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def corridor_scene(seed=7, n_keyframes=25, step=1.5, sensor_range=4.0, n_points=360):
    """25 keyframes along a corridor (walls at y = +-2, floor at z = 0, dense posters on the wall every 3 m) and back.  Each keyframe
    sees the world points within `sensor_range` of the sensor, thinned to n_points, in its own frame.  Returns (clouds in the body
    frame, f32; R K x 3 x 3, t K x 3: the poses, f32)."""
    rng = np.random.default_rng(seed)
    half = n_keyframes // 2
    length = half * step
    n_wall = 6000
    x = rng.uniform(-sensor_range, length + sensor_range, n_wall)
    side = rng.integers(0, 3, n_wall)
    wall = np.stack([x, np.where(side == 0, -2.0, np.where(side == 1, 2.0, rng.uniform(-2, 2, n_wall))),
                     np.where(side == 2, 0.0, rng.uniform(0, 2.0, n_wall))], axis=1)
    posters = []
    for px in np.arange(0.2, length, 3.0):  # 0.4 x 0.4 m, dense: these voxels reach the 20-point cap
        q = rng.uniform(0, 0.4, (260, 2))
        posters.append(np.stack([px + q[:, 0], np.full(len(q), 2.0), 1.05 + q[:, 1]], axis=1))
    world = np.concatenate([wall] + posters)
    clouds, Rs, ts = [], [], []
    for k in range(n_keyframes):
        s = k if k <= half else 2 * half - k
        R = rot_z(0.15 * np.sin(0.7 * k)).astype(np.float32)
        t = np.array([s * step, 0.3 * np.sin(0.5 * k), 1.0], np.float32)
        near = world[np.linalg.norm(world - t.astype(np.float64), axis=1) < sensor_range]
        near = near[rng.permutation(len(near))[:n_points]]
        body = (near - t.astype(np.float64)) @ R.astype(np.float64)  # R^T (p - t)
        clouds.append(body.astype(np.float32))
        Rs.append(R)
        ts.append(t)
    return clouds, np.array(Rs, np.float32), np.array(ts, np.float32)


def corridor_world(clouds, Rs, ts):
    return [world_f32(c, R, t) for c, R, t in zip(clouds, Rs, ts)]


# ---- the hall, end to end ------------------------------------------------------------------------------------------------------
HALL_DRIFT = dict(yaw=0.0, trans=(0.03, 0.02, 0.0))     # per keyframe; chosen in tests/test_map_rebuild_cpu.py
HALL_SIGMA = (1e-4, 0.05)                                # rad, m: every edge's information is diag(1 / sigma^2); a lidar odometry's
                                                         # rotation is stiff, so the loop's error goes into the translations
HALL_CAP = 0.5                                           # m: a nearest distance is capped at one leaf, where the map's own search ends


def hall_case(drift=None):
    """The 36 keyframes of tests/place_scenes.py (every 8th point of each cloud), their true poses, poses that drift by a constant
    increment per keyframe, and the pose graph that corrects them: odometry edges from the drifted poses, one loop edge (0, 35) at
    the true relative pose, pose 0 fixed.  Edges as tests/pose_graph_ref.py takes them: (a, b, Z_R, Z_t, information)."""
    import place_scenes as hall
    drift = drift or HALL_DRIFT
    kfs = hall.keyframes()
    clouds = [np.ascontiguousarray(c[::8]) for _, _, c in kfs]
    true = [hall.pose_of(xy, yaw) for xy, yaw, _ in kfs]
    between = lambda a, b: (a[0].T @ b[0], a[0].T @ (b[1] - a[1]))
    # the increment is constant in the world frame: keyframe k is turned by k * yaw about its own position and moved by k * trans
    drifted = [(rot_z(k * drift["yaw"]) @ R, t + k * np.asarray(drift["trans"], np.float64)) for k, (R, t) in enumerate(true)]
    info = np.diag([1.0 / HALL_SIGMA[0] ** 2] * 3 + [1.0 / HALL_SIGMA[1] ** 2] * 3)
    edges = [(k - 1, k, *between(drifted[k - 1], drifted[k]), info) for k in range(1, len(true))]
    edges.append((0, len(true) - 1, *between(true[0], true[-1]), info))
    fixed = [1] + [0] * (len(true) - 1)
    st = lambda poses: (np.array([p[0] for p in poses]), np.array([p[1] for p in poses]))
    return dict(clouds=clouds, true=st(true), drifted=st(drifted), edges=edges, fixed=fixed)


def capped_rms(d):
    return float(np.sqrt(np.mean(np.minimum(np.asarray(d, np.float64), HALL_CAP) ** 2)))


def nearest_distances(points, target, block=512):
    """brute force: the distance from every point to its nearest target point"""
    points, target = np.asarray(points, np.float64), np.asarray(target, np.float64)
    t2 = (target ** 2).sum(1)
    out = np.empty(len(points))
    for i in range(0, len(points), block):
        p = points[i:i + block]
        d2 = (p ** 2).sum(1)[:, None] - 2.0 * (p @ target.T) + t2[None, :]
        out[i:i + block] = np.sqrt(np.maximum(d2.min(1), 0.0))
    return out
