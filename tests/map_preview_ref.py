"""numpy restatement of the map's sequential insertion rule (gtsam_points::iVox::insert / FlatContainer::add) with per-point
outcomes, for the insert-preview tests.  It works on a dict voxel -> kept points (float32 rows) and is fed from mh_map_get_cloud of
the map under test.  The squared distance is evaluated in the kernels' order, (dx dx + dz dz) + (dy dy + 0.0) in fp64 without FMA,
so a pair that sits on the threshold falls on the same side."""
import math

import numpy as np

ADDED, TOO_CLOSE, VOXEL_FULL = 1, 2, 3


def coord(p, inv_leaf):
    """voxel of a float32 point: floor(double(p) * inv_leaf) per axis"""
    return tuple(int(math.floor(float(c) * inv_leaf)) for c in p)


def cells_of(cloud_xyz, leaf=0.5):
    """dict voxel -> list of the points a map holds there, from its get_cloud()"""
    inv_leaf = 1.0 / leaf
    cells = {}
    for p in np.asarray(cloud_xyz, np.float32).reshape(-1, 3):
        cells.setdefault(coord(p, inv_leaf), []).append(p)
    return cells


def sq_dist(a, b):
    dx, dy, dz = (float(a[0]) - float(b[0])), (float(a[1]) - float(b[1])), (float(a[2]) - float(b[2]))
    return (dx * dx + dz * dz) + (dy * dy + 0.0)


def preview(cells, batch_xyz, leaf=0.5, min_dist=0.15, max_pts=20):
    """What inserting batch_xyz (input order) into `cells` does: the six counts of mh_map_insert_preview, the outcome of every
    point, and the cells afterwards (a copy; `cells` is left as it is)."""
    inv_leaf, min_sq = 1.0 / leaf, min_dist * min_dist
    after = {c: list(v) for c, v in cells.items()}
    batch = np.asarray(batch_xyz, np.float32).reshape(-1, 3)
    outcome = np.zeros(len(batch), np.uint8)
    touched, new = set(), set()
    for i, p in enumerate(batch):
        c = coord(p, inv_leaf)
        if c not in after:
            after[c] = []
            new.add(c)
        touched.add(c)
        kept = after[c]
        if len(kept) >= max_pts:
            outcome[i] = VOXEL_FULL
        elif any(sq_dist(q, p) < min_sq for q in kept):
            outcome[i] = TOO_CLOSE
        else:
            kept.append(p)
            outcome[i] = ADDED
    counts = dict(n_points=len(batch), n_added=int((outcome == ADDED).sum()), n_too_close=int((outcome == TOO_CLOSE).sum()),
                  n_voxel_full=int((outcome == VOXEL_FULL).sum()), n_touched_voxels=len(touched), n_new_voxels=len(new))
    return counts, outcome, after
