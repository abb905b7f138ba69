"""Worker of tests/test_gpu_plane_zoo.py: one cold linearize of every k = 5 zoo (tests/plane_zoo.py), both factors of each, in the
K3 launch class the environment selects (MH_QL2_MAX / MH_QL4_MAX are read once per process); the per-point state of every factor
goes to one .npz, which the parent holds to the multi-precision reference."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_zoo as Z  # noqa: E402
from mimosa_amd import capi  # noqa: E402

out = sys.argv[1]
zoos = [Z.build(*key) for key in Z.K5_ZOOS]  # seconds of host work (the 60-digit references): before the device is opened
ctx = capi.Context(0)
blob = {}
for zi, zoo in enumerate(zoos):
    gm = capi.VoxelMap(ctx, leaf=Z.LEAF, min_dist=0.0, mode=zoo.mode)
    gm.insert(zoo.map_xyz)
    assert gm.stats()["n_points"] == len(zoo.map_xyz)
    for name, idx in zoo.clouds.items():
        f = capi.ICPFactor(ctx, gm, zoo.pts[idx], capi.make_reg_config(**Z.config(zoo.k, far=name == "far")))
        f.linearize(zoo.R, zoo.t)
        blob.update({f"z{zi}_{name}_{i}": a for i, a in enumerate(f.state())})
        f.destroy()
    gm.release()
np.savez(out, **blob)
ctx.close()
print("OK")
