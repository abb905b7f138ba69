"""Worker of tests/test_gpu_degeneracy_zoo.py: one cold linearize (components on) of every case of the degenerate-geometry zoo
(tests/degeneracy_zoo.py) in the K3 launch class the environment selects (MH_QL2_MAX / MH_QL4_MAX are read once per process);
the blocks, localizabilities, bases, component sums and per-point state of every case go to one .npz, which the parent holds
to the multi-precision reference."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import degeneracy_zoo as Z  # noqa: E402
from mimosa_amd import capi  # noqa: E402

KEYS = ("H_ss", "b_s", "loc_rot_final", "loc_trans_final", "eigvec_rot", "eigvec_trans", "loc_rot_comp", "loc_trans_comp", "status_hist")

if __name__ == "__main__":
    out = sys.argv[1]
    scenes = [Z.build(*case) for case in Z.CASES]  # host work before the device is opened
    ctx = capi.Context(0)
    blob = {}
    for ci, sc in enumerate(scenes):
        gm = capi.VoxelMap(ctx, **Z.MAP_KW)
        gm.insert(sc.map_xyz)
        assert gm.stats()["n_points"] == len(sc.map_xyz)
        f = capi.ICPFactor(ctx, gm, sc.pts, capi.make_reg_config(**Z.config()))
        res = f.linearize(sc.R, sc.t, Z.G_UNIT)
        blob.update({f"c{ci}_{k}": np.asarray(res[k]) for k in KEYS})
        blob.update({f"c{ci}_state{i}": a for i, a in enumerate(f.state())})
        f.destroy()
        gm.release()
    np.savez(out, **blob)
    ctx.close()
    print("OK")
