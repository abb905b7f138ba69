"""ICPFactor::poseGrid / scorePoses[Async] / relocalise of the C++ host mirror (tests/cpp/reloc_pipeline.cpp) against the C ABI
binding on the same inputs: the same library on the same poses, so scores, winners, candidates and aligned poses are the C
call's bit for bit.  The grid itself is compared with capi.pose_grid: same order, translations equal, rotations to 4e-16 (one
cos / sin of either math library and a 3 x 3 product)."""
import json
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_host_cpp import build_exe


def test_reloc_case_compiles():
    """CPU-runnable: the mirror's relocalisation calls build warning-free against the C ABI."""
    import os
    assert os.path.exists(build_exe("reloc_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_relocalise_is_the_c_abi_call(ctx, tmp_path):
    from mimosa_amd import capi, synth
    m, pts, aux = synth.small_world()
    Rg, tg = aux["R_W_L"], aux["t_W_L"]
    R0, t0 = synth.rot_z(np.deg2rad(20.0)) @ Rg, tg + np.array([1.2, -0.9, 0.0])
    grid = dict(half_xy=2.0, step_xy=0.5, half_yaw=np.deg2rad(30.0), step_yaw=np.deg2rad(7.5))
    score = dict(gate=1.0, stride=4, top_k=4)
    final_gate = 0.1
    settings = dict(max_iters=30, eps_rot=1e-9, eps_trans=1e-9, damping=1e-9, prior_sigma_rot=0.0, prior_sigma_trans=0.0, check_every=0)
    reg = capi.make_reg_config(**synth.enwide_config())
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            f.write(struct.pack("<Q", arr.size if arr.dtype.itemsize != 32 else len(arr)))
            f.write(arr.tobytes())
        w(m.astype(np.float32).ravel())
        w(pts)
        w(np.frombuffer(bytes(reg), np.uint8))
        w(np.concatenate([R0.ravel(), t0]))
        w(np.array([grid[k] for k in ("half_xy", "step_xy", "half_yaw", "step_yaw")], float))
        w(np.array([score["gate"], score["stride"], score["top_k"], final_gate], float))
        w(np.array([settings[k] for k in ("max_iters", "eps_rot", "eps_trans", "damping", "prior_sigma_rot", "prior_sigma_trans", "check_every")], float))
    out = subprocess.run([build_exe("reloc_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)

    # the grid: capi.pose_grid's enumeration
    Rs, ts = capi.pose_grid(R0, t0, **grid)
    gR = np.array([g["R"] for g in got["grid"]]).reshape(-1, 3, 3)
    gt = np.array([g["t"] for g in got["grid"]])
    assert got["n_poses"] == len(Rs) == 9 * 81
    assert np.array_equal(gt, ts) and np.abs(gR - Rs).max() <= 4e-16

    # the C ABI on the mirror's poses
    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    fac = capi.ICPFactor(ctx, gm, pts, reg)
    fac.set_components(False)
    scores, best = fac.score_poses(gR, gt, **score)
    gs = np.array(got["scores"])
    for k, name in enumerate(("n_points", "n_occupied", "n_inliers")):
        assert np.array_equal(gs[:, k].astype(np.int64), scores[name])
    assert np.array_equal(gs[:, 3], scores["sum_sq"])
    assert got["best"] == [int(b) for b in best]
    assert got["async_equal"] == 1 and got["winners_alone_equal"] == 1 and got["count_before"] == 0
    ref = fac.relocalise(gR, gt, capi.make_reloc_config(align=capi.make_align_config(**settings), final_gate=final_gate, **score))
    r = got["reloc"]
    assert r["best"] == ref["best"] and len(r["candidates"]) == ref["n_candidates"] == score["top_k"]
    assert np.array_equal(np.array(r["pose"]["R"]).reshape(3, 3), ref["R"]) and np.array_equal(np.array(r["pose"]["t"]), ref["t"])
    for a, b in zip(r["candidates"], ref["cand"]):
        assert (a["index"], a["iters"], a["converged"]) == (b["index"], b["iters"], b["converged"])
        assert np.array_equal(np.array(a["R"]).reshape(3, 3), b["R"]) and np.array_equal(np.array(a["t"]), b["t"])
        for which in ("coarse", "fine"):
            assert a[which] == [b[which]["n_points"], b[which]["n_occupied"], b[which]["n_inliers"], b[which]["sum_sq"]]
    # the count moved with the alignments, in the mirror's books as in the library's
    assert got["count_after"] == sum(c["iters"] for c in ref["cand"])
    assert fac.linearize(ref["R"], ref["t"])["linearize_count"] == got["count_after"] + 1
    fac.destroy()
    gm.release()
