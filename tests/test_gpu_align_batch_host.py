"""ICPFactor::alignBatch[Async] / relocaliseBatch of the C++ host mirror (tests/cpp/align_batch_pipeline.cpp) against the C ABI
binding on the same inputs: the same library on the same poses with the same launch classes, so every member's result, the
candidates and the aligned poses are the C call's bit for bit."""
import json
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_host_cpp import build_exe


def test_align_batch_case_compiles():
    """CPU-runnable: the mirror's batch calls build warning-free against the C ABI."""
    import os
    assert os.path.exists(build_exe("align_batch_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_batch_calls_are_the_c_abi_calls(ctx, tmp_path):
    from mimosa_amd import capi, synth
    m, pts, aux = synth.small_world()
    Rg, tg = aux["R_W_L"], aux["t_W_L"]
    R0, t0 = synth.rot_z(np.deg2rad(20.0)) @ Rg, tg + np.array([1.2, -0.9, 0.0])
    grid = dict(half_xy=2.0, step_xy=0.5, half_yaw=np.deg2rad(30.0), step_yaw=np.deg2rad(7.5))
    score = dict(gate=1.0, stride=4, top_k=4)
    final_gate = 0.1
    settings = dict(max_iters=30, eps_rot=1e-9, eps_trans=1e-9, damping=1e-9, prior_sigma_rot=0.0, prior_sigma_trans=0.0, check_every=0)
    starts = [(synth.rot_z(np.deg2rad(a)) @ Rg, tg + np.array(d)) for a, d in ((1.0, [0.05, 0.0, 0.0]), (-3.0, [0.0, 0.2, 0.01]), (5.0, [-0.3, 0.1, 0.0]))]
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
        w(np.concatenate([np.concatenate([R.ravel(), t]) for R, t in starts]))
        w(np.concatenate([R0.ravel(), t0]))
        w(np.array([grid[k] for k in ("half_xy", "step_xy", "half_yaw", "step_yaw")], float))
        w(np.array([score["gate"], score["stride"], score["top_k"], final_gate], float))
        w(np.array([settings[k] for k in ("max_iters", "eps_rot", "eps_trans", "damping", "prior_sigma_rot", "prior_sigma_trans", "check_every")], float))
    out = subprocess.run([build_exe("align_batch_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)

    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    fac = capi.ICPFactor(ctx, gm, pts, reg)
    fac.set_components(False)
    members = [fac.clone() for _ in starts]
    acfg = capi.make_align_config(**settings)
    ref = capi.align_batch(members, starts, acfg)
    assert got["async_equal"] == 1 and len(got["members"]) == len(ref) == 3
    for a, b in zip(got["members"], ref):
        assert (a["iters"], a["converged"], a["n_trace"]) == (b["iters"], b["converged"], len(b["trace"]))
        assert a["count"] == b["iters"] and a["f_last"] == b["trace"][-1]["f"]
        assert np.array_equal(np.array(a["R"]).reshape(3, 3), b["R"]) and np.array_equal(np.array(a["t"]), b["t"])
    assert len({b["iters"] for b in ref}) >= 2  # the members stopped on their own

    # the C ABI on the mirror's own grid (its rotations differ from capi.pose_grid's in the last bit: test_gpu_reloc_host.py)
    gR = np.array([g["R"] for g in got["grid"]]).reshape(-1, 3, 3)
    gt = np.array([g["t"] for g in got["grid"]])
    rr = fac.relocalise(gR, gt, capi.make_reloc_config(align=acfg, final_gate=final_gate, **score), batch=True)
    r = got["reloc"]
    assert r["repeat_equal"] == 1 and r["best"] == rr["best"] and len(r["candidates"]) == rr["n_candidates"] == score["top_k"]
    for a, b in zip(r["candidates"], rr["cand"]):
        assert (a["index"], a["iters"], a["converged"]) == (b["index"], b["iters"], b["converged"])
        assert np.array_equal(np.array(a["R"]).reshape(3, 3), b["R"]) and np.array_equal(np.array(a["t"]), b["t"])
        for which in ("coarse", "fine"):
            assert a[which] == [b[which]["n_points"], b[which]["n_occupied"], b[which]["n_inliers"], b[which]["sum_sq"]]
    assert np.array_equal(np.array(r["pose"]["R"]).reshape(3, 3), rr["R"]) and np.array_equal(np.array(r["pose"]["t"]), rr["t"])
    assert got["count_after"] == 0  # the scored factor was only read
    for x in members + [fac]:
        x.destroy()
    gm.release()
