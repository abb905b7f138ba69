"""ICPFactor::align of the C++ host mirror (tests/cpp/align_pipeline.cpp) against the C ABI binding on the same inputs, and the
replays' opt-in init_align (mimosa_amd/replay.py, host/mimosa_hip/replay.hpp): the first scan after the map is seeded is
aligned before its factor goes to the smoother.

init_align bars: off is the default and leaves the replays as they were (the existing replay tests); on, the trajectory starts
from another first pose; with a zero perturbation of the first pose (no prior error) the trajectory with init_align agrees with
the default one to 1e-9 m at every scan — the alignment and the smoother's own iterations descend to the same minimum of the
same associations."""
import json
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_host_cpp import build_exe


def test_align_case_compiles():
    """CPU-runnable: the mirror's align() builds warning-free against the C ABI."""
    import os
    assert os.path.exists(build_exe("align_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_align_is_the_c_abi_call(ctx, tmp_path):
    from mimosa_amd import capi, synth
    m = synth.make_room(synth.BASE_SEED, 0, 0)
    scan, _ = synth.make_scan(64)
    pts = np.ascontiguousarray(scan[::3][:20000])
    Rt, tt = synth.sensor_pose_gt()
    R0, t0 = Rt @ synth.so3_exp(np.deg2rad([1.5, -1.0, 2.0])), tt + np.array([0.2, -0.15, 0.1])
    reg = capi.make_reg_config(**synth.enwide_config())
    settings = dict(max_iters=25, eps_rot=1e-6, eps_trans=1e-6, damping=1e-9, prior_sigma_rot=0.0, prior_sigma_trans=0.0, check_every=4)
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
        w(np.array([settings[k] for k in ("max_iters", "eps_rot", "eps_trans", "damping", "prior_sigma_rot", "prior_sigma_trans", "check_every")], float))
    out = subprocess.run([build_exe("align_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)

    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    fac = capi.ICPFactor(ctx, gm, pts, reg)
    fac.set_components(False)
    ref = fac.align(R0, t0, capi.make_align_config(**settings))
    assert ref["converged"] == 1 and 2 <= ref["iters"] < 25
    # the same library on the same inputs: the Pose3 that comes back, the trace and the counters are the C call's, bit for bit
    assert got["iters"] == ref["iters"] == got["trace_rows"] and got["converged"] == ref["converged"]
    assert np.array_equal(np.array(got["R"]).reshape(3, 3), ref["R"]) and np.array_equal(np.array(got["t"]), ref["t"])
    for a, b in zip(got["trace"], ref["trace"]):
        assert np.array_equal(np.array(a["R"]).reshape(3, 3), b["R"]) and np.array_equal(np.array(a["t"]), b["t"])
        assert (a["f"], a["step_rot"], a["step_trans"], a["n_knn"], a["degenerate"]) == (b["f"], b["step_rot"], b["step_trans"], b["n_knn"], b["degenerate"])
    # the factor's getters report the last evaluated iteration, and a linearize behind the alignment counts on from there
    assert got["count_after_align"] == ref["iters"] == ref["last"]["linearize_count"]
    assert np.array_equal(np.array(got["last_H"]).reshape(6, 6), ref["last"]["H_ss"]) and np.array_equal(np.array(got["last_b"]), ref["last"]["b_s"])
    assert got["last_f"] == ref["last"]["f"]
    after = fac.linearize(ref["R"], ref["t"])
    assert got["count_after_linearize"] == ref["iters"] + 1 == after["linearize_count"] and got["f_at_aligned_pose"] == after["f"]
    fac.destroy()
    gm.release()


def _cfg(**kw):
    from mimosa_amd import replay
    return replay.ReplayConfig(n_scans=5, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2, keyframe_rot_thresh_deg=5.0,
                               photometric=False, **kw)


def _worst(a, b):
    return max(float(np.linalg.norm(ta - tb)) for (_, ta), (_, tb) in zip(a, b))


@pytest.mark.gpu
def test_replays_init_align(ctx, tmp_path):
    from mimosa_amd import replay
    base = _cfg()
    scans = replay.make_scans(base)
    # ---- with the usual error of the first guess: the trajectory starts elsewhere
    on = _cfg(init_align=True)
    p_off = replay.run(base, replay.HipBackend(ctx, base), scans)
    p_on = replay.run(on, replay.HipBackend(ctx, on), scans)
    n_off, n_on = replay.run_native(base, scans, str(tmp_path)), replay.run_native(on, scans, str(tmp_path))
    assert n_off["init_align_iters"] == 0 and n_on["init_align_iters"] >= 2
    d_py, d_nat = _worst(p_on["poses_est"][:1], p_off["poses_est"][:1]), _worst(n_on["poses_est"][:1], n_off["poses_est"][:1])
    print("first pose, init_align on against off: python %.3e m, native %.3e m" % (d_py, d_nat))
    assert d_py > 0.0 and d_nat > 0.0
    assert _worst(n_on["poses_est"], p_on["poses_est"]) < 1e-7  # the two replays agree with each other as they do without it
    assert max(p_on["trans_err"]) < 0.05  # it still tracks the ground truth
    # ---- zero perturbation of the first pose: the two trajectories agree to 1e-9 m
    z_off, z_on = _cfg(prior_trans_noise=0.0, prior_rot_noise_deg=0.0), _cfg(prior_trans_noise=0.0, prior_rot_noise_deg=0.0, init_align=True)
    a, b = replay.run(z_off, replay.HipBackend(ctx, z_off), scans), replay.run(z_on, replay.HipBackend(ctx, z_on), scans)
    c, d = replay.run_native(z_off, scans, str(tmp_path)), replay.run_native(z_on, scans, str(tmp_path))
    w_py, w_nat = _worst(a["poses_est"], b["poses_est"]), _worst(c["poses_est"], d["poses_est"])
    print("zero perturbation, init_align on against off: python %.3e m, native %.3e m" % (w_py, w_nat))
    assert w_py <= 1e-9 and w_nat <= 1e-9
