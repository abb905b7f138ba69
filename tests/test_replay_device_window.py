"""Sequence replay with the smoother's loop on the device (ReplayConfig.device_window / replay::Config::device_window): the
update_iters Gauss-Newton iterations over the window run as one mh_icp_window_optimise call instead of a batched linearize, a
host solve and the retractions per iteration.  10 scans without the photometric factor, sizes of tests/test_replay.py; the
trajectory must match the one without the switch to 1e-9 m (1e-9 on the rotation entries), in the Python and in the native
replay.  The switch is off by default and refused where it is not offered."""
import dataclasses

import numpy as np
import pytest

from mimosa_amd import replay


def small_cfg(n=10, **kw):
    return replay.ReplayConfig(n_scans=n, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2,
                               keyframe_rot_thresh_deg=5.0, photometric=False, **kw)


def test_switch_is_opt_in_and_refused_where_it_is_not_offered():
    assert not replay.ReplayConfig().device_window

    class NoDevice:  # a backend without mh_icp_window_optimise
        pass

    with pytest.raises(ValueError, match="device_window"):
        replay.run(small_cfg(2, device_window=True), NoDevice(), scans=[])
    with pytest.raises(ValueError, match="photometric"):
        replay.run(dataclasses.replace(small_cfg(2, device_window=True), photometric=True), NoDevice(), scans=[])


def _same_trajectory(a, b, tag):
    dt = max(float(np.max(np.abs(ta - tb))) for (_, ta), (_, tb) in zip(a["poses_est"], b["poses_est"]))
    dR = max(float(np.max(np.abs(Ra - Rb))) for (Ra, _), (Rb, _) in zip(a["poses_est"], b["poses_est"]))
    print(f"{tag}: device_window on vs off: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}")
    assert len(a["poses_est"]) == len(b["poses_est"]) and a["n_keyframes"] == b["n_keyframes"]
    assert dt <= 1e-9 and dR <= 1e-9


@pytest.mark.gpu
def test_python_replay_with_device_window(ctx):
    cfg = small_cfg()
    scans = replay.make_scans(cfg)
    off = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    on_cfg = dataclasses.replace(cfg, device_window=True)
    on = replay.run(on_cfg, replay.HipBackend(ctx, on_cfg), scans)
    _same_trajectory(on, off, "python")
    assert [len(c) for c in on["costs"]] == [cfg.update_iters] * cfg.n_scans
    assert np.allclose(np.concatenate(on["costs"]), np.concatenate(off["costs"]), rtol=1e-6)
    assert max(on["trans_err"]) < 0.012 and max(on["rot_err_deg"]) < 0.06


@pytest.mark.gpu
def test_native_replay_with_device_window(tmp_path):
    cfg = small_cfg()
    scans = replay.make_scans(cfg)
    on_cfg = dataclasses.replace(cfg, device_window=True)
    off = replay.run_native(cfg, scans, str(tmp_path))
    on = replay.run_native(on_cfg, scans, str(tmp_path))
    _same_trajectory(on, off, "native")
    assert np.allclose(on["first_costs"], off["first_costs"], rtol=1e-6)
    seq = replay.run_native(on_cfg, scans, str(tmp_path), sequential=True)
    for (Ra, ta), (Rb, tb) in zip(on["poses_est"], seq["poses_est"]):
        assert np.array_equal(ta, tb) and np.array_equal(Ra, Rb)
    for kw in (dict(through_manager=True), dict(sharded_world=1)):
        with pytest.raises(RuntimeError, match="device_window"):
            replay.run_native(on_cfg, scans[:2], str(tmp_path), **kw)
    with pytest.raises(RuntimeError, match="device_window"):
        replay.run_native(dataclasses.replace(on_cfg, photometric=True), scans[:2], str(tmp_path))


def test_window_case_compiles():
    """CPU-runnable: the mirror's optimiseWindow / optimiseWindowAsync build warning-free against the C ABI."""
    import os
    from test_gpu_host_cpp import build_exe
    assert os.path.exists(build_exe("window_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_optimise_window_is_the_c_abi_call(ctx, tmp_path):
    import json
    import struct
    import subprocess
    from mimosa_amd import capi, synth
    from test_gpu_host_cpp import build_exe
    m, scan, aux = synth.small_world()
    pts = np.ascontiguousarray(scan)
    Rt, tt = np.array(aux["R_W_L"]), np.array(aux["t_W_L"])
    W = 4
    rng = np.random.default_rng(17)
    poses = [(Rt @ synth.so3_exp(rng.standard_normal(3) * 0.02), tt + rng.standard_normal(3) * 0.05) for _ in range(W)]
    has_Z = [0, 1, 0, 1]
    Z = [(np.eye(3), np.zeros(3))] * W
    reg = capi.make_reg_config(**synth.enwide_config())
    cfg = capi.make_window_config(iters=7, eps_rot=1e-7, eps_trans=1e-7, check_every=3)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            f.write(struct.pack("<Q", arr.size if arr.dtype.itemsize != 32 else len(arr)))
            f.write(arr.tobytes())
        w(m.astype(np.float32).ravel())
        w(pts)
        w(np.frombuffer(bytes(reg), np.uint8))
        w(np.concatenate([np.concatenate([R.ravel(), t]) for R, t in poses]))
        w(np.concatenate([np.concatenate([[float(h)], R.ravel(), t]) for h, (R, t) in zip(has_Z, Z)]))
        w(np.array([cfg.iters] + list(cfg.between_info) + list(cfg.prior_info) + [cfg.damping, cfg.eps_rot, cfg.eps_trans, cfg.check_every], float))
    out = subprocess.run([build_exe("window_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    runs = json.loads(out.stdout)["runs"]

    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    fs = [capi.ICPFactor(ctx, gm, pts, reg) for _ in range(W)]
    ref = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z)
    assert 1 <= ref["iters"] <= 7
    for got in runs:  # the blocking and the asynchronous call: the same library on the same inputs, bit for bit
        assert got["iters"] == ref["iters"] and got["converged"] == ref["converged"]
        for i, p in enumerate(got["poses"]):
            assert np.array_equal(np.array(p["R"]).reshape(3, 3), ref["R"][i]) and np.array_equal(np.array(p["t"]), ref["t"][i])
        assert [tuple(r) for r in got["trace"]] == [(r["f"], r["step_rot"], r["step_trans"], r["flags"], r["degenerate"]) for r in ref["trace"]]
        assert got["counts"] == [ref["iters"]] * W == [r["linearize_count"] for r in ref["last"]]
        assert got["last_f"] == [r["f"] for r in ref["last"]]
    for f in fs:
        f.destroy()
    gm.release()
