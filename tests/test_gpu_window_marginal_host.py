"""The C++ host mirror's ICPFactor::marginaliseWindow / marginaliseWindowAsync (mimosa_amd/host/mimosa_hip/lidar.hpp) through
tests/cpp/window_marginal_pipeline.cpp: blocking and asynchronous, the result of the C ABI call on the same inputs, bit for bit
(the same library); and the WindowLinear it returns goes into optimiseWindowLin as capi's dict goes into optimise_window."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import window_edge_ref as ref
import window_lin_ref as lin_ref
from test_gpu_host_cpp import build_exe


def test_window_marginal_case_compiles():
    """CPU-runnable: the mirror's marginaliseWindow / marginaliseWindowAsync build warning-free against the C ABI."""
    assert os.path.exists(build_exe("window_marginal_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_marginalise_window(ctx, tmp_path):
    from mimosa_amd import capi, synth
    m, scan, aux = synth.small_world()
    pts = np.ascontiguousarray(scan)
    Rt, tt = np.array(aux["R_W_L"]), np.array(aux["t_W_L"])
    W = 3
    rng = np.random.default_rng(29)
    poses = [(Rt @ synth.so3_exp(rng.standard_normal(3) * 0.02), tt + rng.standard_normal(3) * 0.05) for _ in range(W)]
    has_Z = [0, 1, 1]
    Z = [(np.eye(3), np.zeros(3))] * W
    linear = [lin_ref.random_linear(rng, i, poses[i]) for i in (0, 1, 0)]
    edges = [ref.random_edge(rng, a, b, poses) for a, b in ((0, 1), (1, 2), (0, 1))]
    reg = capi.make_reg_config(**synth.enwide_config())
    cfg = capi.make_window_config(iters=3, prior_sigma_rot=0.017453292519943295, prior_sigma_trans=0.1)
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
        w(np.concatenate([np.concatenate([[float(l["pose"])], l["at"][0].ravel(), l["at"][1], l["H"].ravel(), l["b"], [l["f"]]]) for l in linear]))
        w(np.concatenate([np.concatenate([[float(e["a"]), float(e["b"])], e["Z"][0].ravel(), e["Z"][1], e["info"].ravel()]) for e in edges]))
    out = subprocess.run([build_exe("window_marginal_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    blocking, asynchronous = got["runs"]
    assert blocking == asynchronous

    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    fs = [capi.ICPFactor(ctx, gm, pts, reg) for _ in range(W)]
    for f in fs:
        f.set_components(False)
    want = capi.marginalise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, linear=linear, edges=edges)
    assert blocking["valid"] == want["valid"] == 1 and blocking["n_ties"] == want["n_ties"] == 3 and blocking["pose"] == want["linear"]["pose"] == 0
    assert np.array_equal(np.array(blocking["H"]).reshape(6, 6), want["linear"]["H"]) and np.array_equal(np.array(blocking["b"]), want["linear"]["b"])
    assert blocking["f"] == want["linear"]["f"] and blocking["oldest_f"] == want["oldest"]["f"]
    assert np.array_equal(np.array(blocking["at_R"]).reshape(3, 3), poses[1][0]) and np.array_equal(np.array(blocking["at_t"]), poses[1][1])
    assert blocking["counts"][0] == want["oldest"]["linearize_count"] == 1
    # the window without its oldest pose, the marginal as its prior
    cfg0 = capi.make_window_config(iters=3, prior_info=[0.0] * 6)
    slid = capi.optimise_window(fs[1:], poses[1:], cfg0, has_Z=[0, 1], Z=Z[1:], linear=[want["linear"]])
    assert got["slid"]["iters"] == slid["iters"] == 3
    for i, p in enumerate(got["slid"]["poses"]):
        assert np.array_equal(np.array(p["R"]).reshape(3, 3), slid["R"][i]) and np.array_equal(np.array(p["t"]), slid["t"][i])
    for f in fs:
        f.destroy()
    gm.release()
