"""The C++ host mirror's ICPFactor::optimiseWindowLin / optimiseWindowLinAsync and windowLinearFrom
(mimosa_amd/host/mimosa_hip/lidar.hpp) through tests/cpp/window_lin_pipeline.cpp: without a linear factor the result of
optimiseWindow, bit for bit; with linear factors, blocking, asynchronous and under the reference's thresholds, the result of
the C ABI call on the same inputs, bit for bit (the same library)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import window_lin_ref as ref
from test_gpu_host_cpp import build_exe


def test_window_lin_case_compiles():
    """CPU-runnable: the mirror's optimiseWindowLin / optimiseWindowLinAsync build warning-free against the C ABI."""
    assert os.path.exists(build_exe("window_lin_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_optimise_window_lin(ctx, tmp_path):
    from mimosa_amd import capi, synth
    m, scan, aux = synth.small_world()
    pts = np.ascontiguousarray(scan)
    Rt, tt = np.array(aux["R_W_L"]), np.array(aux["t_W_L"])
    W = 4
    rng = np.random.default_rng(19)
    poses = [(Rt @ synth.so3_exp(rng.standard_normal(3) * 0.02), tt + rng.standard_normal(3) * 0.05) for _ in range(W)]
    has_Z = [0, 1, 0, 1]
    Z = [(np.eye(3), np.zeros(3))] * W
    linear = [ref.random_linear(rng, i, poses[i]) for i in (0, 2, 2, 3)]
    reg = capi.make_reg_config(**synth.enwide_config())
    cfg = capi.make_window_config(iters=7, eps_rot=1e-7, eps_trans=1e-7, check_every=3)
    relin = (1.75e-2, 5.0e-3)
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
        w(np.array(relin, float))
        w(np.concatenate([np.concatenate([[float(l["pose"])], l["at"][0].ravel(), l["at"][1], l["H"].ravel(), l["b"], [l["f"]]]) for l in linear]))
    out = subprocess.run([build_exe("window_lin_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain, none, given, given_async, given_relin = json.loads(out.stdout)["runs"]
    assert plain["iters"] >= 2 and none["evaluated"] == [] and given["evaluated"] == []
    for key in ("iters", "converged", "poses", "trace", "counts", "last_f"):
        assert none[key] == plain[key], key
        assert given_async[key] == given[key], key
    assert given["poses"] != plain["poses"]

    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    for got, rl in ((given, None), (given_relin, relin)):
        fs = [capi.ICPFactor(ctx, gm, pts, reg) for _ in range(W)]
        for f in fs:
            f.set_components(False)
        want = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, relin=rl, linear=linear)
        assert got["iters"] == want["iters"] and got["converged"] == want["converged"]
        for i, p in enumerate(got["poses"]):
            assert np.array_equal(np.array(p["R"]).reshape(3, 3), want["R"][i]) and np.array_equal(np.array(p["t"]), want["t"][i])
        assert [tuple(r) for r in got["trace"]] == [(r["f"], r["step_rot"], r["step_trans"], r["flags"], r["degenerate"]) for r in want["trace"]]
        assert got["counts"] == [r["linearize_count"] for r in want["last"]]
        assert got["last_f"] == [r["f"] for r in want["last"]]
        if rl is not None:
            assert got["evaluated"] == [int(v) for v in want["evaluated"]]
        for f in fs:
            f.destroy()
    gm.release()
