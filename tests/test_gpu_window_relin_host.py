"""The C++ host mirror's ICPFactor::optimiseWindowRelin / optimiseWindowRelinAsync (mimosa_amd/host/mimosa_hip/lidar.hpp) through
tests/cpp/window_relin_pipeline.cpp: at thresholds 0 the result of optimiseWindow, bit for bit, blocking and asynchronous, the
masks all ones; at the reference's thresholds the result of the C ABI call on the same inputs, bit for bit (the same library)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_host_cpp import build_exe


def test_window_relin_case_compiles():
    """CPU-runnable: the mirror's optimiseWindowRelin / optimiseWindowRelinAsync build warning-free against the C ABI."""
    assert os.path.exists(build_exe("window_relin_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_optimise_window_relin(ctx, tmp_path):
    from mimosa_amd import capi, synth
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
    out = subprocess.run([build_exe("window_relin_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    plain, zero, zero_async, given = json.loads(out.stdout)["runs"]
    assert plain["iters"] >= 2 and plain["evaluated"] == []
    for got in (zero, zero_async):
        assert got["evaluated"] == [(1 << W) - 1] * plain["iters"]
        for key in ("iters", "converged", "poses", "trace", "counts", "last_f"):
            assert got[key] == plain[key], key

    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    fs = [capi.ICPFactor(ctx, gm, pts, reg) for _ in range(W)]
    for f in fs:
        f.set_components(False)
    ref = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, relin=relin)
    assert given["iters"] == ref["iters"] and given["converged"] == ref["converged"]
    assert given["evaluated"] == [int(v) for v in ref["evaluated"]] and any(v != (1 << W) - 1 for v in given["evaluated"])
    for i, p in enumerate(given["poses"]):
        assert np.array_equal(np.array(p["R"]).reshape(3, 3), ref["R"][i]) and np.array_equal(np.array(p["t"]), ref["t"][i])
    assert [tuple(r) for r in given["trace"]] == [(r["f"], r["step_rot"], r["step_trans"], r["flags"], r["degenerate"]) for r in ref["trace"]]
    assert given["counts"] == [r["linearize_count"] for r in ref["last"]] == [sum((int(v) >> i) & 1 for v in ref["evaluated"]) for i in range(W)]
    assert given["last_f"] == [r["f"] for r in ref["last"]]
    for f in fs:
        f.destroy()
    gm.release()
