"""The C++ host mirror's ICPFactor::optimiseWindowEdges / optimiseWindowEdgesAsync and windowEdgeFromSigmas
(mimosa_amd/host/mimosa_hip/lidar.hpp) through tests/cpp/window_edge_pipeline.cpp: without an edge the result of
optimiseWindowLin, bit for bit; with edges (dense information matrices and diagonal sigmas), blocking, asynchronous and under
the reference's thresholds, the result of the C ABI call on the same inputs, bit for bit (the same library)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import window_edge_ref as ref
import window_lin_ref as lin_ref
from test_gpu_host_cpp import build_exe


def test_window_edge_case_compiles():
    """CPU-runnable: the mirror's optimiseWindowEdges / optimiseWindowEdgesAsync build warning-free against the C ABI."""
    assert os.path.exists(build_exe("window_edge_pipeline"))


@pytest.mark.gpu
def test_cpp_mirror_optimise_window_edges(ctx, tmp_path):
    from mimosa_amd import capi, synth
    m, scan, aux = synth.small_world()
    pts = np.ascontiguousarray(scan)
    Rt, tt = np.array(aux["R_W_L"]), np.array(aux["t_W_L"])
    W = 4
    rng = np.random.default_rng(23)
    poses = [(Rt @ synth.so3_exp(rng.standard_normal(3) * 0.02), tt + rng.standard_normal(3) * 0.05) for _ in range(W)]
    has_Z = [0, 1, 0, 1]
    Z = [(np.eye(3), np.zeros(3))] * W
    linear = [lin_ref.random_linear(rng, i, poses[i]) for i in (0, 2)]
    dense = [ref.random_edge(rng, a, b, poses) for a, b in ((0, 3), (1, 2), (1, 2))]
    sigmas = np.array([np.deg2rad(0.5)] * 3 + [0.02] * 3)
    diag = [ref.random_edge(rng, 0, 2, poses, info=np.diag(1.0 / (sigmas * sigmas)))]
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
        w(np.concatenate([np.concatenate([[float(e["a"]), float(e["b"])], e["Z"][0].ravel(), e["Z"][1], e["info"].ravel()]) for e in dense]))
        w(np.concatenate([np.concatenate([[float(e["a"]), float(e["b"])], e["Z"][0].ravel(), e["Z"][1], sigmas]) for e in diag]))
    out = subprocess.run([build_exe("window_edge_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lin_only, none, given, given_async, given_relin = json.loads(out.stdout)["runs"]
    assert lin_only["iters"] >= 2 and none["evaluated"] == [] and given["evaluated"] == []
    for key in ("iters", "converged", "poses", "trace", "counts", "last_f"):
        assert none[key] == lin_only[key], key
        assert given_async[key] == given[key], key
    assert given["poses"] != lin_only["poses"]

    gm = capi.VoxelMap(ctx)
    gm.insert(m)
    for got, rl in ((given, None), (given_relin, relin)):
        fs = [capi.ICPFactor(ctx, gm, pts, reg) for _ in range(W)]
        for f in fs:
            f.set_components(False)
        want = capi.optimise_window(fs, poses, cfg, has_Z=has_Z, Z=Z, relin=rl, linear=linear, edges=dense + diag)
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
