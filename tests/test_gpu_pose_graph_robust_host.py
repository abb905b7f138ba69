"""-m gpu: the pose graph's priors and losses through the C++ host mirror (lidar.hpp: PoseGraph setPriors / setLoss /
priorResiduals / weights, posePrior) against the same calls made through the C ABI (tests/cpp/pose_graph_robust_pipeline.cpp),
and the result against the numpy restatement."""
import json
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_robust_cases as cases
import pose_graph_robust_ref as rref
from test_gpu_host_cpp import build_exe


def test_host_layer_compiles():
    """CPU-runnable: the program builds warning-free against the mirror and the C ABI"""
    import os
    assert os.path.exists(build_exe("pose_graph_robust_pipeline"))


@pytest.mark.gpu
def test_mirror_calls_are_the_c_abi_calls(tmp_path):
    name = "n257_mixed"
    c, want = cases.case(name), cases.restated(name)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr, np.float64).ravel()
            f.write(struct.pack("<Q", arr.size))
            f.write(arr.tobytes())
        w(np.concatenate([c["R"].reshape(-1, 9), c["t"]], axis=1))
        w(c["fixed"])
        w(np.array([np.concatenate([[a, b], ZR.ravel(), Zt, Om.ravel()]) for a, b, ZR, Zt, Om in c["edges"]]))
        w(np.array([np.concatenate([[i], ZR.ravel(), Zt, Om.ravel()]) for i, ZR, Zt, Om in c["priors"]]))
        w(np.array(c["edge_loss"], np.float64))
        w(np.array(c["prior_loss"], np.float64))
        w([cases.ITERS, 3, 0.0, 0.0, 0.0])
    out = subprocess.run([build_exe("pose_graph_robust_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    print({k: v for k, v in got.items() if k not in ("poses", "w_edges")})
    for k in ("priors_equal", "evaluations_equal", "optimise_equal", "dropped"):
        assert got[k] == 1, k
    assert (got["iters"], got["converged"], got["n_far"]) == (cases.ITERS, 0, 4)
    we, wp, f = cases.restated_weights(name)
    assert np.abs(np.array(got["w_edges"]) - we).max() <= cases.W_TOL and np.abs(np.array(got["w_priors"]) - wp).max() <= cases.W_TOL
    chi2 = rref.prior_residuals(c["R"], c["t"], c["priors"])[1]
    assert np.all(np.abs(np.array(got["prior_chi2"]) - chi2) <= cases.F_RTOL * chi2 + cases.base.f_floor(1))
    assert cases.f_close(got["f"], f, cases.n_terms(c)) and got["f_first"] == got["f"]
    P = np.array(got["poses"]).reshape(-1, 12)
    dt, dr = ref.pose_error(P[:, :9], P[:, 9:], want["R"], want["t"])
    assert dt <= cases.POSE_TOL and dr <= cases.POSE_TOL
