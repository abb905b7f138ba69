"""-m gpu: a wide pose graph through the C++ host mirror (lidar.hpp: PoseGraph with a max_far) against the same calls made through
the C ABI (tests/cpp/pose_graph_wide_pipeline.cpp), and the result against the numpy restatement."""
import json
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_ref as ref
import pose_graph_wide_cases as cases
from test_gpu_host_cpp import build_exe


def test_host_layer_compiles():
    """CPU-runnable: the program builds warning-free against the mirror and the C ABI"""
    import os
    assert os.path.exists(build_exe("pose_graph_wide_pipeline"))


@pytest.mark.gpu
def test_mirror_calls_are_the_c_abi_calls(tmp_path):
    name = "w80_far70"
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
        w([cases.ITERS, 3, 0.0, 0.0, 0.0, 70])
    out = subprocess.run([build_exe("pose_graph_wide_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    print({k: v for k, v in got.items() if k != "poses"})
    for k in ("residuals_equal", "optimise_equal", "poses_equal"):
        assert got[k] == 1, k
    assert (got["iters"], got["converged"], got["n_far"]) == (cases.ITERS, 0, 70)
    assert cases.f_close(got["f"], ref.residuals(c["R"], c["t"], c["edges"])[2], len(c["edges"])) and got["f_first"] == got["f"]
    P = np.array(got["poses"]).reshape(-1, 12)
    dt, dr = ref.pose_error(P[:, :9], P[:, 9:], want["R"], want["t"])
    assert dt <= cases.POSE_TOL and dr <= cases.POSE_TOL
