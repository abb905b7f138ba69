"""-m gpu: the pose graph's marginal covariances through the C++ host mirror (lidar.hpp: PoseGraph covariances /
jointCovariances / gate) against the same call made through the C ABI (tests/cpp/pose_graph_cov_pipeline.cpp), and the result
against the dense restatement (tests/pose_graph_cov_ref.py): the 64-pose circuit with a false loop, its far edges held out as
the gate's candidates."""
import json
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_cov_cases as cases
import pose_graph_cov_ref as cref
from test_gpu_host_cpp import build_exe


def test_host_layer_compiles():
    """CPU-runnable: the program builds warning-free against the mirror and the C ABI"""
    import os
    assert os.path.exists(build_exe("pose_graph_cov_pipeline"))


@pytest.mark.gpu
def test_mirror_calls_are_the_c_abi_calls(tmp_path):
    g, cand = cases.held_out(cases.case("n64_false_loop_cauchy"))
    pairs = [q[:2] for q in cand]
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr, np.float64).ravel()
            f.write(struct.pack("<Q", arr.size))
            f.write(arr.tobytes())
        row = lambda edges: np.array([np.concatenate([[a, b], ZR.ravel(), Zt, Om.ravel()]) for a, b, ZR, Zt, Om in edges])
        w(np.concatenate([g["R"].reshape(-1, 9), g["t"]], axis=1))
        w(g["fixed"])
        w(row(g["edges"]))
        w(row(cand))
        w([g["damping"]])
    out = subprocess.run([build_exe("pose_graph_cov_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    print({k: v for k, v in got.items() if k not in ("cov", "joint", "r")})
    assert (got["calls_equal"], got["flags"], got["n_far"], got["valid"]) == (1, 0, 0, 1)
    # against the restatement: the covariances to the measured bar of this graph, the gate's figures and its verdicts
    A = cref.system_of(g)
    want_cov, want_joint = cref.covariances(g, None, pairs, A)
    plain = cref.plain_inverse(g, None, A)
    free = [i for i in want_cov if not g["fixed"][i]]
    scale = max(np.abs(want_cov[i]).max() for i in free)
    bar = max(cases.MARGIN * max(np.abs(plain[i] - want_cov[i]).max() for i in free) / scale, cases.FLOOR)
    cov, joint = np.array(got["cov"]).reshape(-1, 6, 6), np.array(got["joint"]).reshape(-1, 12, 12)
    err = max(max(np.abs(cov[i] - want_cov[i]).max() for i in want_cov), max(np.abs(a - b).max() for a, b in zip(joint, want_joint))) / scale
    print("relative error %.3g, bar %.3g" % (err, bar))
    assert err <= bar
    r, chi2, d2 = cref.gate(g["R"], g["t"], cand, want_joint)
    assert np.allclose(np.array(got["r"]).reshape(-1, 6), r, rtol=0, atol=1e-12) and np.allclose(got["chi2"], chi2, rtol=1e-9) and np.allclose(got["d2"], d2, rtol=1e-6)
    d2 = np.array(got["d2"])
    assert np.all(d2[:3] < cref.CHI2_6_999 / 4.0) and d2[3] > 4.0 * cref.CHI2_6_999 and np.all(np.array(got["chi2"])[:3] > cref.CHI2_6_999)
