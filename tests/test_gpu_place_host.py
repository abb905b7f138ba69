"""-m gpu: place recognition through the C++ host mirror (lidar.hpp: PlaceDatabase, levelRotation, placeCandidatePose) against the same
calls made through the C ABI (tests/cpp/place_pipeline.cpp), and the mirror's two helpers against capi's."""
import json
import struct
import subprocess

import numpy as np
import pytest

import place_ref as ref
import place_scenes as scenes
from test_gpu_host_cpp import _pose12, build_exe
from test_gpu_place import raw_scan_of


def test_host_layer_compiles():
    """CPU-runnable: the program builds warning-free against the mirror and the C ABI"""
    import os
    assert os.path.exists(build_exe("place_pipeline"))


@pytest.mark.gpu
def test_mirror_calls_are_the_c_abi_calls(tmp_path):
    from mimosa_amd import capi
    c = scenes.queries()[0]
    k0, k1 = int(c["top"][0]), int(c["top"][1])
    g = np.array([0.05, -0.08, -1.0])
    g /= np.linalg.norm(g)
    xy, yaw, _ = scenes.keyframes()[k0]
    T_k = scenes.pose_of(xy, yaw)
    shift = int(c["shift"][k0])
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            f.write(struct.pack("<Q", arr.size if arr.dtype.itemsize != 32 else len(arr)))
            f.write(arr.tobytes())
        w(raw_scan_of(scenes.keyframes()[k0][2]))
        w(raw_scan_of(scenes.keyframes()[k1][2]))
        w(raw_scan_of(c["cloud"]))
        w(np.concatenate([g, _pose12(*T_k), [float(shift)]]))
    out = subprocess.run([build_exe("place_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    print({k: v for k, v in got.items() if not k.startswith("level") and k != "candidate_R"})
    for k in ("describe_equal", "get_equal", "query_equal"):
        assert got[k] == 1, k
    assert got["add_indices"] == [0, 1, 1] and got["sizes"] == [2, 2] and got["occupied"] > 100
    # the hits are the restatement's for a database of these two keyframes
    K = scenes.keyframe_descriptors()[[k0, k1]]
    D, s, _ = ref.distances(c["desc"], K, scenes.SCENE_CFG["min_overlap"])
    want = ref.rank(D, 4)
    assert [h[0] for h in got["hits"]] == want.tolist() == [0, 1, -1, -1]
    assert [h[1] for h in got["hits"][:2]] == s[want[:2]].tolist() and [h[3] for h in got["hits"]] == [70, 71, 0, 0]
    assert abs(got["hits"][0][2] - D[0]) <= 1e-12 and abs(got["hits"][1][2] - D[1]) <= 1e-12
    # the helpers are capi's
    L = capi.level_rotation(g)
    assert np.allclose(np.array(got["level"]).reshape(3, 3), L, atol=1e-15)
    assert got["level_down"] == np.eye(3).ravel().tolist() and got["level_up"] == [1, 0, 0, 0, -1, 0, 0, 0, -1]
    R, _ = capi.place_candidate_pose(T_k, L, None, shift)
    assert np.allclose(np.array(got["candidate_R"]).reshape(3, 3), R, atol=1e-14)
