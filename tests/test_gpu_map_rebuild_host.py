"""-m gpu: the keyframe cloud store and the map rebuild through the C++ host mirror (KeyframeStore, Geometric::rebuildMap with
GeometricConfig::map_keyframe_store_capacity) against the map updateMap grew and against a twin made through the C ABI
(tests/cpp/map_rebuild_pipeline.cpp).  With the switch off no store exists and updateMap builds the map it built before."""
import json
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_host_cpp import _pose12, build_exe

K = 12  # iVox purges every 10 inserts: one purge falls inside the run


def test_host_layer_compiles():
    """CPU-runnable: the program builds warning-free against the mirror and the C ABI"""
    import os
    assert os.path.exists(build_exe("map_rebuild_pipeline"))


@pytest.mark.gpu
def test_mirror_rebuild_equals_the_grown_map(tmp_path):
    from mimosa_amd import synth
    room = np.array([6.0, 5.0, 3.0])
    T_B_L = (synth.so3_exp(np.array([0.01, -0.02, 0.03])), np.array([0.05, 0.02, -0.1]))
    poses, clouds = [_pose12(*T_B_L)], []
    for k in range(K):
        sensor = np.array([1.2 + 0.3 * k, 1.5 + 0.15 * k, 1.2])
        scan, aux = synth.make_scan(n_rows=16, seed=1300 + k, n_cols=64, room=room, sensor_local=sensor)
        raw, _ = synth.make_raw_scan(16, seed=1300 + k, n_cols=64, room=room, sensor_local=sensor, dropouts=False, v=(0.0, 0.0, 0.0), w=(0.0, 0.0, 0.0))
        assert np.array_equal(raw["x"], scan["x"])             # a sensor at rest: the raw cloud is the deskewed one
        R_WB = aux["R_W_L"] @ T_B_L[0].T
        poses.append(_pose12(R_WB, aux["t_W_L"] - R_WB @ T_B_L[1]))
        clouds.append((scan, raw))
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            f.write(struct.pack("<Q", arr.size if arr.dtype.itemsize != 32 else len(arr)))
            f.write(arr.tobytes())
        w(np.concatenate(poses))
        for scan, raw in clouds:
            w(scan)
            w(raw)
    out = subprocess.run([build_exe("map_rebuild_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    print(got)
    for k in ("store_roundtrip", "store_full_throws", "device_same_poses_equal", "device_is_a_new_map", "shifted_equal", "shifted_differs_from_grown",
              "map_poses_replaced", "wrong_length_throws", "host_same_poses_equal", "off_no_store", "off_map_unchanged", "off_rebuild_throws",
              "carved_rebuild_throws"):
        assert got[k] == 1, k
    assert got["device_keyframes"] == K and got["device_points"] > 1000
