"""-m gpu: map carving through the C++ host mirror (IncrementalVoxelMapPCL::carve / carveFromScan, Geometric::updateMap with
GeometricConfig::map_carve_grid) against the same calls made through the C ABI (tests/cpp/map_carve_pipeline.cpp).  With the switch
off, updateMap is the copy + transform + insert it was."""
import json
import struct
import subprocess

import numpy as np
import pytest

import map_carve_scenes as scenes
from test_gpu_host_cpp import _pose12, build_exe


def test_host_layer_compiles():
    """CPU-runnable: the program builds warning-free against the mirror and the C ABI"""
    import os
    assert os.path.exists(build_exe("map_carve_pipeline"))


@pytest.mark.gpu
def test_mirror_calls_are_the_c_abi_calls(tmp_path, small_world):
    from mimosa_amd import synth
    room = np.array([6.0, 5.0, 3.0])
    scan, aux = synth.make_scan(n_rows=16, seed=1235, n_cols=64, room=room, sensor_local=np.array([2.3, 2.6, 1.2]))
    raw, _ = synth.make_raw_scan(16, seed=1235, n_cols=64, room=room, sensor_local=np.array([2.3, 2.6, 1.2]), dropouts=False, v=(0.0, 0.0, 0.0),
                                 w=(0.0, 0.0, 0.0))
    assert np.array_equal(raw["x"], scan["x"])             # a sensor at rest: the raw cloud is the deskewed one
    T_B_L = (synth.so3_exp(np.array([0.01, -0.02, 0.03])), np.array([0.05, 0.02, -0.1]))
    R_WB = aux["R_W_L"] @ T_B_L[0].T
    t_WB = aux["t_W_L"] - R_WB @ T_B_L[1]
    S = scenes.random_scene(31, small_world)
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            f.write(struct.pack("<Q", arr.size if arr.dtype.itemsize != 32 else len(arr)))
            f.write(arr.tobytes())
        w(S["map_batches"][0].astype(np.float32).ravel())
        w(S["map_batches"][1].astype(np.float32).ravel())
        w(scan)
        w(raw)
        w(np.concatenate([_pose12(*T_B_L), _pose12(R_WB, t_WB)]))
    out = subprocess.run([build_exe("map_carve_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    print(got)
    for k in ("preview_equal", "preview_moves_nothing", "apply_equal", "apply_clouds_equal", "off_equal", "on_equal", "on_counters_equal", "on_carved",
              "device_equal", "device_counters_equal"):
        assert got[k] == 1, k
    assert got["off_carved"] == 0
    n_removed = got["preview"][3]
    assert n_removed > 100 and got["points_before"] - got["points_after"] == n_removed
    assert got["update_map"] == got["preview"]
    assert got["update_map_device"][0] > 0 and got["update_map_device"][3] > 0
