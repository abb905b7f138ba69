"""Geometric::updateMap of the C++ host mirror with GeometricConfig::map_keyframe_min_new_fraction (tests/cpp/
map_preview_pipeline.cpp): two updateMap calls per run.  At 0 the decisions and the map's stats are those of the pose rule — forced
first keyframe = copy + insert (the same steps through the Python binding), second pose within the pose thresholds = no update —
and no preview runs.  At a fraction > 0 debug().map_new_fraction is n_added / n_points of a previewInsertBodyCloud the driver makes
itself, map_updated follows it, and the host-cloud path (mh_transform_f32 + previewInsert) gives the device path's counts."""
import json
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_host_cpp import _pose12, build_exe

FRACTIONS = [0.0, 1e-6, 0.99]


def test_map_preview_case_compiles():
    """CPU-runnable: the mirror's preview calls and the keyframe switch build warning-free against the C ABI."""
    import os
    assert os.path.exists(build_exe("map_preview_pipeline"))


@pytest.mark.gpu
def test_update_map_by_new_fraction(ctx, tmp_path):
    from mimosa_amd import capi, synth
    room = np.array([6.0, 5.0, 3.0])
    map_xyz = synth.make_room(1234, 0, 0, room=room)
    scan, aux = synth.make_scan(n_rows=32, seed=77, skew=True, n_cols=256, room=room, sensor_local=np.array([2.3, 2.6, 1.2]))
    raw, _ = synth.make_raw_scan(32, seed=77, n_cols=256, room=room, sensor_local=np.array([2.3, 2.6, 1.2]), dropouts=False)
    T_B_L = (synth.so3_exp(np.array([0.01, -0.02, 0.03])), np.array([0.05, 0.02, -0.1]))
    R_WL, t_WL = synth.query_pose(aux["R_W_L"], aux["t_W_L"])
    R_WB = R_WL @ T_B_L[0].T
    t_WB = t_WL - R_WB @ T_B_L[1]
    # 0.3 m and 0.6 degrees on: inside the pose rule's thresholds of the driver (2 m, 30 degrees), far enough to add points
    R_WB2, t_WB2 = R_WB @ synth.so3_exp(np.array([0.0, 0.0, 0.01])), t_WB + np.array([0.25, 0.15, 0.05])
    poses = np.concatenate([aux["Rt12"][g].astype(np.float64) for g in range(len(aux["unique_ns"]))])
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            f.write(struct.pack("<Q", arr.size if arr.dtype.itemsize != 32 else len(arr)))
            f.write(arr.tobytes())
        w(map_xyz.astype(np.float32).ravel())
        w(scan)
        w(aux["unique_ns"].astype(np.uint32))
        w(poses)
        w(np.concatenate([_pose12(*T_B_L), _pose12(R_WB, t_WB), _pose12(R_WB2, t_WB2)]))
        w(raw)
        w(np.array(FRACTIONS, float))
    out = subprocess.run([build_exe("map_preview_pipeline"), str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    assert got["default_fraction"] == 0.0
    runs = {(r["fraction"], r["device"]): r for r in got["runs"]}
    assert sorted(runs) == sorted((f, d) for f in FRACTIONS for d in (0, 1))

    # the same steps through the Python binding: seeded map, copy + insert of the body cloud at the first pose, preview at the second
    sc = capi.Scan(ctx)
    sc.prepare_input(raw, capi.make_input_config(point_skip_divisor=4))
    sc.deskew(aux["Rt12"][np.searchsorted(aux["unique_ns"], sc.unique_ns())])
    sc.preprocess_geometric(T_B_L[0], T_B_L[1], 0.5, 20, 0.15)
    seeded = capi.VoxelMap(ctx, mode=19, lru_horizon=1000)
    seeded.insert(map_xyz)
    first = seeded.copy()
    first.insert_from_scan(sc, R_WB, t_WB)
    s1 = first.stats()
    pv = first.preview_insert_from_scan(sc, R_WB2, t_WB2)
    want_own = [pv[k] for k in ("n_points", "n_added", "n_too_close", "n_voxel_full", "n_touched_voxels", "n_new_voxels")]
    second = first.copy()
    second.insert_from_scan(sc, R_WB2, t_WB2)
    s2 = second.stats()
    for m in (seeded, first, second):
        m.release()
    sc.destroy()
    assert 0 < pv["n_added"] < pv["n_points"]
    fraction = pv["n_added"] / pv["n_points"]
    print("second scan: n_added / n_points = %d / %d = %.4f" % (pv["n_added"], pv["n_points"], fraction))

    for (f, device), r in runs.items():
        a, b = r["first"], r["second"]
        assert r["own_preview"] == want_own, (f, device)
        # the first keyframe is forced, no preview runs for it
        assert a["map_updated"] == 1 and a["map_new_fraction"] == -1 and a["map_preview"] == [0] * 6
        assert (a["n_points"], a["n_voxels"], a["uploads"]) == (s1["n_points"], s1["n_voxels"], s1["uploads"])
        if f == 0:                                       # the pose rule, untouched: no preview, no update at the second pose
            assert b["map_updated"] == 0 and b["map_new_fraction"] == -1 and b["map_preview"] == [0] * 6
        else:
            assert b["map_preview"] == r["own_preview"]
            assert b["map_new_fraction"] == r["own_preview"][1] / r["own_preview"][0] == fraction
            assert b["map_updated"] == int(r["own_preview"][1] >= f * r["own_preview"][0])
        want = s2 if b["map_updated"] else s1             # a preview is no insert: uploads moves with the real inserts only
        assert (b["n_points"], b["n_voxels"], b["uploads"]) == (want["n_points"], want["n_voxels"], want["uploads"])
    assert [runs[(f, 1)]["second"]["map_updated"] for f in FRACTIONS] == [0, 1, 0]
    assert [runs[(f, 0)]["second"]["map_updated"] for f in FRACTIONS] == [0, 1, 0]
