"""Insert preview (mh_map_preview_insert*), the parts that need no device: the symbols and the ABI version, the layout of
mh_map_insert_preview against a compiled C snippet, the NULL refusals, the numpy restatement the GPU tests compare outcomes with
(tests/map_preview_ref.py) against the numpy oracle's insert, and the replay's switch being opt-in and refused where it is not
offered."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_preview_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREVIEW_FUNCS = ["mh_map_preview_insert", "mh_map_preview_insert_device", "mh_map_preview_insert_from_scan"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in PREVIEW_FUNCS:
        assert hasattr(L, f), f
    assert set(PREVIEW_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr
    for f in PREVIEW_FUNCS:
        assert f + "(" in hdr


def test_struct_layout_matches_the_header(tmp_path):
    from mimosa_amd import capi
    cls = capi.MapInsertPreview
    items = [("sizeof(mh_map_insert_preview)", C.sizeof(cls))]
    for name, _ in cls._fields_:
        items.append((f"offsetof(mh_map_insert_preview, {name})", getattr(cls, name).offset))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) {\n' +
                   "".join(f'  printf("%zu\\n", {expr});\n' for expr, _ in items) + "  return 0;\n}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [v for _, v in items], [(e, g, v) for (e, v), g in zip(items, got) if g != v]
    assert C.sizeof(cls) == 48
    assert [n for n, _ in cls._fields_] == ["n_points", "n_added", "n_too_close", "n_voxel_full", "n_touched_voxels", "n_new_voxels"]


def test_null_map_refusals_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    xyz, R, t = np.zeros((4, 3), np.float32), np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    out = capi.MapInsertPreview()
    calls = {
        "mh_map_preview_insert": lambda: L.mh_map_preview_insert(None, capi._p(xyz), 4, 3, C.byref(out), None),
        "mh_map_preview_insert_device": lambda: L.mh_map_preview_insert_device(None, capi._p(xyz), 4, 3, capi._p(R), capi._p(t), C.byref(out), None),
        "mh_map_preview_insert_from_scan": lambda: L.mh_map_preview_insert_from_scan(None, None, capi._p(R), capi._p(t), C.byref(out), None),
    }
    for name, call in calls.items():
        assert call() == capi.MH_ERR_INVALID_ARG
        msg = L.mh_last_error(None)
        assert name.encode() + b":" in msg and b"NULL" in msg, msg


def test_restatement_agrees_with_the_numpy_oracle_on_counts():
    """map_preview_ref.preview against oracle.numpy_ref.VoxelMap.insert: a 2 000-point batch of near-duplicates of resident points
    (min-distance rule, voxels filling up) and of points that open voxels, into a map of 3 000 points"""
    from mimosa_amd import synth
    from oracle import numpy_ref
    m, _, _ = synth.small_world()
    rng = np.random.default_rng(11)
    seed = m[:3000]
    near = seed[rng.integers(0, len(seed), 1400)] + rng.normal(0, 0.05, (1400, 3)).astype(np.float32)
    fresh = m[3000:3600]
    batch = np.concatenate([near, fresh])[rng.permutation(2000)].astype(np.float32)
    vm = numpy_ref.VoxelMap()
    vm.insert(seed)
    cells = {c: [p.astype(np.float32) for p in v[0]] for c, v in vm.cells.items()}
    assert sum(len(v) for v in cells.values()) == vm.num_points
    np0, nv0 = vm.num_points, len(vm.order)
    counts, outcome, after = map_preview_ref.preview(cells, batch)
    vm.insert(batch)
    assert counts["n_points"] == 2000 == len(outcome)
    assert counts["n_added"] + counts["n_too_close"] + counts["n_voxel_full"] == 2000
    assert counts["n_added"] == vm.num_points - np0
    assert counts["n_new_voxels"] == len(vm.order) - nv0
    assert counts["n_touched_voxels"] == len({vm.coord(p.astype(np.float64)) for p in batch})
    assert 0 < counts["n_added"] < 2000 and counts["n_too_close"] > 0 and counts["n_new_voxels"] > 0   # the batch exercises the rule
    assert {c: len(v) for c, v in after.items()} == {c: len(v[0]) for c, v in vm.cells.items()}
    # and from a get_cloud()-style flat export, as the GPU tests feed it
    flat = np.array([p for c in vm.order for p in after[c]], np.float32)
    assert {c: len(v) for c, v in map_preview_ref.cells_of(flat).items()} == {c: len(v) for c, v in after.items() if v}


def test_replay_switch_is_opt_in_and_refused_where_it_is_not_offered(tmp_path):
    from mimosa_amd import replay
    assert replay.ReplayConfig().keyframe_new_fraction == 0

    class NoPreview:  # a backend without mh_map_preview_insert
        pass

    cfg = replay.ReplayConfig(n_scans=2, rows=64, cols=512, photometric=False, keyframe_new_fraction=0.015)
    with pytest.raises(ValueError, match="keyframe_new_fraction"):
        replay.run(cfg, NoPreview(), scans=[])
    with pytest.raises(RuntimeError, match="keyframe_new_fraction"):
        replay.run_native(cfg, [], str(tmp_path))
