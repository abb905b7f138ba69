"""CPU half of the keyframe cloud store and the map rebuild (mh_keyframes_*, mh_map_rebuild_from_keyframes): the ABI without a
device; the chunk plan of mimosa_amd/csrc/rebuild_plan.hpp compiled with g++ (tests/cpp/rebuild_plan_check.cpp) against the
restatement in tests/map_rebuild_ref.py, and once more as a stand-alone binary under AddressSanitizer and UBSan; and the idea
itself on the oracle map: a chunked build with per-keyframe stamps equals the sequential build, LRU purges included, on the
corridor scene the GPU test uses."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import map_rebuild_ref as ref
from oracle import numpy_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("mh_keyframes_create", "mh_keyframes_destroy", "mh_keyframes_size", "mh_keyframes_get_info", "mh_keyframes_add", "mh_keyframes_add_device",
         "mh_keyframes_add_from_scan", "mh_keyframes_get", "mh_keyframes_device_points", "mh_map_rebuild_from_keyframes")


# ---- the ABI without a device -----------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()


def test_header_declares_the_entry_points():
    hdr = header()
    assert "#define MH_ABI_VERSION 3" in hdr  # entry points were added, nothing that exists changed
    for f in FUNCS:
        assert (" %s(" % f) in hdr, f
    for s in ("mh_keyframes_config", "mh_keyframes_info", "mh_map_rebuild_config", "mh_map_rebuild_result"):
        assert ("} %s;" % s) in hdr, s
    # the contract, word for word
    for sentence in ("The returned map is what mh_map_create(cfg) gives, followed by one mh_map_insert_device per listed keyframe, in",
                     "The contract holds when LRU purges fall inside the sequence.",
                     "unchanged: (r0 x + (r1 y + r2 z)) + t, no FMA."):
        assert sentence in hdr, sentence


def test_symbols_resolve():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in FUNCS:
        assert hasattr(L, f) and f in capi.EXPORTS, f
    assert L.mh_abi_version() == 3


def test_struct_layouts_match_the_header(tmp_path):
    from mimosa_amd import capi
    structs = [("mh_keyframes_config", capi.KeyframesConfig, 16), ("mh_keyframes_info", capi.KeyframesInfo, 40),
               ("mh_map_rebuild_config", capi.MapRebuildConfig, 16), ("mh_map_rebuild_result", capi.MapRebuildResult, 48)]
    items = [("MH_ABI_VERSION", 3)]
    for name, cls, size in structs:
        assert C.sizeof(cls) == size
        items.append(("sizeof(%s)" % name, size))
        items += [("offsetof(%s, %s)" % (name, n), getattr(cls, n).offset) for n, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mimosa_hip.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu\\n", (size_t)%s);\n' % e for e, _ in items) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [v for _, v in items], [(e, g, v) for (e, v), g in zip(items, got) if g != v]


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    INV, p = capi.MH_ERR_INVALID_ARG, capi._p
    h, idx, n, tag, d = C.c_void_p(), C.c_int32(), C.c_size_t(), C.c_int64(), C.c_void_p()
    xyz = np.zeros((4, 3), np.float32)
    cfg = capi.KeyframesConfig(16, 0, 1024)
    assert L.mh_keyframes_create(None, None, C.byref(h)) == INV and b"mh_keyframes_create: NULL argument" in L.mh_last_error(None)
    assert L.mh_keyframes_create(None, C.byref(cfg), None) == INV and b"NULL argument" in L.mh_last_error(None)
    assert L.mh_keyframes_create(None, C.byref(cfg), C.byref(h)) == INV and b"NULL argument" in L.mh_last_error(None) and not h.value
    for bad, msg in [((0, 0, 1024), b"capacity_keyframes"), ((65537, 0, 1024), b"capacity_keyframes"), ((-1, 0, 1024), b"capacity_keyframes"),
                     ((16, 0, 0), b"capacity_points"), ((16, 0, -5), b"capacity_points"), ((16, 1, 1024), b"reserved")]:
        c = capi.KeyframesConfig(*bad)
        assert L.mh_keyframes_create(None, C.byref(c), C.byref(h)) == INV and msg in L.mh_last_error(None), bad
    for edge in ((1, 0, 1), (65536, 0, 1024)):  # the ends of the ranges pass the config check
        c = capi.KeyframesConfig(*edge)
        assert L.mh_keyframes_create(None, C.byref(c), C.byref(h)) == INV and b"NULL argument" in L.mh_last_error(None), edge
    info, mcfg, res = capi.KeyframesInfo(), capi.MapConfig(0.5, 0.15, 20, 19, 1000, 10, 0), capi.MapRebuildResult()
    calls = [("mh_keyframes_get_info", lambda: L.mh_keyframes_get_info(None, C.byref(info))),
             ("mh_keyframes_add", lambda: L.mh_keyframes_add(None, p(xyz), 4, 3, 7, C.byref(idx))),
             ("mh_keyframes_add_device", lambda: L.mh_keyframes_add_device(None, None, 0, 3, 7, C.byref(idx))),
             ("mh_keyframes_add_from_scan", lambda: L.mh_keyframes_add_from_scan(None, None, 1, 7, C.byref(idx))),
             ("mh_keyframes_get", lambda: L.mh_keyframes_get(None, 0, None, 0, C.byref(n), C.byref(tag))),
             ("mh_keyframes_device_points", lambda: L.mh_keyframes_device_points(None, 0, C.byref(d), C.byref(n))),
             ("mh_map_rebuild_from_keyframes", lambda: L.mh_map_rebuild_from_keyframes(None, C.byref(mcfg), None, 0, None, None, None, C.byref(h), C.byref(res)))]
    for name, call in calls:
        assert call() == INV and (name + ": NULL argument").encode() in L.mh_last_error(None), name
    assert L.mh_keyframes_size(None) == 0
    L.mh_keyframes_destroy(None)  # a no-op


# ---- the plan header --------------------------------------------------------------------------------------------------------
def plan_cases():
    rng = np.random.default_rng(11)
    cases = []
    for cycle in (1, 3, 10, 2 ** 31 - 1):
        for trial in range(6):
            n = int(rng.integers(0, 40))
            sizes = rng.integers(0, 3000, n)
            sizes[rng.random(n) < 0.2] = 0  # empty keyframes
            if n and trial == 0:
                sizes[:] = 0
            total, largest = int(sizes.sum()), int(sizes.max()) if n else 0
            for budget in (1, max(1, largest - 1), max(1, largest), max(1, total // 3), total + 1, ref.DEFAULT_CHUNK_POINTS):
                for counter0 in (0, 7):
                    cases.append((counter0, cycle, budget, [int(s) for s in sizes]))
    cases.append((0, 10, 100, []))
    cases.append((0, 5, 2 ** 40, [2 ** 33, 1, 0, 2 ** 33]))  # 64-bit totals
    return cases


def plan_text(cases):
    return "".join("%d %d %d %d %s\n" % (c0, cy, b, len(s), " ".join(map(str, s))) for c0, cy, b, s in cases)


def check_plans(exe):
    cases = plan_cases()
    assert any(c0 == 0 for c0, *_ in cases)
    out = subprocess.run([exe], input=plan_text(cases), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (c0, cy, b, sizes), line in zip(cases, lines):
        got = [tuple(v[:4]) + (bool(v[4]),) for v in json.loads(line)]
        want = ref.plan(sizes, c0, cy, b)
        assert got == want, (c0, cy, b, sizes)
        # what the plan promises, stated once more without the restatement
        assert [k for c in want for k in range(c[0], c[1])] == list(range(len(sizes)))
        for k0, k1, pts, start, purge in want:
            assert pts == sum(sizes[k0:k1]) and start == c0 + k0 and purge == ((c0 + k1) % cy == 0)
            assert all((c0 + k) % cy != 0 for k in range(k0 + 1, k1))             # no purge boundary inside a chunk
            assert pts <= b or k1 - k0 == 1                                       # over budget only alone
        for a, nxt in zip(want, want[1:]):                                        # a chunk ended for a reason
            assert a[4] or a[2] + sizes[nxt[0]] > b


def test_plan_header_matches_the_restatement():
    from mimosa_amd import build
    check_plans(build.build_host_test("rebuild_plan_check"))


def test_plan_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rebuild_plan_check_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "mimosa_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "rebuild_plan_check.cpp"), "-o", exe])
    check_plans(exe)


# ---- the idea itself, on the oracle map -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corridor():
    clouds, Rs, ts = ref.corridor_scene()
    return ref.corridor_world(clouds, Rs, ts)


def test_corridor_scene_has_what_the_check_needs(corridor):
    assert len(corridor) == 25 and all(200 <= len(c) <= 500 for c in corridor)
    events = {}
    ref.sequential_build(numpy_ref.VoxelMap(**ref.CORRIDOR_MAP), corridor, events)
    removed = events["removed"]
    assert len(removed) == 5                                        # counters 5, 10, 15, 20, 25
    assert sum(1 for r in removed if r) >= 2                        # at least two purges remove voxels
    gone = set()
    again = 0
    for k, created in enumerate(events["created"]):
        again += sum(1 for c in created if c in gone)               # a removed voxel is created again later
        if (k + 1) % 5 == 0:
            gone |= set(removed[(k + 1) // 5 - 1])
    assert again >= 1
    stats = {}
    ref.chunked_build(numpy_ref.VoxelMap(**ref.CORRIDOR_MAP), corridor, stats=stats)
    assert stats["full_in_chunk"] >= 1                              # a voxel reaches the 20-point cap inside a chunk
    assert stats["chunks"] == 5 and stats["purges"] == 5


@pytest.mark.parametrize("budget", [ref.DEFAULT_CHUNK_POINTS, 1000, 1])
def test_chunked_build_equals_sequential_build(corridor, budget):
    seq = ref.sequential_build(numpy_ref.VoxelMap(**ref.CORRIDOR_MAP), corridor)
    chk = ref.chunked_build(numpy_ref.VoxelMap(**ref.CORRIDOR_MAP), corridor, budget=budget)
    ref.assert_same_map(seq, chk)
    assert seq.lru_counter == 25


def test_chunked_build_with_empty_keyframes_and_a_long_cycle(corridor):
    clouds = list(corridor[:9])
    clouds.insert(4, np.zeros((0, 3), np.float32))
    for cycle in (3, 2 ** 31 - 1):
        cfg = dict(ref.CORRIDOR_MAP, lru_clear_cycle=cycle)
        ref.assert_same_map(ref.sequential_build(numpy_ref.VoxelMap(**cfg), clouds), ref.chunked_build(numpy_ref.VoxelMap(**cfg), clouds))


# ---- the hall: the drift the end-to-end GPU test uses ------------------------------------------------------------------------
def test_hall_drift_is_corrected_to_a_quarter():
    """The drift of map_rebuild_ref.HALL_DRIFT is chosen here: with the restated pose graph, the oracle map and brute-force nearest
    distances, the map rebuilt at the corrected poses lies within a quarter of the drifted map's RMS distance to the true map.
    (tests/test_gpu_map_rebuild.py asserts a half on the device.)"""
    import pose_graph_ref
    case = ref.hall_case()
    got = pose_graph_ref.optimise(*case["drifted"], case["fixed"], case["edges"], 16)
    oracle_points = lambda poses: np.concatenate([np.array(v[0]).reshape(-1, 3) for v in ref.sequential_build(
        numpy_ref.VoxelMap(leaf=0.5, min_dist=0.15, lru_horizon=1000), [ref.world_f32(c, R, t) for c, R, t in zip(case["clouds"], *poses)]).cells.values()])
    true, drifted, corrected = oracle_points(case["true"]), oracle_points(case["drifted"]), oracle_points((got["R"], got["t"]))
    rms_d = ref.capped_rms(ref.nearest_distances(drifted[::10], true))
    rms_c = ref.capped_rms(ref.nearest_distances(corrected[::10], true))
    print("hall, oracle: RMS to the true map drifted %.4f m, corrected %.4f m" % (rms_d, rms_c))
    assert rms_d > 0.1 and rms_c < 0.25 * rms_d
