"""CPU half of place recognition (mh_place_*): the ABI without a device, and the rule of mimosa_amd/csrc/place_device.hpp compiled
with g++ (tests/cpp/place_device_check.cpp) against the numpy restatement (tests/place_ref.py) — descriptors bit for bit, the
sector tables digit for digit, distances to 1e-12 — on the very inputs tests/test_gpu_place.py hands the device.  The same
program once more as a stand-alone binary under AddressSanitizer and UBSan.  The conditions the GPU tests rely on (gaps between
ranked distances, the end-to-end scene) are checked here with the restatement alone."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import place_ref as ref
import place_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLACE_FUNCS = ("mh_place_db_create", "mh_place_db_destroy", "mh_place_db_size", "mh_place_describe", "mh_place_describe_device",
               "mh_place_describe_from_scan", "mh_place_db_add", "mh_place_db_add_from_scan", "mh_place_db_get", "mh_place_db_query",
               "mh_place_db_query_from_scan")
# D to 1e-12 absolute: a column cosine carries at most about 45 roundings of 2^-53 and the mean over <= 60 columns about 60 more,
# under 2e-14 on values in [0, 1]; 1e-12 leaves two orders over that bound
D_TOL = 1e-12
GAP = 1e-9


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("place_device_check")


def hx(v):
    return float(v).hex()


def run(exe, text, timeout=300):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return [json.loads(line) for line in out.stdout.splitlines()]


def params_cmd(cfg, R):
    return "params " + " ".join(hx(v) for v in [cfg["r_min"], cfg["r_max"], cfg["z_min"], cfg["z_max"], *np.asarray(R, np.float64).ravel()])


def points_cmd(name, pts):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return "%s %d %s" % (name, len(pts), " ".join(hx(v) for v in pts.ravel()))


def distance_cmd(q, E, min_overlap):
    E = np.asarray(E, np.float32).reshape(-1, ref.CELLS)
    return "distance %d %d %s %s" % (min_overlap, len(E), " ".join(hx(v) for v in q), " ".join(hx(v) for v in E.ravel()))


def bits(desc):
    return np.asarray(desc, np.float32).view(np.uint32)


def tilted_R():
    from mimosa_amd import synth
    return synth.so3_exp(np.array([0.21, -0.13, 0.9]))


# ---- the descriptor -------------------------------------------------------------------------------------------------------------
def test_sector_tables_digit_for_digit(exe):
    cos, sin = run(exe, "table\n")[0]
    assert cos == ["%.17g" % v for v in ref.COS] and sin == ["%.17g" % v for v in ref.SIN]
    j = np.arange(15)
    assert np.abs(ref.COS - np.cos(np.deg2rad(6.0 * j))).max() < 2e-16 and np.abs(ref.SIN - np.sin(np.deg2rad(6.0 * j))).max() < 2e-16


@pytest.mark.parametrize("r_max", [40.0, 33.3, 0.7, 1e-3, 12345.678])
def test_ring_table_bit_for_bit(exe, r_max):
    got = run(exe, params_cmd(dict(scenes.DESIGNED_CFG, r_max=r_max, r_min=r_max / 100.0), np.eye(3)) + "\n")[0]
    assert [float.fromhex(v) for v in got] == ref.ring_table(r_max).tolist()


def test_cells_by_hand(exe):
    """the axes fall into sectors 0 / 15 / 30 / 45, (1, 1) into 7; rings count the boundaries at or below r2; the gates are half open
    as stated"""
    cfg = scenes.DESIGNED_CFG
    pts = [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [1, 1, 0], [2, 0, 0], [39.99, 0, 0], [40, 0, 0], [0.5, 0, 0], [0.49, 0, 0], [0, 0, 1],
           [3, 4, -2], [3, 4, 30], [3, 4, 29.5], [-1, 1e-30, 0], [-1, -1e-30, 0], [1, -1e-30, 0]]
    got = run(exe, params_cmd(cfg, np.eye(3)) + "\n" + points_cmd("cells", pts) + "\n")[1]
    cells = [c for c, _ in got]
    assert cells == [0, 15, 30, 45, 7, 60, 19 * 60, -1, 0, -1, -1, -1, -1, 2 * 60 + 8, 29, 30, 59]
    assert np.array([got[13][1]], np.uint32).view(np.float32)[0] == np.float32(31.5)


def test_sector_rule_is_floor_atan2():
    """the comparison rule against floor(atan2 * 60 / 2 pi) on float-valued points: no mismatch away from the edges' last bits"""
    rng = np.random.default_rng(1)
    xy = (rng.standard_normal((400000, 2)) * 10.0 ** rng.integers(-2, 2, (400000, 1))).astype(np.float32)
    pts = np.concatenate([xy, np.zeros((len(xy), 1), np.float32)], axis=1)
    cell, _ = ref.cells(pts, np.eye(3), dict(r_min=1e-30, r_max=1e30, z_min=-1.0, z_max=1.0))
    a = np.arctan2(xy[:, 1].astype(np.float64), xy[:, 0].astype(np.float64)) % (2.0 * np.pi)
    want = np.floor(a * 60.0 / (2.0 * np.pi)).astype(np.int64) % 60
    ok = cell >= 0
    assert ok.sum() > 390000
    assert np.array_equal(cell[ok] % 60, want[ok])


@pytest.mark.parametrize("n", scenes.DESIGNED_SIZES)
def test_descriptor_against_the_restatement_bit_for_bit(exe, n):
    xyz, R = scenes.designed_cloud(n)
    for Rm in (R, tilted_R()):
        text = params_cmd(scenes.DESIGNED_CFG, Rm) + "\n" + points_cmd("cells", xyz) + "\n" + points_cmd("describe", xyz[::-1]) + "\n"
        _, got_cells, got_desc = run(exe, text)
        cell, value = ref.cells(xyz, Rm, scenes.DESIGNED_CFG)
        assert [c for c, _ in got_cells] == cell.tolist()
        ok = cell >= 0
        assert [b for (c, b) in got_cells if c >= 0] == bits(value[ok]).tolist()
        assert np.array_equal(np.array(got_desc, np.uint32), bits(ref.describe(xyz, Rm, scenes.DESIGNED_CFG)))  # (and in the other point order)


def test_designed_cloud_is_what_it_is_for():
    """every gate is bracketed, every ring and sector is occupied, and points of each kind are refused"""
    g = scenes.designed_levelled()
    xyz, R = scenes.designed_cloud(len(g))
    fin = np.isfinite(g).all(axis=1)
    assert np.array_equal((R @ xyz[fin].astype(np.float64).T).T.astype(np.float32), g[fin])
    assert np.isinf(xyz).any() and np.isnan(xyz).any()
    cell, _ = ref.cells(xyz, R, scenes.DESIGNED_CFG)
    assert cell[:5].tolist() == [-1, 0, 0, -1, 45] and cell[5:10].tolist() == [19 * 60, -1, -1, 19 * 60 + 45, -1]      # r_min, r_max
    assert (cell[10:16] >= 0).tolist() == [False, False, True, True, False, False]                                    # z_min, z_max
    d = ref.describe(xyz, R, scenes.DESIGNED_CFG).reshape(ref.RINGS, ref.SECTORS)
    assert (d.max(axis=1) > 0).all() and (d.max(axis=0) > 0).all()
    assert d[3, 7] == np.float32(9.5)                    # (5, 5): ring 3, sector 7, the highest of its three points
    assert (~np.isfinite(xyz).all(axis=1)).sum() == 7


# ---- the distance -----------------------------------------------------------------------------------------------------------------
def check_distances(got, D, shift, gap):
    gD = np.array([float.fromhex(d) for d, _ in got])
    gs = np.array([s for _, s in got])
    err = np.abs(gD - D).max()
    assert err <= D_TOL, err
    assert np.array_equal(gD == ref.NO_MATCH, D == ref.NO_MATCH)
    decided = gap > GAP
    assert np.array_equal(gs[decided], shift[decided]) and (gs[D == ref.NO_MATCH] == 0).all()
    return err, int(decided.sum())


def test_distance_against_the_restatement_query_set(exe):
    q, E = scenes.query_set()
    got = run(exe, distance_cmd(q, E, scenes.QUERY_MIN_OVERLAP) + "\n")[0]
    D, shift, gap = ref.distances(q, E, scenes.QUERY_MIN_OVERLAP)
    err, n = check_distances(got, D, shift, gap)
    print("largest |D - restatement| over the query set: %.3g (%d of %d shifts decided by more than %g)" % (err, n, len(D), GAP))
    assert D[0] == ref.NO_MATCH and D[1] == ref.NO_MATCH and shift[0] == 0          # all zero; too few columns
    assert D[3] == D[17] and D[3] < 0.01                                             # the duplicate pair
    for e, s in scenes.ROTATED.items():
        assert shift[e] == s and D[e] < 1e-3, (e, s, shift[e], D[e])


def test_distance_against_the_restatement_scene(exe):
    K = scenes.keyframe_descriptors()
    worst = 0.0
    text = "".join(distance_cmd(c["desc"], K, scenes.SCENE_CFG["min_overlap"]) + "\n" for c in scenes.queries())
    for c, got in zip(scenes.queries(), run(exe, text)):
        err, _ = check_distances(got, c["D"], c["shift"], c["gap"])
        worst = max(worst, err)
    print("largest |D - restatement| over the scene's six queries: %.3g" % worst)


def test_a_rotated_cloud_answers_with_its_yaw():
    """T_W_Fq = T_W_Fk Rz(+s 6 deg): the same place seen with the heading turned by +s sectors gives shift s"""
    xy = (15.0, 11.0)
    base = ref.describe(scenes.cast(xy, 0.3), np.eye(3), scenes.SCENE_CFG)
    for s in (0, 1, 17, 59):
        turned = ref.describe(scenes.cast(xy, 0.3 + np.deg2rad(6.0 * s)), np.eye(3), scenes.SCENE_CFG)
        D, shift, _ = ref.distances(turned, base[None], scenes.SCENE_CFG["min_overlap"])
        assert shift[0] == s and D[0] < 0.05, (s, shift, D)


def test_query_set_conditions():
    """what test_gpu_place.py's equalities rest on: every shift decided by more than 1e-9, and among each database size's ranked
    distances no two within 1e-9 of each other but the exact duplicates"""
    q, E = scenes.query_set()
    D, _, gap = ref.distances(q, E, scenes.QUERY_MIN_OVERLAP)
    assert (gap[D < ref.NO_MATCH] > GAP).all()
    assert np.array_equal(E[3], E[17])
    for M in scenes.QUERY_SIZES:
        r = ref.rank(D[:M], ref.MAX_HITS + 1 if M > ref.MAX_HITS else ref.MAX_HITS)
        r = r[r >= 0]
        for a, b in zip(r[:-1], r[1:]):
            assert D[b] - D[a] > GAP or (int(a), int(b)) == (3, 17), (M, a, b)
    assert ref.rank(D[:2], 4).tolist() == [-1, -1, -1, -1]
    assert ref.rank(D, 6).tolist() == [5, 9, 40, 41, 3, 17]


def test_ranking_as_the_select_kernel_does_it(exe):
    q, E = scenes.query_set()
    D, _, _ = ref.distances(q, E, scenes.QUERY_MIN_OVERLAP)
    text = ""
    for M in scenes.QUERY_SIZES:
        for k in (1, 4, 16):
            text += "rank %d %d %s\n" % (k, M, " ".join(hx(v) for v in D[:M]))
    got = iter(run(exe, text))
    for M in scenes.QUERY_SIZES:
        for k in (1, 4, 16):
            assert next(got) == ref.rank(D[:M], k).tolist(), (M, k)


def test_scene_conditions():
    """for every chosen query the nearest keyframe is among the restatement's top 4 and consecutive distances among its top 5
    differ by more than 1e-9"""
    qs = scenes.queries()
    assert len(qs) == 6
    for c in qs:
        top = c["top"]
        assert (top >= 0).all() and c["nearest"] in top[:4].tolist()
        assert (np.diff(c["D"][top]) > GAP).all(), np.diff(c["D"][top])
        assert (c["gap"][top[:4]] > GAP).all()
        kxy = scenes.KEYFRAME_XY[c["nearest"]]
        assert np.hypot(c["xy"][0] - kxy[0], c["xy"][1] - kxy[1]) <= 1.0 + 1e-9
    assert len({c["nearest"] for c in qs}) >= 4          # not six views of one place


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined and run on what the other tests feed the plain
    build: same output, no report"""
    from mimosa_amd import build
    san = str(tmp_path / "place_device_check_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "place_device_check.cpp"), "-o", san])
    xyz, R = scenes.designed_cloud(1025)
    q, E = scenes.query_set()
    D, _, _ = ref.distances(q, E, scenes.QUERY_MIN_OVERLAP)
    text = ["table", params_cmd(scenes.DESIGNED_CFG, R), points_cmd("cells", xyz), points_cmd("describe", xyz), params_cmd(scenes.DESIGNED_CFG, tilted_R()),
            points_cmd("describe", xyz), distance_cmd(q, E[:65], scenes.QUERY_MIN_OVERLAP), distance_cmd(E[0], E[:3], 1),
            "rank 16 300 " + " ".join(hx(v) for v in D), "rank 4 2 " + " ".join(hx(v) for v in D[:2])]
    text = "\n".join(text) + "\n"
    a = subprocess.run([san], input=text, capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0 and a.stdout == b.stdout


# ---- the host helpers ---------------------------------------------------------------------------------------------------------
def test_level_rotation():
    from mimosa_amd import capi
    assert np.array_equal(capi.level_rotation([0.0, 0.0, -1.0]), np.eye(3))
    assert np.array_equal(capi.level_rotation([0.0, 0.0, 9.81]), np.diag([1.0, -1.0, -1.0]))       # antipodal: a turn by pi about x
    rng = np.random.default_rng(2)
    for _ in range(20):
        g = rng.standard_normal(3)
        R = capi.level_rotation(g)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1.0) < 1e-12
        assert np.allclose(R @ (-g / np.linalg.norm(g)), [0.0, 0.0, 1.0], atol=1e-12)
        # the smallest such rotation: its axis is horizontal in G and its angle the angle between -g and z
        ang = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
        assert abs(ang - np.arccos(np.clip(-g[2] / np.linalg.norm(g), -1.0, 1.0))) < 1e-9


def test_candidate_pose():
    from mimosa_amd import capi
    R_k, t_k = ref.rz(0.7), np.array([1.0, 2.0, 3.0])
    R, t = capi.place_candidate_pose((R_k, t_k), None, None, 5)
    assert np.allclose(R, ref.rz(0.7 + np.deg2rad(30.0)), atol=1e-15) and np.array_equal(t, t_k)
    Lk, Lq = capi.level_rotation([0.1, 0.0, -1.0]), capi.level_rotation([0.0, -0.2, -1.0])
    R, _ = capi.place_candidate_pose((R_k, t_k), Lk, Lq, 59)
    assert np.allclose(R, R_k @ Lk.T @ ref.rz(np.deg2rad(354.0)) @ Lq, atol=1e-15)


# ---- the ABI without a device -----------------------------------------------------------------------------------------------
def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in PLACE_FUNCS:
        assert hasattr(L, f) and f in capi.EXPORTS, f
    assert L.mh_abi_version() == 3
    assert (capi.MH_PLACE_RINGS, capi.MH_PLACE_SECTORS, capi.MH_PLACE_MAX_HITS) == (ref.RINGS, ref.SECTORS, ref.MAX_HITS) == (20, 60, 16)


def test_struct_layouts_match_the_header(tmp_path):
    from mimosa_amd import capi
    structs = [("mh_place_config", capi.PlaceConfig, 40), ("mh_place_hit", capi.PlaceHit, 24), ("mh_place_score", capi.PlaceScore, 16)]
    items = [("MH_PLACE_RINGS", 20), ("MH_PLACE_SECTORS", 60), ("MH_PLACE_MAX_HITS", 16), ("MH_ABI_VERSION", 3)]
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
    assert capi.PLACE_HIT_DTYPE.itemsize == 24 and capi.PLACE_SCORE_DTYPE.itemsize == 16
    assert [capi.PLACE_HIT_DTYPE.fields[n][1] for n, _ in capi.PlaceHit._fields_] == [getattr(capi.PlaceHit, n).offset for n, _ in capi.PlaceHit._fields_]


def test_refusals_that_need_no_device():
    """a NULL argument everywhere, and every config mh_place_db_create refuses: the config is judged before the context is looked at"""
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    INV, p = capi.MH_ERR_INVALID_ARG, capi._p
    h = C.c_void_p()
    good = dict(r_min=0.5, r_max=40.0, z_min=-2.0, z_max=30.0, min_overlap=30, capacity=16)
    assert L.mh_place_db_create(None, None, C.byref(h)) == INV and b"mh_place_db_create: NULL argument" in L.mh_last_error(None)
    cfg = capi.make_place_config(**good)
    assert L.mh_place_db_create(None, C.byref(cfg), None) == INV and b"NULL argument" in L.mh_last_error(None)
    assert L.mh_place_db_create(None, C.byref(cfg), C.byref(h)) == INV and b"NULL argument" in L.mh_last_error(None) and not h.value
    bad = [(dict(r_min=np.nan), b"not finite"), (dict(r_max=np.inf), b"not finite"), (dict(z_min=-np.inf), b"not finite"), (dict(z_max=np.nan), b"not finite"),
           (dict(r_min=0.0), b"0 < r_min < r_max"), (dict(r_min=-1.0), b"0 < r_min < r_max"), (dict(r_max=0.5), b"0 < r_min < r_max"),
           (dict(r_max=0.25), b"0 < r_min < r_max"), (dict(z_min=30.0), b"z_min < z_max"), (dict(z_min=31.0), b"z_min < z_max"),
           (dict(min_overlap=0), b"min_overlap"), (dict(min_overlap=61), b"min_overlap"), (dict(capacity=0), b"capacity"), (dict(capacity=65537), b"capacity"),
           (dict(capacity=-3), b"capacity")]
    for change, msg in bad:
        cfg = capi.make_place_config(**dict(good, **change))
        assert L.mh_place_db_create(None, C.byref(cfg), C.byref(h)) == INV and msg in L.mh_last_error(None), (change, L.mh_last_error(None))
    for edge in (dict(min_overlap=1), dict(min_overlap=60), dict(capacity=1), dict(capacity=65536)):     # the ends of the ranges pass the config check
        cfg = capi.make_place_config(**dict(good, **edge))
        assert L.mh_place_db_create(None, C.byref(cfg), C.byref(h)) == INV and b"NULL argument" in L.mh_last_error(None), edge
    xyz, R, desc = np.zeros((4, 3), np.float32), np.eye(3).ravel(), np.zeros(ref.CELLS, np.float32)
    hits, idx, tag = np.zeros(4, capi.PLACE_HIT_DTYPE), C.c_int32(), C.c_int64()
    calls = [("mh_place_describe", lambda: L.mh_place_describe(None, p(xyz), 4, 3, p(R), p(desc))),
             ("mh_place_describe_device", lambda: L.mh_place_describe_device(None, None, 0, 3, p(R), p(desc))),
             ("mh_place_describe_from_scan", lambda: L.mh_place_describe_from_scan(None, None, 0, p(R), p(desc))),
             ("mh_place_db_add", lambda: L.mh_place_db_add(None, p(desc), 7, C.byref(idx))),
             ("mh_place_db_add_from_scan", lambda: L.mh_place_db_add_from_scan(None, None, 0, p(R), 7, C.byref(idx))),
             ("mh_place_db_get", lambda: L.mh_place_db_get(None, 0, p(desc), C.byref(tag))),
             ("mh_place_db_query", lambda: L.mh_place_db_query(None, p(desc), 0, 4, p(hits), None)),
             ("mh_place_db_query_from_scan", lambda: L.mh_place_db_query_from_scan(None, None, 0, p(R), 0, 4, p(hits), None))]
    for name, call in calls:
        assert call() == INV and (name + ": NULL argument").encode() in L.mh_last_error(None), name
    assert L.mh_place_db_size(None) == 0
    L.mh_place_db_destroy(None)                          # a no-op
