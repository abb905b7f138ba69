"""CPU half of map carving (mh_map_carve*): the ABI without a device, and the rule of mimosa_amd/csrc/carve_device.hpp compiled with
g++ (tests/cpp/map_carve_cells.cpp) against the numpy restatement (tests/map_carve_ref.py) on a designed list — all six faces, the
ties of the major-axis rule, u or v exactly at -1, 0 and +1, the zero vector, and each of the three gates at the last double on
either side.  The same program once more as a stand-alone binary under AddressSanitizer and UBSan."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import map_carve_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CARVE_FUNCS = ("mh_map_carve", "mh_map_carve_device", "mh_map_carve_from_scan")
I9, Z3 = np.eye(3).ravel(), np.zeros(3)


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("map_carve_cells")


def hx(v):
    return float(v).hex()


def run(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return [json.loads(line) for line in out.stdout.splitlines()]


def params_cmd(cfg, R=I9, t=Z3, origin=Z3):
    vals = [cfg["range_min"], cfg["range_max"], cfg["margin_abs"], cfg["margin_rel"], *R, *t, *origin]
    return "params %d %d %s" % (cfg["grid"], cfg["ring"], " ".join(hx(v) for v in vals))


def points_cmd(name, pts):
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    return "%s %d %s" % (name, len(pts), " ".join(hx(v) for v in pts.ravel()))


def image_cmd(img):
    hit = np.flatnonzero(np.isfinite(img))
    return "image %d %s" % (len(hit), " ".join("%d %s" % (c, hx(img[c])) for c in hit))


# ---- the cell function ---------------------------------------------------------------------------------------------------
def designed_vectors():
    v = []
    for f in range(3):                                   # all six faces, off-centre
        for sign in (1.0, -1.0):
            s = np.array([0.3, -0.2, 0.0])
            s = np.roll(np.array([sign * 2.0, 0.3, -0.7]), f)
            v.append(s)
    for sa in (1.0, -1.0):                               # ties of the major-axis rule, with every sign
        for sb in (1.0, -1.0):
            v += [[sa, sb, 0.5], [sa, 0.5, sb], [0.5, sa, sb], [sa, sb, sb], [sa, sb, -sb]]
    for f in range(3):                                   # u or v exactly at -1, 0 and +1
        for u in (-1.0, 0.0, 1.0):
            for w in (-1.0, 0.0, 1.0, 0.25):
                v.append(np.roll(np.array([3.0, 3.0 * u, 3.0 * w]), f))
                v.append(np.roll(np.array([-3.0, 3.0 * u, 3.0 * w]), f))
    v += [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0]]            # no cell
    v += [[np.inf, 1.0, 1.0], [np.nan, 1.0, 1.0], [1.0, np.nan, 0.0], [1e308, -1e308, 5.0], [5e-324, 0.0, 0.0], [1.0, np.nextafter(1.0, 0.0), 0.0]]
    rng = np.random.default_rng(11)
    v += list(rng.standard_normal((200, 3)) * 10.0 ** rng.integers(-3, 4, (200, 1)))
    # cell edges: u just below, at and just above a multiple of 2 / N
    for N in (4, 7, 8, 512):
        for k in (1, N // 2, N - 1):
            u = -1.0 + 2.0 * k / N
            v += [[1.0, np.nextafter(u, -2.0), 0.1], [1.0, u, 0.1], [1.0, np.nextafter(u, 2.0), 0.1]]
    return np.array(v, np.float64)


@pytest.mark.parametrize("N", [4, 7, 8, 16, 511, 512])
def test_cells_against_the_restatement(exe, N):
    v = designed_vectors()
    got = np.array(run(exe, "cells %d %d %s" % (N, len(v), " ".join(hx(x) for x in v.ravel())))[0])
    cell, face, i, j = ref.cells(v, N)
    assert np.array_equal(got[:, 0], cell), np.flatnonzero(got[:, 0] != cell)[:10]
    ok = cell >= 0
    assert np.array_equal(got[ok, 1], face[ok]) and np.array_equal(got[ok, 2], i[ok]) and np.array_equal(got[ok, 3], j[ok])
    assert (got[~ok, 1:] == -1).all()
    assert ((cell >= -1) & (cell < 6 * N * N)).all()


def test_cells_by_hand(exe):
    """written out, so that the program and the restatement cannot be wrong together"""
    N = 4
    cases = [([2.0, 0.0, 0.0], (0, 2, 2)), ([-2.0, 0.0, 0.0], (1, 2, 2)), ([0.0, 2.0, 0.0], (2, 2, 2)), ([0.0, -2.0, 0.0], (3, 2, 2)),
             ([0.0, 0.0, 2.0], (4, 2, 2)), ([0.0, 0.0, -2.0], (5, 2, 2)),
             ([1.0, 1.0, 1.0], (0, 3, 3)),               # all equal: axis 0; u = v = +1 land in the last cell, not one past it
             ([1.0, -1.0, -1.0], (0, 0, 0)),             # u = v = -1: cell 0
             ([-1.0, 1.0, 0.5], (1, 3, 3)),              # a0 == a1 > a2: axis 0, face 1; u = s1 / m = 1, v = s2 / m = 0.5 -> i 3, j 3
             ([0.5, 1.0, -1.0], (2, 0, 2)),              # a1 == a2 > a0: axis 1; u = s2 / m = -1 -> i 0, v = s0 / m = 0.5 -> j 3?
             ([0.5, 0.25, -1.0], (5, 3, 2))]             # axis 2 negative: u = s0 / m = 0.5 -> i 3, v = s1 / m = 0.25 -> j 2
    cases[9] = ([0.5, 1.0, -1.0], (2, 0, 3))
    v = np.array([c[0] for c in cases])
    got = run(exe, "cells %d %d %s" % (N, len(v), " ".join(hx(x) for x in v.ravel())))[0]
    for (s, (face, i, j)), g in zip(cases, got):
        assert g == [(face * N + j) * N + i, face, i, j], (s, g)


# ---- the gates -------------------------------------------------------------------------------------------------------------
def gate_cases():
    """(name, cfg, image as {cell: value}, points): one map point straight ahead on face 0 at range x (f32, so r2 = x * x exactly)"""
    x = float(np.float32(7.3))
    up, dn = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    base = dict(grid=8, ring=0, range_min=1.0, range_max=50.0, margin_abs=0.25, margin_rel=0.0625)
    cell = int(ref.cells(np.array([[x, 0.0, 0.0]]), 8)[0][0])
    far = {cell: 1.0e4}                                   # an observation far behind the point
    out = []
    for name, field in (("range_min", "range_min"), ("range_max", "range_max")):
        for tag, val in (("below", dn(x)), ("at", x), ("above", up(x))):
            out.append(("%s %s" % (name, tag), dict(base, **{field: val}), far, [[x, 0.0, 0.0]]))
    r = np.sqrt(x * x)
    for ma in (0.25, dn(0.25), up(0.25)):
        lim = r + (ma + 0.0625 * r)
        for tag, q in (("below", dn(lim * lim)), ("at", lim * lim), ("above", up(lim * lim))):
            out.append(("margin %r %s" % (ma, tag), dict(base, margin_abs=ma), {cell: q}, [[x, 0.0, 0.0]]))
    return out, cell


def test_gates_at_the_last_double_on_either_side(exe):
    cases, cell = gate_cases()
    text, want = [], []
    for name, cfg, image, pts in cases:
        img = np.full(6 * cfg["grid"] ** 2, np.inf)
        for c, q in image.items():
            img[c] = q
        text += [params_cmd(cfg), image_cmd(img), points_cmd("decide", pts)]
        want.append(ref.decide(np.array(pts, np.float32), img, Z3, I9, Z3, cfg).tolist())
    got = run(exe, "\n".join(text))[2::3]
    assert got == want, [(c[0], g, w) for c, g, w in zip(cases, got, want) if g != w]
    by_name = {c[0]: g[0] for c, g in zip(cases, got)}
    # written out: range_min <= r <= range_max is inclusive on both sides; the margin test is strict
    assert by_name["range_min below"] == ref.SEEN_THROUGH and by_name["range_min at"] == ref.SEEN_THROUGH and by_name["range_min above"] == ref.UNTESTED
    assert by_name["range_max below"] == ref.UNTESTED and by_name["range_max at"] == ref.SEEN_THROUGH and by_name["range_max above"] == ref.SEEN_THROUGH
    for ma in (0.25, float(np.nextafter(0.25, -np.inf)), float(np.nextafter(0.25, np.inf))):
        assert [by_name["margin %r %s" % (ma, t)] for t in ("below", "at", "above")] == [ref.KEPT, ref.KEPT, ref.SEEN_THROUGH]


def scene(seed, ring, N=8):
    """a random pose, observations and map points around the sensor, some non-finite observations"""
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    R, t, origin = A.ravel(), rng.uniform(-3, 3, 3), rng.uniform(-0.2, 0.2, 3)
    cfg = dict(grid=N, ring=ring, range_min=0.8, range_max=9.0, margin_abs=0.2, margin_rel=0.01)
    d = rng.standard_normal((3000, 3))
    far = rng.random((3000, 1)) < 0.9                    # most observations lie 9 m out, the rest between 0.15 and 7 m
    obs = (d / np.linalg.norm(d, axis=1, keepdims=True) * np.where(far, 9.0, rng.uniform(0.15, 7.0, (3000, 1)))).astype(np.float32) + origin.astype(np.float32)
    obs[::97, 1] = np.nan
    obs[5, 2] = np.inf
    d = rng.standard_normal((500, 3))
    pts_F = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 11.0, (500, 1)) + origin
    pts = (pts_F @ A.T + t).astype(np.float32)
    return cfg, R, t, origin, obs, pts


@pytest.mark.parametrize("ring", [0, 1, 2])
def test_observe_and_decide_against_the_restatement(exe, ring):
    cfg, R, t, origin, obs, pts = scene(100 + ring, ring)
    img, n_used = ref.image(obs, origin, cfg)
    got = run(exe, "\n".join([params_cmd(cfg, R, t, origin), points_cmd("observe", obs), image_cmd(img), points_cmd("decide", pts)]))
    mine = np.full(len(img), np.inf)
    used = 0
    for g in got[1]:
        if g[0] >= 0:
            used += 1
            mine[g[0]] = min(mine[g[0]], float.fromhex(g[1]))
    assert used == n_used and 0 < used < len(obs)
    assert np.array_equal(mine, img)
    dec = ref.decide(pts, img, origin, R, t, cfg)
    assert got[3] == dec.tolist()
    assert {ref.UNTESTED, ref.KEPT, ref.SEEN_THROUGH} == set(dec.tolist())


def test_ring_is_clipped_at_the_face_edge_and_needs_every_cell(exe):
    """a point in the corner cell of face 0 with ring 1: only the four cells on the face count; one of them not hit keeps the point"""
    N = 4
    cfg = dict(grid=N, ring=1, range_min=0.5, range_max=50.0, margin_abs=0.1, margin_rel=0.0)
    p = np.array([[4.0, -3.9, -3.9]], np.float32)        # face 0, i = j = 0
    cell, face, i, j = ref.cells(p.astype(np.float64), N)
    assert (int(face[0]), int(i[0]), int(j[0])) == (0, 0, 0)
    on_face = [0, 1, N, N + 1]
    full = np.full(6 * N * N, np.inf)
    full[on_face] = 1.0e4
    text, want = [params_cmd(cfg)], []
    for drop in (None, 0, 1, N, N + 1):
        img = full.copy()
        if drop is not None:
            img[drop] = np.inf
        text += [image_cmd(img), points_cmd("decide", p)]
        want.append([ref.SEEN_THROUGH if drop is None else ref.KEPT])
        assert ref.decide(p, img, Z3, I9, Z3, cfg).tolist() == want[-1]
    near = full.copy()
    near[N + 1] = 30.0                                   # the ring's minimum decides: 30 < lim^2
    text += [image_cmd(near), points_cmd("decide", p)]
    want.append([ref.KEPT])
    assert run(exe, "\n".join(text))[2::2] == want


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined and run on what the other tests feed the plain
    build: same output, no report"""
    from mimosa_amd import build
    san = str(tmp_path / "map_carve_cells_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "map_carve_cells.cpp"), "-o", san])
    v = designed_vectors()
    text = ["cells %d %d %s" % (N, len(v), " ".join(hx(x) for x in v.ravel())) for N in (4, 7, 512)]
    for ring in (0, 1, 2):
        cfg, R, t, origin, obs, pts = scene(100 + ring, ring)
        img, _ = ref.image(obs, origin, cfg)
        text += [params_cmd(cfg, R, t, origin), points_cmd("observe", obs), image_cmd(img), points_cmd("decide", pts)]
    text = "\n".join(text) + "\n"
    a = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0 and a.stdout == b.stdout


# ---- the ABI without a device -----------------------------------------------------------------------------------------------
def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in CARVE_FUNCS:
        assert hasattr(L, f) and f in capi.EXPORTS, f
    assert L.mh_abi_version() == 3


def test_struct_layouts_match_the_header(tmp_path):
    from mimosa_amd import capi
    items = [("sizeof(mh_map_carve_config)", C.sizeof(capi.MapCarveConfig)), ("sizeof(mh_map_carve_result)", C.sizeof(capi.MapCarveResult))]
    items += [("offsetof(mh_map_carve_config, %s)" % n, getattr(capi.MapCarveConfig, n).offset) for n, _ in capi.MapCarveConfig._fields_]
    items += [("offsetof(mh_map_carve_result, %s)" % n, getattr(capi.MapCarveResult, n).offset) for n, _ in capi.MapCarveResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mimosa_hip.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu\\n", (size_t)%s);\n' % e for e, _ in items) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [v for _, v in items], [(e, g, v) for (e, v), g in zip(items, got) if g != v]
    assert C.sizeof(capi.MapCarveConfig) == 48 == C.sizeof(capi.MapCarveResult)
    assert tuple(n for n, _ in capi.MapCarveResult._fields_) == ref.COUNTERS


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    cfg, out = capi.make_carve_config(), capi.MapCarveResult()
    xyz, o, R, t = np.zeros((4, 3), np.float32), Z3.copy(), I9.copy(), Z3.copy()
    p = capi._p
    assert L.mh_map_carve(None, p(xyz), 4, 3, p(o), p(R), p(t), C.byref(cfg), C.byref(out)) == capi.MH_ERR_INVALID_ARG
    assert b"mh_map_carve: NULL argument" in L.mh_last_error(None)
    assert L.mh_map_carve_device(None, None, 0, 3, p(o), p(R), p(t), C.byref(cfg), C.byref(out)) == capi.MH_ERR_INVALID_ARG
    assert b"mh_map_carve_device" in L.mh_last_error(None)
    assert L.mh_map_carve_from_scan(None, None, 0, p(o), p(R), p(t), C.byref(cfg), C.byref(out)) == capi.MH_ERR_INVALID_ARG
    assert b"mh_map_carve_from_scan" in L.mh_last_error(None)


def test_restatement_voxel_counts():
    cloud = np.array([[0.1, 0.1, 0.1], [0.2, 0.1, 0.4], [0.6, 0.1, 0.1], [0.1, 0.1, 0.2], [-0.1, 0.0, 0.0], [-0.2, 0.0, 0.0]], np.float32)
    assert ref.voxel_counts(cloud, 0.5).tolist() == [2, 1, 1, 2]
    assert ref.voxel_counts(cloud[:0], 0.5).tolist() == []


def test_replay_switch_is_opt_in_and_refused_where_it_is_not_offered(tmp_path):
    from mimosa_amd import replay
    assert replay.ReplayConfig().carve_keyframes is False

    class NoCarve:  # a backend without mh_map_carve
        pass

    cfg = replay.ReplayConfig(n_scans=2, rows=64, cols=512, photometric=False, carve_keyframes=True)
    with pytest.raises(ValueError, match="carve_keyframes"):
        replay.run(cfg, NoCarve(), scans=[])
    with pytest.raises(RuntimeError, match="carve_keyframes"):
        replay.run_native(cfg, [], str(tmp_path))
