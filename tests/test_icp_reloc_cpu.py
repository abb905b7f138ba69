"""CPU: the host-testable half of the relocalisation kernels (mimosa_amd/csrc/reloc_device.hpp, compiled by g++ through
tests/cpp/reloc_select.cpp) against numpy, the numpy restatement of the score (tests/reloc_ref.py) against a brute-force
nearest point over the oracle's map, and the ABI additions.

Bars.  Ranking, voxel range check, transform and the fixed-order folds: exact (the transform and the folds bit for bit against
the same expression written out here — both sides round every product and sum on their own).  The restatement against the
oracle's k-NN: counts equal, sum_sq to 1e-14 relative (the oracle's squared distance is the same three products summed in
another order)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import reloc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_host_test("reloc_select")


def run(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return [json.loads(line) for line in out.stdout.splitlines()]


def select_cmd(n_inliers, sum_sq, top_k):
    toks = ["select", str(len(n_inliers)), str(top_k)]
    for a, b in zip(n_inliers, sum_sq):
        toks += [str(int(a)), repr(float(b))]
    return " ".join(toks)


def expected_top(n_inliers, sum_sq, top_k):
    order = list(reloc_ref.rank(n_inliers, sum_sq)[:top_k])
    return [int(i) for i in order] + [-1] * (8 - len(order))


# hand-made score tables: (n_inliers, sum_sq, top_k)
def select_cases():
    rng = np.random.default_rng(21)
    big_n = rng.integers(0, 40, 65536)
    big_s = np.round(rng.uniform(0, 3, 65536), 2)  # two decimals: plenty of fully equal entries among 65 536
    return {
        "equal_inliers_unequal_sums": ([5, 5, 5, 4], [0.3, 0.1, 0.2, 0.0], 4),
        "fully_equal_lower_index_wins": ([7, 7, 7, 7, 7], [0.5, 0.5, 0.5, 0.5, 0.5], 3),
        "top_k_above_n_poses": ([1, 3, 2], [0.1, 0.9, 0.4], 8),
        "one_pose": ([0], [0.0], 8),
        "one_pose_top_0": ([4], [1.0], 0),
        "more_inliers_beat_smaller_sum": ([10, 11, 10], [0.0, 9.0, 0.0], 3),
        "zero_sums_with_signs": ([2, 2, 2], [0.0, -0.0, 0.0], 3),  # compared as they are: -0.0 == 0.0, so the index decides
        "lane_boundaries": (list(range(300)), [0.0] * 300, 8),      # more poses than lanes; the winners sit at the high end
        "65536": (big_n, big_s, 8),
    }


def test_ranking_key_on_hand_made_tables(exe):
    cases = select_cases()
    got = run(exe, "\n".join(select_cmd(*c) for c in cases.values()))
    for (name, (n, s, k)), g in zip(cases.items(), got):
        assert g == expected_top(n, s, k), name
    assert got[1][:3] == [0, 1, 2] and got[2] == [1, 2, 0, -1, -1, -1, -1, -1] and got[3] == [0] + [-1] * 7 and got[4] == [-1] * 8
    # the 65 536 table has ties that only the index breaks among its first eight
    n, s, _ = cases["65536"]
    top = got[-1]
    assert len({(n[i], s[i]) for i in top}) < 8


VOXEL_VALUES = [2.0 ** 20 - 1, -(2.0 ** 20 - 1), 2.0 ** 20, -(2.0 ** 20), 1e30, -1e30, float("inf"), float("-inf"), float("nan"),
                np.nextafter(2.0 ** 20, 0.0), -np.nextafter(2.0 ** 20, 0.0), 0.5, -0.5, -1.0, 3.999]


def test_voxel_range_check(exe):
    got = run(exe, "voxel %d %s" % (len(VOXEL_VALUES), " ".join(repr(float(v)) for v in VOXEL_VALUES)))[0]
    for v, g in zip(VOXEL_VALUES, got):
        ok = bool(abs(v) < 2.0 ** 20)  # False for NaN
        assert g[0] == int(ok), v
        if ok:
            assert g[1:] == [int(np.floor(v)), 0, -1], v
        else:
            assert g[1:] == [12345, 12345, 12345], v  # nothing was written: nothing can be indexed with it
    assert [g[0] for g in got[:9]] == [1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(reloc_ref.in_range(np.array([[v, 0.25, -0.25] for v in VOXEL_VALUES])), [bool(g[0]) for g in got])


def test_transform_matches_the_expression_written_out(exe):
    rng = np.random.default_rng(3)
    toks, exp = [], []
    for i in range(64):
        R = rng.standard_normal(9) * (1e6 if i % 7 == 0 else 1.0)
        t = rng.standard_normal(3) * 10.0 ** rng.integers(-3, 7)
        p = (rng.standard_normal(3) * 30).astype(np.float32)
        x, y, z = float(p[0]), float(p[1]), float(p[2])
        exp.append([((R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z) + t[a] for a in range(3)])
        toks += [repr(float(v)) for v in list(R) + list(t) + [x, y, z]]
        assert np.array_equal(reloc_ref.transform(R, t, p[None])[0], exp[-1])  # the restatement is the same expression
    got = run(exe, "transform 64 " + " ".join(toks))[0]
    assert np.array_equal(np.array(got), np.array(exp))  # bit for bit: %.17g round-trips a double


def test_folds_add_in_the_fixed_order(exe):
    rng = np.random.default_rng(5)
    n_waves, n_chunks = 4, 9
    occ, inl = rng.integers(0, 64, (n_chunks, n_waves)), rng.integers(0, 64, (n_chunks, n_waves))
    s = rng.uniform(0, 1, (n_chunks, n_waves)) * 10.0 ** rng.integers(-8, 3, (n_chunks, n_waves))
    toks = ["fold", str(n_waves), str(n_chunks)]
    for c in range(n_chunks):
        for w in range(n_waves):
            toks += [str(occ[c, w]), str(inl[c, w]), repr(float(s[c, w]))]
    got = run(exe, " ".join(toks))[0]
    total = None
    for c in range(n_chunks):
        cs = s[c, 0]
        for w in range(1, n_waves):
            cs = cs + s[c, w]
        total = cs if total is None else total + cs
    assert got == [7, int(occ.sum()), int(inl.sum()), float(total)]


def test_the_same_program_under_asan_and_ubsan(exe, tmp_path):
    """a stand-alone executable of its own, built with -fsanitize=address,undefined and run on everything the other tests feed
    the plain build: same output, no report"""
    from mimosa_amd import build
    san = str(tmp_path / "reloc_select_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", build.CSRC, os.path.join(ROOT, "tests", "cpp", "reloc_select.cpp"), "-o", san])
    text = "\n".join(select_cmd(*c) for c in select_cases().values())
    text += "\nvoxel %d %s" % (len(VOXEL_VALUES), " ".join(repr(float(v)) for v in VOXEL_VALUES))
    text += "\ntransform 1 1 0 0 0 1 0 0 0 1 0.5 0.25 -3 1.5 2.5 3.5\nfold 2 2 1 1 0.5 2 2 0.25 3 3 0.125 4 4 1\n"
    a = subprocess.run([san], input=text, capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and a.stderr == "", a.stderr[-2000:]
    b = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert b.returncode == 0 and a.stdout == b.stdout


# ---- the restatement against the oracle ------------------------------------------------------------------------------------
def restatement_poses(aux):
    from mimosa_amd import synth
    Rg, tg = aux["R_W_L"], aux["t_W_L"]
    Rq, tq = synth.query_pose(Rg, tg)
    return [(Rg, tg), (Rq, tq), (synth.rot_z(np.pi / 2) @ Rg, tg), (Rg, tg + np.array([1.0, 0.0, 0.0])), (Rg, tg + np.array([1e7, 0.0, 0.0])),
            (Rg, tg + np.array([0.0, 0.0, 40.0]))]


@pytest.mark.parametrize("mode", [7, 19, 27])
def test_restatement_against_brute_force_over_the_oracle_map(mode):
    """reloc_ref.score_pose with knn = the oracle's knn_search (k = 1) against the same with a brute-force nearest point over
    the oracle's exported map restricted to the neighbour voxels"""
    from mimosa_amd import synth
    from oracle import ref_cpu
    m, pts, aux = synth.small_world()
    M = ref_cpu.Map(mode=mode)
    M.insert(m)
    coords, counts, xyz = M.export()
    occupied = set(map(tuple, coords.astype(np.int64)))
    assert occupied == reloc_ref.occupied_set(xyz)  # the voxels the oracle files its points under are floor(p / leaf)

    def oracle_knn(q):
        _, sq, found, _ = M.knn(q, 1)
        return found > 0, sq[:, 0]

    brute = reloc_ref.brute_knn(xyz, mode)
    cloud = synth.points_xyz(pts)
    some_inliers = False
    for R, t in restatement_poses(aux):
        for gate, stride in ((0.3, 1), (1.0, 3)):
            a = reloc_ref.score_pose(R, t, cloud, gate, stride, oracle_knn, occupied)
            b = reloc_ref.score_pose(R, t, cloud, gate, stride, brute, occupied)
            assert np.array_equal(a["found"], b["found"])
            edge = np.abs(b["d2"][b["found"]] - gate * gate) <= 1e-9 * gate * gate
            assert not edge.any()  # no point sits on the gate, where the last digit of d2 would decide
            assert (a["n_points"], a["n_occupied"], a["n_inliers"]) == (b["n_points"], b["n_occupied"], b["n_inliers"])
            assert abs(a["sum_sq"] - b["sum_sq"]) <= 1e-14 * max(b["sum_sq"], 1e-300)
            some_inliers = some_inliers or a["n_inliers"] > 0
    far = reloc_ref.score_pose(*restatement_poses(aux)[4], cloud, 1.0, 1, brute, occupied)
    assert (far["n_occupied"], far["n_inliers"], far["sum_sq"]) == (0, 0, 0.0) and far["n_points"] == len(cloud)
    assert some_inliers


# ---- ABI -------------------------------------------------------------------------------------------------------------------
RELOC_FUNCS = ["mh_icp_score_poses", "mh_icp_score_poses_async", "mh_icp_relocalise"]


def test_abi_symbols_and_version():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    for f in RELOC_FUNCS:
        assert hasattr(L, f), f
    assert set(RELOC_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    assert "#define MH_ABI_VERSION 3" in hdr


def test_struct_layouts_match_the_header(tmp_path):
    from mimosa_amd import capi
    items = [
        ("sizeof(mh_pose_score)", C.sizeof(capi.PoseScore)), ("sizeof(mh_icp_score_config)", C.sizeof(capi.ScoreConfig)),
        ("sizeof(mh_icp_reloc_config)", C.sizeof(capi.RelocConfig)), ("sizeof(mh_icp_reloc_candidate)", C.sizeof(capi.RelocCandidate)),
        ("sizeof(mh_icp_reloc_result)", C.sizeof(capi.RelocResult)),
        ("(size_t)MH_RELOC_MAX_POSES", capi.MH_RELOC_MAX_POSES), ("(size_t)MH_RELOC_MAX_REFINE", capi.MH_RELOC_MAX_REFINE),
    ]
    for struct, cls in (("mh_pose_score", capi.PoseScore), ("mh_icp_score_config", capi.ScoreConfig), ("mh_icp_reloc_config", capi.RelocConfig),
                        ("mh_icp_reloc_candidate", capi.RelocCandidate), ("mh_icp_reloc_result", capi.RelocResult)):
        for name, _ in cls._fields_:
            items.append((f"offsetof({struct}, {name})", getattr(cls, name).offset))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mimosa_hip.h"\nint main(void) {\n' +
                   "".join(f'  printf("%zu\\n", {expr});\n' for expr, _ in items) + "  return 0;\n}\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [v for _, v in items], [(e, g, v) for (e, v), g in zip(items, got) if g != v]
    assert C.sizeof(capi.PoseScore) == 24 == capi.POSE_SCORE_DTYPE.itemsize
    assert [capi.POSE_SCORE_DTYPE.fields[n][1] for n, _ in capi.PoseScore._fields_] == [getattr(capi.PoseScore, n).offset for n, _ in capi.PoseScore._fields_]


def test_refusals_that_need_no_device():
    from mimosa_amd import capi
    L = capi.load()
    L.mh_last_error.restype = C.c_char_p
    I, z, g = np.eye(3).ravel().copy(), np.zeros(3), np.array([0.0, 0.0, -1.0])
    scfg = capi.ScoreConfig(1.0, 1, 1)
    scores, best = np.zeros(1, capi.POSE_SCORE_DTYPE), np.zeros(8, np.int32)
    for fn in (L.mh_icp_score_poses, L.mh_icp_score_poses_async):
        rc = fn(None, capi._p(I), capi._p(z), 1, C.byref(scfg), capi._p(scores), capi._p(best))
        assert rc == capi.MH_ERR_INVALID_ARG
        assert b"mh_icp_score_poses" in L.mh_last_error(None) and b"NULL" in L.mh_last_error(None)
    rcfg, out = capi.make_reloc_config(), capi.RelocResult()
    rc = L.mh_icp_relocalise(None, capi._p(I), capi._p(z), 1, capi._p(g), C.byref(rcfg), C.byref(out))
    assert rc == capi.MH_ERR_INVALID_ARG
    assert b"mh_icp_relocalise" in L.mh_last_error(None) and b"NULL" in L.mh_last_error(None)


def test_pose_grid_order_is_the_documented_one():
    from mimosa_amd import capi
    R0 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t0 = np.array([1.0, 2.0, 3.0])
    R, t = capi.pose_grid(R0, t0, 1.0, 0.5, 0.2, 0.1)
    nx, nw, side = 2, 2, 5
    assert R.shape == (5 * 25, 3, 3) and t.shape == (125, 3)
    for iw in (-2, 0, 2):
        for ix in (-2, 1):
            for iy in (-1, 2):
                i = (iw + nw) * side * side + (ix + nx) * side + (iy + nx)
                a = iw * 0.1
                Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
                assert np.array_equal(R[i], Rz @ R0) and np.array_equal(t[i], [1.0 + ix * 0.5, 2.0 + iy * 0.5, 3.0])
    R1, t1 = capi.pose_grid(R0, t0, 0.0, 0.5, 0.0, 0.0)
    assert R1.shape == (1, 3, 3) and np.array_equal(R1[0], R0) and np.array_equal(t1[0], t0)
