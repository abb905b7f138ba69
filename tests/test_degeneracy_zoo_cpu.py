"""The degenerate-geometry zoo (tests/degeneracy_zoo.py) without a GPU: the scenes run through the CPU oracle (oracle/ref_cpu.hpp),
the scene conditions are asserted on the reference alone (intended rank and clusters per family, decidable thresholds, no more
than four points with a component at 0.5), the oracle's own localizabilities, bases, component sums, 4-DoF projection and
degeneracy decisions are held to the zoo's bars, and the zoo's blocks go through the HOST build of math3.hpp / align_device.hpp
(tests/cpp/degeneracy_eigen_check.cpp: sym_eigen3, sym_eigvec3_fast, compute_localizability, align_block_degenerate), once more
under AddressSanitizer + UBSan as a stand-alone program.  This proves the bars on the host branches before anything runs on a
device.  Per case the spectrum, the clusters, the thresholds kept and nb are printed, and the worst ratio to every bar (pytest -s).
tests/test_gpu_degeneracy_zoo.py runs the same checks on the device."""
import functools
import os
import subprocess

import numpy as np
import pytest

import degeneracy_zoo as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_worst = Z.Ratios()


@functools.lru_cache(maxsize=None)
def oracle_case(name, pose, reg4=0):
    from oracle import ref_cpu

    sc = Z.build(name, pose)
    m = ref_cpu.Map(**Z.MAP_KW)
    m.insert(sc.map_xyz)
    assert m.num_points == len(sc.map_xyz)  # every map point is present
    f = ref_cpu.ICP(m, sc.pts, ref_cpu.make_config(**Z.config(reg_4_dof=reg4)))
    res = f.linearize(sc.R, sc.t, Z.G_UNIT)
    return sc, res, f.state()


@pytest.mark.parametrize("name,pose", Z.CASES)
def test_scene_conditions_and_oracle(name, pose):
    sc, res, state = oracle_case(name, pose)
    fam = sc.family
    assert int(res["status_hist"][Z.VALID]) == sc.n_designed and int(res["status_hist"][1]) == len(sc.pts) - sc.n_designed
    B = Z.blocks_of(res)
    rt, rr = Z.reference(B["trans"]), Z.reference(B["rot"])
    # intended spectrum
    if fam in Z.INTENDED_RANK_AXIS:
        want_t, want_r = Z.INTENDED_RANK_AXIS[fam]
        if pose == "axis":
            assert (Z.rank_of(rt), Z.rank_of(rr)) == (want_t, want_r), (rt.rel, rr.rel)
            assert all(r == 0.0 for r in rt.rel[: 3 - want_t]), rt.rel  # exact zeros in the axis pose
        else:  # the float32 rounding of the map at 100 m: vanishing eigenvalues at rounding level, the others as designed
            assert all(abs(r) <= 1e-8 for r in rt.rel[: 3 - want_t]) and all(r > 1e-3 for r in rt.rel[3 - want_t:]), rt.rel
            assert all(abs(r) <= 1e-8 for r in rr.rel[: 3 - want_r]) and all(r > 1e-3 for r in rr.rel[3 - want_r:]), rr.rel
    if fam == "square_tunnel" and pose == "axis":
        assert rt.clusters == [[0], [1, 2]]
    if fam == "square_tunnel":
        assert rt.rel[2] - rt.rel[1] <= 1e-5  # (equal up to the float32 rounding of the map)
    if fam == "cube_centre":
        assert rt.rel[2] - rt.rel[0] <= 1e-5 and (pose != "axis" or rt.clusters == [[0, 1, 2]])
    if fam == "near_parallel":
        e = float(name.rsplit("_", 1)[1])
        assert 0.02 * e * e <= rt.rel[0] <= 0.5 * e * e or (e == 1e-6 and abs(rt.rel[0]) <= 1e-10), rt.rel
    if fam == "tunnel_end":  # a small eigenvalue that is decided: thresholds on both of its sides
        for blk in ("trans", "rot"):
            kept, dropped, p = Z.thresholds(B[blk])
            assert p == 0 and dropped == 0 and sorted(d for _, d in kept) == [False, False, True, True]
    if fam == "few":
        m = int(name.rsplit("_", 1)[1])
        assert Z.rank_of(rt) == min(m, 3) or pose == "generic"
    # thresholds
    for blk in ("trans", "rot"):
        kept, dropped, p = Z.thresholds(B[blk])
        if fam not in Z.EXEMPT:
            assert dropped == 0 and p is not None, (name, pose, blk, dropped)
    print(Z.describe(name, pose, res))
    # the oracle's own results
    r = Z.Ratios()
    Z.check_result(res, f"oracle {name} {pose}", r)
    Z.check_components(res, sc.pts, sc.R, state, f"oracle {name} {pose}", r)
    _, _, n, nb = Z.component_sums(sc.pts, sc.R, state, res["eigvec_trans"], res["eigvec_rot"])
    print(f"[degeneracy-zoo] {name} {pose}: valid {n}, nb {nb}; " + r.line("oracle ratios"))
    _worst.merge(r)
    print(_worst.line("[degeneracy-zoo] oracle, worst so far"))


def test_some_block_of_every_family_is_decided_on_both_sides():
    """every family but the exempt ones has a block whose smallest eigenvalue carries thresholds on both of its sides"""
    for name in Z.FAMILIES:
        if Z.family_of(name) in Z.EXEMPT or Z.family_of(name) == "slab":  # (slab: both blocks rank deficient by design)
            continue
        for pose in Z.POSES:
            B = Z.blocks_of(oracle_case(name, pose)[1])
            assert any({d for _, d in Z.thresholds(B[blk])[0]} == {False, True} for blk in B), (name, pose)


@pytest.mark.parametrize("name,pose", Z.CASES)
def test_oracle_decisions(name, pose):
    """projection_matrix of the oracle on its own localizabilities, at every kept threshold"""
    from oracle import ref_cpu

    _, res, _ = oracle_case(name, pose)
    for blk, A in Z.blocks_of(res).items():
        for t, want in Z.thresholds(A)[0]:
            got, _, _ = ref_cpu.projection_matrix(res[f"loc_{blk}_final"], t, res[f"eigvec_{blk}"])
            assert got == want, (name, pose, blk, t, want, Z.reference(A).rel)


@pytest.mark.parametrize("name,pose", [c for c in Z.CASES if c[0] in ("floor", "tunnel", "cube_centre", "near_parallel_1e-6", "few_3")])
def test_oracle_four_dof(name, pose):
    sc, plain, _ = oracle_case(name, pose)
    _, reg, _ = oracle_case(name, pose, 1)
    r = Z.check_reg4(plain, reg, sc.R, Z.G_UNIT, f"oracle {name} {pose}")
    print(r.line(f"[degeneracy-zoo] oracle reg_4_dof {name} {pose}"))


def _hex(x):
    return float(x).hex()


def _unhex(s):
    return float("nan") if "nan" in s else float.fromhex(s)


def _run_host_check(tmp_path, exe, tag):
    rows = []
    for name, pose in Z.CASES:
        for bi, blk in enumerate(("rot", "trans")):
            A = Z.blocks_of(oracle_case(name, pose)[1])[blk]
            kept = Z.thresholds(A)[0]
            rows.append((name, pose, bi, A, kept))
    # blocks no scene gives: the zero block (what the degeneracy projection leaves), and scaled copies (1e-6, 1e9)
    rows.append(("zero", "-", 0, np.zeros((3, 3)), []))
    for name, pose, bi, A, _ in list(rows[:8]):
        for s in (2.0 ** -20, 2.0 ** 30):
            rows.append((name + f" x{s:g}", pose, bi, A * s, Z.thresholds(A * s)[0]))
    fin, fout = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")
    with open(fin, "w") as f:
        for _, _, bi, A, kept in rows:
            ts = [t for t, _ in kept] + [1.0] * (4 - len(kept))
            f.write(" ".join([str(bi)] + [_hex(x) for x in A.ravel()] + [_hex(t) for t in ts]) + "\n")
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    lines = open(fout).read().splitlines()
    assert len(lines) == len(rows)
    ratios, accepted = Z.Ratios(), 0
    for (name, pose, bi, A, kept), line in zip(rows, lines):
        tok = line.split()
        w, V = np.array([_unhex(x) for x in tok[0:3]]), np.array([_unhex(x) for x in tok[3:12]]).reshape(3, 3)
        ok, F = int(tok[12]), np.array([_unhex(x) for x in tok[13:22]]).reshape(3, 3)
        loc, E = np.array([_unhex(x) for x in tok[22:25]]), np.array([_unhex(x) for x in tok[25:34]]).reshape(3, 3)
        dec = [int(x) for x in tok[34:38]]
        label = f"{tag} {name} {pose} block {bi}"
        # sym_eigen3's eigenvalues as the localizabilities' squares: a negative rounding-level one is the NaN root
        with np.errstate(invalid="ignore"):
            Z.check_block(A, np.sqrt(w), V, label + " sym_eigen3", ratios)
        Z.check_block(A, loc, E, label + " compute_localizability", ratios)
        if ok:
            accepted += 1
            Z.check_block(A, loc, F, label + " sym_eigvec3_fast", ratios, eigenvalues=False)
        for (t, want), got in zip(kept, dec):
            assert bool(got) == want, (label, "align_block_degenerate", t, want, Z.reference(A).rel)
    assert accepted >= len(rows) // 4, accepted  # the fast path takes part
    print(ratios.line(f"[degeneracy-zoo] {tag}: {len(rows)} blocks, sym_eigvec3_fast accepted {accepted}; worst ratios"))
    return ratios


def test_host_solvers_on_the_zoo_blocks(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "degeneracy_eigen_check.cpp")
    exe = str(tmp_path / "degeneracy_eigen_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", src, "-o", exe])
    _run_host_check(tmp_path, exe, "host")


def test_host_solvers_under_sanitizers(tmp_path):
    """the same stand-alone program built with AddressSanitizer and UBSan, run directly"""
    src = os.path.join(ROOT, "tests", "cpp", "degeneracy_eigen_check.cpp")
    exe = str(tmp_path / "degeneracy_eigen_check_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Wno-unknown-pragmas", "-Werror", src, "-o", exe])
    _run_host_check(tmp_path, exe, "host-sanitized")
