"""-m gpu: the degenerate-geometry zoo (tests/degeneracy_zoo.py) on the device.  Every family and pose goes through
mh_icp_linearize with the component pass on (eigvec_* are K4's bases: sym_eigvec3_fast with compute_localizability behind it, on
the DEVICE branches of math3.hpp) and off (the host epilogue's), unary and, for three families, binary; through
mh_icp_linearize_batch alone and in a window of nine factors (the staged launch form: another launch class); through the one-,
two- and four-lane classes in a worker each; one case tiled past 65 536 points (the 512-thread class).  Every result is held to the
multi-precision reference of the blocks it reports itself: loc_*_final, eigvec_*, the component sums on the reported bases,
the 4-DoF projection.  The degeneracy decision is approached from both sides of every kept threshold through four routes:
mh_icp_linearize with project_on_degneneracy (H_ss and b_s exactly zero iff degenerate), mh_icp_align with one iteration (the
trace's degenerate bits), mh_icp_align_batch with members on either side, mh_icp_window_optimise with W = 2 (kWRowDegen).
No oracle takes part in any of that; one further test holds the sums, counters and per-point state of the same scenes to the CPU
oracle at parity.py's bar, so that nothing a result carries goes uncompared here.  tests/test_degeneracy_zoo_cpu.py runs the same checks on the CPU oracle and on the host build of the
solvers.  The worst ratio to every bar is printed per route (pytest -s); the measured figures are in DESIGN.md."""
import os
import subprocess
import sys

import numpy as np
import pytest

import degeneracy_zoo as Z

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_worst = {}


def _report(route, ratios):
    _worst.setdefault(route, Z.Ratios()).merge(ratios)
    print(_worst[route].line(f"[degeneracy-zoo] device, {route}, worst so far"))


@pytest.fixture(scope="module")
def dev(ctx):
    from mimosa_amd import capi

    maps, factors = {}, []

    def factor(sc, pts=None, binary=False, **cfg):
        key = (sc.name, sc.pose)
        if key not in maps:
            maps[key] = capi.VoxelMap(ctx, **Z.MAP_KW)
            maps[key].insert(sc.map_xyz)
            assert maps[key].stats()["n_points"] == len(sc.map_xyz)  # every map point is present
        f = capi.ICPFactor(ctx, maps[key], np.ascontiguousarray(sc.pts if pts is None else pts), capi.make_reg_config(**Z.config(**cfg)), binary=binary)
        factors.append(f)
        return f

    yield factor
    for f in factors:
        f.destroy()
    for m in maps.values():
        m.release()


@pytest.mark.parametrize("name,pose", Z.CASES)
def test_linearize(dev, name, pose):
    sc = Z.build(name, pose)
    label = f"device {name} {pose}"
    r = Z.Ratios()
    f = dev(sc)
    k4 = f.linearize(sc.R, sc.t, Z.G_UNIT)
    assert int(k4["status_hist"][Z.VALID]) == sc.n_designed
    Z.check_result(k4, label + " K4 bases", r)
    Z.check_components(k4, sc.pts, sc.R, f.state(), label, r)
    print(Z.describe(name, pose, k4))
    _report("linearize, K4's bases", r)
    # the host epilogue's bases (component pass off), on the same sums
    r = Z.Ratios()
    g = dev(sc)
    g.set_components(False)
    host = g.linearize(sc.R, sc.t, Z.G_UNIT)
    assert np.array_equal(host["H_ss"], k4["H_ss"])
    Z.check_result(host, label + " host bases", r)
    for k in ("loc_rot_final", "loc_trans_final"):
        assert np.array_equal(host[k], k4[k], equal_nan=True), k  # (the localizabilities are the host's either way)
    _report("linearize, the host's bases", r)
    # reg_4_dof on the same sums
    r = Z.Ratios()
    reg = dev(sc, reg_4_dof=1).linearize(sc.R, sc.t, Z.G_UNIT)
    Z.check_reg4(k4, reg, sc.R, Z.G_UNIT, label, r)
    _report("linearize, reg_4_dof", r)


@pytest.mark.parametrize("name,pose", [c for c in Z.CASES if c[0] in Z.BINARY_FAMILIES])
def test_linearize_binary(dev, name, pose):
    sc = Z.build(name, pose)
    r = Z.Ratios()
    f = dev(sc, binary=True)
    Rs, ts, Rt, tt = Z.binary_poses(sc)
    res = f.linearize(Rs, ts, Z.G_UNIT, R_tgt=Rt, t_tgt=tt)
    assert int(res["status_hist"][Z.VALID]) == sc.n_designed
    Z.check_result(res, f"device binary {name} {pose}", r)
    Z.check_components(res, sc.pts, sc.R, f.state(), f"device binary {name} {pose}", r)
    _report("linearize, binary", r)


@pytest.mark.parametrize("name,pose", Z.CASES)
def test_linearize_batch(dev, name, pose):
    from mimosa_amd import capi

    sc = Z.build(name, pose)
    label = f"device batch {name} {pose}"
    r = Z.Ratios()
    f = dev(sc)
    res = capi.linearize_batch([f], [sc.R], [sc.t], g_units=[Z.G_UNIT])[0]
    assert int(res["status_hist"][Z.VALID]) == sc.n_designed
    Z.check_result(res, label, r)
    Z.check_components(res, sc.pts, sc.R, f.state(), label, r)
    _report("batch, one factor", r)
    # a window of nine: the full cloud and eight small parts of it (every part a more degenerate scene of its own)
    r = Z.Ratios()
    parts = [sc.pts] + [sc.pts[:m] for m in (1, 2, 3, 5, 17, 64, 65, 100)]
    fs = [dev(sc, pts=p) for p in parts]
    out = capi.linearize_batch(fs, [sc.R] * 9, [sc.t] * 9, g_units=[Z.G_UNIT] * 9)
    for fi, p, o in zip(fs, parts, out):
        assert int(o["status_hist"][Z.VALID]) == min(len(p), sc.n_designed)
        Z.check_result(o, f"{label} window of nine, {len(p)} points", r)
        Z.check_components(o, p, sc.R, fi.state(), f"{label} window of nine, {len(p)} points", r)
    _report("batch, window of nine", r)


@pytest.mark.parametrize("name,pose", Z.CASES)
def test_sums_and_counters_against_the_oracle(dev, name, pose):
    """What the decompositions start from, at the same scenes: status histogram, H_ss, b_s, f (binary: H_st, H_tt, b_t), the
    component sums and the k-NN counters against the CPU oracle at parity.py's bar, the per-point state to 1e-9.  (parity.py
    compares eigenvectors and the Schur degeneracy info only at well-conditioned blocks: the zoo's checks above are what holds
    the bases here.)"""
    from oracle import ref_cpu
    from parity import assert_result_parity, assert_state_parity

    sc = Z.build(name, pose)
    rm = ref_cpu.Map(**Z.MAP_KW)
    rm.insert(sc.map_xyz)
    for binary in (False, True) if name in Z.BINARY_FAMILIES else (False,):
        gf = dev(sc, binary=binary)
        rf = ref_cpu.ICP(rm, sc.pts, ref_cpu.make_config(**Z.config()), binary=binary)
        if binary:
            Rs, ts, Rt, tt = Z.binary_poses(sc)
            got, ref = gf.linearize(Rs, ts, Z.G_UNIT, R_tgt=Rt, t_tgt=tt), rf.linearize(Rs, ts, Z.G_UNIT, R_tgt=Rt, t_tgt=tt)
        else:
            got, ref = gf.linearize(sc.R, sc.t, Z.G_UNIT), rf.linearize(sc.R, sc.t, Z.G_UNIT)
        assert_result_parity(got, ref, binary=binary, check_eigvec=False)
        assert_state_parity(gf.state(), rf.state())


def _worker(tmp_path, tag, env):
    out = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "degeneracy_zoo_worker.py"), out], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:]
    return np.load(out)


@pytest.mark.parametrize("tag,env", (("one-lane", {"MH_QL2_MAX": "0", "MH_QL4_MAX": "0"}), ("two-lane", {"MH_QL2_MAX": "32768", "MH_QL4_MAX": "0"}),
                                     ("four-lane", {"MH_QL2_MAX": "32768", "MH_QL4_MAX": "32768"})))
def test_lane_classes(tmp_path, tag, env):
    blob = _worker(tmp_path, tag, env)
    r = Z.Ratios()
    for ci, (name, pose) in enumerate(Z.CASES):
        sc = Z.build(name, pose)
        res = {k[len(f"c{ci}_"):]: blob[k] for k in blob.files if k.startswith(f"c{ci}_")}
        assert int(res["status_hist"][Z.VALID]) == sc.n_designed
        Z.check_result(res, f"device {tag} {name} {pose}", r)
        Z.check_components(res, sc.pts, sc.R, [res[f"state{i}"] for i in range(3)], f"device {tag} {name} {pose}", r)
    _report(f"{tag} class", r)


def test_tiled_cloud_runs_the_512_thread_class(dev):
    sc = Z.build(*Z.TILED)
    pts = Z.tiled_points(sc)
    r = Z.Ratios()
    f = dev(sc, pts=pts)
    res = f.linearize(sc.R, sc.t, Z.G_UNIT)
    assert int(res["status_hist"][Z.VALID]) == Z.TILES * sc.n_designed
    Z.check_result(res, "device tiled", r)
    Z.check_components(res, pts, sc.R, f.state(), "device tiled", r)
    print(Z.describe(sc.name + f" x{Z.TILES}", sc.pose, res))
    _report("tiled, 512-thread class", r)


def _bit(blk):
    return 1 if blk == "rot" else 2


@pytest.mark.parametrize("name,pose", Z.CASES)
def test_decisions(dev, name, pose):
    from mimosa_amd import capi

    sc = Z.build(name, pose)
    plain = dev(sc).linearize(sc.R, sc.t)
    B = Z.blocks_of(plain)
    acfg = capi.make_align_config(max_iters=1, damping=1e-9, prior_sigma_rot=0.1, prior_sigma_trans=0.1)
    wcfg = capi.make_window_config(iters=1)
    n = dict(linearize=0, linearize_one_sided=0, align=0, batch=0, window=0)
    members = []  # (block, threshold, factor) of the chain routes
    for blk, other in (("rot", "trans"), ("trans", "rot")):
        kept, dropped, _ = Z.thresholds(B[blk])
        assert dropped == 0 or sc.family in Z.EXEMPT, (name, pose, blk, dropped)
        for t, want in kept:
            label = f"device {name} {pose} {blk} threshold {t!r} (lambda / |A| {Z.reference(B[blk]).rel})"
            # 1. linearize with the projection: H_ss and b_s are exactly zero iff degenerate
            res = dev(sc, project_on_degneneracy=1, **{f"degen_thresh_{blk}": t, f"degen_thresh_{other}": -1.0}).linearize(sc.R, sc.t)
            if want:
                assert Z.is_zero_result(res), label
                Z.check_zero_localizabilities(res, label)
                n["linearize"] += 1
            elif Z.never_degenerate(B[other]):
                assert np.array_equal(res["H_ss"], plain["H_ss"]) and np.array_equal(res["b_s"], plain["b_s"]) and np.any(res["H_ss"]), label
                for k in ("loc_rot_final", "loc_trans_final", "eigvec_rot", "eigvec_trans"):
                    assert np.array_equal(res[k], plain[k]), (label, k)
                n["linearize"] += 1
            else:  # the other block has a rounding-level eigenvalue, whose root may be NaN: it may project whatever this block does
                assert np.array_equal(res["H_ss"], plain["H_ss"]) or Z.is_zero_result(res), label
                n["linearize_one_sided"] += 1
            # 2. mh_icp_align, one iteration: the trace's bit of this block, against the blocks this chain reports
            g = dev(sc, **{f"degen_thresh_{blk}": t, f"degen_thresh_{other}": -1.0})
            got = g.align(sc.R, sc.t, acfg)
            ok, want_a = Z.decision(Z.blocks_of(got["first"])[blk], t)
            assert ok, label
            assert bool(got["trace"][0]["degenerate"] & _bit(blk)) == want_a, (label, "align", got["trace"][0]["degenerate"])
            n["align"] += 1
            g.reset()
            members.append((blk, t, g, label))
    if members:
        # 3. mh_icp_align_batch: every kept threshold of both blocks side by side (members on either side of each eigenvalue)
        got = capi.align_batch([m[2] for m in members], [(sc.R, sc.t)] * len(members), acfg)
        for (blk, t, g, label), o in zip(members, got):
            ok, want_b = Z.decision(Z.blocks_of(o["first"])[blk], t)
            assert ok, label
            assert bool(o["trace"][0]["degenerate"] & _bit(blk)) == want_b, (label, "align_batch", o["trace"][0]["degenerate"])
            n["batch"] += 1
            g.reset()
        # 4. mh_icp_window_optimise, W = 2: the two float32 neighbours of an eigenvalue's root, then the two at 1 -+ 1e-3
        for i in range(0, len(members) - 1, 2):
            pair = members[i:i + 2]
            if pair[0][0] != pair[1][0]:
                continue
            got = capi.optimise_window([m[2] for m in pair], [(sc.R, sc.t)] * 2, wcfg, has_Z=[0, 1], Z=[(np.eye(3), np.zeros(3))] * 2)
            assert got["iters"] == 1
            for j, (blk, t, g, label) in enumerate(pair):
                ok, want_w = Z.decision(Z.blocks_of(got["first"][j])[blk], t)
                assert ok, label
                assert bool((got["trace"][0]["degenerate"] >> (2 * j)) & _bit(blk)) == want_w, (label, "window", j, got["trace"][0]["degenerate"])
                n["window"] += 1
                g.reset()
    print(f"[degeneracy-zoo] decisions {name} {pose}: " + ", ".join(f"{k} {v}" for k, v in n.items()))
    if sc.family not in Z.EXEMPT:
        assert n["align"] == 8 and n["batch"] == 8 and n["window"] == 8 and n["linearize"] + n["linearize_one_sided"] == 8
