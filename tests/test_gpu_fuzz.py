"""-m gpu: randomised configurations of the hot path against the oracle — room size, map density (sparse to
saturated voxels), leaf size, neighbour mode, k, Huber on/off, 4-DoF, pose error, and a re-linearization walk
whose steps straddle the data-association threshold (a mix of cached and re-associated points per call)."""
import numpy as np
import pytest

from degeneracy_zoo import check_result
from mimosa_amd import synth
from parity import assert_result_parity, assert_state_parity

pytestmark = pytest.mark.gpu


def _EXTRA(base):
    """MH_FUZZ_EXTRA=N: N more seeds per fuzz test (a bug hunt on demand, not part of the default suite)"""
    import os
    return [base + i for i in range(int(os.environ.get("MH_FUZZ_EXTRA", "0")))]


def _case(seed):
    rng = np.random.default_rng(1000 + seed)
    room = np.array([rng.uniform(5, 14), rng.uniform(4, 11), rng.uniform(2.5, 5)])
    grid = float(rng.choice([0.07, 0.11, 0.16, 0.3, 0.45]))       # 0.07: saturated 20-point voxels; 0.45: ~1 point / voxel
    leaf = float(rng.choice([0.3, 0.5, 1.0]))
    m = synth.make_room(4000 + seed, 0, 0, grid=grid, room=room)
    loc = np.array([rng.uniform(1.5, room[0] - 1.5), rng.uniform(1.5, room[1] - 1.5), rng.uniform(0.8, room[2] - 0.8)])
    pts, aux = synth.make_scan(n_rows=int(rng.choice([8, 16, 32])), seed=5000 + seed, n_cols=int(rng.choice([64, 128])),
                               room=room, sensor_local=loc)
    cfg = synth.enwide_config()
    cfg.update(target_ivox_map_leaf_size=leaf, source_voxel_grid_filter_leaf_size=leaf,
               target_ivox_map_min_dist_in_voxel=float(rng.choice([0.02, 0.1, 0.15])),
               num_corres_points=int(rng.choice([5, 5, 5, 8, 3])), use_huber=int(rng.integers(0, 2)),
               reg_4_dof=int(rng.integers(0, 2)), max_corres_distance=float(rng.choice([0.3, 1.0, 2.24])),
               plane_validity_distance=float(rng.choice([0.04, 0.07, 0.2])),
               project_on_degneneracy=int(rng.integers(0, 2)), degen_thresh_rot=float(rng.choice([0.0, 10.0])),
               degen_thresh_trans=float(rng.choice([15.0, 40.0])))
    mode = int(rng.choice([7, 19, 19, 27]))
    dR = synth.so3_exp(np.deg2rad(rng.normal(0, 1.0, 3)))
    R = aux["R_W_L"] @ dR
    t = aux["t_W_L"] + aux["R_W_L"] @ rng.normal(0, 0.06, 3)
    return m, pts, cfg, mode, R, t, rng


# 225, 271, 356, 923: found by the wide sweep (MH_FUZZ_EXTRA=1500) — neighbourhoods whose two smallest covariance
# eigenvalues are within 1-10 % of each other; 356 put one Valid point's normal 5 degrees off (H 3.5e-5 off) before
# plane_eigen got its Rayleigh refinement.  238, 1303: 4-5 valid points in all, H singular
@pytest.mark.parametrize("seed", list(range(40)) + [225, 238, 271, 356, 923, 1303] + _EXTRA(100))
def test_random_configuration(ctx, seed):
    from mimosa_amd import capi
    from oracle import ref_cpu

    m, pts, cfg, mode, R, t, rng = _case(seed)
    leaf, md = cfg["target_ivox_map_leaf_size"], cfg["target_ivox_map_min_dist_in_voxel"]
    gm = capi.VoxelMap(ctx, leaf=leaf, min_dist=md, mode=mode)
    rm = ref_cpu.Map(leaf=leaf, min_dist=md, mode=mode)
    for chunk in np.array_split(m, 2):
        gm.insert(chunk)
        rm.insert(chunk)
    assert gm.stats()["n_points"] == rm.num_points
    gf = capi.ICPFactor(ctx, gm, pts, capi.make_reg_config(**cfg))
    rf = ref_cpu.ICP(rm, pts, ref_cpu.make_config(**cfg))
    g_unit = np.array([0.02, -0.01, -1.0])
    g_unit /= np.linalg.norm(g_unit)
    thr = md / 4.0
    for step in range(4):
        got, ref = gf.linearize(R, t, g_unit), rf.linearize(R, t, g_unit)
        assert_result_parity(got, ref, check_eigvec=False)
        assert_state_parity(gf.state(), rf.state())
        # next pose: translation around the DA threshold so that only part of the cloud re-associates,
        # plus a rotation that moves far points more than near ones
        t = t + rng.normal(0, 1.0, 3) * thr * rng.choice([0.3, 1.0, 3.0])
        R = R @ synth.so3_exp(rng.normal(0, 1.0, 3) * thr / 5.0)
    gf.destroy()
    gm.release()


def _random_cloud(rng, n):
    """Points with every kind of voxel population: uniform background, tight clusters (hundreds to thousands of points in one
    voxel), exact duplicates, points on voxel faces, a few far away."""
    xyz = rng.uniform(-30.0, 30.0, size=(n, 3))
    for _ in range(int(rng.integers(1, 6))):
        m = min(n, int(rng.integers(50, max(51, n // 4))))
        c = rng.uniform(-20, 20, 3)
        sel = rng.permutation(n)[:m]
        xyz[sel] = c + rng.uniform(0, float(rng.choice([0.05, 0.4, 1.5])), size=(m, 3))
    dup = rng.permutation(n)[: n // 20]
    xyz[dup] = xyz[rng.permutation(n)[: len(dup)]]
    face = rng.permutation(n)[: n // 50]
    xyz[face] = np.round(xyz[face] * 2.0) / 2.0               # exactly on 0.5 m voxel boundaries
    return xyz.astype(np.float32)


@pytest.mark.parametrize("seed", list(range(20)) + _EXTRA(200))
def test_random_scan_frontend(ctx, seed):
    """prepareInput -> preprocess on random clouds and filter settings: same points, same order, same bits as the oracle."""
    from mimosa_amd import capi
    from oracle import ref_cpu

    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([1, 63, 64, 65, 1000, 4097, 20000]))
    raw = np.zeros(n, dtype=synth.OUSTER_DTYPE)
    xyz = _random_cloud(rng, n)
    raw["x"], raw["y"], raw["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    raw["intensity"] = rng.uniform(0, 2000, n).astype(np.float32)
    raw["t"] = rng.integers(0, int(rng.choice([3, 200, 5000, 2**31])), n, dtype=np.uint32)
    raw["ring"] = rng.integers(0, 64, n).astype(np.uint16)
    bad = rng.permutation(n)[: n // 30]
    raw["x"][bad] = np.nan
    kw = dict(point_skip_divisor=int(rng.choice([1, 2, 3])), ring_skip_divisor=int(rng.choice([1, 2])),
              range_min=float(rng.choice([0.0, 2.0])), range_max=float(rng.choice([25.0, 100.0])),
              intensity_min=float(rng.choice([0.0, 300.0])), create_full_res_pointcloud=int(rng.integers(0, 2)), ns_max=1.0e10)
    leaf, min_dist = float(rng.choice([0.25, 0.5, 1.0])), float(rng.choice([0.0, 0.05, 0.15]))
    R = synth.so3_exp(rng.normal(0, 0.3, 3)).astype(np.float32)
    tt = rng.normal(0, 0.5, 3).astype(np.float32)
    o = ref_cpu.prepare_input(raw, ref_cpu.make_input_config(**kw))
    full = np.frombuffer(np.ascontiguousarray(o["points_full"]).tobytes(), dtype=synth.POINT_DTYPE)
    body = ref_cpu.transform_f32(full[o["geometric_idxs"].astype(np.int64)], R, tt)
    kept = ref_cpu.downsample(body, leaf, 20, min_dist)
    sc = capi.Scan(ctx)
    info = sc.prepare_input(raw, capi.make_input_config(**kw))
    assert info["n_full"] == len(full) and info["n_geometric"] == len(o["geometric_idxs"]) and info["last_point_ns"] == o["last_point_ns"]
    assert np.array_equal(sc.unique_ns(), o["unique_ns"])
    assert sc.points(capi.Scan.FULL).tobytes() == full.tobytes()
    assert np.array_equal(sc.indices(0), o["geometric_idxs"].astype(np.uint32))
    info = sc.preprocess_geometric(R, tt, leaf, 20, min_dist)
    assert info["n_downsampled"] == len(kept)
    assert np.array_equal(sc.indices(1), kept)
    assert sc.points(capi.Scan.DOWNSAMPLED).tobytes() == body[kept].tobytes()
    sc.destroy()


@pytest.mark.parametrize("seed", list(range(15)) + _EXTRA(300))
def test_random_map_insert_sequences(ctx, seed):
    """iVox insert + LRU purge over random batch sequences (clusters that saturate voxels, duplicates, boundary points, tiny and
    large batches): getCloud — points AND order — equals the oracle's after every insert."""
    from mimosa_amd import capi
    from oracle import ref_cpu

    rng = np.random.default_rng(9000 + seed)
    leaf, md = float(rng.choice([0.3, 0.5, 1.0])), float(rng.choice([0.0, 0.05, 0.15]))
    horizon, cycle = int(rng.choice([2, 3, 1000])), int(rng.choice([2, 3, 10]))
    gm = capi.VoxelMap(ctx, leaf=leaf, min_dist=md, mode=19, lru_horizon=horizon, lru_clear_cycle=cycle)
    rm = ref_cpu.Map(leaf=leaf, min_dist=md, mode=19, lru_horizon=horizon)
    rm.set_lru_clear_cycle(cycle)
    for b in range(7):
        n = int(rng.choice([1, 5, 64, 700, 5000, 30000]))
        xyz = _random_cloud(rng, n) + np.float32(rng.choice([0.0, 0.0, 15.0]))   # some batches land somewhere new
        gm.insert(xyz)
        rm.insert(xyz)
        assert gm.stats()["n_points"] == rm.num_points, b
        assert np.array_equal(gm.get_cloud(), rm.export()[2]), b
    gm.release()


@pytest.mark.parametrize("seed", list(range(12)) + _EXTRA(400))
def test_random_window_batches(ctx, seed):
    """mh_icp_linearize_batch over random windows — 1..9 factors, ragged sizes from empty to several thousand points, unary or
    binary, components on for a random subset — is bit-identical to the same factors linearized one call at a time, cold
    and over a re-linearization walk."""
    from mimosa_amd import capi

    m, pts, cfg, mode, R, t, rng = _case(seed)
    leaf, md = cfg["target_ivox_map_leaf_size"], cfg["target_ivox_map_min_dist_in_voxel"]
    gm = capi.VoxelMap(ctx, leaf=leaf, min_dist=md, mode=mode)
    gm.insert(m)
    binary = bool(rng.integers(0, 2))
    nf = int(rng.integers(1, 10))
    rc = capi.make_reg_config(**cfg)
    fa, fb, on = [], [], []
    for i in range(nf):
        n = int(rng.choice([0, 1, 63, 64, 65, 300, len(pts) // 2, len(pts)]))
        sub = np.ascontiguousarray(pts[rng.permutation(len(pts))[:n]])
        fa.append(capi.ICPFactor(ctx, gm, sub, rc, binary=binary))
        fb.append(capi.ICPFactor(ctx, gm, sub, rc, binary=binary))
        on.append(bool(rng.integers(0, 2)))
        fa[-1].set_components(on[-1])
        fb[-1].set_components(on[-1])
    keys = ("H_ss", "b_s", "f", "loc_trans_final", "loc_rot_final", "eigvec_rot", "eigvec_trans", "degen_rot", "degen_trans", "n_knn",
            "mean_candidates", "linearize_count", "H_st", "H_tt", "b_t", "loc_trans_comp", "loc_rot_comp", "status_hist")
    thr = md / 4.0
    Rt, tt = R @ synth.so3_exp(rng.normal(0, 0.01, 3)), t + rng.normal(0, 0.05, 3)
    for step in range(3):
        Rs = [R @ synth.so3_exp(rng.normal(0, 1.0, 3) * thr / 5.0) for _ in range(nf)]
        ts = [t + rng.normal(0, 1.0, 3) * thr * rng.choice([0.3, 1.0, 3.0]) for _ in range(nf)]
        kw = dict(R_tgts=[Rt] * nf, t_tgts=[tt] * nf) if binary else {}
        got = capi.linearize_batch(fa, Rs, ts, **kw)
        for i in range(nf):
            one = fb[i].linearize(Rs[i], ts[i], R_tgt=Rt, t_tgt=tt) if binary else fb[i].linearize(Rs[i], ts[i])
            # K3's launch class: a window of more than 8 factors goes through the staged launch form, which runs one lane per
            # point; a small k = 5 cloud on its own runs several (icp_kernels.hip, "Launchers").  Then the per-point results are
            # still identical (the state below) and the sums differ in the order their rows are added.
            same_class = cfg["num_corres_points"] != 5 or (nf <= 8 and sum(f.n for f in fa) <= 32768) or nf == 1
            for k in keys:
                a_, b_ = np.asarray(got[i][k], float), np.asarray(one[k], float)
                if same_class or k in ("n_knn", "mean_candidates", "linearize_count", "status_hist"):
                    assert np.array_equal(a_, b_, equal_nan=True), (step, i, k)
                elif k in ("degen_rot", "degen_trans"):
                    continue  # the Schur degeneracy info, inverses of possibly singular blocks: compared under parity.py's condition only
                elif k in ("eigvec_rot", "eigvec_trans", "loc_trans_final", "loc_rot_final"):
                    continue  # functions of H's last digits: each result is held to the reference of its own blocks below
                else:
                    assert np.allclose(a_, b_, rtol=1e-11, atol=1e-11 * max(np.abs(b_).max() if b_.size else 0.0, 1e-300), equal_nan=True), (step, i, k)
            if not same_class:
                # loc_*_final and eigvec_* of both results against the multi-precision decomposition of the blocks each one reports
                # (tests/degeneracy_zoo.py).  A unary reg_4_dof factor reports the PROJECTED rotation block, not the one that was
                # decomposed: there the translation block alone.  (A result the degeneracy projection zeroed reports zero blocks
                # and the localizabilities of the zero matrix.)
                blocks = ("trans",) if cfg["reg_4_dof"] and not binary else ("rot", "trans")
                for tag, res in (("batch", got[i]), ("single", one)):
                    check_result(res, f"seed {seed} step {step} factor {i} {tag}", blocks=blocks)
            for x, y in zip(fa[i].state(), fb[i].state()):
                assert np.array_equal(x, y, equal_nan=True)
    for f in fa + fb:
        f.destroy()
    gm.release()


@pytest.mark.parametrize("seed", [0, 1, 2] + _EXTRA(500))
def test_random_large_clouds(ctx, seed):
    """The 512-thread / multi-XCD regime (clouds of 66 k - 131 k points against rooms sampled with 0.1 - 1.5 M points): random
    room, density, sensor pose, pose error and registration options; cold + one partial re-association."""
    from mimosa_amd import capi
    from oracle import ref_cpu

    rng = np.random.default_rng(64000 + seed)
    room = np.array([rng.uniform(15, 40), rng.uniform(12, 25), rng.uniform(3, 6)])
    grid = float(rng.choice([0.05, 0.08, 0.12]))
    m = synth.make_room(8000 + seed, 0, 0, grid=grid, room=room)
    loc = np.array([rng.uniform(2, room[0] - 2), rng.uniform(2, room[1] - 2), rng.uniform(0.8, room[2] - 0.8)])
    pts, aux = synth.make_scan(n_rows=128, seed=9000 + seed, n_cols=int(rng.choice([520, 777, 1024])), room=room, sensor_local=loc)
    cfg = synth.enwide_config()
    cfg.update(use_huber=int(rng.integers(0, 2)), reg_4_dof=int(rng.integers(0, 2)), num_corres_points=int(rng.choice([5, 5, 8])),
               max_corres_distance=float(rng.choice([0.5, 1.0])))
    mode = int(rng.choice([7, 19, 27]))
    gm, rm = capi.VoxelMap(ctx, mode=mode), ref_cpu.Map(mode=mode)
    for chunk in np.array_split(m, 3):
        gm.insert(chunk)
        rm.insert(chunk)
    assert gm.stats()["n_points"] == rm.num_points
    R = aux["R_W_L"] @ synth.so3_exp(np.deg2rad(rng.normal(0, 0.5, 3)))
    t = aux["t_W_L"] + aux["R_W_L"] @ rng.normal(0, 0.04, 3)
    gf = capi.ICPFactor(ctx, gm, pts, capi.make_reg_config(**cfg))
    rf = ref_cpu.ICP(rm, pts, ref_cpu.make_config(**cfg))
    assert len(pts) > 65536
    for step in range(2):
        got, ref = gf.linearize(R, t), rf.linearize(R, t)
        assert_result_parity(got, ref, check_eigvec=False)
        assert_state_parity(gf.state(), rf.state())
        R, t = R @ synth.so3_exp(np.array([0.0, 0.0, 1.5e-3])), t + rng.normal(0, 0.02, 3)
    gf.destroy()
    gm.release()



def test_non_finite_and_far_inputs_do_not_fault(ctx, small_world):
    """NaN / Inf / absurdly far source points and poses: the reference computes NaNs and moves on; the device path must neither
    fault nor hang, must keep every finite point's result intact, and must report the bad points as rejected."""
    from mimosa_amd import capi

    w = small_world
    gm = capi.VoxelMap(ctx)
    gm.insert(w["map_xyz"])
    pts = w["pts"].copy()
    n = len(pts)
    bad = np.arange(0, n, 97)
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, 1e-30]
    for j, i in enumerate(bad):
        pts["xyz"[j % 3]][i] = np.float32(vals[j % len(vals)])
    rc = capi.make_reg_config(**w["cfg"])
    gf, clean = capi.ICPFactor(ctx, gm, pts, rc), capi.ICPFactor(ctx, gm, np.delete(w["pts"], bad), rc)
    g, c = gf.linearize(w["R"], w["t"]), clean.linearize(w["R"], w["t"])
    st = gf.state()[0]
    finite = np.isfinite(pts["x"]) & np.isfinite(pts["y"]) & np.isfinite(pts["z"]) & (np.abs(pts["x"]) < 1e6) & (np.abs(pts["y"]) < 1e6) & (np.abs(pts["z"]) < 1e6)
    assert np.all(st[~finite] != 8)
    assert np.array_equal(np.delete(st, bad), clean.state()[0])
    # (a coordinate replaced by 1e-30 leaves a finite point that may well register: it counts, and contributes to H)
    extra = st[bad] == 8
    assert g["status_hist"][8] == c["status_hist"][8] + int(extra.sum())
    assert np.all(np.isfinite(g["H_ss"]))
    if not extra.any():
        assert np.allclose(g["H_ss"], c["H_ss"], rtol=1e-12, atol=0)
    # a NaN pose: everything is rejected or NaN, nothing faults, and the factor is usable afterwards
    Rn = w["R"].copy()
    Rn[0, 0] = np.nan
    gf.linearize(Rn, w["t"])
    gf.reset()
    g2 = gf.linearize(w["R"], w["t"])
    assert np.array_equal(g2["H_ss"], g["H_ss"])
    # k-NN queries far outside the map / non-finite
    q = np.array([[1e30, 0, 0], [np.nan, 0, 0], [np.inf, -np.inf, 0], [3e9, 3e9, 3e9], [0.1, 0.2, 0.3]])
    _, _, found = gm.knn(q, 5)
    assert list(found[:4]) == [0, 0, 0, 0]
    for f in (gf, clean):
        f.destroy()
    gm.release()


@pytest.mark.parametrize("seed", list(range(6)) + _EXTRA(600))
def test_random_map_generations_with_live_factors(ctx, seed):
    """Geometric::updateMap's pattern under random schedules: copy -> insert -> occasional LRU purge, while factors
    built on EARLIER generations stay alive, are re-linearized, cloned and destroyed in random order, and old generations are
    released as soon as the caller lets go of them.  Every factor must keep seeing exactly the generation it was built on
    (the oracle does the same steps with deep copies)."""
    from mimosa_amd import capi
    from oracle import ref_cpu

    m, pts, cfg, mode, R, t, rng = _case(seed)
    leaf, md = cfg["target_ivox_map_leaf_size"], cfg["target_ivox_map_min_dist_in_voxel"]
    horizon = int(rng.choice([2, 4, 1000]))
    gm = capi.VoxelMap(ctx, leaf=leaf, min_dist=md, mode=mode, lru_horizon=horizon, lru_clear_cycle=2)
    rm = ref_cpu.Map(leaf=leaf, min_dist=md, mode=mode, lru_horizon=horizon)
    rm.set_lru_clear_cycle(2)
    chunks = np.array_split(m[rng.permutation(len(m))], 8)
    gm.insert(chunks[0]), rm.insert(chunks[0])
    rc, rrc = capi.make_reg_config(**cfg), ref_cpu.make_config(**cfg)
    live = []            # (hip factor, oracle factor)
    thr = md / 4.0
    for gen in range(1, 8):
        op = rng.integers(0, 3)
        if op == 0:      # a factor on the current generation
            sub = np.ascontiguousarray(pts[rng.permutation(len(pts))[: int(rng.choice([64, 500, len(pts)]))]])
            live.append((capi.ICPFactor(ctx, gm, sub, rc), ref_cpu.ICP(rm, sub, rrc)))
        # the next generation: copy, then insert — the old handle is released right away (factors keep it alive)
        rng.integers(0, 2)  # (the draw the fork / copy choice of ABI version 1 made: keeps the schedules what they were)
        new_g = gm.copy()
        new_r = rm.copy()
        gm.release()
        gm, rm = new_g, new_r
        gm.insert(chunks[gen]), rm.insert(chunks[gen])
        assert gm.stats()["n_points"] == rm.num_points
        # every live factor, at a moved pose: sees its own generation
        for gf, rf in live:
            Rk = R @ synth.so3_exp(rng.normal(0, 1.0, 3) * thr / 5.0)
            tk = t + rng.normal(0, 1.0, 3) * thr * rng.choice([0.3, 3.0])
            assert_result_parity(gf.linearize(Rk, tk), rf.linearize(Rk, tk), check_eigvec=False)
        if live and rng.integers(0, 2):          # drop one, clone another
            gf, rf = live.pop(int(rng.integers(0, len(live))))
            gf.destroy()
        if live and rng.integers(0, 3) == 0:
            gf, rf = live[int(rng.integers(0, len(live)))]
            c = gf.clone()
            gf.destroy()
            live[[i for i, p in enumerate(live) if p[0] is gf][0]] = (c, rf)
    assert np.array_equal(gm.get_cloud(), rm.export()[2])
    for gf, _ in live:
        gf.destroy()
    gm.release()


def test_host_threads_with_their_own_contexts_share_a_map(ctx, small_world):
    """Four host threads, each with its own context (stream), factor and scratch, linearize against ONE map concurrently —
    synchronous calls, pipelined calls, factor creation / destruction in the loop.  Every result must be the bits a single
    thread produces (the library's shared state: allocation cache, pinned rings, error slots)."""
    import threading
    from mimosa_amd import capi

    w = small_world
    gm = capi.VoxelMap(ctx)
    gm.insert(w["map_xyz"])
    rc = capi.make_reg_config(**w["cfg"])
    subs = [np.ascontiguousarray(w["pts"][i::4]) for i in range(4)]
    want = []
    for i in range(4):
        f = capi.ICPFactor(ctx, gm, subs[i], rc)
        want.append((f.linearize(w["R"], w["t"]), f.linearize(w["R"], w["t"] + np.array([0.002, 0.0, 0.001]))))
        f.destroy()
    errors = []

    def worker(i):
        try:
            c = capi.Context(0)
            for rep in range(40 + len(_EXTRA(0))):
                f = capi.ICPFactor(c, gm, subs[i], rc)
                a = f.linearize(w["R"], w["t"])
                outs = [f.linearize_async(w["R"], w["t"] + np.array([0.002, 0.0, 0.001])) for _ in range(2)]
                f.wait()
                for k in ("H_ss", "b_s", "f", "status_hist", "loc_trans_comp"):
                    assert np.array_equal(a[k], want[i][0][k]), (i, rep, k)
                    assert np.array_equal(outs[0].as_dict()[k], want[i][1][k]), (i, rep, k)
                f.destroy()
            c.destroy() if hasattr(c, "destroy") else None
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not any(x.is_alive() for x in th), "a worker hung"
    assert not errors, errors[:3]
    gm.release()
