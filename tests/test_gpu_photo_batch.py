"""-m gpu: the photometric window batch (mh_photo_factor_linearize_batch[_async]) — a window of PhotometricFactors on
different frames linearized in one launch gives, factor by factor, the bits of its own mh_photo_factor_linearize, and
matches the CPU oracle (oracle/photo_ref.hpp) as a single call does."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from parity import rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES = 6
FIELDS = ("H_bb", "H_ba", "H_aa", "b_b", "b_a", "f", "loc_trans_final", "loc_rot_final", "eigvec_trans", "eigvec_rot",
          "status_hist", "n_exceptions")


def _both(ctx, cfg):
    from mimosa_amd import capi
    from oracle import photo_ref

    return capi.Photo(ctx, cfg), photo_ref.Photo(cfg)


def _pre(P, f):
    return P.preprocess(f["raw"], f["deskewed"], f["unique_ns"], f["T_Le_Lt"])


def _vsvt():
    from mimosa_amd import synth

    V = synth.so3_exp(np.array([0.3, -0.2, 0.5]))
    V6 = np.block([[V, np.zeros((3, 3))], [np.zeros((3, 3)), V.T]])
    return V6 @ np.diag([1.0, 0, 1, 0, 1, 1]) @ V6.T


@pytest.fixture(scope="module")
def frames():
    from mimosa_amd import synth_photo as sp

    cfg = sp.photo_config()
    return cfg, [sp.make_frame(cfg, k) for k in range(N_FRAMES)]


class Window:
    """One factor per frame, each on its own frame, built while the features are tracked through update_map — on the
    product (g) and the oracle (r) in lockstep.  Kinds: plain, V S V^T, binary, a subset of the tracked features, and one
    linearized far from its pose (no feature survives)."""

    def __init__(self, ctx, cfg, fr):
        from mimosa_amd import synth_photo as sp

        self.g, self.r = _both(ctx, cfg)
        for P in (self.g, self.r):
            _pre(P, fr[0])
            P.update_map(None, fr[0]["R_W_Be"], fr[0]["t_W_Be"], sp.BIAS_DIRECTIONS)
        self.gf, self.rf, self.binary, self.poses, self.far = [], [], [], [], []
        kinds = ["plain", "vsvt", "binary", "subset", "vsvt"]
        for k in range(1, N_FRAMES):
            f = fr[k]
            for P in (self.g, self.r):
                _pre(P, f)
            kind = kinds[(k - 1) % len(kinds)]
            for P, out in ((self.g, self.gf), (self.r, self.rf)):
                if kind == "subset":
                    full = P.features()
                    P.set_features(full[: len(full) // 2 + 3])
                    out.append(P.make_factor())
                    P.set_features(full)
                else:
                    out.append(P.make_factor(_vsvt() if kind == "vsvt" else None, binary=kind == "binary"))
            self.binary.append(kind == "binary")
            self.poses.append((f["R_W_Be"], f["t_W_Be"]))
            self.far.append(False)
            # tracking: a plain factor of this frame drives update_map on both sides
            tg, tr = self.g.make_factor(), self.r.make_factor()
            tg.linearize(f["R_W_Be"], f["t_W_Be"]), tr.linearize(f["R_W_Be"], f["t_W_Be"])
            self.g.update_map(tg, f["R_W_Be"], f["t_W_Be"], sp.BIAS_DIRECTIONS)
            self.r.update_map(tr, f["R_W_Be"], f["t_W_Be"], sp.BIAS_DIRECTIONS)
            tg.destroy()
        # a clone of the first factor, 40 m away from its frame: every feature fails to project (the oracle's counterpart
        # is the first factor itself, read back right after each of its linearizes)
        self.gf.append(self.gf[0].clone())
        self.rf.append(self.rf[0])
        self.binary.append(False)
        self.poses.append((fr[1]["R_W_Be"], fr[1]["t_W_Be"] + np.array([40.0, 0.0, 0.0])))
        self.far.append(True)

    def pose_arrays(self, poses):
        n = len(poses)
        Rb = np.stack([p[0] for p in poses])
        tb = np.stack([p[1] for p in poses])
        # binary factors: T_a = identity, the frame the features were tracked in (world)
        Ra = np.tile(np.eye(3), (n, 1, 1))
        ta = np.zeros((n, 3))
        return Rb, tb, Ra, ta

    def perturbed(self, s):
        from mimosa_amd import synth

        out = []
        for i, (R, t) in enumerate(self.poses):
            w = s * np.array([0.001 * (i + 1), -0.0015, 0.002])
            out.append((R @ synth.so3_exp(w), t + s * np.array([0.01, -0.005 * i, 0.004])))
        return out

    def single(self, fs, poses, Ra, ta):
        res, st = [], []
        for i, f in enumerate(fs):
            res.append(f.linearize(poses[i][0], poses[i][1], Ra[i] if self.binary[i] else None, ta[i] if self.binary[i] else None))
            st.append(f.state(rows=True))
        return res, st

    def destroy(self):
        for f in self.gf:
            f.destroy()
        self.g.destroy()


@pytest.fixture(scope="module")
def window(ctx, frames):
    cfg, fr = frames
    w = Window(ctx, cfg, fr)
    yield w
    w.destroy()


def _assert_same(a, b, sa=None, sb=None):
    for k in FIELDS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    if sa is not None:
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)


def test_window_shape(window):
    """the window really is what the bit-identity test claims: different frames, feature counts and kinds"""
    assert len(window.gf) >= 5 and any(window.binary)
    counts = [f.n for f in window.gf]
    assert len(set(counts)) >= 2, counts
    Rb, tb, Ra, ta = window.pose_arrays(window.poses)
    res, _ = window.single(window.gf, window.poses, Ra, ta)
    valid = [r["status_hist"][8] for r in res]
    assert all(v >= 10 for v, far in zip(valid, window.far) if not far), valid
    assert valid[-1] == 0 and window.far[-1]


def test_batch_is_bit_identical_to_single_calls(window):
    from mimosa_amd import capi

    for s in (0.0, 1.0):  # the window's poses, then a second (warm) set
        poses = window.poses if s == 0.0 else window.perturbed(s)
        Rb, tb, Ra, ta = window.pose_arrays(poses)
        ref, ref_st = window.single(window.gf, poses, Ra, ta)
        got = capi.photo_linearize_batch(window.gf, Rb, tb, Ra, ta)
        assert len(got) == len(ref)
        for i, f in enumerate(window.gf):
            _assert_same(got[i], ref[i], f.state(rows=True), ref_st[i])
        # async: enqueue once, collect in reverse order
        capi.photo_linearize_batch_async(window.gf, Rb, tb, Ra, ta)
        for i in reversed(range(len(window.gf))):
            _assert_same(window.gf[i].wait(), ref[i], window.gf[i].state(rows=True), ref_st[i])


def test_batch_matches_the_oracle(window):
    from mimosa_amd import capi

    poses = window.perturbed(0.5)
    Rb, tb, Ra, ta = window.pose_arrays(poses)
    got = capi.photo_linearize_batch(window.gf, Rb, tb, Ra, ta)
    tol = 1e-5
    for i, (gf, rf) in enumerate(zip(window.gf, window.rf)):
        rr = rf.linearize(Rb[i], tb[i], Ra[i] if window.binary[i] else None, ta[i] if window.binary[i] else None)
        gr = got[i]
        assert np.array_equal(gr["status_hist"], rr["status_hist"]), i
        assert gr["n_exceptions"] == rr["n_exceptions"]
        gs, rs = gf.state(rows=True), rf.state()
        assert np.array_equal(gs[0], rs[0])
        v = gs[0] == 8
        if window.far[i]:
            assert not v.any()
            continue
        assert np.abs(gs[1][v] - rs[1][v]).max() <= 1e-8
        assert rel(gr["H_bb"], rr["H_bb"]) <= tol and rel(gr["b_b"], rr["b_b"]) <= tol
        assert abs(gr["f"] - rr["f"]) <= tol * abs(rr["f"])
        if window.binary[i]:
            assert rel(gr["H_ba"], rr["H_ba"]) <= tol and rel(gr["H_aa"], rr["H_aa"]) <= tol and rel(gr["b_a"], rr["b_a"]) <= tol
        ga, ra = gs[2][v], rs[2][v]
        assert np.array_equal(ga[:, :, 7], ra[:, :, 7])
        assert rel(ga[:, :, 0], ra[:, :, 0]) <= tol and rel(ga[:, :, 1:7], ra[:, :, 1:7]) <= tol


def test_one_factor_and_the_largest_batch(window):
    from mimosa_amd import capi

    f = window.gf[1]
    R, t = window.poses[1]
    one = capi.photo_linearize_batch([f], R[None], t[None])[0]
    ref = f.linearize(R, t)
    _assert_same(one, ref)
    L = f.L
    assert capi.photo_linearize_batch([f], R[None], t[None])  # repeatable
    limit = 256
    clones = [f.clone() for _ in range(limit)]
    try:
        got = capi.photo_linearize_batch(clones, np.tile(R, (limit, 1, 1)), np.tile(t, (limit, 1)))
        st = f.state(rows=True)
        for c, g in zip(clones, got):
            _assert_same(g, ref, c.state(rows=True), st)
        over = clones + [f]
        hs = (C.c_void_p * len(over))(*[x.h for x in over])
        Rs = np.ascontiguousarray(np.tile(R, (len(over), 1, 1)))
        ts = np.ascontiguousarray(np.tile(t, (len(over), 1)))
        out = (capi.PhotoResult * len(over))()
        assert L.mh_photo_factor_linearize_batch(hs, len(over), Rs.ctypes.data, ts.ctypes.data, None, None, out) == capi.MH_ERR_INVALID_ARG
    finally:
        for c in clones:
            c.destroy()


def test_8x8_patches(ctx):
    from mimosa_amd import capi, synth, synth_photo as sp

    cfg = sp.photo_config(patch=8)
    fr = [sp.make_frame(cfg, k) for k in range(3)]
    g = capi.Photo(ctx, cfg)
    _pre(g, fr[0])
    g.detect(60, fr[0]["R_W_Be"], fr[0]["t_W_Be"], sp.BIAS_DIRECTIONS)
    _pre(g, fr[1])
    a = g.make_factor()
    t0 = a.linearize(fr[1]["R_W_Be"], fr[1]["t_W_Be"])
    g.update_map(a, fr[1]["R_W_Be"], fr[1]["t_W_Be"], sp.BIAS_DIRECTIONS)
    _pre(g, fr[2])
    b = g.make_factor(binary=True)
    assert all(len(x["Le_ps"]) == 64 for x in g.features()) and t0["status_hist"][8] >= 10
    poses = [(fr[1]["R_W_Be"] @ synth.so3_exp(np.array([0.002, 0.001, -0.001])), fr[1]["t_W_Be"] + np.array([0.01, 0.02, -0.01])),
             (fr[2]["R_W_Be"], fr[2]["t_W_Be"])]
    Ra, ta = np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3))
    ref = [a.linearize(*poses[0]), b.linearize(*poses[1], Ra[1], ta[1])]
    st = [a.state(rows=True), b.state(rows=True)]
    got = capi.photo_linearize_batch([a, b], np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses]), Ra, ta)
    for x, y, s, f in zip(got, ref, st, (a, b)):
        _assert_same(x, y, f.state(rows=True), s)
    for f in (a, b):
        f.destroy()
    g.destroy()


def test_rejections_leave_nothing_in_flight(ctx, window, frames):
    from mimosa_amd import capi

    cfg, fr = frames
    fs = window.gf[:3]
    Rb, tb, Ra, ta = window.pose_arrays(window.poses[:3])
    L = fs[0].L
    INV = capi.MH_ERR_INVALID_ARG

    def raw(handles, n, R=Rb, t=tb, R_a=Ra, t_a=ta):
        hs = (C.c_void_p * max(len(handles), 1))(*handles)
        keep = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (R, t, R_a, t_a)]
        out = (capi.PhotoResult * max(n, 1))()
        return L.mh_photo_factor_linearize_batch(hs, n, *[None if a is None else a.ctypes.data for a in keep], out)

    def plain_calls_work():
        for i, f in enumerate(fs):
            r = f.linearize(Rb[i], tb[i], Ra[i] if window.binary[i] else None, ta[i] if window.binary[i] else None)
            assert r["status_hist"].sum() == f.n

    hs = [f.h for f in fs]
    assert raw(hs, 0) == INV
    plain_calls_work()
    assert raw([None, hs[1], hs[2]], 3) == INV
    plain_calls_work()
    assert raw(hs, 3, R=None) == INV
    plain_calls_work()
    assert L.mh_photo_factor_linearize_batch(None, 3, Rb.ctypes.data, tb.ctypes.data, None, None, (capi.PhotoResult * 3)()) == INV
    plain_calls_work()
    assert raw([hs[0], hs[1], hs[0]], 3) == INV                       # the same factor twice
    plain_calls_work()
    assert window.binary[2]
    assert raw(hs, 3, R_a=None, t_a=None) == INV                      # a binary factor without T_a
    plain_calls_work()
    other = capi.Photo(ctx, cfg)                                      # a factor of another mh_photo
    _pre(other, fr[1])
    other.detect(20, fr[1]["R_W_Be"], fr[1]["t_W_Be"], np.eye(3))
    of = other.make_factor()
    assert raw([hs[0], hs[1], of.h], 3) == INV
    plain_calls_work()
    with pytest.raises(capi.MhError):
        capi.photo_linearize_batch([fs[0], of], Rb[:2], tb[:2])
    fs[1].linearize_async(Rb[1], tb[1])                               # a factor with a call in flight
    assert raw(hs, 3) == INV
    fs[1].wait()
    plain_calls_work()
    assert capi.photo_linearize_batch(fs, Rb, tb, Ra, ta)             # and the batch itself still works
    of.destroy()
    other.destroy()


def test_destroying_a_member_of_an_async_batch(window):
    from mimosa_amd import capi

    src = window.gf[:4]
    fs = [f.clone() for f in src]
    Rb, tb, Ra, ta = window.pose_arrays(window.poses[:4])
    ref, ref_st = window.single(fs, window.poses[:4], Ra, ta)
    capi.photo_linearize_batch_async(fs, Rb, tb, Ra, ta)
    fs[1].destroy()                                                   # waits for the launch
    for i in (3, 0, 2):
        _assert_same(fs[i].wait(), ref[i], fs[i].state(rows=True), ref_st[i])
    for i in (0, 2, 3):
        fs[i].destroy()


def _pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()])


def _write_mirror_input(path, cfg, frames):
    """the input format of tests/cpp/photo_pipeline.cpp (binio::read_photo_config, bias directions, then per frame)"""
    from mimosa_amd import synth_photo as sp

    with open(path, "wb") as f:
        def w(arr, dtype=None):
            arr = np.ascontiguousarray(arr if dtype is None else np.asarray(arr, dtype))
            f.write(struct.pack("<Q", len(arr) if arr.dtype.itemsize == 32 else arr.size))
            f.write(arr.tobytes())
        w([cfg["rows"], cfg["cols"], cfg["destagger"], cfg["erosion_buffer"], cfg["patch_size"], cfg["margin_size"], cfg["remove_lines"],
           cfg["filter_brightness"], cfg["gaussian_blur"], cfg["gaussian_blur_size"], cfg["nma_radius"], cfg["num_features_detect"],
           cfg["max_feature_life_time"], cfg["rotate_patch_to_align_with_gradient"], cfg["use_robust_cost_function"],
           cfg["robust_cost_function"], cfg["brightness_window_size"][0], cfg["brightness_window_size"][1]], np.int32)
        w([cfg["range_min"], cfg["range_max"], cfg["intensity_scale"], cfg["intensity_gamma"], cfg["gradient_threshold"],
           cfg["max_dist_from_mean"], cfg["max_dist_from_plane"], cfg["occlusion_range_diff_threshold"],
           cfg["lidar_origin_to_beam_origin_mm"], cfg["robust_cost_function_parameter"], cfg["error_scale"], cfg["max_error"],
           cfg["sigma"]], np.float64)
        w(cfg["pixel_shift_by_row"], np.int32)
        w(cfg["beam_altitude_angles"], np.float32)
        w(cfg["high_pass_fir"], np.float64)
        w(cfg["low_pass_fir"], np.float64)
        w(np.asarray(cfg["patch_offsets"], np.int32).ravel())
        w(_pose12(cfg["T_B_L_R"], cfg["T_B_L_t"]))
        w(np.asarray(sp.BIAS_DIRECTIONS, np.float64).ravel())
        for fr in frames:
            w(fr["raw"])
            w(fr["deskewed"])
            w(fr["unique_ns"].astype(np.uint32))
            w(np.asarray(fr["T_Le_Lt"], np.float64).ravel())
            w(_pose12(fr["R_W_Be"], fr["t_W_Be"]))


def test_host_mirror_batch_equals_a_loop_of_linearize(tmp_path):
    """PhotometricFactor::linearizeBatch / linearizeBatchAsync of the C++ mirror == linearize() per factor, bit for bit"""
    from mimosa_amd import build, synth_photo as sp

    cfg = sp.photo_config(rows=64, cols=512)
    n = 4
    frames = [sp.make_frame(cfg, k) for k in range(n)]
    inp = tmp_path / "photo.bin"
    _write_mirror_input(inp, cfg, frames)
    lib = build.build()
    exe = str(tmp_path / "photo_batch")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I",
                           os.path.join(ROOT, "mimosa_amd", "host", "gtsam_sig"), os.path.join(ROOT, "tests", "cpp", "photo_batch.cpp"),
                           "-o", exe, "-L", os.path.dirname(lib), "-lmimosa_hip", "-lpthread", f"-Wl,-rpath,{os.path.dirname(lib)}"])
    out = subprocess.run([exe, str(inp), str(n)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    assert got["n_factors"] == n - 1 and got["n_valid"] >= 20
    assert got["equal"] == 1 and got["async_equal"] == 1
