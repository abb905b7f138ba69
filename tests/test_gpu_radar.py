"""-m gpu: the radar Doppler path (mh_radar_*) against the independent restatement in tests/radar_ref.py, its bit-identity
guarantees (batch / async / repeats / device-resident targets / clone), physics sanity on a synthetic scene, and the C++ host
mirror (mimosa_amd/host/mimosa_hip/radar.hpp) through the library."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import radar_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BLOCKS = ("G11", "G12", "G13", "G22", "G23", "G33", "g1", "g2", "g3")


def _cfg_struct(cfg):
    from mimosa_amd import capi
    return capi.make_radar_config(**cfg)


def _factor(ctx, targets, st, sigma=0.1):
    from mimosa_amd import capi
    return capi.RadarFactor(ctx, targets, st["R_B_S"], st["t_B_S"], st["omega"], sigma)


def _lin(f, st):
    return f.linearize(st["R_W_B"], st["v_W"], st["bias_gyro"])


def _same_bits(a, b):
    for k in BLOCKS + ("f",):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k  # (+0.0 and -0.0 differ here)
    assert a["n_targets"] == b["n_targets"]


@pytest.mark.parametrize("kind", ["mmwave", "rio"])
def test_front_end_matches_restatement(ctx, kind):
    from mimosa_amd import capi, synth_radar
    sc = synth_radar.make_scene(n_static=3000, n_dynamic=100, seed=11 if kind == "rio" else 12)
    raw, lay = synth_radar.pack(sc["points"], kind)
    n = len(sc["labels"])
    scan = capi.RadarScan(ctx)
    info = scan.prepare_input(raw, synth_radar.capi_layout(lay), _cfg_struct(sc["cfg"]))
    got = scan.targets()
    x, y, z, i, v = radar_ref.decode(raw, n, kind, lay["point_step"], lay)
    idx, ref = radar_ref.preprocess(x, y, z, i, v, sc["cfg"])
    assert info == {"n_points_in": n, "n_points_valid": len(idx)}
    assert np.array_equal(idx, np.nonzero(sc["labels"] != 2)[0])  # every gate dropped exactly the points built for it
    g = got.view(np.float64).reshape(-1, 8)
    assert g.shape == ref.shape
    for c in (0, 1, 2, 3, 6, 7):  # x, y, z, range, radial_speed, intensity: bit-exact
        assert g[:, c].tobytes() == ref[:, c].tobytes(), radar_ref.TARGET_FIELDS[c]
    for c in (4, 5):  # azimuth, elevation: within one float ulp
        mag = np.maximum(np.abs(ref[:, c]), np.abs(g[:, c])).astype(np.float32)
        ulp = np.spacing(mag).astype(np.float64)
        assert np.all(np.abs(g[:, c] - ref[:, c]) <= ulp), radar_ref.TARGET_FIELDS[c]
    # the Doppler-residual point type is recognised and refused, as Manager::callback does
    lay_r = dict(lay, kind="doppler_residual")
    with pytest.raises(capi.MhError) as e:
        scan.prepare_input(raw, synth_radar.capi_layout(lay_r), _cfg_struct(sc["cfg"]))
    assert e.value.code == capi.MH_ERR_UNSUPPORTED
    scan.destroy()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4096, 100000])
def test_factor_parity(ctx, n):
    from mimosa_amd import synth_radar
    rng = np.random.default_rng(100 + n)
    st = synth_radar.random_state(rng)
    tg = synth_radar.random_targets(rng, n)
    sigma = float(np.float32(0.1))  # the manager passes its float config value
    f = _factor(ctx, tg, st, sigma)
    got = _lin(f, st)
    ref = radar_ref.linearize(tg, st["R_B_S"], st["t_B_S"], st["omega"], sigma, st["R_W_B"], st["v_W"], st["bias_gyro"])
    assert got["n_targets"] == n
    for k in BLOCKS:
        nr = np.linalg.norm(ref[k])
        assert np.linalg.norm(got[k] - ref[k]) <= 1e-12 * nr, (k, n)
    assert abs(got["f"] - ref["f"]) <= 1e-12 * abs(ref["f"])
    # structural zeros (translation columns of X, accelerometer columns of B) are exactly 0.0; diagonal blocks exactly symmetric
    zeros = [got["G11"][3:, :], got["G11"][:, 3:], got["G12"][3:, :], got["G13"][3:, :], got["G13"][:, :3], got["G23"][:, :3],
             got["G33"][:3, :], got["G33"][:, :3], got["g1"][3:], got["g3"][:3]]
    assert all(not z.any() for z in zeros)
    for k in ("G11", "G22", "G33"):
        assert np.array_equal(got[k], got[k].T)
    if n == 0:
        assert got["f"] == 0.0 and not any(got[k].any() for k in BLOCKS)
    else:
        e, w = f.residuals()
        assert np.max(np.abs(e - ref["e_whitened"])) <= 1e-13 * max(1.0, np.max(np.abs(ref["e_whitened"])))
        assert np.max(np.abs(w - ref["weight"])) <= 1e-13
    f.destroy()


def test_batch_async_repeat_scan_and_clone_are_bit_identical(ctx):
    from mimosa_amd import capi, synth_radar
    rng = np.random.default_rng(5)
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 3000] + list(rng.integers(0, 1500, 245))
    facs, states = [], []
    for n in sizes:
        st = synth_radar.random_state(rng)
        facs.append(_factor(ctx, synth_radar.random_targets(rng, int(n)), st))
        states.append(st)
    single = [_lin(f, st) for f, st in zip(facs, states)]
    for m in (1, 7, 64, 256):  # windows of 1 ... 256 factors of mixed sizes, zeros included
        batch = capi.radar_linearize_batch(facs[:m], [s["R_W_B"] for s in states[:m]], [s["v_W"] for s in states[:m]],
                                           [s["bias_gyro"] for s in states[:m]])
        for a, b in zip(batch, single[:m]):
            _same_bits(a, b)
    for f, st, ref in list(zip(facs, states, single))[:20]:  # async / wait == sync; three repeats give the same bits
        f.linearize_async(st["R_W_B"], st["v_W"], st["bias_gyro"])
        _same_bits(f.wait(), ref)
        for _ in range(3):
            _same_bits(_lin(f, st), ref)
    # over the limit, or factors of two contexts: MH_ERR_INVALID_ARG
    st = states[3]
    k = capi.MH_RADAR_MAX_BATCH + 1
    with pytest.raises(capi.MhError) as e:
        capi.radar_linearize_batch([facs[3]] * k, [st["R_W_B"]] * k, [st["v_W"]] * k, [st["bias_gyro"]] * k)
    assert e.value.code == capi.MH_ERR_INVALID_ARG
    ctx2 = capi.Context(0)
    other = _factor(ctx2, synth_radar.random_targets(rng, 10), st)
    with pytest.raises(capi.MhError) as e:
        capi.radar_linearize_batch([facs[3], other], [st["R_W_B"]] * 2, [st["v_W"]] * 2, [st["bias_gyro"]] * 2)
    assert e.value.code == capi.MH_ERR_INVALID_ARG
    other.destroy()
    ctx2.close()
    for f in facs:
        f.destroy()

    # create_from_scan == create from the host targets mh_radar_get_targets returns
    sc = synth_radar.make_scene(n_static=2000, n_dynamic=50, seed=3)
    raw, lay = synth_radar.pack(sc["points"], "rio")
    scan = capi.RadarScan(ctx)
    scan.prepare_input(raw, synth_radar.capi_layout(lay), _cfg_struct(sc["cfg"]))
    st = sc["state"]
    f_dev = _factor(ctx, scan, st)
    f_host = _factor(ctx, scan.targets(), st)
    scan.destroy()  # the factor owns its targets
    r_dev = _lin(f_dev, st)
    _same_bits(r_dev, _lin(f_host, st))
    # a clone is independent of its source
    c = f_dev.clone()
    f_dev.destroy()
    _same_bits(_lin(c, st), r_dev)
    c.destroy()
    f_host.destroy()


def test_physics_sanity_on_a_synthetic_scene(ctx):
    from mimosa_amd import capi, synth_radar
    sc = synth_radar.make_scene(n_static=2000, n_dynamic=10, seed=21, doppler_noise=0.02)
    raw, lay = synth_radar.pack(sc["points"], "mmwave")
    scan = capi.RadarScan(ctx)
    scan.prepare_input(raw, synth_radar.capi_layout(lay), _cfg_struct(sc["cfg"]))
    lab = sc["labels"][sc["labels"] != 2]  # kept targets in input order
    st, sigma = sc["state"], sc["cfg"]["noise_sigma"]
    f = _factor(ctx, scan, st, sigma)
    _lin(f, st)
    e, w = f.residuals()
    es = e[lab == 0] * sigma  # static targets at the true state: Doppler noise level (0.02 m/s)
    assert abs(es.mean()) < 0.005 and 0.015 < es.std() < 0.025
    assert np.all(np.abs(e[lab == 1]) * sigma > 0.9)  # the moving targets stand out
    # one Gauss-Newton step on the V block from a velocity 0.5 m/s off recovers v_W
    rng = np.random.default_rng(4)
    d = rng.normal(size=3)
    v0 = st["v_W"] + 0.5 * d / np.linalg.norm(d)
    r = f.linearize(st["R_W_B"], v0, st["bias_gyro"])
    v1 = v0 + np.linalg.solve(r["G22"], r["g2"])
    assert np.linalg.norm(v1 - st["v_W"]) < 1e-2
    f.destroy()
    scan.destroy()


def _build_pipeline(tmp_path):
    from mimosa_amd import build
    # the library the session already loaded (build() would recompile it where the object files are absent)
    lib = build.LIB if os.path.exists(build.LIB) else build.build()
    exe = str(tmp_path / "radar_pipeline")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I",
                           os.path.join(ROOT, "mimosa_amd", "host", "gtsam_sig"), os.path.join(ROOT, "tests", "cpp", "radar_pipeline.cpp"),
                           "-o", exe, "-L", os.path.dirname(lib), "-lmimosa_hip", "-lpthread", f"-Wl,-rpath,{os.path.dirname(lib)}"])
    return exe


def test_host_mirror_matches_the_binding(ctx, tmp_path):
    from mimosa_amd import capi, synth_radar
    sc = synth_radar.make_scene(n_static=800, n_dynamic=20, seed=8)
    raw, lay = synth_radar.pack(sc["points"], "rio")
    st, cfg = sc["state"], sc["cfg"]
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as fh:
        def w(arr):
            arr = np.ascontiguousarray(arr)
            fh.write(struct.pack("<Q", arr.size))
            fh.write(arr.tobytes())
        w(raw.astype(np.uint8))
        w(np.array([capi.MH_RADAR_RIO, lay["point_step"], lay["x"], lay["y"], lay["z"], lay["intensity"], lay["velocity"]], np.int32))
        w(np.array([cfg[k] for k in ("range_min", "range_max", "threshold_azimuth_deg", "threshold_elevation_deg", "filter_min_db",
                                     "noise_sigma")], np.float32))
        w(np.concatenate([st["R_B_S"].ravel(), st["t_B_S"]]).astype(np.float64))
        w(np.asarray(st["omega"], np.float64))
        w(np.concatenate([st["R_W_B"].ravel(), [1.0, 2.0, 3.0], st["v_W"], st["bias_gyro"]]).astype(np.float64))
    out = subprocess.run([_build_pipeline(tmp_path), str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)
    # the same input through the Python binding
    scan = capi.RadarScan(ctx)
    info = scan.prepare_input(raw, synth_radar.capi_layout(lay), _cfg_struct(cfg))
    f = _factor(ctx, scan, st, float(np.float32(cfg["noise_sigma"])))
    r = _lin(f, st)
    G = np.block([[r["G11"], r["G12"], r["G13"]], [r["G12"].T, r["G22"], r["G23"]], [r["G13"].T, r["G23"].T, r["G33"]]])
    g = np.concatenate([r["g1"], r["g2"], r["g3"]])
    assert res["n_points_in"] == info["n_points_in"] and res["n_points_valid"] == info["n_points_valid"] == res["n_targets"]
    assert res["dim"] == 15 and res["corrected_ts"] == 100.0
    assert (res["X0"], res["V0"], res["B0"]) == (ord("x") << 56, ord("v") << 56, ord("b") << 56)
    for name in ("from_scan", "from_targets", "clone", "batch0"):
        h = res[name]
        assert h["keys"] == [res["X0"], res["V0"], res["B0"]]
        assert np.array(h["information"]).reshape(15, 15).tobytes() == G.tobytes(), name
        assert np.array(h["linear"]).tobytes() == g.tobytes(), name
        assert h["f"] == r["f"], name
    f.destroy()
    scan.destroy()
