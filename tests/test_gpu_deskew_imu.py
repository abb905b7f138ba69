"""-m gpu: mh_scan_deskew_imu — Manager::deskewPoints with its per-timestamp pose part (src/lidar/manager.cpp:455-499) on the
device — through the C ABI: the pose table against oracle/numpy_ref.py: deskew_poses, the deskewed cloud against the existing
mh_scan_deskew (bit for bit) and against numpy_ref.deskew, the error paths, and the photometric frame built from the resident
table against the one built from an uploaded table."""
import numpy as np
import pytest

import deskew_imu_cases as dc

pytestmark = pytest.mark.gpu

CASES = {"imu100hz_147ts": (dc.small_case, 64), "per_point_24000ts_40seg": (dc.per_point_case, 1)}


def _scan(ctx, raw, keep_raw=False):
    from mimosa_amd import capi
    sc = capi.Scan(ctx)
    if keep_raw:
        ctx.check(ctx.L.mh_scan_keep_raw(sc.h, 1))
    info = sc.prepare_input(raw, capi.make_input_config(range_min=0.0, range_max=1000.0))
    assert info["n_full"] == len(raw)
    return sc


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    make, per_ts = CASES[request.param]
    c = make()
    return c, dc.raw_cloud(c["unique_ns"], per_ts), dc.oracle_poses(c)


def test_poses_match_the_oracle(ctx, case):
    """mh_scan_get_deskew_poses vs numpy_ref.deskew_poses: rotation entries < 1e-12, translation < 1e-11 (the bounds
    tests/test_deskew_poses.py holds the host mirror to)."""
    c, raw, want = case
    sc = _scan(ctx, raw)
    assert np.array_equal(sc.unique_ns(), c["unique_ns"])
    sc.deskew_imu(*dc.call_args(c))
    got = sc.deskew_poses()
    assert got.shape == want.shape
    dR, dt = np.abs(got[:, :9] - want[:, :9]).max(), np.abs(got[:, 9:] - want[:, 9:]).max()
    print(f"max |dR| = {dR:.3e}, max |dt| = {dt:.3e} over {len(got)} timestamps")
    assert dR < 1e-12 and dt < 1e-11
    sc.destroy()


def test_cloud_is_bit_identical_to_mh_scan_deskew_with_the_downloaded_table(ctx, case):
    c, raw, _ = case
    a, b = _scan(ctx, raw), _scan(ctx, raw)
    a.deskew_imu(*dc.call_args(c))
    T = a.deskew_poses()
    b.deskew(T.astype(np.float32))                      # toFloat12
    pa, pb = a.points(0), b.points(0)
    assert pa.tobytes() == pb.tobytes()
    assert not np.array_equal(pa["x"], raw["x"])        # and it did move the points
    a.destroy()
    b.destroy()


def test_cloud_matches_the_oracle_end_to_end(ctx, case):
    """numpy_ref.deskew with the ORACLE's poses: every coordinate within one f32 ulp of its own magnitude, at most 1 % of the
    points not bit-identical."""
    from oracle import numpy_ref
    c, raw, want = case
    sc = _scan(ctx, raw)
    before = sc.points(0)
    sc.deskew_imu(*dc.call_args(c))
    got = sc.points(0)
    xyz = np.stack([before["x"], before["y"], before["z"]], 1)
    ref = numpy_ref.deskew(xyz, before["t"], c["unique_ns"], want.astype(np.float32))
    g = np.stack([got["x"], got["y"], got["z"]], 1)
    ulp = np.spacing(np.abs(ref).astype(np.float32))
    differ = np.any(g != ref, axis=1)
    print(f"{int(differ.sum())} of {len(g)} points differ, max |d| / ulp = {float((np.abs(g - ref) / ulp).max()):.2f}")
    assert np.all(np.abs(g - ref) <= ulp)
    assert differ.mean() <= 0.01
    sc.destroy()


def test_no_segments_is_the_first_cloud_identity_and_untouched(ctx):
    c = dc.small_case()
    raw = dc.raw_cloud(c["unique_ns"], 16)
    sc = _scan(ctx, raw)
    before = sc.points(0)
    seg, header_ts, g, T_Le_W, T_B_S = dc.call_args(c)
    sc.deskew_imu(seg[:0], header_ts, g, T_Le_W, T_B_S)
    T = sc.deskew_poses()
    assert T.shape == (len(c["unique_ns"]), 12) and np.array_equal(T, np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (len(T), 1)))
    assert sc.points(0).tobytes() == before.tobytes()
    sc.destroy()


def test_imu_buffer_that_ends_too_early_is_reported_at_the_next_wait(ctx):
    from mimosa_amd import capi
    c = dc.small_case()
    raw = dc.raw_cloud(c["unique_ns"], 16)
    want = dc.oracle_poses(c)
    sc = _scan(ctx, raw)
    before = sc.points(0)
    sc.deskew_imu(*dc.call_args(c, n_samples=6))         # the enqueueing call itself cannot know
    for call in (lambda: sc.points(0), sc.deskew_poses, lambda: sc.preprocess_geometric(np.eye(3), np.zeros(3))):
        with pytest.raises(capi.MhError) as e:
            call()
        assert e.value.code == capi.MH_ERR_INVALID_ARG and "IMU samples end before the last point of the cloud" in str(e.value)
    # nothing was moved with a made-up pose
    out = np.zeros(len(before), before.dtype)
    n = capi.C.c_size_t()
    assert ctx.L.mh_scan_get_points(sc.h, 0, out.ctypes.data_as(capi.C.c_void_p), len(out), capi.C.byref(n)) == capi.MH_ERR_INVALID_ARG
    assert out.tobytes() == before.tobytes()
    # the object works again after the next prepare_input
    sc.prepare_input(raw, capi.make_input_config(range_min=0.0, range_max=1000.0))
    sc.deskew_imu(*dc.call_args(c))
    got = sc.deskew_poses()
    assert np.abs(got[:, :9] - want[:, :9]).max() < 1e-12 and np.abs(got[:, 9:] - want[:, 9:]).max() < 1e-11
    sc.preprocess_geometric(np.eye(3), np.zeros(3))
    sc.destroy()


def test_argument_checks_on_a_real_scan(ctx):
    from mimosa_amd import capi, synth_photo
    C = capi.C
    c = dc.small_case()
    seg, header_ts, g, T_Le_W, T_B_S = dc.call_args(c)
    sc = capi.Scan(ctx)
    with pytest.raises(capi.MhError) as e:               # never prepared
        sc.deskew_imu(seg, header_ts, g, T_Le_W, T_B_S)
    assert e.value.code == capi.MH_ERR_INVALID_ARG and "no mh_scan_prepare_input before" in str(e.value)
    sc.prepare_input(dc.raw_cloud(c["unique_ns"], 4), capi.make_input_config(range_min=0.0, range_max=1000.0))
    with pytest.raises(capi.MhError) as e:
        sc.deskew_imu(np.zeros(65, capi.IMU_SEGMENT_DTYPE), header_ts, g, T_Le_W, T_B_S)
    assert e.value.code == capi.MH_ERR_UNSUPPORTED
    n = C.c_size_t()
    assert ctx.L.mh_scan_get_deskew_poses(sc.h, None, 0, C.byref(n)) == capi.MH_ERR_INVALID_ARG   # no mh_scan_deskew_imu on this cloud
    ph = capi.Photo(ctx, synth_photo.photo_config())
    ctx.check(ctx.L.mh_scan_keep_raw(sc.h, 1))
    sc.prepare_input(dc.raw_cloud(c["unique_ns"], 4), capi.make_input_config(range_min=0.0, range_max=1000.0))
    sc.deskew(dc.oracle_poses(c).astype(np.float32))     # deskewed, but not by mh_scan_deskew_imu
    for fn in (ctx.L.mh_photo_preprocess_scan_resident, ctx.L.mh_photo_preprocess_scan_begin_resident):
        assert fn(ph.h, sc.h) == capi.MH_ERR_INVALID_ARG
    ph.destroy()
    sc.destroy()


# ---- the photometric frame from the resident table -----------------------------------------------------------------------

def _photo_scan(ctx, cfg, f):
    """the 128 x 1024 scene of tests/test_gpu_photo.py as a resident scan (raw kept), not yet deskewed"""
    from mimosa_amd import synth
    raw = np.zeros(len(f["raw"]), dtype=synth.OUSTER_DTYPE)
    for k in ("x", "y", "z", "intensity", "t"):
        raw[k] = f["raw"][k]
    full = np.zeros(cfg["rows"] * cfg["cols"], dtype=synth.OUSTER_DTYPE)
    full["x"] = np.nan
    full[f["raw"]["idx"]] = raw
    full["ring"] = (np.arange(len(full)) // cfg["cols"]).astype(np.uint16)
    from mimosa_amd import capi
    sc = capi.Scan(ctx)
    ctx.check(ctx.L.mh_scan_keep_raw(sc.h, 1))
    sc.prepare_input(full, capi.make_input_config(range_min=0.0, range_max=1000.0))
    return sc


def _twist_imu(f, v=(1.2, 0.2, 0.0), w=(0.0, 0.0, 0.35), header_ts=77.0, n_imu=12):
    """IMU samples at 100 Hz and the states at their times for the constant body twist synth_photo.make_frame moves the sensor
    with (body = sensor): deskew_imu's poses then come out close to the frame's own table."""
    from mimosa_amd import synth
    v, w = np.asarray(v, float), np.asarray(w, float)
    g = np.array([0.0, 0.0, -9.81])
    imu_t = header_ts - 0.003 + np.arange(n_imu) * 0.01
    t_end = header_ts + float(f["unique_ns"][-1]) * 1e-9
    nav_R, nav_p, nav_v, acc = [], [], [], []
    for t in imu_t:
        d = t - t_end
        R = f["R_W_L"] @ synth.so3_exp(w * d)
        nav_R.append(R)
        nav_p.append(f["t_W_L"] + f["R_W_L"] @ (v * d))          # first order, as make_frame's t_rel = -v dt
        nav_v.append(f["R_W_L"] @ v)
        acc.append(R.T @ (-g))                                    # no world acceleration: the accelerometer reads -g in the body
    gyro = np.tile(w, (n_imu, 1))
    # scan end = the state handed over as T_W_Be: make it the last entry the way Manager has propagated_state_ in hand
    nav_R.append(f["R_W_L"]); nav_p.append(f["t_W_L"]); nav_v.append(f["R_W_L"] @ v)
    return dict(imu_t=imu_t, acc=np.array(acc), gyro=gyro, nav_R=nav_R, nav_p=nav_p, nav_v=nav_v, bias_a=np.zeros(3), bias_g=np.zeros(3),
                g_unit=np.array([0.0, 0.0, -1.0]), g_norm=9.81, header_ts=header_ts, T_B_S=(np.eye(3), np.zeros(3)))


@pytest.fixture(scope="module")
def frame():
    from mimosa_amd import synth_photo as sp
    cfg = sp.photo_config()
    return cfg, sp.make_frame(cfg, 1)


def _deskew_imu_frame(sc, f):
    from mimosa_amd import capi
    c = _twist_imu(f)
    m = len(c["imu_t"])
    seg = capi.imu_segments(c["imu_t"], c["acc"], c["gyro"], c["nav_R"][:m], c["nav_p"][:m], c["nav_v"][:m])
    T_Le_W = np.linalg.inv(dc.hom(c["nav_R"][-1], c["nav_p"][-1]))
    sc.deskew_imu(seg, c["header_ts"], c["g_unit"] * c["g_norm"], (T_Le_W[:3, :3], T_Le_W[:3, 3]), c["T_B_S"])


IMAGES = ("intensity", "range", "dx", "dy", "mask", "idx", "yaw", "proj_idx", "grad", "detection_mask")


def test_photometric_frame_from_the_resident_table(ctx, frame):
    """mh_photo_preprocess_scan_resident vs mh_photo_preprocess_scan fed the downloaded table: every image of mh_photo_get_image and
    the corrected cloud, bit for bit; the same for _begin_resident + _commit."""
    from mimosa_amd import capi
    cfg, f = frame
    a, b, c = (_photo_scan(ctx, cfg, f) for _ in range(3))
    for sc in (a, b, c):
        _deskew_imu_frame(sc, f)
    T = a.deskew_poses()
    assert np.abs(T - f["T_Le_Lt"][np.searchsorted(f["unique_ns"], a.unique_ns())]).max() < 1e-3   # the IMU describes the frame's motion
    pa, pb, pc = capi.Photo(ctx, cfg), capi.Photo(ctx, cfg), capi.Photo(ctx, cfg)
    pa.preprocess_scan(a, T)
    pb.preprocess_scan_resident(b)
    pc.preprocess_scan_begin_resident(c)
    pc.preprocess_commit()
    for name in IMAGES:
        want = pa.image(name)
        assert np.array_equal(want, pb.image(name)), name
        assert np.array_equal(want, pc.image(name)), name
    assert pa.image("mask").mean() > 0.5
    assert a.points(0).tobytes() == b.points(0).tobytes() == c.points(0).tobytes()
    for o in (pa, pb, pc, a, b, c):
        o.destroy()


def test_resident_photometric_calls_report_an_imu_buffer_that_ends_too_early(ctx, frame):
    from mimosa_amd import capi
    cfg, f = frame
    c = _twist_imu(f)
    seg = capi.imu_segments(c["imu_t"][:5], c["acc"][:5], c["gyro"][:5], c["nav_R"][:5], c["nav_p"][:5], c["nav_v"][:5])
    T_Le_W = np.linalg.inv(dc.hom(c["nav_R"][-1], c["nav_p"][-1]))
    ph = capi.Photo(ctx, cfg)
    for begin in (False, True):
        sc = _photo_scan(ctx, cfg, f)
        sc.deskew_imu(seg, c["header_ts"], c["g_unit"] * c["g_norm"], (T_Le_W[:3, :3], T_Le_W[:3, 3]), c["T_B_S"])
        with pytest.raises(capi.MhError) as e:
            if begin:
                ph.preprocess_scan_begin_resident(sc)
                ph.preprocess_commit()
            else:
                ph.preprocess_scan_resident(sc)
        assert e.value.code == capi.MH_ERR_INVALID_ARG and "IMU samples end before the last point of the cloud" in str(e.value)
        with pytest.raises(capi.MhError) as e:           # neither form made the failed frame current
            ph.image("mask")
        assert "no frame" in str(e.value)
        sc.destroy()
    ph.destroy()


# ---- the replays with the option on ----------------------------------------------------------------------------------------

def _same_run(on, off):
    """device_poses on against off: poses within 1e-9 m / 1e-9 (the bar tests/test_replay.py holds sharded against unsharded runs
    to), same keyframe decisions, same tracked-feature counts."""
    assert len(on["poses_est"]) == len(off["poses_est"])
    dt = max(float(np.max(np.abs(ta - tb))) for (_, ta), (_, tb) in zip(on["poses_est"], off["poses_est"]))
    dR = max(float(np.max(np.abs(Ra - Rb))) for (Ra, _), (Rb, _) in zip(on["poses_est"], off["poses_est"]))
    print(f"device_poses on vs off: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}; photo_valid on {on['photo_valid']} off {off['photo_valid']}")
    assert dt <= 1e-9 and dR <= 1e-9
    assert on["n_keyframes"] == off["n_keyframes"]
    assert on["photo_valid"] == off["photo_valid"]


def test_native_replay_with_device_poses(tmp_path):
    """20 scans of the full-size sequence of tests/test_replay.py, pipelined and sequential forms."""
    import dataclasses
    from mimosa_amd import replay
    cfg = replay.ReplayConfig(n_scans=20, rows=128)
    scans = replay.make_scans(cfg)
    cfg_on = dataclasses.replace(cfg, device_poses=True)
    off = replay.run_native(cfg, scans, str(tmp_path))
    assert off["n_keyframes"] >= 2 and min(off["photo_valid"]) >= 20
    assert off["device_pose_scans"] == 0
    for sequential in (False, True):
        on = replay.run_native(cfg_on, scans, str(tmp_path), sequential=sequential)
        assert on["device_pose_scans"] == 20
        _same_run(on, off)


def test_python_replay_with_device_poses(ctx):
    import dataclasses
    from mimosa_amd import replay
    cfg = replay.ReplayConfig(n_scans=5, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2)
    scans = replay.make_scans(cfg)
    off = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    on = replay.run(dataclasses.replace(cfg, device_poses=True), replay.HipBackend(ctx, cfg), scans)
    _same_run(on, off)


def _small_replay_cfg(n, **kw):
    from mimosa_amd import replay
    return replay.ReplayConfig(n_scans=n, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2, keyframe_rot_thresh_deg=5.0, **kw)


def test_sharded_replay_with_device_poses(tmp_path):
    """The sharded replay shares the loop: 2 ranks in one process, photometric path replicated, option on against off."""
    import dataclasses
    from mimosa_amd import replay
    cfg = _small_replay_cfg(6)
    scans = replay.make_scans(cfg)
    off = replay.run_native(cfg, scans, str(tmp_path), sharded_world=2)
    on = replay.run_native(dataclasses.replace(cfg, device_poses=True), scans, str(tmp_path), sharded_world=2)
    assert on["n_ranks"] == 2 and on["max_rank_deviation_m"] <= 1e-9 and len(off["photo_valid"]) >= 4
    assert (on["device_pose_scans"], off["device_pose_scans"]) == (6, 0)
    _same_run(on, off)


def test_manager_mirror_with_device_poses(tmp_path):
    """lidar::Manager::setDevicePoses through the native replay's `manager` form (every scan through Manager::callback): the first
    cloud is not deskewed either way, every later one takes its poses from the device; option on against off."""
    import dataclasses
    from mimosa_amd import replay
    cfg = _small_replay_cfg(7, prior_trans_noise=0.0, prior_rot_noise_deg=0.0)
    scans = replay.make_scans(cfg)
    off = replay.run_native(cfg, scans, str(tmp_path), through_manager=True)
    on = replay.run_native(dataclasses.replace(cfg, device_poses=True), scans, str(tmp_path), through_manager=True)
    assert len(off["poses_est"]) == 7 and off["n_keyframes"] >= 2 and len(off["photo_valid"]) >= 5
    assert (on["device_pose_scans"], off["device_pose_scans"]) == (6, 0)    # every cloud but the first (manager.cpp:399-408)
    _same_run(on, off)

