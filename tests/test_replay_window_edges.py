"""Sequence replay with an external odometry source (ReplayConfig.odometry_every / replay::Config::odometry_every): at every
second scan the synthetic source reports the true pose with noise from a fixed seed; the message goes through the odometry
manager's rules and becomes a between factor on the window poses of scans k - 2 and k, beside the IMU ties, dropped once its
older pose has left the window.  10 scans of 64 x 512 without the photometric factor, sizes of tests/test_replay.py.

With device_window the edges go to mh_icp_window_optimise_edges; the trajectory must match the host loop's, which adds the same
terms to its dense system, to 1e-9 m (1e-9 on the rotation entries) — the bar of tests/test_replay_device_window.py, since both
sides compute the same iteration — in the Python and in the native replay.  Native against Python as tests/test_replay.py holds
them (1e-7 m, 1e-8 on the rotation entries: the two differ in the order of the host-side operations).  The odometry moves the
trajectory by more than 1e-6 m.  Off by default, the native input file and command line are then what they were; refused
through lidar::Manager's replay and the sharded replay, as device_window is."""
import dataclasses

import numpy as np
import pytest

from mimosa_amd import replay

SIGMAS = dict(odometry_sigma_rot_deg=0.06, odometry_sigma_trans_m=0.005)  # the source's own noise (1e-3 rad, 5e-3 m)


def small_cfg(n=10, **kw):
    return replay.ReplayConfig(n_scans=n, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2,
                               keyframe_rot_thresh_deg=5.0, photometric=False, **kw)


def odo_cfg(n=10, **kw):
    return small_cfg(n, odometry_every=2, **SIGMAS, **kw)


def deviation(a, b):
    dt = max(float(np.max(np.abs(ta - tb))) for (_, ta), (_, tb) in zip(a["poses_est"], b["poses_est"]))
    dR = max(float(np.max(np.abs(Ra - Rb))) for (Ra, _), (Rb, _) in zip(a["poses_est"], b["poses_est"]))
    return dt, dR


def test_switch_is_off_by_default_and_the_input_file_is_then_unchanged(tmp_path):
    cfg = small_cfg(2)
    assert cfg.odometry_every == 0 and replay.odometry_messages(cfg, [None] * 4) == []
    scans = replay.make_scans(cfg)
    replay.write_native_input(str(tmp_path / "off.bin"), cfg, scans)
    replay.write_native_input(str(tmp_path / "on.bin"), odo_cfg(2), scans)
    off, on = (tmp_path / "off.bin").read_bytes(), (tmp_path / "on.bin").read_bytes()
    assert on.startswith(off) and len(on) > len(off)  # a trailing section, nothing else
    assert [m[0] for m in replay.odometry_messages(odo_cfg(2), scans)] == [0]


def test_python_manager_rules():
    """the gate, the NaN pass-through, the first-message rule and the sigmas of the Python mirror of odometry::Manager"""
    m = replay.OdometryManager(0.5, 0.25)
    I, z = np.eye(3), np.zeros(3)
    assert m.callback(0, I, z, np.eye(6) * 1.5) is None and m.prev is None      # rejected: does not initialise
    assert m.callback(1, I, z, np.eye(6) * 0.5) is None and m.prev[0] == 1        # the first accepted message only initialises
    assert m.callback(2, I, z, np.eye(6) * 1.5) is None and m.prev[0] == 1        # rejected: the previous pose does not advance
    neg = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -2.0])                                # NaN > thresh is false: passes
    pk, Z, info = m.callback(3, I, np.array([1.0, 0.0, 0.0]), neg)
    sr = 0.5 * np.pi / 180.0
    assert pk == 1 and np.array_equal(Z[1], [1.0, 0.0, 0.0]) and np.array_equal(info, np.diag([1.0 / (sr * sr)] * 3 + [16.0] * 3))


@pytest.mark.gpu
def test_python_replay_with_odometry_edges(ctx):
    cfg = odo_cfg()
    scans = replay.make_scans(cfg)
    off = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    on_cfg = dataclasses.replace(cfg, device_window=True)
    on = replay.run(on_cfg, replay.HipBackend(ctx, on_cfg), scans)
    dt, dR = deviation(on, off)
    print(f"python: odometry edges, device_window on vs off: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}")
    assert on["n_keyframes"] == off["n_keyframes"]
    assert dt <= 1e-9 and dR <= 1e-9
    assert np.allclose(np.concatenate(on["costs"]), np.concatenate(off["costs"]), rtol=1e-6)
    plain_cfg = small_cfg()
    plain = replay.run(plain_cfg, replay.HipBackend(ctx, plain_cfg), scans)
    moved = deviation(off, plain)[0]
    print(f"python: the odometry moves the trajectory by {moved:.3e} m")
    assert moved > 1e-6
    assert max(on["trans_err"]) < 0.012 and max(on["rot_err_deg"]) < 0.06


@pytest.mark.gpu
def test_native_replay_with_odometry_edges(ctx, tmp_path):
    cfg = odo_cfg()
    scans = replay.make_scans(cfg)
    on_cfg = dataclasses.replace(cfg, device_window=True)
    off = replay.run_native(cfg, scans, str(tmp_path))
    on = replay.run_native(on_cfg, scans, str(tmp_path))
    dt, dR = deviation(on, off)
    print(f"native: odometry edges, device_window on vs off: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}")
    assert on["n_keyframes"] == off["n_keyframes"]
    assert dt <= 1e-9 and dR <= 1e-9
    assert np.allclose(on["first_costs"], off["first_costs"], rtol=1e-6)
    # native against Python, host loop against host loop and device chain against device chain
    for native, c in ((off, cfg), (on, on_cfg)):
        py = replay.run(c, replay.HipBackend(ctx, c), scans)
        dt, dR = deviation(native, py)
        print(f"native vs python (device_window={c.device_window}): max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}")
        assert native["n_keyframes"] == py["n_keyframes"]
        assert dt < 1e-7 and dR < 1e-8
    plain = replay.run_native(small_cfg(), scans, str(tmp_path))
    moved = deviation(off, plain)[0]
    print(f"native: the odometry moves the trajectory by {moved:.3e} m")
    assert moved > 1e-6
    for kw in (dict(through_manager=True), dict(sharded_world=1)):
        with pytest.raises(RuntimeError, match="odometry_every"):
            replay.run_native(cfg, scans[:2], str(tmp_path), **kw)
        with pytest.raises(RuntimeError, match="device_window|odometry_every"):
            replay.run_native(on_cfg, scans[:2], str(tmp_path), **kw)
