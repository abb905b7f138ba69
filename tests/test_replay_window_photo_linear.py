"""Sequence replay with the device window loop carrying the photometric factor as a linear factor
(ReplayConfig.window_photo_linear / replay::Config::window_photo_linear): opt-in, only offered with device_window; with it
device_window accepts the photometric factor — before each window call the host linearizes it once at the call's initial poses
(photo_window: every live one, through the batch call) and mh_icp_window_optimise_lin carries the result along.

10 scans of 64 x 512, photometric on, in the Python and in the native replay, with and without photo_window.  The host-loop
replay of the same configuration, computed in the same test, is the reference: it evaluates the photometric factor again in
every iteration, the new path freezes its linearization for the call, so the trajectories differ; the replay is chaotic at the
level of association-gate flips, so the bound is ten times the deviation measured on an MI355X (MEASURED below: max |dt| in m,
max |dR| on the rotation entries), the margin tests/test_replay_window_relin.py takes for the same kind of difference.  The
error against the synthetic ground truth must stay within 1.5 times the host-loop run's own (measured: 5.558 mm and 0.0435
degrees against the host loop's 5.554 mm and 0.0435 degrees; with photo_window 5.561 against 5.557 mm)."""
import dataclasses

import numpy as np
import pytest

from mimosa_amd import replay


def photo_cfg(n=10, **kw):
    return replay.ReplayConfig(n_scans=n, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2, keyframe_rot_thresh_deg=5.0,
                               photometric=True, **kw)


# (replay, photo_window) -> max |dt| (m), max |dR| against the host loop over the 10 scans, on an MI355X
MEASURED = {
    ("python", False): (4.303e-5, 1.027e-5),
    ("python", True): (8.000e-5, 1.120e-5),
    ("native", False): (4.303e-5, 1.027e-5),
    ("native", True): (8.000e-5, 1.120e-5),
}


def test_switch_is_opt_in_and_needs_device_window(tmp_path):
    assert not replay.ReplayConfig().window_photo_linear

    class NoDevice:
        pass

    with pytest.raises(ValueError, match="window_photo_linear"):
        replay.run(photo_cfg(2, window_photo_linear=True), NoDevice(), scans=[])
    with pytest.raises(RuntimeError, match="window_photo_linear"):
        replay.run_native(photo_cfg(2, window_photo_linear=True), [], str(tmp_path))
    # without the switch the refusal of the photometric factor stays
    with pytest.raises(ValueError, match="photometric"):
        replay.run(photo_cfg(2, device_window=True), NoDevice(), scans=[])


def deviation(a, b):
    assert len(a["poses_est"]) == len(b["poses_est"]) and a["n_keyframes"] == b["n_keyframes"]
    dt = max(float(np.max(np.abs(ta - tb))) for (_, ta), (_, tb) in zip(a["poses_est"], b["poses_est"]))
    dR = max(float(np.max(np.abs(Ra - Rb))) for (Ra, _), (Rb, _) in zip(a["poses_est"], b["poses_est"]))
    return dt, dR


def truth_error(r, scans):
    te = max(float(np.linalg.norm(t - s["t_gt"])) for (_, t), s in zip(r["poses_est"], scans))
    re = max(float(np.degrees(np.arccos(np.clip((np.trace(R.T @ s["R_gt"]) - 1.0) / 2.0, -1.0, 1.0)))) for (R, _), s in zip(r["poses_est"], scans))
    return te, re


def check(which, photo_window, on, ref, scans):
    dt, dR = deviation(on, ref)
    (te, re), (te0, re0) = truth_error(on, scans), truth_error(ref, scans)
    print(f"{which} photo_window={photo_window}: window_photo_linear vs the host loop: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}; "
          f"error against the truth {te:.3e} m {re:.3e} deg (host loop {te0:.3e} m {re0:.3e} deg)")
    m_dt, m_dR = MEASURED[(which, photo_window)]
    assert dt <= 10.0 * m_dt and dR <= 10.0 * m_dR
    assert te <= 1.5 * te0 and re <= 1.5 * re0


@pytest.mark.gpu
@pytest.mark.parametrize("photo_window", [False, True])
def test_python_replay_with_window_photo_linear(ctx, photo_window):
    cfg = photo_cfg(photo_window=photo_window)
    scans = replay.make_scans(cfg)
    ref = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    on_cfg = dataclasses.replace(cfg, device_window=True, window_photo_linear=True)
    on = replay.run(on_cfg, replay.HipBackend(ctx, on_cfg), scans)  # (raises without the switch: device_window refuses the photometric factor)
    assert [len(c) for c in on["costs"]] == [cfg.update_iters] * cfg.n_scans
    assert any(v > 0 for v in ref["photo_valid"])  # the photometric factor took part
    check("python", photo_window, on, ref, scans)


@pytest.mark.gpu
@pytest.mark.parametrize("photo_window", [False, True])
def test_native_replay_with_window_photo_linear(tmp_path, photo_window):
    cfg = photo_cfg(photo_window=photo_window)
    scans = replay.make_scans(cfg)
    ref = replay.run_native(cfg, scans, str(tmp_path))
    on_cfg = dataclasses.replace(cfg, device_window=True, window_photo_linear=True)
    on = replay.run_native(on_cfg, scans, str(tmp_path))
    check("native", photo_window, on, ref, scans)
    if not photo_window:
        with pytest.raises(RuntimeError, match="device_window"):  # lidar::Manager and the sharded replay keep refusing
            replay.run_native(on_cfg, scans[:2], str(tmp_path), through_manager=True)
        with pytest.raises(RuntimeError, match="device_window"):
            replay.run_native(on_cfg, scans[:2], str(tmp_path), sharded_world=1)
