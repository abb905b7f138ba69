"""Sequence replay with the device window loop and relinearization thresholds (ReplayConfig.window_relin /
replay::Config::window_relin): the pair is opt-in, only offered with device_window, and (0, 0) leaves the device_window
trajectory exactly as it is, in the Python and in the native replay.  With the reference's thresholds (1.75e-2 rad, 5e-3 m) fewer
factors are evaluated per iteration and the trajectory moves a little; the replay is chaotic at the level of association-gate
flips, so the bound is ten times the deviation measured on an MI355X against the device_window trajectory over the 10 scans
below: max |dt| = 3.092e-4 m and max |dR| = 9.450e-5 on the rotation entries, the same figures in the Python and in the native
replay (trajectory errors against the truth then: 5.5 mm, 0.047 degrees)."""
import dataclasses

import numpy as np
import pytest

from mimosa_amd import replay
from test_replay_device_window import small_cfg

RELIN = (1.75e-2, 5.0e-3)
MEASURED_DT, MEASURED_DR = 3.092e-4, 9.450e-5  # max |dt| (m), max |dR| over the trajectory, on an MI355X


def test_pair_is_opt_in_and_needs_device_window(tmp_path):
    assert replay.ReplayConfig().window_relin is None

    class NoDevice:
        pass

    with pytest.raises(ValueError, match="window_relin"):
        replay.run(small_cfg(2, window_relin=RELIN), NoDevice(), scans=[])
    with pytest.raises(RuntimeError, match="window_relin"):
        replay.run_native(small_cfg(2, window_relin=RELIN), [], str(tmp_path))


def deviation(a, b):
    assert len(a["poses_est"]) == len(b["poses_est"]) and a["n_keyframes"] == b["n_keyframes"]
    dt = max(float(np.max(np.abs(ta - tb))) for (_, ta), (_, tb) in zip(a["poses_est"], b["poses_est"]))
    dR = max(float(np.max(np.abs(Ra - Rb))) for (Ra, _), (Rb, _) in zip(a["poses_est"], b["poses_est"]))
    return dt, dR


@pytest.mark.gpu
def test_python_replay_with_window_relin(ctx):
    cfg = small_cfg(device_window=True)
    scans = replay.make_scans(cfg)
    ref = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    zero_cfg = dataclasses.replace(cfg, window_relin=(0.0, 0.0))
    zero = replay.run(zero_cfg, replay.HipBackend(ctx, zero_cfg), scans)
    assert deviation(zero, ref) == (0.0, 0.0)
    assert np.array_equal(np.concatenate(zero["costs"]), np.concatenate(ref["costs"]))
    on_cfg = dataclasses.replace(cfg, window_relin=RELIN)
    on = replay.run(on_cfg, replay.HipBackend(ctx, on_cfg), scans)
    dt, dR = deviation(on, ref)
    print(f"python: window_relin {RELIN} vs device_window: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}")
    assert dt <= 10.0 * MEASURED_DT and dR <= 10.0 * MEASURED_DR
    assert max(on["trans_err"]) < 0.012 and max(on["rot_err_deg"]) < 0.06  # the bars of the device_window replay


@pytest.mark.gpu
def test_native_replay_with_window_relin(tmp_path):
    cfg = small_cfg(device_window=True)
    scans = replay.make_scans(cfg)
    ref = replay.run_native(cfg, scans, str(tmp_path))
    zero = replay.run_native(dataclasses.replace(cfg, window_relin=(0.0, 0.0)), scans, str(tmp_path))
    assert deviation(zero, ref) == (0.0, 0.0)
    on = replay.run_native(dataclasses.replace(cfg, window_relin=RELIN), scans, str(tmp_path))
    dt, dR = deviation(on, ref)
    print(f"native: window_relin {RELIN} vs device_window: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}")
    assert dt <= 10.0 * MEASURED_DT and dR <= 10.0 * MEASURED_DR
