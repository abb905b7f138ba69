"""Sequence replay with the marginal prior of the pose that leaves the window (ReplayConfig.window_marginal /
replay::Config::window_marginal, the native driver's `+marginal`): opt-in, only offered with device_window, refused with
odometry_every > 1.  Off, the trajectory, the costs and the native input file are those of device_window.  On, no window call
is singular (the replay raises on one), every marginal is valid, the Python and the native replay agree as tests/test_replay.py
holds them (1e-7 m, 1e-8 on the rotation entries), and the mean translation error against the synthetic truth stays within
twice that of the pinned replay run beside it — a guard against a gross error, not an accuracy claim: a real marginal is looser
than a 1e-4 pin on a synthetic trajectory whose oldest pose is already good to millimetres."""
import dataclasses
import filecmp

import numpy as np
import pytest

from mimosa_amd import replay
from test_replay_device_window import small_cfg
from test_replay_window_relin import deviation


def test_switch_is_opt_in_and_refused_where_it_is_not_offered(tmp_path):
    assert not replay.ReplayConfig().window_marginal

    class NoDevice:
        pass

    with pytest.raises(ValueError, match="window_marginal is only offered with device_window"):
        replay.run(small_cfg(2, window_marginal=True), NoDevice(), scans=[])
    with pytest.raises(RuntimeError, match="window_marginal is only offered with device_window"):
        replay.run_native(small_cfg(2, window_marginal=True), [], str(tmp_path))
    far = small_cfg(2, device_window=True, window_marginal=True, odometry_every=2)
    with pytest.raises(ValueError, match="beyond pose 1"):
        replay.run(far, NoDevice(), scans=[])
    with pytest.raises(RuntimeError, match="beyond pose 1"):
        replay.run_native(far, [], str(tmp_path))


def test_native_input_does_not_know_the_switch(tmp_path):
    cfg = small_cfg(2, device_window=True)
    scans = replay.make_scans(cfg)
    replay.write_native_input(str(tmp_path / "off.bin"), cfg, scans)
    replay.write_native_input(str(tmp_path / "on.bin"), dataclasses.replace(cfg, window_marginal=True), scans)
    assert filecmp.cmp(str(tmp_path / "off.bin"), str(tmp_path / "on.bin"), shallow=False)


@pytest.mark.gpu
def test_replays_with_the_marginal_prior(ctx, tmp_path):
    cfg = small_cfg(device_window=True)
    on_cfg = dataclasses.replace(cfg, window_marginal=True)
    scans = replay.make_scans(cfg)
    pinned = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    on = replay.run(on_cfg, replay.HipBackend(ctx, on_cfg), scans)  # (a singular window call raises)
    assert pinned["marginal_valid"] == []
    assert on["marginal_valid"] == [1] * (len(scans) - cfg.window), on["marginal_valid"]
    assert all(len(fs) == cfg.update_iters for fs in on["costs"])
    # until the window first slides the two replays are the same replay
    for k in range(cfg.window):
        assert np.array_equal(on["poses_est"][k][0], pinned["poses_est"][k][0]) and np.array_equal(on["poses_est"][k][1], pinned["poses_est"][k][1])
    dt, dR = deviation(on, pinned)
    e_on, e_pin = float(np.mean(on["trans_err"])), float(np.mean(pinned["trans_err"]))
    print(f"python: marginal prior vs pin: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}; mean translation error {e_on * 1e3:.3f} mm against {e_pin * 1e3:.3f} mm pinned")
    assert dt > 0.0
    assert e_on <= 2.0 * e_pin, (e_on, e_pin)
    native = replay.run_native(on_cfg, scans, str(tmp_path))
    ndt, ndR = deviation(native, on)
    print(f"native vs python with the marginal prior: max |dt| = {ndt:.3e} m, max |dR| = {ndR:.3e}")
    assert native["marginal_valid"] == on["marginal_valid"]
    assert ndt < 1e-7 and ndR < 1e-8
