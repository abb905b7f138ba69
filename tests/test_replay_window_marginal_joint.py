"""Sequence replay with the JOINT marginal prior of the pose that leaves the window (ReplayConfig.window_marginal_joint /
replay::Config::window_marginal_joint, the native driver's `+marginal-joint`): window_marginal for a window whose oldest pose
external odometry ties beyond pose 1.  Opt-in, only offered with device_window and odometry_every 1 .. 4, refused otherwise.
Off, the trajectory and the native input file are those of device_window.  With odometry_every = 1 every odometry edge ends on
pose 1, the separator is {1} and the replay is the window_marginal replay (1e-9 m).  With odometry_every = 2 and 3 every marginal
is valid, no window call is singular (the replay raises on one), the Python and the native replay agree as tests/test_replay.py
holds them (1e-7 m, 1e-8 on the rotation entries), and the mean translation error against the synthetic truth stays within twice
that of the pinned replay run beside it (the bar of tests/test_replay_window_marginal.py: a guard against a gross error).

The separator sizes.  Each marginal's separator must be the Markov blanket of the oldest pose in the replay's factor graph:
`expected_separators` below works it out with sets of scan indices, independently of the library.  The replay's odometry source
reports at every odometry_every-th scan, so its edges are (0, m), (m, 2m), ...: one ends on every m-th scan only, and the blanket
is at most m poses wide — 2 is reached for m = 2; for m = 3 the widest is {1, 3} and {1, 2}, two poses.  The sequences worked out
for an edge (k - m, k) ending on EVERY scan ({1,2} for m = 2; {1,3} -> {1,2,3} -> {1,2,3} for m = 3, the blanket settling at m
poses) are asserted where that graph is built: tests/test_gpu_icp_window_joint.py, test_sliding_separators_settle_at_the_edge_span."""
import dataclasses
import filecmp

import numpy as np
import pytest

from mimosa_amd import replay
from test_replay_device_window import small_cfg
from test_replay_window_relin import deviation


def expected_separators(n_scans, window, every):
    """per marginalisation the separator as window indices: pose 1, the far ends of the live odometry edges from pose 0, the poses
    of the carried prior (the previous separator) other than pose 0"""
    win, edges, carried, out = [], [], None, []
    for k in range(n_scans):
        win.append(k)
        if len(win) > window:
            live = win[:-1]
            S = {live[1]} | {b for a, b in edges if a == live[0]} | ({s for s in carried if s != live[0]} if carried else set())
            out.append(sorted(s - live[0] for s in S))
            carried = S
            win.pop(0)
        if every > 0 and k >= every and k % every == 0:
            edges.append((k - every, k))
        edges = [e for e in edges if e[0] >= win[0]]
    return out


def test_expected_separators_of_the_replays_graph():
    assert expected_separators(10, 5, 1) == [[1]] * 5
    assert expected_separators(10, 5, 2) == [[1, 2], [1], [1, 2], [1], [1, 2]]
    assert expected_separators(10, 5, 3) == [[1, 3], [1, 2], [1], [1, 3], [1, 2]]
    assert all(len(s) <= 4 for m in (1, 2, 3, 4) for s in expected_separators(40, 5, m))


def test_switch_is_opt_in_and_refused_where_it_is_not_offered(tmp_path):
    assert not replay.ReplayConfig().window_marginal_joint

    class NoDevice:
        pass

    off = small_cfg(2, window_marginal_joint=True, odometry_every=2)
    with pytest.raises(ValueError, match="window_marginal_joint is only offered with device_window"):
        replay.run(off, NoDevice(), scans=[])
    with pytest.raises(RuntimeError, match="window_marginal_joint is only offered with device_window"):
        replay.run_native(off, [], str(tmp_path))
    for every in (5, 0):
        far = small_cfg(2, device_window=True, window_marginal_joint=True, odometry_every=every)
        with pytest.raises(ValueError, match="odometry_every 1 .. 4"):
            replay.run(far, NoDevice(), scans=[])
        with pytest.raises(RuntimeError, match="odometry_every 1 .. 4"):
            replay.run_native(far, [], str(tmp_path))
    both = small_cfg(2, device_window=True, window_marginal_joint=True, window_marginal=True, odometry_every=1)
    with pytest.raises(ValueError, match="not offered together"):
        replay.run(both, NoDevice(), scans=[])
    # window_marginal itself still refuses the far edge
    with pytest.raises(ValueError, match="beyond pose 1"):
        replay.run(small_cfg(2, device_window=True, window_marginal=True, odometry_every=2), NoDevice(), scans=[])


def test_native_input_does_not_know_the_switch(tmp_path):
    cfg = small_cfg(2, device_window=True, odometry_every=2)
    scans = replay.make_scans(cfg)
    replay.write_native_input(str(tmp_path / "off.bin"), cfg, scans)
    replay.write_native_input(str(tmp_path / "on.bin"), dataclasses.replace(cfg, window_marginal_joint=True), scans)
    assert filecmp.cmp(str(tmp_path / "off.bin"), str(tmp_path / "on.bin"), shallow=False)


@pytest.mark.gpu
def test_odometry_at_every_scan_is_the_window_marginal_replay(ctx):
    cfg = small_cfg(device_window=True, odometry_every=1)
    scans = replay.make_scans(cfg)
    one_cfg, joint_cfg = dataclasses.replace(cfg, window_marginal=True), dataclasses.replace(cfg, window_marginal_joint=True)
    one = replay.run(one_cfg, replay.HipBackend(ctx, one_cfg), scans)
    joint = replay.run(joint_cfg, replay.HipBackend(ctx, joint_cfg), scans)
    n = len(scans) - cfg.window
    assert joint["marginal_valid"] == one["marginal_valid"] == [1] * n and joint["separator_sizes"] == [1] * n
    dt, dR = deviation(joint, one)
    print(f"odometry_every = 1: joint marginal vs window_marginal: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}")
    assert dt <= 1e-9 and dR <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("every", [2, 3])
def test_replays_with_the_joint_marginal_prior(ctx, tmp_path, every):
    cfg = small_cfg(device_window=True, odometry_every=every)
    on_cfg = dataclasses.replace(cfg, window_marginal_joint=True)
    scans = replay.make_scans(cfg)
    pinned = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    on = replay.run(on_cfg, replay.HipBackend(ctx, on_cfg), scans)  # (a singular window call raises)
    n = len(scans) - cfg.window
    want = expected_separators(len(scans), cfg.window, every)
    assert pinned["marginal_valid"] == [] and pinned["separator_sizes"] == []
    assert on["marginal_valid"] == [1] * n, on["marginal_valid"]
    assert on["separator_sizes"] == [len(s) for s in want], (on["separator_sizes"], want)
    assert max(on["separator_sizes"]) == 2  # an edge from the oldest pose past pose 1 went into a marginal: window_marginal refuses this replay
    assert all(len(fs) == cfg.update_iters for fs in on["costs"])
    for k in range(cfg.window):  # until the window first slides the two replays are the same replay
        assert np.array_equal(on["poses_est"][k][0], pinned["poses_est"][k][0]) and np.array_equal(on["poses_est"][k][1], pinned["poses_est"][k][1])
    dt, dR = deviation(on, pinned)
    e_on, e_pin = float(np.mean(on["trans_err"])), float(np.mean(pinned["trans_err"]))
    print(f"odometry_every = {every}: separators {on['separator_sizes']}; joint prior vs pin: max |dt| = {dt:.3e} m, max |dR| = {dR:.3e}; "
          f"mean translation error {e_on * 1e3:.3f} mm against {e_pin * 1e3:.3f} mm pinned")
    assert dt > 0.0
    assert e_on <= 2.0 * e_pin, (e_on, e_pin)
    native = replay.run_native(on_cfg, scans, str(tmp_path))
    ndt, ndR = deviation(native, on)
    print(f"odometry_every = {every}: native vs python with the joint prior: max |dt| = {ndt:.3e} m, max |dR| = {ndR:.3e}")
    assert native["marginal_valid"] == on["marginal_valid"] and native["separator_sizes"] == on["separator_sizes"]
    assert ndt < 1e-7 and ndR < 1e-8
