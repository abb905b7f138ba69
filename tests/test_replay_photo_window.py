"""Sequence replay with the reference's window of photometric factors (ReplayConfig.photo_window / replay::Config::photo_window):
every scan's photometric factor stays in the smoother window on its own pose, and all of them are re-linearized per
Gauss-Newton iteration — through ONE mh_photo_factor_linearize_batch per iteration on the HIP backend, one call per factor
on the oracle backend.  Sizes and bounds are those of tests/test_replay.py."""
import numpy as np
import pytest

from mimosa_amd import replay
from oracle.replay_backend import OracleBackend


def small_cfg(n=6, **kw):
    return replay.ReplayConfig(n_scans=n, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2,
                               keyframe_rot_thresh_deg=5.0, **kw)


def _window_counts(r, cfg):
    """photometric factors in the window per scan: none before features are tracked, then one more per scan up to the window"""
    counts = r["photo_in_window"]
    assert len(counts) == cfg.n_scans
    k0 = next(k for k, c in enumerate(counts) if c)
    assert all(c == 0 for c in counts[:k0])
    assert counts[k0:] == [min(k - k0 + 1, cfg.window) for k in range(k0, cfg.n_scans)]
    return k0


def test_photo_window_replay_tracks_ground_truth_on_oracle():
    cfg = small_cfg(7, photo_window=True)
    assert not replay.ReplayConfig().photo_window                         # opt-in
    scans = replay.make_scans(cfg)
    r = replay.run(cfg, OracleBackend(cfg), scans)
    assert _window_counts(r, cfg) == 1
    assert max(r["trans_err"]) < 0.012 and max(r["rot_err_deg"]) < 0.06
    assert len(r["photo_valid"]) == cfg.n_scans - 1 and min(r["photo_valid"]) >= 20
    off = replay.run(small_cfg(7), OracleBackend(small_cfg(7)), scans)
    assert off["photo_in_window"] == []
    # the older factors do constrain the older poses: the trajectory is not the one of the newest-factor window
    assert max(np.max(np.abs(a[1] - b[1])) for a, b in zip(r["poses_est"], off["poses_est"])) > 1e-9


@pytest.mark.gpu
def test_photo_window_replay_hip_equals_oracle(ctx):
    cfg = small_cfg(6, photo_window=True)
    scans = replay.make_scans(cfg)
    ro = replay.run(cfg, OracleBackend(cfg), scans)
    rh = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    assert rh["n_keyframes"] == ro["n_keyframes"] and rh["photo_valid"] == ro["photo_valid"]
    assert rh["photo_in_window"] == ro["photo_in_window"]
    _window_counts(rh, cfg)
    for (Ra, ta), (Rb, tb) in zip(rh["poses_est"], ro["poses_est"]):
        assert np.max(np.abs(ta - tb)) < 1e-7 and np.max(np.abs(Ra - Rb)) < 1e-8
    assert max(rh["trans_err"]) < 0.012 and max(rh["rot_err_deg"]) < 0.06


@pytest.mark.gpu
def test_photo_window_native_equals_python(ctx, tmp_path):
    """FixedLagReplay with the switch (the sixth entry of the driver's int block) against replay.run on the C ABI binding,
    pipelined and sequential; the manager and sharded replays refuse the switch."""
    cfg = small_cfg(7, photo_window=True)
    scans = replay.make_scans(cfg)
    rp = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    rn = replay.run_native(cfg, scans, str(tmp_path))
    rs = replay.run_native(cfg, scans, str(tmp_path), sequential=True)
    assert rn["n_keyframes"] == rp["n_keyframes"] and rn["photo_valid"] == rp["photo_valid"]
    assert rn["photo_in_window"] == rp["photo_in_window"]
    _window_counts(rn, cfg)
    assert np.allclose(rn["first_costs"], rp["costs"][0], rtol=1e-9)
    for (Ra, ta), (Rb, tb) in zip(rn["poses_est"], rp["poses_est"]):
        assert np.max(np.abs(ta - tb)) < 1e-7 and np.max(np.abs(Ra - Rb)) < 1e-8
    for (Ra, ta), (Rb, tb) in zip(rn["poses_est"], rs["poses_est"]):
        assert np.array_equal(ta, tb) and np.array_equal(Ra, Rb)
    assert max(rn["trans_err"] if "trans_err" in rn else rp["trans_err"]) < 0.012
    for kw in (dict(through_manager=True), dict(sharded_world=1)):
        with pytest.raises(RuntimeError, match="photo_window"):
            replay.run_native(cfg, scans[:2], str(tmp_path), **kw)
