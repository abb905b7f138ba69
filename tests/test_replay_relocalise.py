"""The replay's opt-in relocalise_first (mimosa_amd/replay.py): the first scan's pose comes from mh_icp_relocalise over a grid
around a guess that is wrong by (1.5 m, 20 degrees), instead of from first_state's truth-based guess.  5 scans at 64 x 512.

Bar: from scan 1 on the trajectory agrees with the same replay started from first_state to within 10 x the difference of the two
FIRST poses before the smoother sees them — the relocalised pose against the propagated first guess, which is what the two runs
hand to the first window.  Measured once (MI355X): that difference is 3.8e-2 m / 0.14 degrees (the propagated guess carries the
0.03 m prior noise; both runs end scan 0 at 5.5 mm from the truth); the trajectories differ by 1.3e-3 m at scan 0 and by at most
8.4e-5 m from scan 1 on.  The test prints the figures again."""
import numpy as np
import pytest


def _cfg(**kw):
    from mimosa_amd import replay
    return replay.ReplayConfig(n_scans=5, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2, keyframe_rot_thresh_deg=5.0,
                               photometric=False, **kw)


def test_relocalise_first_is_refused_without_the_hip_backend():
    from mimosa_amd import replay
    from oracle.replay_backend import OracleBackend
    cfg = _cfg(relocalise_first=True)
    with pytest.raises(ValueError, match="relocalise_first needs a backend with mh_icp_relocalise"):
        replay.run(cfg, OracleBackend(cfg), [])
    with pytest.raises(RuntimeError, match="relocalise_first"):
        replay.run_native(cfg, [], "/nonexistent")
    assert _cfg().relocalise_first is False  # off by default


@pytest.mark.gpu
def test_relocalise_first_is_refused_with_init_align(ctx):
    from mimosa_amd import replay
    cfg = _cfg(relocalise_first=True, init_align=True)
    with pytest.raises(ValueError, match="init_align"):
        replay.run(cfg, replay.HipBackend(ctx, cfg), [])


@pytest.mark.gpu
def test_replay_from_a_relocalised_first_pose(ctx):
    from mimosa_amd import replay
    base, on = _cfg(), _cfg(relocalise_first=True)
    assert np.linalg.norm(on.relocalise_guess_offset) == pytest.approx(1.5) and on.relocalise_guess_yaw_deg == 20.0
    scans = replay.make_scans(base)
    a = replay.run(base, replay.HipBackend(ctx, base), scans)
    b = replay.run(on, replay.HipBackend(ctx, on), scans)
    assert a["relocalised"] is None
    rel = b["relocalised"]
    (Rg, tg), (Rw, tw), (Rp, tp) = rel["guess"], rel["pose"], rel["predicted"]
    # the guess was wrong by more than the gate; the relocalised pose is back at the propagated one
    assert np.linalg.norm(tg - tp) == pytest.approx(1.5)
    d0 = float(np.linalg.norm(tw - tp))
    r0 = float(np.rad2deg(np.arccos(np.clip((np.trace(Rw.T @ Rp) - 1.0) / 2.0, -1.0, 1.0))))
    print("first pose, relocalised against propagated: %.4e m %.4e deg; candidates %s best %d" % (d0, r0, rel["candidates"], rel["best"]))
    assert d0 < 0.1  # it found the basin (the gate is 1 m, the grid step 0.5 m)
    worst = [float(np.linalg.norm(ta - tb)) for (_, ta), (_, tb) in zip(a["poses_est"], b["poses_est"])]
    print("trajectory difference per scan:", ["%.3e" % w for w in worst], "first-pose error of either run: %.4f / %.4f m" % (a["trans_err"][0], b["trans_err"][0]))
    assert max(worst[1:]) <= 10.0 * d0
    assert max(b["trans_err"]) < 0.05  # and it tracks the ground truth as the default replay does
