"""The replay's opt-in relocalise_batch (mimosa_amd/replay.py): with relocalise_first, the candidates of the first scan are aligned
side by side by mh_icp_relocalise_batch instead of one after another.  2 scans at 64 x 512.

Bar: the relocalised pose with the switch on agrees with the switch off to 1e-9 m / 1e-9 rad (the candidates' launch class follows
the batch's total point count, so the sums differ in their last bits, not more), with the same winner and the same candidate
indices.  The trajectory difference behind it is printed, not held."""
import numpy as np
import pytest


def _cfg(**kw):
    from mimosa_amd import replay
    return replay.ReplayConfig(n_scans=2, rows=64, cols=512, room=(12.0, 10.0, 3.0), keyframe_trans_thresh=0.2, keyframe_rot_thresh_deg=5.0,
                               photometric=False, **kw)


def test_relocalise_batch_is_off_by_default_and_refused_alone():
    from mimosa_amd import replay
    from oracle.replay_backend import OracleBackend
    assert _cfg().relocalise_batch is False and _cfg(relocalise_first=True).relocalise_batch is False
    cfg = _cfg(relocalise_batch=True)
    with pytest.raises(ValueError, match="relocalise_batch is only offered with relocalise_first"):
        replay.run(cfg, OracleBackend(cfg), [])


@pytest.mark.gpu
def test_relocalised_pose_on_against_off(ctx):
    from mimosa_amd import replay
    off, on = _cfg(relocalise_first=True), _cfg(relocalise_first=True, relocalise_batch=True)
    scans = replay.make_scans(off)
    a = replay.run(off, replay.HipBackend(ctx, off), scans)
    b = replay.run(on, replay.HipBackend(ctx, on), scans)
    ra, rb = a["relocalised"], b["relocalised"]
    (Ra, ta), (Rb, tb) = ra["pose"], rb["pose"]
    M = Ra.T @ Rb
    dt = float(np.linalg.norm(ta - tb))
    dr = float(np.arctan2(np.linalg.norm(M - M.T) / (2.0 * np.sqrt(2.0)), (np.trace(M) - 1.0) / 2.0))
    print("relocalised pose, batch on against off: %.3e m %.3e rad; candidates %s best %d" % (dt, dr, rb["candidates"], rb["best"]))
    assert dt <= 1e-9 and dr <= 1e-9
    assert ra["best"] == rb["best"] and ra["candidates"] == rb["candidates"]
    assert [f["n_inliers"] for f in ra["fine"]] == [f["n_inliers"] for f in rb["fine"]]
    worst = max(float(np.linalg.norm(pa[1] - pb[1])) for pa, pb in zip(a["poses_est"], b["poses_est"]))
    print("trajectory difference: %.3e m (reported; the relocalised pose above is the bar)" % worst)
