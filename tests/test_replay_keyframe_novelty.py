"""Sequence replay with the keyframe decision made by what a scan would add to the map (ReplayConfig.keyframe_new_fraction):
an insert preview of the scan's body cloud at the estimated pose instead of the pose test.  10 scans of 64 x 512 without the
photometric factor, the sizes of tests/test_replay_device_window.py.  Off (0, the default) the run is the pose-rule run bit for bit
and reports no fractions.  On, the first scan is a keyframe, every later one iff its fraction reaches the threshold; one scan's
fraction is rechecked through copy + insert + stats on the map as it stood.

Accuracy: the rule changes what the map holds, so the trajectory is not the pose rule's.  The only bar is a guard against a map
that stopped serving associations: the maximum translation error stays under ten times that of the default run beside it."""
import dataclasses

import numpy as np
import pytest

from mimosa_amd import replay
from test_replay_device_window import small_cfg

pytestmark = pytest.mark.gpu

# The CPU estimate of the fractions of these ten scans (numpy oracle, ground-truth poses, pose-rule map) lies between 0.034 and
# 0.010, so the search for a threshold that shows both kinds of decision started at 0.015.  There the device run takes scan 0 alone
# (fractions 0.0163, 0.0100, 0.0088, 0.0100, 0.0109, 0.0100, 0.0106, 0.0121, 0.0125, 0.0109: without further keyframes the map is fed
# less than in the estimate).  At 0.0105 scans 0 and 4 are keyframes: a keyframe by fraction and refusals by fraction.  The fractions
# at the chosen value are in DESIGN.md.
THRESHOLD = 0.0105
RECHECK_SCAN = 4


def test_off_is_the_pose_rule_bit_for_bit(ctx):
    cfg = small_cfg()
    assert cfg.keyframe_new_fraction == 0
    scans = replay.make_scans(cfg)
    a = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    b = replay.run(dataclasses.replace(cfg, keyframe_new_fraction=0.0), replay.HipBackend(ctx, cfg), scans)
    assert a["new_fraction"] == [] == b["new_fraction"]
    assert a["n_keyframes"] == b["n_keyframes"] == len(a["keyframe_scans"]) and a["keyframe_scans"] == b["keyframe_scans"]
    for (Ra, ta), (Rb, tb) in zip(a["poses_est"], b["poses_est"]):
        assert np.array_equal(Ra, Rb) and np.array_equal(ta, tb)


def test_keyframes_by_new_fraction(ctx):
    cfg = small_cfg()
    scans = replay.make_scans(cfg)
    off = replay.run(cfg, replay.HipBackend(ctx, cfg), scans)
    on_cfg = dataclasses.replace(cfg, keyframe_new_fraction=THRESHOLD)
    backend = replay.HipBackend(ctx, on_cfg)
    rechecked = []
    preview_map = backend.preview_map

    def preview_and_recheck(R, t):                       # one scan's preview against copy + insert + stats on the map as it stands
        pv = preview_map(R, t)
        if len(rechecked) == 0 and preview_and_recheck.calls == RECHECK_SCAN:
            before = backend.map.stats()
            twin = backend.map.copy()
            twin.insert_from_scan(backend.scan, R, t)
            after = twin.stats()
            twin.release()
            assert backend.map.stats() == before
            rechecked.append((after["n_points"] - before["n_points"], after["n_voxels"] - before["n_voxels"], pv))
        preview_and_recheck.calls += 1
        return pv

    preview_and_recheck.calls = 0
    backend.preview_map = preview_and_recheck
    on = replay.run(on_cfg, backend, scans)
    fr = on["new_fraction"]
    print("keyframe_new_fraction = %g: new_fraction = %s" % (THRESHOLD, ", ".join("%.4f" % v for v in fr)))
    print("keyframes at scans %s (pose rule: %s)" % (on["keyframe_scans"], off["keyframe_scans"]))
    print("trans_err, pose rule:    %s" % ", ".join("%.5f" % v for v in off["trans_err"]))
    print("trans_err, new fraction: %s" % ", ".join("%.5f" % v for v in on["trans_err"]))
    assert len(fr) == cfg.n_scans and all(0.0 <= v <= 1.0 for v in fr)
    assert 1 <= on["n_keyframes"] < cfg.n_scans           # both kinds of decision
    assert on["keyframe_scans"] == [k for k, v in enumerate(fr) if k == 0 or v >= THRESHOLD]
    assert on["n_keyframes"] == len(on["keyframe_scans"])
    assert len(rechecked) == 1
    d_points, d_voxels, pv = rechecked[0]
    assert (d_points, d_voxels) == (pv["n_added"], pv["n_new_voxels"])
    assert fr[RECHECK_SCAN] == pv["n_added"] / pv["n_points"]
    assert max(on["trans_err"]) < 10.0 * max(off["trans_err"])
