"""Sequence replay with the forked map carved by every keyframe's own scan before the insert (ReplayConfig.carve_keyframes,
mh_map_carve_from_scan on the body cloud at the estimated pose).  10 scans of 64 x 512 in the static room without the photometric
factor, the sizes of tests/test_replay_device_window.py.  Off (the default) the run is today's bit for bit and reports no counters.
On, the run completes, every keyframe reports its six counters, and the map never holds more points than the uncarved run's.

The room is static, so whatever the carve removes there is a false positive of the rule at the replay's settings; the removed
fraction per keyframe and the trajectory difference are printed, and the measured figures are in DESIGN.md.  No bar is asserted on
either: neither was known before the first run."""
import dataclasses

import numpy as np
import pytest

from mimosa_amd import replay
from test_replay_device_window import small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def off_run(ctx):
    cfg = small_cfg()
    assert cfg.carve_keyframes is False
    scans = replay.make_scans(cfg)
    return cfg, scans, replay.run(cfg, replay.HipBackend(ctx, cfg), scans)


def test_off_is_todays_run_bit_for_bit(ctx, off_run):
    cfg, scans, a = off_run
    off_cfg = dataclasses.replace(cfg, carve_keyframes=False, carve_grid=16, carve_margin_abs=0.0)   # the other fields are not looked at
    b = replay.run(off_cfg, replay.HipBackend(ctx, off_cfg), scans)
    assert a["carve"] == [] == b["carve"]
    assert a["keyframe_scans"] == b["keyframe_scans"] and a["map_points"] == b["map_points"]
    for (Ra, ta), (Rb, tb) in zip(a["poses_est"], b["poses_est"]):
        assert np.array_equal(Ra, Rb) and np.array_equal(ta, tb)


def test_carved_keyframes(ctx, off_run):
    cfg, scans, off = off_run
    on_cfg = dataclasses.replace(cfg, carve_keyframes=True)
    on = replay.run(on_cfg, replay.HipBackend(ctx, on_cfg), scans)
    assert len(on["poses_est"]) == cfg.n_scans
    assert len(on["carve"]) == on["n_keyframes"] == len(on["map_points"]) >= 1
    before = [None] + on["map_points"][:-1]
    for k, c, n_before in zip(on["keyframe_scans"], on["carve"], before):
        assert set(c) == {"n_obs_used", "n_cells_hit", "n_tested", "n_removed", "n_voxels_touched", "n_voxels_emptied"}
        assert 0 < c["n_obs_used"] and 0 < c["n_cells_hit"] <= 6 * on_cfg.carve_grid ** 2
        assert 0 <= c["n_voxels_emptied"] <= c["n_voxels_touched"] <= c["n_removed"] <= c["n_tested"]
        print("keyframe at scan %d: %s%s" % (k, c, "" if n_before is None else "  removed fraction of the map %.6f" % (c["n_removed"] / n_before)))
    print("keyframes: carved %s, uncarved %s" % (on["keyframe_scans"], off["keyframe_scans"]))
    print("map points after each keyframe: carved %s, uncarved %s" % (on["map_points"], off["map_points"]))
    print("trans_err, uncarved: %s" % ", ".join("%.5f" % v for v in off["trans_err"]))
    print("trans_err, carved:   %s" % ", ".join("%.5f" % v for v in on["trans_err"]))
    print("largest pose difference: %.3e m" % max(float(np.linalg.norm(ta - tb)) for (_, ta), (_, tb) in zip(on["poses_est"], off["poses_est"])))

    def held(run):                                       # map points held after every scan (a scan that is no keyframe leaves the map)
        at, out = dict(zip(run["keyframe_scans"], run["map_points"])), []
        for k in range(cfg.n_scans):
            out.append(at.get(k, out[-1] if out else 0))
        return out

    assert all(a <= b for a, b in zip(held(on), held(off))), (held(on), held(off))
