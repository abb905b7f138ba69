"""Synthetic radar scenes for the Doppler path (tests, tools/radar_time.py).

A sensor with known R_W_B, v_W, gyro rate, gyro bias and T_B_S sees static targets whose Doppler values are consistent with
that motion (DopplerHessianFactor's model, include/mimosa/radar/factor.hpp:100-143: a static target at bearing b has
radial_speed = -b . v_R) plus Gaussian noise, a few dynamic outliers, and points that each gate of Manager::preprocess
(src/radar/manager.cpp:143-171) must drop: a NaN in every field, intensity below filter_min_db, range below / above the
bounds, azimuth / elevation beyond the thresholds.  Every generated point keeps 1e-4 rad from the angle thresholds and
1e-5 m from the range bounds (in float32), so the kept set does not depend on the last ulp of atan2f.

Records are packed as raw sensor_msgs::PointCloud2 bytes of both layouts the reference decodes (point.hpp): mmWavePoint and
rioPoint (the inverse of manager.cpp:126-134's axis swap applied), each with padding in the record.
"""
from __future__ import annotations

import numpy as np

from .synth import so3_exp

# record layouts: (point_step, field offsets); PCL_ADD_POINT4D pads x, y, z to 16 bytes
MMWAVE = dict(point_step=32, x=0, y=4, z=8, intensity=16, velocity=20)
RIO = dict(point_step=36, x=0, y=4, z=8, intensity=16, noise=20, velocity=24)  # intensity = snr_db, velocity = v_doppler_mps

DEFAULT_CFG = dict(range_min=0.1, range_max=20.0, threshold_azimuth_deg=60.0, threshold_elevation_deg=60.0, filter_min_db=5.0,
                   noise_sigma=0.1)
ANGLE_MARGIN, RANGE_MARGIN = 1e-4, 1e-5


def _thr(deg):
    return float(np.float32(np.float32(deg) * np.float32(np.pi)) / np.float32(180.0))


def _margins_ok(x, y, z, cfg):
    """float32 range / angles of the points at least the margins away from every bound"""
    x, y, z = (np.asarray(a, np.float32) for a in (x, y, z))
    with np.errstate(invalid="ignore"):
        r = np.sqrt((x * x + y * y) + z * z).astype(np.float64)
        az = np.abs(np.arctan2(y, x).astype(np.float64))
        el = np.abs(np.arctan2(z, np.sqrt(x * x + y * y)).astype(np.float64))
    ok = (np.abs(r - np.float32(cfg["range_min"])) > RANGE_MARGIN) & (np.abs(r - np.float32(cfg["range_max"])) > RANGE_MARGIN)
    ok &= np.abs(az - _thr(cfg["threshold_azimuth_deg"])) > ANGLE_MARGIN
    ok &= np.abs(el - _thr(cfg["threshold_elevation_deg"])) > ANGLE_MARGIN
    return ok


def _sample_inside(rng, n, cfg):
    out = []
    while sum(len(a) for a in out) < n:
        m = 2 * n + 16
        r = rng.uniform(cfg["range_min"], cfg["range_max"], m)
        az = rng.uniform(-1, 1, m) * np.deg2rad(cfg["threshold_azimuth_deg"])
        el = rng.uniform(-1, 1, m) * np.deg2rad(cfg["threshold_elevation_deg"])
        p = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)
        out.append(p[_margins_ok(p[:, 0], p[:, 1], p[:, 2], cfg)])
    return np.concatenate(out)[:n]


def sensor_velocity(state: dict) -> np.ndarray:
    """v_R of the model (factor.hpp:108-118)"""
    v_from_ang = np.cross(state["omega"] - state["bias_gyro"], state["t_B_S"])
    return state["R_B_S"].T @ (state["R_W_B"].T @ state["v_W"] + v_from_ang)


def random_state(rng) -> dict:
    return dict(R_W_B=so3_exp(rng.normal(0, 0.8, 3)), v_W=rng.normal(0, 2.0, 3), omega=rng.normal(0, 0.4, 3),
                bias_gyro=rng.normal(0, 0.01, 3), R_B_S=so3_exp(rng.normal(0, 0.3, 3)), t_B_S=rng.normal(0, 0.2, 3))


def make_scene(n_static: int = 400, n_dynamic: int = 20, seed: int = 0, cfg: dict | None = None, bad: bool = True,
               state: dict | None = None, doppler_noise: float | None = None) -> dict:
    """Points in the mmWavePoint frame (float32 x, y, z, intensity, velocity), shuffled, with a label per point:
    0 static, 1 dynamic, 2 dropped by a gate.  doppler_noise: standard deviation of the Doppler noise (default noise_sigma)."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    rng = np.random.default_rng(seed)
    st = state or random_state(rng)
    vR = sensor_velocity(st)
    n_good = n_static + n_dynamic
    p = _sample_inside(rng, n_good, cfg)
    b = p.astype(np.float64) / np.linalg.norm(p.astype(np.float64), axis=1, keepdims=True)
    dop = -(b @ vR) + rng.normal(0, cfg["noise_sigma"] if doppler_noise is None else doppler_noise, n_good)
    dop[n_static:] += rng.choice([-1, 1], n_dynamic) * rng.uniform(1.0, 5.0, n_dynamic)  # moving targets
    inten = rng.uniform(cfg["filter_min_db"] + 1, 40.0, n_good)
    lab = np.r_[np.zeros(n_static, int), np.ones(n_dynamic, int)]
    cols = [p[:, 0], p[:, 1], p[:, 2], inten, dop]
    if bad:
        bx = []
        base = _sample_inside(rng, 9, cfg)
        for k in range(5):  # a NaN in every field
            r = [base[k, 0], base[k, 1], base[k, 2], 20.0, 0.5]
            r[k] = np.nan
            bx.append(r)
        bx.append([*base[5], cfg["filter_min_db"] - 1.0, 0.5])  # weak return
        d = base[6] / np.linalg.norm(base[6])
        bx.append([*(d * cfg["range_min"] * 0.5), 20.0, 0.5])  # too close
        bx.append([*(d * cfg["range_max"] * 1.5), 20.0, 0.5])  # too far
        a = np.deg2rad(cfg["threshold_azimuth_deg"]) + 0.2
        bx.append([5 * np.cos(a), 5 * np.sin(a), 0.0, 20.0, 0.5])  # outside the azimuth cone
        e = np.deg2rad(cfg["threshold_elevation_deg"]) + 0.2
        bx.append([5 * np.cos(e), 0.0, 5 * np.sin(e), 20.0, 0.5])  # outside the elevation cone
        bx.append([-5 * np.cos(a), -5 * np.sin(a), 0.0, 20.0, 0.5])  # behind the sensor
        bx = np.array(bx, np.float64)
        cols = [np.r_[c, bx[:, k]] for k, c in enumerate(cols)]
        lab = np.r_[lab, np.full(len(bx), 2)]
    perm = rng.permutation(len(lab))
    pts = {k: np.asarray(c, np.float64)[perm].astype(np.float32) for k, c in zip(("x", "y", "z", "intensity", "velocity"), cols)}
    return dict(points=pts, labels=lab[perm], state=st, cfg=cfg)


def pack(points: dict, kind: str = "mmwave", pad_value: float = 7.0) -> tuple[np.ndarray, dict]:
    """(raw record bytes as uint8, layout dict with kind / point_step / offsets)."""
    lay = dict(RIO if kind == "rio" else MMWAVE)
    n = len(points["x"])
    step = lay["point_step"]
    rec = np.full((n, step // 4), np.float32(pad_value), np.float32)  # padding words carry junk, never read
    x, y = points["x"], points["y"]
    if kind == "rio":  # inverse of manager.cpp:126-134 (x' = y, y' = -x): y_rio = x', x_rio = -y'
        x, y = (-y).astype(np.float32), x
        rec[:, lay["noise"] // 4] = -90.0
    rec[:, lay["x"] // 4] = x
    rec[:, lay["y"] // 4] = y
    rec[:, lay["z"] // 4] = points["z"]
    rec[:, lay["intensity"] // 4] = points["intensity"]
    rec[:, lay["velocity"] // 4] = points["velocity"]
    lay["kind"] = kind
    return rec.view(np.uint8).reshape(-1), lay


def capi_layout(lay: dict):
    from . import capi

    kind = {"rio": capi.MH_RADAR_RIO, "mmwave": capi.MH_RADAR_MMWAVE, "doppler_residual": capi.MH_RADAR_MMWAVE_DOPPLER_RESIDUAL}[lay["kind"]]
    return capi.radar_layout(kind, lay["point_step"], lay["x"], lay["y"], lay["z"], lay["intensity"], lay["velocity"])


def random_targets(rng, n: int) -> np.ndarray:
    """n x 8 TargetData rows (float32-valued like the front end's) at random positions inside the default gates."""
    p = _sample_inside(rng, n, DEFAULT_CFG) if n else np.zeros((0, 3), np.float32)
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(np.float32)
    az = np.arctan2(p[:, 1], p[:, 0]).astype(np.float32)
    el = np.arctan2(p[:, 2], np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).astype(np.float32)).astype(np.float32)
    dop = rng.normal(0, 2.0, n).astype(np.float32)
    inten = rng.uniform(6, 40, n).astype(np.float32)
    return np.stack([p[:, 0], p[:, 1], p[:, 2], r, az, el, dop, inten], 1).astype(np.float64)
