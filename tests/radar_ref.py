"""Independent numpy restatement of the reference's radar path, transcribed from its semantics (test infrastructure only:
nothing under mimosa_amd/ imports it).

  Manager::preprocess      src/radar/manager.cpp:111-181 (rioPoint remap :126-134, gates :143-171, TargetData :173-174)
  DopplerHessianFactor     include/mimosa/radar/factor.hpp:98-188 (linearize)

The front end is restated in float32 exactly as the reference's float arithmetic runs: numpy's float32 +, *, sqrt are
correctly rounded, and atan2 is the host libm's atan2f itself (numpy's own float32 arctan2 is a few ulp off), which may
differ from the device's correctly rounded value by an ulp; the tests allow for that.  The factor is
restated in float64 with one target per row; its sums are taken by numpy, in another order than the device's.
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


def atan2f(y, x) -> np.ndarray:
    """std::atan2(float, float) of the host libm, element-wise."""
    y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
    return np.array([_libm.atan2f(float(a), float(b)) for a, b in zip(y, x)], np.float32).reshape(y.shape)


TARGET_FIELDS = ("x", "y", "z", "range", "azimuth", "elevation", "radial_speed", "intensity")
ROBUST_C = 2.3849  # factor.hpp:162


def deg2rad_f(deg) -> np.float32:
    """deg2rad<float> (include/mimosa/utils.hpp): (deg * float(M_PI)) / 180.f in float."""
    return np.float32(np.float32(deg) * np.float32(np.pi)) / np.float32(180.0)


def decode(raw: np.ndarray, n: int, kind: str, point_step: int, offs: dict):
    """Fields of the n records as float32 in the mmWavePoint frame (x, y, z, intensity, velocity)."""
    b = np.frombuffer(np.ascontiguousarray(raw).tobytes(), np.uint8)[: n * point_step].reshape(n, point_step)

    def field(name):
        o = offs[name]
        return b[:, o:o + 4].copy().view(np.float32).reshape(n)

    x, y, z, i, v = (field(k) for k in ("x", "y", "z", "intensity", "velocity"))
    if kind == "rio":  # manager.cpp:126-134: x' = y, y' = -x, intensity = snr_db, velocity = v_doppler_mps
        x, y = y.copy(), (-x).astype(np.float32)
    return x, y, z, i, v


def preprocess(x, y, z, intensity, velocity, cfg: dict):
    """Manager::preprocess's filter loop.  Returns (indices kept, in input order; targets as n x 8 float64)."""
    f32 = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        keep = ~(np.isnan(x) | np.isnan(y) | np.isnan(z) | np.isnan(intensity) | np.isnan(velocity))
        keep &= ~(intensity < f32(cfg["filter_min_db"]))
        rng = np.sqrt((x * x + y * y) + z * z).astype(f32)  # getVector3fMap().norm()
        keep &= ~((rng < f32(cfg["range_min"])) | (rng > f32(cfg["range_max"])))
        az = atan2f(y, x)  # std::atan2(float, float)
        keep &= ~(np.abs(az) > deg2rad_f(cfg["threshold_azimuth_deg"]))
        rxy = np.sqrt(x * x + y * y).astype(f32)
        el = atan2f(z, rxy)
        keep &= ~(np.abs(el) > deg2rad_f(cfg["threshold_elevation_deg"]))
    idx = np.nonzero(keep)[0]
    t = np.stack([x[idx], y[idx], z[idx], rng[idx], az[idx], el[idx], velocity[idx], intensity[idx]], axis=1).astype(np.float64)
    return idx, t


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def residuals_unweighted(targets, R_B_S, t_B_S, omega, R_W_B, v_W, bias_gyro):
    """e = -bearing . v_R - doppler per target (factor.hpp:100-118, :137-143)."""
    t = np.asarray(targets, np.float64).reshape(-1, 8)
    rot_R_B, l_R_B = np.asarray(R_B_S, float), np.asarray(t_B_S, float)
    rot_B_W = np.asarray(R_W_B, float)
    v_from_ang = np.cross(np.asarray(omega, float) - np.asarray(bias_gyro, float), l_R_B)
    v_R = rot_R_B.T @ (rot_B_W.T @ np.asarray(v_W, float) + v_from_ang)
    bearing = t[:, 0:3] / t[:, 3:4]
    return -(bearing @ v_R) - t[:, 6]


def jacobians(targets, R_B_S, t_B_S, R_W_B, v_W):
    """J1 (n x 6: rotation, translation), J2 (n x 3), J3 (n x 6: accelerometer, gyroscope), factor.hpp:145-152."""
    t = np.asarray(targets, np.float64).reshape(-1, 8)
    rot_R_B, l_R_B = np.asarray(R_B_S, float), np.asarray(t_B_S, float)
    rot_B_W = np.asarray(R_W_B, float)
    bearing = t[:, 0:3] / t[:, 3:4]
    n = t.shape[0]
    J1 = np.zeros((n, 6))
    J1[:, 0:3] = -bearing @ rot_R_B.T @ (rot_B_W.T @ skew(v_W) @ rot_B_W)
    J2 = -bearing @ rot_R_B.T @ rot_B_W.T
    J3 = np.zeros((n, 6))
    J3[:, 3:6] = -bearing @ rot_R_B.T @ skew(l_R_B)
    return J1, J2, J3


def linearize(targets, R_B_S, t_B_S, omega, noise_sigma, R_W_B, v_W, bias_gyro) -> dict:
    """DopplerHessianFactor::linearize: the blocks of HessianFactor(X, V, B, G11, G12, G13, g1, G22, G23, g2, G33, g3, f),
    plus the per-target e_whitened (before the weight) and weight."""
    sigma = float(noise_sigma)
    e = residuals_unweighted(targets, R_B_S, t_B_S, omega, R_W_B, v_W, bias_gyro)
    J1, J2, J3 = jacobians(targets, R_B_S, t_B_S, R_W_B, v_W)
    e_w = e / sigma
    weight = np.sqrt(1.0 / (1.0 + (e_w / ROBUST_C) ** 2))
    J1w = J1 / sigma * weight[:, None]
    J2w = J2 / sigma * weight[:, None]
    J3w = J3 / sigma * weight[:, None]
    eww = e_w * weight
    return {
        "G11": J1w.T @ J1w, "G12": J1w.T @ J2w, "G13": J1w.T @ J3w, "G22": J2w.T @ J2w, "G23": J2w.T @ J3w, "G33": J3w.T @ J3w,
        "g1": -J1w.T @ eww, "g2": -J2w.T @ eww, "g3": -J3w.T @ eww, "f": float(eww @ eww),
        "e_whitened": e_w, "weight": weight,
    }
