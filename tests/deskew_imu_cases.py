"""Inputs shared by tests/test_deskew_imu_cpu.py and tests/test_gpu_deskew_imu.py: IMU samples, the states at the sample times,
distinct timestamps and a raw cloud, in the form oracle/numpy_ref.py: deskew_poses takes them."""
import numpy as np

from mimosa_amd import synth


def _trajectory(imu_t, acc, gyro, bias_a, bias_g, g_unit, g_norm, R, p, v):
    """NavStates at the IMU times: any smooth trajectory (they come from the caller's preintegrator)."""
    nav_R, nav_p, nav_v = [], [], []
    for j in range(len(imu_t)):
        nav_R.append(R.copy()); nav_p.append(p.copy()); nav_v.append(v.copy())
        d = imu_t[j + 1] - imu_t[j] if j + 1 < len(imu_t) else 0.0
        R = R @ synth.so3_exp((gyro[j] - bias_g) * d)
        p = p + v * d
        v = v + (R @ (acc[j] - bias_a) + g_unit * g_norm) * d
    return nav_R, nav_p, nav_v


def small_case():
    """The inputs of tests/test_deskew_poses.py::test_deskew_poses_match_numpy: 12 samples at 100 Hz, 147 timestamps."""
    rng = np.random.default_rng(11)
    n_imu, header_ts = 12, 1000.25
    imu_t = header_ts - 0.004 + np.arange(n_imu) * 0.01            # 100 Hz, first sample before the scan starts
    acc = rng.normal(0, 0.5, (n_imu, 3)) + np.array([0, 0, 9.81])
    gyro = rng.normal(0, 0.2, (n_imu, 3))
    bias_a, bias_g = rng.normal(0, 0.02, 3), rng.normal(0, 0.005, 3)
    g_unit, g_norm = np.array([0.0, 0.0, -1.0]), 9.81
    nav_R, nav_p, nav_v = [], [], []
    R, p, v = synth.so3_exp(np.array([0.02, -0.01, 0.4])), np.array([3.0, -2.0, 1.0]), np.array([1.5, 0.2, -0.1])
    for j in range(n_imu):
        nav_R.append(R.copy()); nav_p.append(p.copy()); nav_v.append(v.copy())
        R = R @ synth.so3_exp((gyro[j] - bias_g) * 0.01)
        p = p + v * 0.01
        v = v + (R @ (acc[j] - bias_a) + g_unit * g_norm) * 0.01
    unique_ns = (np.arange(0, 1024, 7) * 97_656).astype(np.uint32)   # 0 .. ~0.0999 s
    T_B_S = (synth.so3_exp(np.array([0.01, 0.02, -0.03])), np.array([-0.006253, 0.011775, 0.0028525]))
    return dict(imu_t=imu_t, acc=acc, gyro=gyro, nav_R=nav_R, nav_p=nav_p, nav_v=nav_v, bias_a=bias_a, bias_g=bias_g, g_unit=g_unit,
                g_norm=g_norm, unique_ns=unique_ns, header_ts=header_ts, T_B_S=T_B_S)


def per_point_case(n_ts=24_000):
    """A sensor with per-point times: n_ts distinct timestamps over 0.0995 s, 41 samples at 400 Hz (40 segments), the first
    sample 0.5 ms AFTER the scan starts (timestamps before it are extrapolated backwards, src/lidar/manager.cpp:469-476)."""
    rng = np.random.default_rng(23)
    n_imu, header_ts = 41, 52_340.5
    imu_t = header_ts + 0.0005 + np.arange(n_imu) * 0.0025
    acc = rng.normal(0, 0.8, (n_imu, 3)) + np.array([0, 0, 9.81])
    gyro = rng.normal(0, 0.4, (n_imu, 3))
    bias_a, bias_g = rng.normal(0, 0.02, 3), rng.normal(0, 0.005, 3)
    g_unit, g_norm = np.array([0.0, 0.0, -1.0]), 9.81
    nav_R, nav_p, nav_v = _trajectory(imu_t, acc, gyro, bias_a, bias_g, g_unit, g_norm, synth.so3_exp(np.array([-0.3, 0.1, 1.2])),
                                      np.array([12.0, -7.5, 1.8]), np.array([2.5, -0.4, 0.2]))
    unique_ns = np.unique(rng.integers(0, 99_500_000, int(n_ts * 1.01), dtype=np.int64))[:n_ts].astype(np.uint32)
    unique_ns[0] = 0
    assert len(unique_ns) == n_ts and header_ts + unique_ns[0] * 1e-9 < imu_t[0] and header_ts + unique_ns[-1] * 1e-9 <= imu_t[-1]
    T_B_S = (synth.so3_exp(np.array([0.01, 0.02, -0.03])), np.array([-0.006253, 0.011775, 0.0028525]))
    return dict(imu_t=imu_t, acc=acc, gyro=gyro, nav_R=nav_R, nav_p=nav_p, nav_v=nav_v, bias_a=bias_a, bias_g=bias_g, g_unit=g_unit,
                g_norm=g_norm, unique_ns=unique_ns, header_ts=header_ts, T_B_S=T_B_S)


def oracle_poses(c):
    """numpy_ref.deskew_poses as (n, 12): R row-major, then t."""
    from oracle import numpy_ref
    want = numpy_ref.deskew_poses(c["imu_t"], c["acc"], c["gyro"], c["nav_R"], c["nav_p"], c["nav_v"], c["bias_a"], c["bias_g"], c["g_unit"],
                                  c["g_norm"], c["unique_ns"], c["header_ts"], c["T_B_S"])
    assert len(want) == len(c["unique_ns"])
    return np.array([np.concatenate([T[:3, :3].ravel(), T[:3, 3]]) for T in want])


def hom(R, p):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, p
    return T


def call_args(c, n_samples=None):
    """(segments, header_ts, gravity, T_Le_W, T_B_S) for Scan.deskew_imu; n_samples: only the first IMU samples (a buffer that
    ends too early), the scan-end state stays the last one."""
    from mimosa_amd import capi
    m = len(c["imu_t"]) if n_samples is None else n_samples
    seg = capi.imu_segments(c["imu_t"][:m], c["acc"][:m], c["gyro"][:m], c["nav_R"][:m], c["nav_p"][:m], c["nav_v"][:m], c["bias_a"], c["bias_g"])
    T_Le_W = np.linalg.inv(hom(*c["T_B_S"])) @ np.linalg.inv(hom(c["nav_R"][-1], c["nav_p"][-1]))
    return seg, c["header_ts"], np.asarray(c["g_unit"]) * c["g_norm"], (T_Le_W[:3, :3], T_Le_W[:3, 3]), c["T_B_S"]


def raw_cloud(unique_ns, per_ts, seed=5):
    """An Ouster-layout raw cloud with per_ts points for each timestamp (ranges 2 .. 40 m, every point passes prepareInput)."""
    rng = np.random.default_rng(seed)
    n = len(unique_ns) * per_ts
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz = d * rng.uniform(2.0, 40.0, n)[:, None]
    raw = np.zeros(n, dtype=synth.OUSTER_DTYPE)
    raw["x"], raw["y"], raw["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    raw["intensity"] = rng.uniform(1.0, 200.0, n)
    # ring-major like the driver's grid: timestamps repeat across the rings
    raw["t"] = np.tile(np.asarray(unique_ns, np.uint32), per_ts)
    raw["ring"] = np.repeat(np.arange(per_ts), len(unique_ns)).astype(np.uint16)
    return raw
