"""CPU suite of the device-side deskew poses (mh_scan_deskew_imu, mh_scan_get_deskew_poses, mh_photo_preprocess_scan[_begin]_resident):
the ABI surface, argument checks that need no device, and the C++ host mirror's segment builder against the intervals
oracle/numpy_ref.py: deskew_poses walks.  No GPU.  (A scan object cannot exist without a context, so "never prepared" is checked
on a real scan in tests/test_gpu_deskew_imu.py.)"""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np

import deskew_imu_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCS = ["mh_scan_deskew_imu", "mh_scan_get_deskew_poses", "mh_photo_preprocess_scan_resident", "mh_photo_preprocess_scan_begin_resident"]




def test_header_declares_and_library_exports_the_four_entry_points():
    from mimosa_amd import build, capi
    src = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    fns = set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", src))
    assert set(NEW_FUNCS) <= fns
    L = C.CDLL(build.build())
    missing = [f for f in NEW_FUNCS if not hasattr(L, f)]
    assert not missing, missing
    assert set(NEW_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3
    assert capi.IMU_SEGMENT_DTYPE.itemsize == 23 * 8 and capi.MH_MAX_IMU_SEGMENTS == 64


def test_bad_arguments_are_refused_without_a_device():
    from mimosa_amd import build, capi
    L = C.CDLL(build.build())
    vp, sz = C.c_void_p, C.c_size_t
    L.mh_scan_deskew_imu.argtypes = [vp, vp, sz, C.c_double, vp, vp, vp, vp, vp]
    L.mh_scan_get_deskew_poses.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.mh_photo_preprocess_scan_resident.argtypes = [vp, vp]
    L.mh_photo_preprocess_scan_begin_resident.argtypes = [vp, vp]
    L.mh_last_error.restype = C.c_char_p
    L.mh_last_error.argtypes = [vp]
    seg = np.zeros(65, capi.IMU_SEGMENT_DTYPE)
    d = np.zeros(9)
    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    assert L.mh_scan_deskew_imu(None, p(seg), 1, 0.0, p(d), p(d), p(d), p(d), p(d)) == capi.MH_ERR_INVALID_ARG
    assert b"NULL argument" in L.mh_last_error(None)
    # more than MH_MAX_IMU_SEGMENTS is refused before anything else is looked at
    assert L.mh_scan_deskew_imu(None, p(seg), 65, 0.0, p(d), p(d), p(d), p(d), p(d)) == capi.MH_ERR_UNSUPPORTED
    assert b"64" in L.mh_last_error(None)
    n = sz()
    assert L.mh_scan_get_deskew_poses(None, None, 0, C.byref(n)) == capi.MH_ERR_INVALID_ARG
    assert L.mh_photo_preprocess_scan_resident(None, None) == capi.MH_ERR_INVALID_ARG
    assert L.mh_photo_preprocess_scan_begin_resident(None, None) == capi.MH_ERR_INVALID_ARG


def _exe(name, tmp_path):
    from mimosa_amd import build
    lib = build.build()
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(ROOT, "mimosa_amd", "host", "gtsam_sig"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", os.path.dirname(lib), "-lmimosa_hip", "-lpthread",
                           f"-Wl,-rpath,{os.path.dirname(lib)}"])
    return exe


def _write_inputs(path, c):
    n_imu = len(c["imu_t"])
    with open(path, "wb") as f:
        def w(a, dt):
            a = np.ascontiguousarray(a, dtype=dt)
            f.write(struct.pack("<Q", a.size))
            f.write(a.tobytes())
        w(c["imu_t"], np.float64)
        w(np.concatenate([c["acc"], c["gyro"]], 1), np.float64)
        w(np.concatenate([np.reshape(c["nav_R"], (n_imu, 9)), np.array(c["nav_p"]), np.array(c["nav_v"])], 1), np.float64)
        w(np.concatenate([c["bias_a"], c["bias_g"], c["g_unit"], [c["g_norm"], c["header_ts"]], c["T_B_S"][0].ravel(), c["T_B_S"][1]]), np.float64)
        w(c["unique_ns"], np.uint32)


def test_host_mirror_compiles_and_builds_the_oracles_intervals(tmp_path):
    """lidar.hpp (deskewPointsFromImu, imuSegments) and photometric.hpp (preprocessResident) compile warning-free against
    host/gtsam_sig; imuSegments gives, for the inputs of test_deskew_poses_match_numpy, exactly the (t0, t1, R, p, v, acc, omega)
    the oracle's loop uses for interval c: imu_t[c], imu_t[c + 1], nav[c], measurement c minus the bias."""
    c = dc.small_case()
    inp = tmp_path / "in.bin"
    _write_inputs(inp, c)
    out = subprocess.run([_exe("imu_segments", tmp_path), str(inp)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = np.array(json.loads(out.stdout))
    m = len(c["imu_t"])
    assert got.shape == (m - 1, 23)
    for j in range(m - 1):
        want = np.concatenate([[c["imu_t"][j], c["imu_t"][j + 1]], np.asarray(c["nav_R"][j]).ravel(), c["nav_p"][j], c["nav_v"][j],
                               c["acc"][j] - c["bias_a"], c["gyro"][j] - c["bias_g"]])
        assert np.array_equal(got[j], want), j
    from mimosa_amd import capi
    seg = dc.call_args(c)[0]                       # the Python builder makes the same records
    assert np.array_equal(seg.view(np.float64).reshape(-1, 23), got)
    assert capi.imu_segments(c["imu_t"][:1], c["acc"][:1], c["gyro"][:1], c["nav_R"][:1], c["nav_p"][:1], c["nav_v"][:1]).shape == (0,)
    src = open(os.path.join(ROOT, "mimosa_amd", "host", "mimosa_hip", "lidar.hpp")).read()
    assert "mh_scan_deskew_imu" in src and "deskewPointsFromImu" in src
    assert "preprocessResident" in open(os.path.join(ROOT, "mimosa_amd", "host", "mimosa_hip", "photometric.hpp")).read()


def test_cloud_of_the_gpu_test_stays_far_below_the_one_percent_cap(tmp_path):
    """The end-to-end GPU test allows 1 % of the points to differ in the last bit from numpy_ref.deskew run with the oracle's
    poses.  Here the HOST MIRROR's poses (tests/cpp/deskew_poses.cpp: computeDeskewPoses, glibc's sin / cos) stand in for the
    device's, on both clouds of that test: they differ from the oracle's by ~1e-15, f32 spacing is ~1e-7 relative, so a cast
    flips for about one entry in 1e5 or fewer.  Asserted: under a tenth of the cap (0.1 % of the points), and every difference
    within one ulp — the cap is not what makes the GPU test pass."""
    from oracle import numpy_ref
    exe = _exe("deskew_poses", tmp_path)
    for name, make, per_ts in (("small", dc.small_case, 64), ("per_point", dc.per_point_case, 1)):
        c = make()
        inp = tmp_path / (name + ".bin")
        _write_inputs(inp, c)
        out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        mirror = np.array(json.loads(out.stdout))
        want = dc.oracle_poses(c)
        assert mirror.shape == want.shape
        assert np.abs(mirror[:, :9] - want[:, :9]).max() < 1e-12 and np.abs(mirror[:, 9:] - want[:, 9:]).max() < 1e-11
        raw = dc.raw_cloud(c["unique_ns"], per_ts)
        xyz = np.stack([raw["x"], raw["y"], raw["z"]], 1)
        a = numpy_ref.deskew(xyz, raw["t"], c["unique_ns"], want.astype(np.float32))
        b = numpy_ref.deskew(xyz, raw["t"], c["unique_ns"], mirror.astype(np.float32))
        share = float(np.any(a != b, axis=1).mean())
        print(f"{name}: {share:.2e} of {len(a)} points differ between the mirror's and the oracle's poses")
        assert share < 1e-3
        assert np.all(np.abs(a - b) <= np.spacing(np.abs(a)))


def test_python_replay_refuses_device_poses_on_a_backend_without_a_device_table():
    import dataclasses
    import pytest
    from mimosa_amd import replay

    class NoTable:
        pass

    cfg = replay.ReplayConfig(n_scans=2, rows=64, cols=512, device_poses=True)
    with pytest.raises(ValueError):
        replay.run(cfg, NoTable(), scans=[])
    assert dataclasses.replace(cfg, device_poses=False).device_poses is False    # off is the default path
    assert replay.ReplayConfig().device_poses is False
