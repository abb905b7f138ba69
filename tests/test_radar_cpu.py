"""CPU suite of the radar Doppler path (mh_radar_*): the ABI surface, struct layouts, the independent restatement's
Jacobians against finite differences, and the C++ host mirror's compilation.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import radar_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADAR_FUNCS = ["mh_radar_scan_create", "mh_radar_scan_destroy", "mh_radar_prepare_input", "mh_radar_get_targets",
               "mh_radar_factor_create", "mh_radar_factor_create_from_scan", "mh_radar_factor_clone", "mh_radar_factor_destroy",
               "mh_radar_factor_size", "mh_radar_factor_linearize", "mh_radar_factor_linearize_async", "mh_radar_factor_wait",
               "mh_radar_factor_linearize_batch", "mh_radar_factor_get_residuals"]


def header_functions():
    src = open(os.path.join(ROOT, "include", "mimosa_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_and_library_exports_the_radar_surface():
    from mimosa_amd import build, capi
    fns = header_functions()
    assert sorted(f for f in fns if f.startswith("mh_radar_")) == sorted(RADAR_FUNCS)
    L = C.CDLL(build.build())
    missing = [f for f in RADAR_FUNCS if not hasattr(L, f)]
    assert not missing, missing
    assert set(RADAR_FUNCS) <= set(capi.EXPORTS)
    assert L.mh_abi_version() == 3


def _compile(src, out, link=False):
    from mimosa_amd import build
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(ROOT, "mimosa_amd", "host", "gtsam_sig"),
           os.path.join(ROOT, "tests", "cpp", src), "-o", out]
    if link:
        lib = build.build()
        cmd += ["-L", os.path.dirname(lib), "-lmimosa_hip", "-lpthread", f"-Wl,-rpath,{os.path.dirname(lib)}"]
    subprocess.check_call(cmd)
    return out


def test_ctypes_structs_match_the_c_layout(tmp_path):
    from mimosa_amd import capi
    exe = _compile("radar_layout.cpp", str(tmp_path / "radar_layout"))
    c = json.loads(subprocess.check_output([exe]).decode())
    for name, cls in (("mh_radar_config", capi.RadarConfig), ("mh_radar_layout", capi.RadarLayout), ("mh_radar_target", capi.RadarTarget),
                      ("mh_radar_info", capi.RadarInfo), ("mh_radar_result", capi.RadarResult)):
        assert C.sizeof(cls) == c[name], name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == c[f"{name}.{f}"], (name, f)
    assert c["MH_RADAR_MAX_BATCH"] == capi.MH_RADAR_MAX_BATCH >= 256
    assert (c["MH_RADAR_RIO"], c["MH_RADAR_MMWAVE"], c["MH_RADAR_MMWAVE_DOPPLER_RESIDUAL"]) == (
        capi.MH_RADAR_RIO, capi.MH_RADAR_MMWAVE, capi.MH_RADAR_MMWAVE_DOPPLER_RESIDUAL)
    assert capi.RADAR_TARGET_DTYPE.itemsize == c["mh_radar_target"]


def _problem(seed, n=50):
    from mimosa_amd import synth_radar
    rng = np.random.default_rng(seed)
    st = synth_radar.random_state(rng)
    return synth_radar.random_targets(rng, n), st


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_jacobians_match_finite_differences(seed):
    """J1 / J2 / J3 against central differences of the UNWEIGHTED residual under GTSAM's retractions: R Exp(d) for the pose
    rotation, v + d for the velocity, b + d for the gyro bias.  Pins the sign conventions independently of the transcription."""
    from mimosa_amd.synth import so3_exp
    tg, s = _problem(seed)
    args = (tg, s["R_B_S"], s["t_B_S"], s["omega"])
    J1, J2, J3 = radar_ref.jacobians(tg, s["R_B_S"], s["t_B_S"], s["R_W_B"], s["v_W"])
    h = 1e-6
    fd1, fd2, fd3 = np.zeros((len(tg), 3)), np.zeros((len(tg), 3)), np.zeros((len(tg), 3))
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        e = lambda R, v, b: radar_ref.residuals_unweighted(*args, R, v, b)  # noqa: E731
        fd1[:, k] = (e(s["R_W_B"] @ so3_exp(d), s["v_W"], s["bias_gyro"]) - e(s["R_W_B"] @ so3_exp(-d), s["v_W"], s["bias_gyro"])) / (2 * h)
        fd2[:, k] = (e(s["R_W_B"], s["v_W"] + d, s["bias_gyro"]) - e(s["R_W_B"], s["v_W"] - d, s["bias_gyro"])) / (2 * h)
        fd3[:, k] = (e(s["R_W_B"], s["v_W"], s["bias_gyro"] + d) - e(s["R_W_B"], s["v_W"], s["bias_gyro"] - d)) / (2 * h)
    for J, fd in ((J1[:, 0:3], fd1), (J2, fd2), (J3[:, 3:6], fd3)):
        assert np.linalg.norm(J - fd) <= 1e-6 * np.linalg.norm(fd)
    assert not J1[:, 3:6].any() and not J3[:, 0:3].any()


def test_restatement_structural_zeros_and_symmetry():
    tg, s = _problem(7, 200)
    r = radar_ref.linearize(tg, s["R_B_S"], s["t_B_S"], s["omega"], 0.1, s["R_W_B"], s["v_W"], s["bias_gyro"])
    assert not r["G11"][3:, :].any() and not r["G11"][:, 3:].any()
    assert not r["G12"][3:, :].any() and not r["G13"][3:, :].any() and not r["G13"][:, :3].any()
    assert not r["G23"][:, :3].any() and not r["G33"][:3, :].any() and not r["G33"][:, :3].any()
    assert not r["g1"][3:].any() and not r["g3"][:3].any()
    for k in ("G11", "G22", "G33"):
        np.testing.assert_allclose(r[k], r[k].T, rtol=0, atol=1e-12 * np.abs(r[k]).max())
    z = radar_ref.linearize(np.zeros((0, 8)), s["R_B_S"], s["t_B_S"], s["omega"], 0.1, s["R_W_B"], s["v_W"], s["bias_gyro"])
    assert z["f"] == 0.0 and not z["G11"].any() and not z["g2"].any()


def test_host_mirror_compiles_against_gtsam_sig(tmp_path):
    """radar.hpp and tests/cpp/radar_pipeline.cpp compile warning-free against host/gtsam_sig; the mirror stays free of the
    spellings test_host_mirror_is_written_against_gtsam_headers forbids."""
    assert os.path.exists(_compile("radar_pipeline.cpp", str(tmp_path / "radar_pipeline"), link=True))
    src = open(os.path.join(ROOT, "mimosa_amd", "host", "mimosa_hip", "radar.hpp")).read()
    assert "MIMOSA_HIP_WITH_GTSAM" not in src and "atPose3" not in src and "gravityUnit" not in src
    assert "c.at<Pose3>(keys()[0])" in src and "c.at<gtsam::imuBias::ConstantBias>(keys()[2])" in src
