"""CPU: odometry::Manager of the C++ host mirror (mimosa_amd/host/mimosa_hip/odometry.hpp) through
tests/cpp/odometry_manager.cpp — the mirror of the reference's odometry manager (src/odometry/manager.cpp:22-67,
include/mimosa/odometry/utils.hpp:19-32) without ROS.

D-optimality exp(log(pow(det, 1/6))) against numpy on diagonal and dense covariances: 1e-12 relative (a 6 x 6 elimination with
partial pivoting against LAPACK's, covariances of condition up to 1e4).  The quirk of a negative determinant (NaN, which passes
the gate), the gate itself (a rejected message does not advance the previous pose), the conjugation by T_B_S, the
first-message rule, the emitted keys and sigmas, and the window edge made from the same measurement: exact, or 1e-14 where a
product of rotations is restated in numpy."""
import json
import os
import subprocess

import numpy as np
import pytest

import window_lin_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = lambda j: (ord("x") << 56) | j  # noqa: E731


@pytest.fixture(scope="module")
def exe():
    from mimosa_amd import build
    return build.build_odometry_test()


def run(exe, msgs, T_B_S=(np.eye(3), np.zeros(3)), thresh=1.0, sigma_rot_deg=1.0, sigma_trans_m=0.5):
    vals = [thresh, sigma_rot_deg, sigma_trans_m] + list(T_B_S[0].ravel()) + list(T_B_S[1]) + [len(msgs)]
    for key, T, cov in msgs:
        vals += [key] + list(T[0].ravel()) + list(T[1]) + list(np.asarray(cov, float).ravel())
    out = subprocess.run([exe], input=" ".join(repr(float(v)) for v in vals), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def pose(rng, rot=0.5, trans=2.0):
    return ref.exp_so3(rng.standard_normal(3) * rot), rng.standard_normal(3) * trans


def dense_cov(rng, lo=1e-4, hi=1.0):
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    return (Q * np.logspace(np.log10(lo), np.log10(hi), 6)) @ Q.T


def mul(A, B):
    return A[0] @ B[0], A[1] + A[0] @ B[1]


def inv(A):
    return A[0].T, -A[0].T @ A[1]


def test_d_optimality_against_numpy(exe):
    rng = np.random.default_rng(1)
    covs = [np.diag(rng.uniform(1e-4, 2.0, 6)) for _ in range(4)] + [dense_cov(rng) for _ in range(8)] + [np.eye(6) * 4.0]
    got = run(exe, [(k, pose(rng), c) for k, c in enumerate(covs)], thresh=1e9)
    for g, c in zip(got, covs):
        want = np.exp(np.log(np.linalg.det(c) ** (1.0 / 6.0)))
        assert abs(g["d_opt"] - want) <= 1e-12 * want, (g["d_opt"], want)
        assert abs(g["det"] - np.linalg.det(c)) <= 1e-12 * abs(np.linalg.det(c))
    assert abs(got[-1]["d_opt"] - 4.0) <= 1e-14


def test_negative_determinant_is_nan_and_passes_the_gate(exe):
    rng = np.random.default_rng(2)
    neg = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -2.0])
    got = run(exe, [(0, pose(rng), np.eye(6) * 0.1), (1, pose(rng), neg)], thresh=0.5)
    assert got[0]["outcome"] == "initialised"
    assert got[1]["det"] == -2.0 and np.isnan(got[1]["d_opt"]) and got[1]["outcome"] == "factor"


def test_gate_rejects_without_advancing_the_previous_pose(exe):
    rng = np.random.default_rng(3)
    T0, T1, T2 = pose(rng), pose(rng), pose(rng)
    ok, bad = np.eye(6) * 0.5, np.eye(6) * 1.5  # d_opt = 0.5 and 1.5 around a threshold of 1
    got = run(exe, [(0, T0, ok), (1, T1, bad), (2, T2, ok)])
    assert [g["outcome"] for g in got] == ["initialised", "rejected", "factor"]
    assert got[1]["d_opt"] > 1.0 >= got[2]["d_opt"]
    Z = mul(inv(T0), T2)  # from the last ACCEPTED pose, under its key
    assert np.abs(np.array(got[2]["R"]).reshape(3, 3) - Z[0]).max() <= 1e-14 and np.abs(np.array(got[2]["t"]) - Z[1]).max() <= 1e-14
    assert got[2]["key1"] == X(0) and got[2]["prev_key"] == 0 and got[2]["key2"] == X(0)
    # exactly at the threshold the message passes: the gate is strict
    got = run(exe, [(0, T0, np.eye(6)), (1, T1, np.eye(6))])
    assert [g["outcome"] for g in got] == ["initialised", "factor"]
    # a rejected first message does not initialise
    got = run(exe, [(0, T0, bad), (1, T1, ok), (2, T2, ok)])
    assert [g["outcome"] for g in got] == ["rejected", "initialised", "factor"] and got[2]["prev_key"] == 1


def test_measurement_is_conjugated_by_T_B_S(exe):
    rng = np.random.default_rng(4)
    T_B_S = pose(rng, 0.8, 0.3)
    Ts = [pose(rng) for _ in range(4)]
    got = run(exe, [(10 + k, T, np.eye(6) * 0.1) for k, T in enumerate(Ts)], T_B_S=T_B_S)
    assert got[0]["outcome"] == "initialised" and "R" not in got[0]
    for k in range(1, 4):
        want = mul(mul(mul(T_B_S, inv(Ts[k - 1])), Ts[k]), inv(T_B_S))
        assert np.abs(np.array(got[k]["R"]).reshape(3, 3) - want[0]).max() <= 1e-14
        assert np.abs(np.array(got[k]["t"]) - want[1]).max() <= 1e-13
        assert got[k]["key1"] == X(10 + k - 1) and got[k]["key2"] == X(0) and got[k]["dim"] == 6
    # with T_B_S = I the measurement is the sensor's own relative motion
    plain = run(exe, [(k, T, np.eye(6) * 0.1) for k, T in enumerate(Ts)])
    want = mul(inv(Ts[0]), Ts[1])
    assert np.abs(np.array(plain[1]["R"]).reshape(3, 3) - want[0]).max() <= 1e-14 and np.abs(np.array(plain[1]["t"]) - want[1]).max() <= 1e-14


def test_emitted_sigmas_and_the_window_edge(exe):
    rng = np.random.default_rng(5)
    got = run(exe, [(0, pose(rng), np.eye(6) * 0.1), (1, pose(rng), np.eye(6) * 0.1)], sigma_rot_deg=0.25, sigma_trans_m=0.125)[1]
    sr = 0.25 * np.pi / 180.0
    assert got["sigmas"] == [sr] * 3 + [0.125] * 3
    e = got["edge"]
    assert (e["a"], e["b"]) == (1, 3) and e["R"] == got["R"] and e["t"] == got["t"]
    assert np.array_equal(np.array(e["info"]).reshape(6, 6), np.diag([1.0 / (sr * sr)] * 3 + [1.0 / (0.125 * 0.125)] * 3))
    # the reference's defaults: 1 degree, 0.5 m
    got = run(exe, [(0, pose(rng), np.eye(6) * 0.1), (1, pose(rng), np.eye(6) * 0.1)])[1]
    assert got["sigmas"] == [np.pi / 180.0] * 3 + [0.5] * 3
