"""-m gpu: the neighbourhood zoo (tests/plane_zoo.py) on the device: status, mean and normal of every designed case after
capi.ICPFactor(...).linearize, read back with state(), within the zoo's bounds of the mpmath reference (status exact, mean
4 eps |mean|, normal 4 delta / gap + 8 eps).  Unlike the parity and fuzz tests no oracle takes part and the spectra are chosen,
not drawn: this is where plane_eigen / null_vector3 (device branches of math3.hpp), the kFast plane fit, the lane merges of the
2- and 4-lane classes and every gate of K3 are held to an independent answer.  tests/test_plane_zoo_cpu.py runs the same checks
on the CPU oracle.  The worst error / bound per family is printed (pytest -s); the measured figures are in DESIGN.md.

k = 5 runs K3's kFast form in the two-lanes-per-point class; k = 8 and k = 4 the generic K = 8 instantiation; the batch test
icp_linearize_batch_kernel; the workers the one- and four-lane classes; the tiled cloud (65 600 points) the 512-thread class."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_zoo as Z

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE19 = tuple(z for z in Z.K5_ZOOS if z[1] == 19)
SUMS_ZOOS = tuple(z for z in Z.K5_ZOOS if z[2] == 0.0)


@pytest.fixture(scope="module")
def make(ctx):
    from mimosa_amd import capi

    maps, factors = {}, []

    def _make(zoo, idx, far=False, warm=False, huber=1, binary=False, pts=None):
        key = (zoo.k, zoo.mode, zoo.offset)
        if key not in maps:
            maps[key] = capi.VoxelMap(ctx, leaf=Z.LEAF, min_dist=0.0, mode=zoo.mode)
            maps[key].insert(zoo.map_xyz)
            assert maps[key].stats()["n_points"] == len(zoo.map_xyz)  # every map point is present
        f = capi.ICPFactor(ctx, maps[key], zoo.pts[idx] if pts is None else pts, capi.make_reg_config(**Z.config(zoo.k, far, warm, huber)), binary=binary)
        factors.append(f)
        return f

    yield _make
    for f in factors:
        f.destroy()
    for m in maps.values():
        m.release()


@pytest.mark.parametrize("key", Z.K5_ZOOS)
def test_k5_unary(make, key):
    Z.check_cold(make, key, label="device ")


@pytest.mark.parametrize("key", Z.K5_ZOOS)
def test_k5_binary(make, key):
    Z.check_cold(make, key, binary=True, label="device binary ")


@pytest.mark.parametrize("key", Z.K8_ZOOS + Z.K4_ZOOS)
def test_generic_k(make, key):
    Z.check_cold(make, key, label="device ")


@pytest.mark.parametrize("key", MODE19)
def test_linearize_batch(make, key):
    from mimosa_amd import capi

    Z.check_cold(make, key, batch=capi.linearize_batch, label="device batch ")


def _worker(tmp_path, tag, env):
    out = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plane_zoo_worker.py"), out], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:]
    return np.load(out)


@pytest.mark.parametrize("tag,env", (("one-lane", {"MH_QL2_MAX": "0", "MH_QL4_MAX": "0"}),
                                     ("four-lane", {"MH_QL2_MAX": "32768", "MH_QL4_MAX": "32768"})))
def test_lane_classes(tmp_path, tag, env):
    blob = _worker(tmp_path, tag, env)
    ratios = {}
    for zi, key in enumerate(Z.K5_ZOOS):
        zoo, ref = Z.build(*key), Z.reference(*key, 0)
        for name, idx in zoo.clouds.items():
            Z.merge_ratios(ratios, Z.check_state(zoo, ref, idx, [blob[f"z{zi}_{name}_{i}"] for i in range(3)], True, f"{tag} {name}"))
    print(Z.format_ratios(ratios, f"device {tag} class, k 5, all zoos"))


@pytest.mark.parametrize("key", MODE19)
def test_tiled_cloud_runs_the_512_thread_class(make, key):
    Z.check_tiled(make, key, label="device tiled ")


@pytest.mark.parametrize("key", MODE19)
def test_warm_path(make, key):
    Z.check_warm(make, key, label="device warm ")


@pytest.mark.parametrize("huber", (0, 1))
@pytest.mark.parametrize("key", SUMS_ZOOS)
def test_sums(make, key, huber):
    Z.check_sums(make, key, huber, label="device sums ")
