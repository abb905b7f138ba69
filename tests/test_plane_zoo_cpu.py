"""The neighbourhood zoo (tests/plane_zoo.py) on the CPU oracle (oracle/ref_cpu.hpp): every case's status, mean and normal within
the zoo's bounds of the mpmath reference.  This validates the generator and the reference without a GPU, and it is where the
layout rules run: every map point survives the insert, every point and query keeps its margin from the voxel faces, no cluster
reaches another query's 27 voxels, at most 1 % of a zoo is ambiguous and nothing in valid, pair or iso.  The worst error / bound
per family is printed (pytest -s) and recorded in plane_zoo's docstring.  tests/test_gpu_plane_zoo.py runs the same checks on
the device."""
import numpy as np
import pytest

import plane_zoo as Z

ALL_ZOOS = Z.K5_ZOOS + Z.K8_ZOOS + Z.K4_ZOOS
WARM_ZOOS = tuple(z for z in Z.K5_ZOOS if z[1] == 19)
SUMS_ZOOS = tuple(z for z in Z.K5_ZOOS if z[2] == 0.0)


@pytest.fixture(scope="module")
def make():
    from oracle import ref_cpu

    maps = {}

    def _make(zoo, idx, far=False, warm=False, huber=1, binary=False, pts=None):
        key = (zoo.k, zoo.mode, zoo.offset)
        if key not in maps:
            maps[key] = ref_cpu.Map(leaf=Z.LEAF, min_dist=0.0, mode=zoo.mode)
            maps[key].insert(zoo.map_xyz)
            assert maps[key].num_points == len(zoo.map_xyz)  # every map point is present
        return ref_cpu.ICP(maps[key], zoo.pts[idx] if pts is None else pts, ref_cpu.make_config(**Z.config(zoo.k, far, warm, huber)), binary=binary)

    return _make


@pytest.mark.parametrize("key", ALL_ZOOS)
def test_zoo_layout_and_ambiguity(key):
    zoo = Z.build(*key)  # asserts margins, isolation, the per-voxel cap and the ambiguity rule
    ref = Z.reference(*key, 0)
    assert zoo.n == Z.N_CASES == 176 and not ref.knn_open.any()
    assert ref.ambiguous.sum() <= 0.01 * zoo.n
    for fam in ("valid", "pair", "iso"):
        assert not ref.ambiguous[zoo.family == Z.FAMILIES.index(fam)].any()
    fam = lambda name: ref.status[zoo.family == Z.FAMILIES.index(name)]  # noqa: E731
    assert np.all(fam("few") == 1) and np.all(np.isin(fam("flat"), (1, 4))) and np.all(np.isin(fam("duplicates"), (1, 4)))
    # every family in every placement
    assert len(set(zip(zoo.family.tolist(), zoo.placement.tolist()))) == len(Z.FAMILIES) * len(Z.PLACEMENTS)
    print(key, "status histogram", np.bincount(ref.status, minlength=9).tolist(), "ambiguous", int(ref.ambiguous.sum()),
          "normal determined", int((ref.nb <= Z.NORMAL_DETERMINED).sum()))


@pytest.mark.parametrize("zoos", (Z.K5_ZOOS, Z.K8_ZOOS, Z.K4_ZOOS))
def test_gate_families_reach_both_sides(zoos):
    """Over the zoos of one k, every family built next to a gate has cases on both sides of it."""
    for name, both in (("low", (4, 8)), ("line", (5, 8)), ("gate", (6, 8)), ("maxerr", (7, 8)), ("far", (2, 8))):
        st = np.concatenate([Z.reference(*key, 0).status[Z.build(*key).family == Z.FAMILIES.index(name)] for key in zoos])
        assert all(s in st for s in both), (name, np.bincount(st, minlength=9).tolist())


_worst = {}


@pytest.mark.parametrize("key", ALL_ZOOS)
def test_oracle_cold(make, key):
    r = Z.check_cold(make, key, label="oracle ")
    if key in Z.K5_ZOOS:
        Z.merge_ratios(_worst, r)
        print(Z.format_ratios(_worst, "oracle, k = 5 so far"))


@pytest.mark.parametrize("key", Z.K5_ZOOS)
def test_oracle_binary(make, key):
    Z.check_cold(make, key, binary=True, label="oracle binary ")


@pytest.mark.parametrize("key", WARM_ZOOS)
def test_oracle_warm(make, key):
    Z.check_warm(make, key, label="oracle warm ")


@pytest.mark.parametrize("huber", (0, 1))
@pytest.mark.parametrize("key", SUMS_ZOOS)
def test_oracle_sums(make, key, huber):
    Z.check_sums(make, key, huber, label="oracle sums ")
