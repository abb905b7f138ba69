"""-m gpu: the photometric factor zoo (tests/photo_zoo.py) on the device, through capi.Photo and PhotoFactor.  Every scene is
preprocessed and linearized once (module fixture) and the multi-precision reference is evaluated on the images the DEVICE built.
Statuses, the centres' pixel, n_exceptions and status_hist are exact against the reference; every row of every Valid feature is
within the row bound (K_DEVICE), row by row; H_bb, b_b and f are held to math.fsum sums of the device's own reported rows, the
binary blocks to sums of the reference's rows with the row bound propagated, the unary V H V, b and localizabilities to the
reported blocks; linearize, linearize_async + wait, clone and photo_linearize_batch give identical bits, the batch mixing factors
of 1, 3, 4, 5 and all features (a factor of no features is refused at creation, as the reference's constructor throws).  No
oracle takes part.  The worst row ratio is printed (pytest -s); the measured figure is in photo_zoo's docstring and DESIGN.md."""
import numpy as np
import pytest

import photo_zoo as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zoo(ctx):
    from mimosa_amd import capi

    out, keep = {}, []
    for sc in Z.build():
        P = capi.Photo(ctx, sc.cfg)
        images, F, res, state = Z.run(P, sc)
        keep += [F, P]
        out[sc.name] = (sc, Z.reference(sc, images), res, state, P, F)
    yield out
    for o in keep:
        o.destroy()


def test_margins_hold_on_the_device_images(zoo):
    """the yaw table comes from another libm's atan2: the condition on the inputs is checked again on these images"""
    mg = Z.Margins()
    for sc, refs, *_ in zoo.values():
        mg.merge(Z.zoo_margins(sc, refs))
    assert mg.smallest() >= Z.MARGIN, mg
    recorded = {t for _, refs, *_ in zoo.values() for r in refs for t in r.tags}
    assert set(Z.REFERENCE_TAGS) <= recorded, set(Z.REFERENCE_TAGS) - recorded


@pytest.mark.parametrize("name", Z.SCENES)
def test_statuses_centres_counters(zoo, name):
    sc, refs, res, state, _, _ = zoo[name]
    Z.check_discrete(sc, refs, res, state, label=f"device {name}")


def test_rows_within_the_bound(zoo):
    worst = {}
    for name, (sc, refs, res, state, _, _) in zoo.items():
        if [r.status for r in refs] == state[0].tolist():
            worst[name] = Z.row_ratios(refs, state[2])
    print("[photo-zoo] device, worst row ratio per scene:", {k: round(v, 1) for k, v in worst.items()})
    for name, (sc, refs, res, state, _, _) in zoo.items():
        Z.row_ratios(refs, state[2], K=Z.K_DEVICE, label=f"device {name}")


@pytest.mark.parametrize("name", Z.SCENES)
def test_sums(zoo, name):
    sc, refs, res, state, _, _ = zoo[name]
    Z.check_sums(sc, refs, res, state, Z.K_DEVICE, label=f"device {name}")


def _same(a, b, label):
    for k in a:
        if k != "gpu_ms":
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (label, k)   # NaN: sqrt of a -0 eigenvalue under V S V^T


def _same_state(a, b, label):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), label
    v = a[0] == 8
    assert np.array_equal(a[1][v], b[1][v]), label


@pytest.mark.parametrize("name", ["identity5", "pose_missing5", "rows5_binary", "rows5_unary_vsvt", "rows8_unary"])
def test_async_and_clone_give_the_same_bits(zoo, name):
    sc, refs, res, state, P, F = zoo[name]
    F.linearize_async(*sc.pose)
    _same(F.wait(), res, f"{name} async")
    _same_state(F.state(), state, f"{name} async")
    C = F.clone()
    _same(C.linearize(*sc.pose), res, f"{name} clone")
    _same_state(C.state(), state, f"{name} clone")
    C.destroy()


@pytest.mark.parametrize("name", ["rows5_binary", "rows5_unary"])
def test_batch_of_unlike_sizes(zoo, name):
    """factors of 1, 3, 4, 5 and all features (kFeatPerBlock = 4: partial last blocks) of one Photo in one launch: each the bits of
    its own linearize, each held to the reference of its own features"""
    from mimosa_amd import capi

    sc, refs, res, state, P, F = zoo[name]
    with pytest.raises(capi.MhError):
        P.set_features([])
        P.make_factor(sc.VSVt, sc.binary)                  # "No features in a_features" (photometric_factor.hpp:94-96)
    subs = [idx for idx in sc.subsets if idx] + [list(range(len(sc.features)))]
    assert [len(s) for s in subs][:4] == [1, 3, 4, 5]
    factors = []
    for idx in subs:
        P.set_features([sc.features[i] for i in idx])
        factors.append(P.make_factor(sc.VSVt, sc.binary))
    n = len(factors)
    Rb, tb = np.stack([sc.pose[0]] * n), np.stack([sc.pose[1]] * n)
    Ra, ta = (np.stack([sc.pose[2]] * n), np.stack([sc.pose[3]] * n)) if sc.binary else (None, None)
    got = capi.photo_linearize_batch(factors, Rb, tb, Ra, ta)
    for idx, f, g in zip(subs, factors, got):
        sub, sub_refs = Z.subset(sc, idx), [refs[i] for i in idx]
        st = f.state()
        Z.check_discrete(sub, sub_refs, g, st, label=f"device batch {sub.name}")
        assert np.array_equal(st[2], state[2][idx]), sub.name              # a feature's rows do not depend on its company
        Z.check_sums(sub, sub_refs, g, st, Z.K_DEVICE, label=f"device batch {sub.name}")
        _same(f.linearize(*sc.pose), g, f"{sub.name} alone")
        _same_state(f.state(), st, f"{sub.name} alone")
    _same(got[-1], res, f"{name} whole")
    for f in factors:
        f.destroy()
    P.set_features(sc.features)
