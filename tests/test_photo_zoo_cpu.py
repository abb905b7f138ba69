"""The photometric factor zoo (tests/photo_zoo.py) on the CPU oracle (oracle/photo_ref.hpp): the zoo builds, every decision of
the multi-precision reference keeps its distance from the tie, every designed and every recorded tag occurs, the oracle's statuses
and exception counters equal the reference's for every feature, and every row of every Valid feature is within the row bound.
This validates the builder and the reference without a GPU; tests/test_gpu_photo_zoo.py runs the same zoo on the device.  The
worst row ratio per scene is printed (pytest -s) and recorded in photo_zoo's docstring and DESIGN.md."""
import numpy as np
import pytest

import photo_zoo as Z


@pytest.fixture(scope="module")
def zoo():
    """every scene through the oracle once, the reference once (on the oracle's images)"""
    from oracle import photo_ref

    out = []
    for sc in Z.build():
        images, F, res, state = Z.run(photo_ref.Photo(sc.cfg), sc)
        out.append((sc, Z.reference(sc, images), res, state))
    return out


def test_margins_hold(zoo):
    """a condition on the inputs: no feature is left out, only the designed tie (the (-r, 0, 0) point) is exempt"""
    mg = Z.Margins()
    for sc, refs, _, _ in zoo:
        assert len(refs) == len(sc.features) == len(sc.designed)
        assert all(sc.designed[i] in ("throw_first", "throw_after_fail") for i in sc.expect)
        mg.merge(Z.zoo_margins(sc, refs))
    print({k: (f"{d:.3g}", w) for k, (d, w) in mg.items()})
    assert set(mg) == {"pixel", "rad", "deg", "m", "1", "ulp_f32"}
    assert mg.smallest() >= Z.MARGIN, mg


def test_every_tag_occurs(zoo):
    designed = {t for sc, _, _, _ in zoo for t in sc.designed}
    recorded = {t for _, refs, _, _ in zoo for r in refs for t in r.tags}
    assert designed == set(Z.DESIGNED_TAGS), (designed ^ set(Z.DESIGNED_TAGS))
    assert set(Z.REFERENCE_TAGS) <= recorded, set(Z.REFERENCE_TAGS) - recorded
    hist = np.bincount([r.status for _, refs, _, _ in zoo for r in refs], minlength=9)
    assert all(hist[s] > 0 for s in (1, 2, 4, 5, 6, 7, 8)) and hist[0] == 0 and hist[3] == 0, hist.tolist()
    sizes = {len(s) for sc, _, _, _ in zoo for s in sc.subsets}
    assert {0, 1, 3, 4, 5} <= sizes
    assert any(sc.VSVt is not None for sc, _, _, _ in zoo) and {sc.binary for sc, _, _, _ in zoo} == {True, False}
    assert {len(sc.features[0]["Le_ps"]) for sc, _, _, _ in zoo} == {25, 64}


def test_designed_outcomes(zoo):
    """what each design is for, read off the reference: the failing point's index, the exception, the side of the threshold"""
    want = {"valid": (8, None), "valid_low_contrast": (8, None), "range_far": (2, 1), "range_near": (2, 1), "range_at_0": (2, 1), "range_at_mid": (2, 13),
            "range_at_last": (2, None), "seam_low": (1, 1), "seam_high": (1, 1), "theta_above": (1, 1), "theta_below": (1, 1), "throw_first": (1, 1),
            "throw_after_fail": (2, 4), "first_fail_range": (2, 4), "first_fail_mask": (4, 4), "empty_search": (8, None), "empty_column": (1, 1),
            "dup_vote": (8, None), "dup_tie": (8, None), "mask": (4, 1), "margin": (5, 1), "margin_pass": (8, None), "occlusion": (6, 1),
            "occlusion_pass": (8, None), "maxerr_negated": (7, None), "maxerr_permuted": (7, None), "footprint": (8, None), "second_project_false": (1, 1)}
    need = {"seam_low": "ref_seam", "seam_high": "ref_seam", "theta_above": "ref_theta", "theta_below": "ref_theta", "empty_search": "ref_empty_search",
            "empty_column": "ref_empty_column", "dup_vote": "ref_dup_vote", "dup_tie": "ref_dup_tie", "footprint": "ref_footprint",
            "second_project_false": "second_project_false", "throw_first": "ref_throw_project"}
    for sc, refs, _, _ in zoo:
        exp = Z.expected(sc, refs)
        for i, (tag, r) in enumerate(zip(sc.designed, refs)):
            if tag == "pose_missing":
                continue
            st, n_eval = want[tag]
            assert exp[i][0] == st and (n_eval is None or r.n_eval == n_eval), (sc.name, i, tag, exp[i], r.n_eval)
            assert tag not in need or need[tag] in r.tags, (sc.name, i, tag, r.tags)
            if tag == "range_at_last":
                assert r.n_eval == r.m
        if sc.name == "pose_missing5":
            thrown = [e[1] == "pose" for e in exp]
            assert 0 < sum(thrown) < len(exp) and all(e[0] == (1 if t else 8) for e, t in zip(exp, thrown))
    # the lowest-contrast Valid feature is the worst conditioned
    k = {t: r.kappa for sc, refs, _, _ in zoo if sc.name == "identity5" for t, r in zip(sc.designed, refs) if r.status == 8}
    assert k["valid_low_contrast"] == max(k.values())


def test_oracle_statuses_and_counters(zoo):
    for sc, refs, res, state in zoo:
        Z.check_discrete(sc, refs, res, state, label=f"oracle {sc.name}")


def test_oracle_rows_within_the_bound(zoo):
    worst = {}
    for sc, refs, res, state in zoo:
        worst[sc.name] = Z.row_ratios(refs, state[2], K=Z.K_ORACLE, label=f"oracle {sc.name}")
    print("[photo-zoo] oracle, worst row ratio per scene:", {k: round(v, 1) for k, v in worst.items()})
    assert 8 * max(worst.values()) <= Z.K_DEVICE                      # the device's bound is still eight times what the oracle needs


def test_oracle_sums(zoo):
    """the aggregate checks of the GPU module, on the oracle (sequential sums: the same bounds hold)"""
    for sc, refs, res, state in zoo:
        Z.check_sums(sc, refs, res, state, Z.K_ORACLE, label=f"oracle {sc.name}")


def test_oracle_factor_sizes(zoo):
    """factors of 0, 1, 3, 4 and 5 features: per-feature results do not depend on the company they keep"""
    from oracle import photo_ref

    for sc, refs, _, state in zoo:
        for idx in sc.subsets:
            sub = Z.subset(sc, idx)
            _, F, res, st = Z.run(photo_ref.Photo(sub.cfg), sub)
            sub_refs = [refs[i] for i in idx]
            Z.check_discrete(sub, sub_refs, res, st, label=f"oracle {sub.name}")
            assert np.array_equal(st[2], state[2][idx])
            Z.check_sums(sub, sub_refs, res, st, Z.K_ORACLE, label=f"oracle {sub.name}")
