"""-m gpu: the 512-thread one-lane-per-point class of K3 at its smallest shapes.  In that class a wave sets its issue priority
from the work it has left (icp_kernels.hip, K3Prio).  Priority moves time only and cannot change a result; what these tests hold
is the code around it — wave-wide votes over partly empty waves, scalar code inside divergent regions — where it is most
exposed: 65 537 points are the first size that takes the class, the grid is padded to 136 workgroups, so the launch holds whole
empty workgroups, empty waves and one wave with a single live lane.
  * one factor, cold and after a small pose step, against the CPU oracle: status histogram equal, per-point state <= 1e-9,
    H / b / f relative <= 1e-12
  * the same cold call five times: every field of the result and the per-point state equal to the bit (the summation order is
    fixed)
  * a window of 40 000 + 25 600 + 333 points (65 933 in all: every member runs the 512-thread class) against each member's own
    call: per-point state identical to the bit, sums to 1e-12 ("K3b / K4b"), k-NN counters equal."""
import numpy as np
import pytest

from parity import assert_result_parity, assert_state_parity, rel

pytestmark = pytest.mark.gpu

N_ONE = 65537
SIZES = (40000, 25600, 333)


@pytest.fixture(scope="module")
def world():
    from mimosa_amd import synth

    rooms = [xyz for _, _, xyz in synth.make_map_rooms(1, 1)]
    pts, _ = synth.make_scan(65)
    assert len(pts) >= max(N_ONE, sum(SIZES))
    R, t = synth.query_pose()
    return dict(rooms=rooms, pts=pts, R=R, t=t, cfg=synth.enwide_config())


@pytest.fixture(scope="module")
def gmap(ctx, world):
    from mimosa_amd import capi

    gm = capi.VoxelMap(ctx)
    for xyz in world["rooms"]:
        gm.insert(xyz)
    yield gm
    gm.release()


def _hold_to_oracle(got, ref, what):
    figs = {k: rel(got[k], ref[k]) for k in ("H_ss", "b_s")}
    figs["f"] = abs(got["f"] - ref["f"]) / max(abs(ref["f"]), 1e-300)
    print(what, "relative to the oracle:", {k: f"{v:.2e}" for k, v in figs.items()}, "status_hist", got["status_hist"].tolist())
    assert np.array_equal(got["status_hist"], ref["status_hist"]), (what, got["status_hist"], ref["status_hist"])
    for k, v in figs.items():
        assert v <= 1e-12, (what, k, v)
    assert_result_parity(got, ref)


def test_first_size_of_the_class_against_the_oracle(ctx, world, gmap):
    from mimosa_amd import capi, synth
    from oracle import ref_cpu

    pts = np.ascontiguousarray(world["pts"][:N_ONE])
    rm = ref_cpu.Map()
    for xyz in world["rooms"]:
        rm.insert(xyz)
    gf = capi.ICPFactor(ctx, gmap, pts, capi.make_reg_config(**world["cfg"]))
    rf = ref_cpu.ICP(rm, pts, ref_cpu.make_config(**world["cfg"]))
    R, t = world["R"], world["t"]
    got = gf.linearize(R, t)  # cold: every point runs the k-NN
    assert got["n_knn"] == N_ONE
    _hold_to_oracle(got, rf.linearize(R, t), "cold")
    assert_state_parity(gf.state(), rf.state(), tol=1e-9)
    # a step around the re-association threshold (0.0375 m): 0.015 m of translation and 1 mrad of rotation at ranges of 24-44 m
    # move ~27 600 of the points past it — in most waves some lanes run the k-NN again and the others reuse their plane
    R2, t2 = R @ synth.so3_exp(np.array([0.0003, -0.0002, 0.001])), t + np.array([0.012, -0.009, 0.003])
    got = gf.linearize(R2, t2)
    assert 0 < got["n_knn"] < N_ONE
    _hold_to_oracle(got, rf.linearize(R2, t2), "after a pose step")
    assert_state_parity(gf.state(), rf.state(), tol=1e-9)
    gf.destroy()


def test_cold_call_repeats_to_the_bit(ctx, world, gmap):
    from mimosa_amd import capi

    pts = np.ascontiguousarray(world["pts"][:N_ONE])
    gf = capi.ICPFactor(ctx, gmap, pts, capi.make_reg_config(**world["cfg"]))
    first, first_state = None, None
    for rep in range(5):
        gf.reset()
        got, state = gf.linearize(world["R"], world["t"]), gf.state()
        if first is None:
            first, first_state = got, state
            continue
        for k in got:
            if k.startswith("gpu_ms") or k == "linearize_count":  # timings, and the factor's running call count
                continue
            assert np.array_equal(np.asarray(got[k]), np.asarray(first[k]), equal_nan=True), (rep, k)
        for a, b in zip(state, first_state):
            assert np.array_equal(a, b, equal_nan=True), rep
    gf.destroy()


def test_window_members_equal_their_own_calls(ctx, world, gmap):
    from mimosa_amd import capi, synth

    cfg = capi.make_reg_config(**world["cfg"])
    bounds = np.concatenate([[0], np.cumsum(SIZES)])
    subs = [np.ascontiguousarray(world["pts"][bounds[i]:bounds[i + 1]]) for i in range(len(SIZES))]
    fa = [capi.ICPFactor(ctx, gmap, s, cfg) for s in subs]
    fb = [capi.ICPFactor(ctx, gmap, s, cfg) for s in subs]
    Rs = [world["R"] @ synth.so3_exp(np.array([0.001 * i, -0.0007 * i, 0.002 * i])) for i in range(len(SIZES))]
    ts = [world["t"] + np.array([0.01 * i, -0.004 * i, 0.002 * i]) for i in range(len(SIZES))]
    got = capi.linearize_batch(fa, Rs, ts)
    for i, n in enumerate(SIZES):
        one = fb[i].linearize(Rs[i], ts[i])
        for x, y in zip(fa[i].state(), fb[i].state()):
            assert np.array_equal(x, y, equal_nan=True), n
        for k in ("status_hist", "n_knn", "mean_candidates", "n_exact_fallback"):
            assert np.array_equal(np.asarray(got[i][k]), np.asarray(one[k])), (n, k)
        assert got[i]["n_knn"] == n
        for k in ("H_ss", "b_s", "loc_trans_comp", "loc_rot_comp"):
            assert rel(got[i][k], one[k]) <= 1e-12, (n, k, rel(got[i][k], one[k]))
        assert abs(got[i]["f"] - one["f"]) <= 1e-12 * abs(one["f"]), n
    for f in fa + fb:
        f.destroy()
