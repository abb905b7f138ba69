"""-m gpu: ICPFactor::linearize on the device (K3 / K4, icp_kernels.hip, through the C ABI) held to finite differences of the
cost it reports itself and to exact identities between its outputs.  NO ORACLE takes part: f and the factor come from the same
call of the same kernels, so a misreading shared by the device code, oracle/ref_cpu.hpp and oracle/numpy_ref.py (a tangent-order
slip, a sign in cross(ns, p), the adjoint of the binary factor's target block, the whitening, the 4-DoF projector) fails here
although every parity test passes.  The arithmetic, the bars and what is out of scope (Huber-on gradient, photometric factor,
the window chains' between factors, radar) are in tests/icp_derivatives.py; tests/test_icp_derivatives_cpu.py runs the same
checks on the oracle.  Every measured deviation is printed (pytest -s).

k = 5 runs K3's two-lanes-per-point class, the other k the one-lane 256-thread class, the tiled cloud (66 560 points) the
512-thread class.

Measured on an MI355X (bars: 1e-7 gradients, 1e-6 second differences, 1e-12 exact identities; the oracle's figures are in
the CPU module and are the same to two digits wherever truncation dominates):
  unary gradient                      2.1e-10 (5, 19), 2.3e-10 (8, 27), 2.2e-10 (4, 7), 3.1e-10 (6, 1)
  unary Hessian, corrected            rot-rot 3.7e-9 / 4.3e-9 (k 5 / 8), rot-trans 1.7e-10, trans-trans 1.5e-10 / 1.2e-10
  unary Hessian, uncorrected          7.3e-3 / 7.1e-3 off (the curvature term is exercised)
  4-DoF                               f identical, gradient 2.2e-11, Hessian blocks <= 5.0e-9 (unprojected: 1.3 off)
  binary gradient, 12 coordinates     1.5e-9 (source half 2.1e-10, target half 1.7e-9)
  binary translation sub-block        1.3e-9
  adjoint identities (Huber on)       b_t 6.4e-16, H_st 3.6e-16, H_tt 8.3e-16
  unary factor at T_rel               H_ss 6.8e-17, b_s 7.9e-15, f 2.5e-15
  sigma 0.0625 / 0.03125, Huber 1e6   bit for bit; plain enwide f 228.006 with Huber against 244.895 without
  66 560 points (512-thread class)    gradient 2.1e-10; H_ss, b_s, f against 65 x the 1024-point factor 1.5e-16, 1.7e-16, 2.3e-16
The whole module takes under a second.
"""
import pytest

import icp_derivatives as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make(ctx, small_world):
    from mimosa_amd import capi

    maps, factors = {}, []

    def _make(k, mode, binary=False, pts=None, **changes):
        if mode not in maps:
            maps[mode] = capi.VoxelMap(ctx, mode=mode)  # leaf 0.5, min_dist 0.15, 20 points per voxel: the enwide map
            maps[mode].insert(small_world["map_xyz"])
        f = capi.ICPFactor(ctx, maps[mode], small_world["pts"] if pts is None else pts, capi.make_reg_config(**D.config(k, **changes)), binary=binary)
        factors.append(f)
        return f

    yield _make
    for f in factors:
        f.destroy()
    for m in maps.values():
        m.release()


@pytest.mark.parametrize("k,mode", D.UNARY_CASES)
def test_unary_gradient_is_twice_b(make, small_world, k, mode):
    D.check_unary_gradient(make, small_world, k, mode)


@pytest.mark.parametrize("k,mode", D.HESSIAN_CASES)
def test_unary_hessian_is_half_the_second_differences_less_the_curvature(make, small_world, k, mode):
    D.check_unary_hessian(make, small_world, k, mode)


def test_four_dof_factor_is_the_projected_one(make, small_world):
    D.check_four_dof(make, small_world)


def test_binary_gradient_over_twelve_coordinates(make, small_world):
    D.check_binary_gradient(make, small_world)


def test_binary_target_block_is_the_adjoint_of_the_source_block(make, small_world):
    D.check_binary_adjoint(make, small_world)


def test_whitening_and_huber_switch_bit_for_bit(make, small_world):
    D.check_whitening_and_huber(make, small_world)


def test_tiled_cloud_runs_the_512_thread_class(make, small_world):
    D.check_tiled(make, small_world)
