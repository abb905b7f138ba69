// One Gauss-Newton step of a scan-to-map alignment (mh_icp_align): from the 28 Hessian sums K3 folded for a unary factor to
// the next pose.  Plain fp64 functions for the device (align_kernels.hip: icp_align_step_kernel) and the host (chain_api.hip's
// argument checks, tests/cpp/align_step.cpp under g++); both are compiled without floating-point contraction.
//
// What is repeated here of the host epilogue of linearize() (mh_api.hip: finish_result) is exactly what decides the step:
// the unpack of H_ss, b_s, f; computeLocalizability of the rotation and translation blocks; the 4-DoF projection; the
// degeneracy projection with the reference's quirk that a degenerate direction leaves H and b zero.  The Schur
// degeneracy info, the eigenvectors and the counters are not needed for a step and stay with the host.
#pragma once

#include <cmath>

#include "math3.hpp"

namespace mh
{
struct AlignParams
{
  double gz[3];                   // global_z = -g_unit (geometric_factor.hpp:257)
  double eps_rot, eps_trans;      // converged: |xi_r| < eps_rot and |xi_t| < eps_trans
  double damping;                 // added to the diagonal
  double prior_rot, prior_trans;  // 1 / sigma^2 on the diagonal (0 = none): a prior centred on the step's own pose
  double thresh_rot, thresh_trans;  // RegistrationConfig::degen_thresh_*
  int reg_4_dof, project_on_degeneracy;
};

enum AlignBits
{
  kAlignRotDegenerate = 1,    // a rotation localizability is not above its threshold
  kAlignTransDegenerate = 2,  // ... a translation one
  kAlignSingular = 4,         // the 6 x 6 system has no positive pivot: no step was taken and the chain stops
};

struct AlignStep
{
  double H[36], b[6], f;  // what mh_icp_linearize returns as H_ss, b_s, f at this pose
  double xi[6];           // the step, (rotation, translation) tangent order
  double step_rot, step_trans;
  double R[9], t[3];  // the pose after the step
  int bits;           // AlignBits
  int converged;
};

// index of (r, c) in the packed upper triangle of the 7 x 7 sum of v v^T, v = [J_s (6), e]
MH_HD int align_ent(int r, int c)
{
  if (r > c) {
    const int s = r;
    r = c;
    c = s;
  }
  return r * 7 - r * (r - 1) / 2 + (c - r);
}

// block 0: rotation, 1: translation.  true = projection_matrix (include/mimosa/lidar/utils.hpp:191-213) would project
MH_HD bool align_block_degenerate(const double * sums, int block, double thresh)
{
  double B[9], loc[3], E[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) B[3 * r + c] = sums[align_ent(3 * block + r, 3 * block + c)];
  compute_localizability(B, loc, E);
  return !(loc[0] > thresh && loc[1] > thresh && loc[2] > thresh);
}

// H_ss, b_s, f of finish_result for a unary factor at rotation R (same operations in the same order)
MH_HD void align_hessian(const double * sums, const double R[9], const AlignParams & p, bool rot_degen, bool trans_degen, double H[36],
                         double b[6], double & f)
{
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) H[6 * r + c] = sums[align_ent(r, c)];
    b[r] = sums[align_ent(r, 6)];
  }
  f = sums[align_ent(6, 6)];
  if (p.reg_4_dof) {
    double Hrr[9], Hrt[9], Htr[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        Hrr[3 * r + c] = H[6 * r + c];
        Hrt[3 * r + c] = H[6 * r + 3 + c];
        Htr[3 * r + c] = H[6 * (3 + r) + c];
      }
    double lz[3];
    for (int i = 0; i < 3; ++i) lz[i] = R[i] * p.gz[0] + (R[3 + i] * p.gz[1] + R[6 + i] * p.gz[2]);
    double Pi[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Pi[3 * r + c] = lz[r] * lz[c];
    double a[9], bb[9], c9[9], tmp[9];
    mat3_mul(Pi, Hrr, tmp);
    mat3_mul(tmp, Pi, a);
    mat3_mul(Pi, Hrt, bb);
    mat3_mul(Htr, Pi, c9);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        H[6 * r + c] = a[3 * r + c];
        H[6 * r + 3 + c] = bb[3 * r + c];
        H[6 * (3 + r) + c] = c9[3 * r + c];
      }
    double br[3];
    for (int i = 0; i < 3; ++i) br[i] = Pi[3 * i] * b[0] + (Pi[3 * i + 1] * b[1] + Pi[3 * i + 2] * b[2]);
    for (int i = 0; i < 3; ++i) b[i] = br[i];
  }
  if (p.project_on_degeneracy && (rot_degen || trans_degen)) {
    for (int i = 0; i < 36; ++i) H[i] = 0.0;
    for (int i = 0; i < 6; ++i) b[i] = 0.0;
  }
}

// A x = rhs for a symmetric positive definite 6 x 6 A (row-major): L D L^T without pivoting, then two refinement steps whose
// residual is accumulated in twice the working precision (error-free products through fma, two-sum), so that the answer is
// good to the last digits of fp64 up to condition numbers of 1e8 and beyond, where a plain factorisation keeps eight digits.
// false: a pivot is not positive (or not a number) — A is not positive definite to working precision.
MH_HD bool align_solve6(const double A[36], const double rhs[6], double x[6])
{
  double L[36], D[6];
  for (int j = 0; j < 6; ++j) {
    double d = A[6 * j + j];
    for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k] * D[k];
    if (!(d > 0.0) || !(d < 1e300)) return false;
    D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[6 * i + j];
      for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k] * D[k];
      L[6 * i + j] = s / d;
    }
  }
  auto solve = [&](const double * r, double * y) {
    for (int i = 0; i < 6; ++i) {
      double s = r[i];
      for (int k = 0; k < i; ++k) s -= L[6 * i + k] * y[k];
      y[i] = s;
    }
    for (int i = 0; i < 6; ++i) y[i] = y[i] / D[i];
    for (int i = 5; i >= 0; --i) {
      double s = y[i];
      for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * y[k];
      y[i] = s;
    }
  };
  solve(rhs, x);
  for (int it = 0; it < 2; ++it) {
    double r[6], d[6];
    for (int i = 0; i < 6; ++i) {
      double hi = rhs[i], lo = 0.0;
      for (int j = 0; j < 6; ++j) {
        const double a = A[6 * i + j], pr = a * x[j], pe = fma(a, x[j], -pr);  // a x = pr + pe exactly
        const double s = hi - pr, bv = s - hi;
        lo += ((hi - (s - bv)) + (-pr - bv)) - pe;  // two-sum of hi and -pr
        hi = s;
      }
      r[i] = hi + lo;
    }
    solve(r, d);
    for (int i = 0; i < 6; ++i) x[i] += d[i];
  }
  for (int i = 0; i < 6; ++i)
    if (!(fabs(x[i]) < 1e300)) return false;
  return true;
}

// gtsam::Rot3::Expmap (Rodrigues), as the replay's so3Expmap (host/mimosa_hip/replay.hpp)
MH_HD void align_expmap(const double w[3], double R[9])
{
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double A, B;
  if (th < 1e-10) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
  } else {
    A = sin(th) / th;
    B = (1.0 - cos(th)) / th2;
  }
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double kk = 0;
      for (int m = 0; m < 3; ++m) kk += K[3 * i + m] * K[3 * m + j];
      R[3 * i + j] += A * K[3 * i + j] + B * kk;
    }
}

// the replay's retract: R <- R Exp(xi_r), t <- t + R xi_t (first order in the translation); no re-orthonormalisation
MH_HD void align_retract(const double R[9], const double t[3], const double xi[6], double Rn[9], double tn[3])
{
  double E[9];
  align_expmap(xi, E);
  for (int i = 0; i < 3; ++i) tn[i] = t[i] + (R[3 * i] * xi[3] + R[3 * i + 1] * xi[4] + R[3 * i + 2] * xi[5]);
  mat3_mul(R, E, Rn);
}

// One step at pose (R, t).  The sign convention is WindowSmootherT::optimise's for a window of one pose without a between
// factor: (H_ss + diag(prior) + damping I) xi = -b_s.  A singular system takes no step (pose unchanged, kAlignSingular).
MH_HD void align_step(const double * sums, const double R[9], const double t[3], const AlignParams & p, bool rot_degen, bool trans_degen,
                      AlignStep & o)
{
  align_hessian(sums, R, p, rot_degen, trans_degen, o.H, o.b, o.f);
  o.bits = (rot_degen ? kAlignRotDegenerate : 0) | (trans_degen ? kAlignTransDegenerate : 0);
  double A[36], rhs[6];
  for (int i = 0; i < 36; ++i) A[i] = o.H[i];
  for (int i = 0; i < 6; ++i) {
    A[7 * i] = (A[7 * i] + (i < 3 ? p.prior_rot : p.prior_trans)) + p.damping;
    rhs[i] = -o.b[i];
  }
  o.converged = 0;
  if (!align_solve6(A, rhs, o.xi)) {
    o.bits |= kAlignSingular;
    for (int i = 0; i < 6; ++i) o.xi[i] = 0.0;
    o.step_rot = o.step_trans = 0.0;
    for (int i = 0; i < 9; ++i) o.R[i] = R[i];
    for (int i = 0; i < 3; ++i) o.t[i] = t[i];
    return;
  }
  o.step_rot = sqrt(o.xi[0] * o.xi[0] + o.xi[1] * o.xi[1] + o.xi[2] * o.xi[2]);
  o.step_trans = sqrt(o.xi[3] * o.xi[3] + o.xi[4] * o.xi[4] + o.xi[5] * o.xi[5]);
  align_retract(R, t, o.xi, o.R, o.t);
  o.converged = (o.step_rot < p.eps_rot && o.step_trans < p.eps_trans) ? 1 : 0;
}

// ---- the chain's device-side bookkeeping ---------------------------------------------------------------------------------
// The pose the chain has reached and whether it still moves.  Once `stopped` is set (convergence, or a singular system) every
// later step of the chain passes the pose on unchanged and empties the K3 launch queued behind it.
struct AlignState
{
  double R[9], t[3];
  int stopped, converged, iters, pad;
};

// One row per queued iteration, published as flagged words (icp_device.hpp) behind the sums of the call's slot.
enum AlignRow
{
  kRowF = 0,
  kRowStepRot,
  kRowStepTrans,
  kRowKnn,
  kRowBits,
  kRowFlags,  // 1 stopped after this step | 2 converged | 4 this step was queued behind the stop: nothing was evaluated
  kRowIters,
  kRowR,              // 9
  kRowT = kRowR + 9,  // 3
  kRowWords = kRowT + 3
};

// What the step kernel's lane 0 does with one queued iteration: the chain's state in, the state and the iteration's row out.
// have_sums: K3's words of this iteration carry the call's number (they always do; a chain that finds otherwise stops).
// Returns the row's flags.  Once st.stopped is set the pose is passed on unchanged, whatever the sums say.
MH_HD int align_advance(AlignState & st, const double * sums, bool have_sums, const AlignParams & p, bool rot_degen, bool trans_degen, double * row)
{
  for (int i = 0; i < kRowWords; ++i) row[i] = 0.0;
  int flags = 0;
  if (st.stopped) {
    flags = 1 | (st.converged ? 2 : 0) | 4;
  } else if (!have_sums) {
    st.stopped = 1;
    st.iters += 1;
    row[kRowBits] = static_cast<double>(kAlignSingular | 8);
    flags = 1;
  } else {
    AlignStep o;
    align_step(sums, st.R, st.t, p, rot_degen, trans_degen, o);
    for (int i = 0; i < 9; ++i) st.R[i] = o.R[i];
    for (int i = 0; i < 3; ++i) st.t[i] = o.t[i];
    st.stopped = (o.converged || (o.bits & kAlignSingular)) ? 1 : 0;
    st.converged = o.converged;
    st.iters += 1;
    row[kRowF] = o.f;
    row[kRowStepRot] = o.step_rot;
    row[kRowStepTrans] = o.step_trans;
    row[kRowKnn] = sums[28];
    row[kRowBits] = static_cast<double>(o.bits);
    flags = st.stopped | (o.converged ? 2 : 0);
  }
  row[kRowFlags] = static_cast<double>(flags);
  row[kRowIters] = static_cast<double>(st.iters);
  for (int i = 0; i < 9; ++i) row[kRowR + i] = st.R[i];
  for (int i = 0; i < 3; ++i) row[kRowT + i] = st.t[i];
  return flags;
}

}  // namespace mh

#if defined(__HIPCC__)
#include "icp_device.hpp"

namespace mh
{
// align_kernels.hip — one member's step of an alignment chain (mh_icp_align, mh_icp_align_batch), launched behind the K3
// (staged batch form, tail = 1) whose flagged words landed in ll_dev.  `next`: the member's argument block of the K3 launch
// queued behind this step (in the chain's device block; null behind the last launch of the call): the step writes R, t there,
// and n = 0 once the member has stopped.
struct AlignStepArgs
{
  const uint4 * ll_dev;  // K3's 28 sums + 4 counters of this iteration (device memory)
  uint4 * ll_host;       // the iteration's slot in mapped pinned memory: sums at 0, the trace row at kLlSums
  IcpArgs * next;
  AlignState * state;
  AlignParams p;
  unsigned int seq;      // tags K3's words and everything this step publishes
};

// align_kernels.hip — one step of a chain of n_members: one member runs icp_align_step_kernel on m[0]; several run
// icp_align_batch_step_kernel, whose workgroup m is the same step for member m, on m[m] alone.  Either way the arguments travel
// in the kernel-argument segment.
constexpr int kAlignBatchMax = 16;
struct AlignBatchStepArgs
{
  AlignStepArgs m[kAlignBatchMax];
};
static_assert(sizeof(AlignBatchStepArgs) <= 3072, "mh_icp_align_batch: the step's arguments ride in the kernel-argument segment");
hipError_t launch_align_chain_step(const AlignBatchStepArgs & a, int n_members, hipStream_t stream);
}  // namespace mh
#endif
