// One Gauss-Newton iteration over a fixed-lag window of poses (mh_icp_window_optimise, chain_api.hip): from the 28 Hessian sums K3 folded for
// each of the window's unary factors to the next W poses.  It restates one iteration of WindowSmootherT::optimise
// (host/mimosa_hip/replay.hpp) without the photometric terms, in that function's sign conventions: per pose the H_ss, b_s, f
// of the factor at its own rotation (align_device.hpp: align_hessian, with the 4-DoF projection and the degeneracy quirk),
// per between factor Z_i of poses i - 1, i the residual [Log(Z.R^T R_ab), Z.R^T (t_ab - Z.t)] with J_a = -Ad(between^-1),
// J_b = I and diagonal weights, a diagonal prior on the oldest pose, a damping on every diagonal, right-hand side -g.
//
// The system is symmetric positive definite and block-tridiagonal in 6 x 6 blocks.  It is solved by a block L D L^T sweep
// (S_0 = A_00, G_i = S_{i-1}^-1 E_i^T, S_i = A_ii - E_i G_i; every S_i factorised as align_solve6 factorises its matrix), forward
// over the W blocks and back, followed by two refinement steps whose residual is accumulated in twice the working precision.
// A window of one pose without a between factor goes through exactly the operations of align_step, in the same order.
// With edges (mh_icp_window_optimise_edges: between factors on any pair of poses) the system has blocks away from the
// sub-diagonal; it is then solved by the same block L D L^T over its row profile, with fill (window_factor_profile below).
//
// Plain fp64 for the device (window_kernels.hip: icp_window_step_kernel) and the host (tests/cpp/window_step.cpp under g++),
// both compiled without floating-point contraction.  The work is written as PHASES: in one phase every index of a range
// computes its own outputs from what earlier phases left, so the host runs a phase as a loop and the kernel as one index per
// lane with a barrier behind it (the `Par` argument) — the same arithmetic per value either way, hence the same digits.
#pragma once

#include "align_device.hpp"

namespace mh
{
constexpr int kWindowMax = 16;  // poses per window call

struct WindowParams
{
  int W;
  unsigned int has_Z;    // bit i: a between factor ties poses i - 1 and i (bit 0 is never set)
  unsigned int have;     // bit i: pose i's factor has points (an empty factor contributes nothing)
  unsigned int reg_4_dof, project_on_degeneracy;  // bit i: pose i's factor has the option set
  double gz[3];          // global_z = -g_unit
  double Wb[6];          // between_info: the diagonal weights of every between factor
  double prior[6];       // prior_info: on the diagonal of the oldest pose
  double damping;
  double eps_rot, eps_trans;  // stop when EVERY pose's |xi_r| < eps_rot and |xi_t| < eps_trans (0 = never)
  double thresh_rot[kWindowMax], thresh_trans[kWindowMax];  // RegistrationConfig::degen_thresh_* of each factor
};

// The poses the chain has reached, the between measurements (constant over a call) and whether the chain still moves.
struct WindowState
{
  double R[kWindowMax][9], t[kWindowMax][3];
  double ZR[kWindowMax][9], Zt[kWindowMax][3];
  int stopped, converged, iters, pad;
};

// mh_icp_window_optimise_relin: per pose the linearization pose L_i of its factor's last evaluation and the factor's H_ss, b_s, f
// (after the 4-DoF projection and the degeneracy quirk) as evaluated there.  A factor whose pose stays within the thresholds of
// L_i (component-wise in L_i's tangent, strict) is not evaluated again: its quadratic model is carried to the current pose.
struct WindowRelin
{
  double LR[kWindowMax][9], Lt[kWindowMax][3];
  double H[kWindowMax][36], b[kWindowMax][6], f[kWindowMax];
  double d[kWindowMax][6];      // the current pose in L_i's tangent: [Log(L.R^T R), L.R^T (t - L.t)], as the last step left it
  int degen[2 * kWindowMax];    // the degeneracy bits of the last evaluation (reported while the factor is kept)
  int next[kWindowMax];         // the decision of the step in flight, per pose
  unsigned int eval, pad;       // bit i: factor i is evaluated in the iteration queued behind the last step
};
struct WindowRelinParams
{
  double relin_rot, relin_trans;  // rad, m
  int first, pad;                 // the call's first iteration: every non-empty factor is evaluated, nothing is read from WindowRelin
};

// mh_icp_window_optimise_lin: Hessian factors the host linearized once, each on one pose, in the convention of the ICP factor's
// H_ss, b_s, f (the model f + 2 b^T x + x^T H x in the tangent of its linearization pose L).  Read-only to the chain: every
// iteration carries each of them from L to the current pose of its variable (window_transport) into WindowLinWork.
constexpr int kWindowLinMax = 32;
struct WindowLinear
{
  int n, pad;
  int pose[kWindowLinMax];  // 0 .. W - 1
  double LR[kWindowLinMax][9], Lt[kWindowLinMax][3];
  double H[kWindowLinMax][36], b[kWindowLinMax][6], f[kWindowLinMax];
};
struct WindowLinWork
{
  double H[kWindowLinMax][36], b[kWindowLinMax][6], f[kWindowLinMax];  // factor j at the current pose of its variable
  double tmp[kWindowLinMax][36];
};

// mh_icp_window_optimise_edges: between factors on any pair of poses a < b, each with its own measurement and a dense 6 x 6
// information matrix.  Read-only to the chain: every iteration evaluates each of them at the current poses
// (window_between_dense) into WindowEdgeWork.  With them the system is no longer block-tridiagonal: its strictly lower blocks
// (i, k), k < i, are kept packed, block (i, k) at window_pair(i, k), and solved over the row profile lo (window_factor_profile).
constexpr int kWindowEdgeMax = 32;
constexpr int kWindowPairs = kWindowMax * (kWindowMax - 1) / 2;
MH_HD int window_pair(int i, int k) { return i * (i - 1) / 2 + k; }
struct WindowEdges
{
  int n, pad;
  int a[kWindowEdgeMax], b[kWindowEdgeMax];  // 0 <= a < b <= W - 1
  double ZR[kWindowEdgeMax][9], Zt[kWindowEdgeMax][3];  // the measured T_a^-1 T_b
  double Om[kWindowEdgeMax][36];
};
struct WindowEdgeWork
{
  double Baa[kWindowEdgeMax][36], Eba[kWindowEdgeMax][36];  // edge e: J_a^T Om J_a, Om J_a (block row b, block column a)
  double ga[kWindowEdgeMax][6], gb[kWindowEdgeMax][6], cz[kWindowEdgeMax];  // J_a^T Om r, Om r, r^T Om r
  double B[kWindowPairs][36];  // the system's block (i, k); during window_factor_profile the updated block T_ik
  double G[kWindowPairs][36];  // G_ik = S_k^-1 T_ik^T
  int lo[kWindowMax];          // the smallest block column with a nonzero in block row i (i: none)
};

// mh_icp_window_optimise_joint: ONE dense factor on up to four poses of the window (ascending), the model f + 2 b^T x + x^T H x
// in the stacked tangents of its members at their linearization poses L; member m owns rows / columns 6 m .. 6 m + 5 of H (row
// stride kWindowJointDim) and b.  Read-only to the chain: every iteration carries it to the current poses of its members
// (window_joint_transport) into WindowJointWork.  Its blocks between two members lie off the diagonal: they go into ew.B and
// the profile.
constexpr int kWindowJointMax = 4;
constexpr int kWindowJointDim = 6 * kWindowJointMax;
struct WindowJoint
{
  int n, pad;
  int pose[kWindowJointMax];
  double LR[kWindowJointMax][9], Lt[kWindowJointMax][3];
  double H[kWindowJointDim * kWindowJointDim], b[kWindowJointDim], f;
};
struct WindowJointWork
{
  double H[kWindowJointDim * kWindowJointDim], b[kWindowJointDim], f;  // the factor at the current poses of its members
  double d[kWindowJointMax][6], M[kWindowJointMax][18];                // member m: its offset from L_m; Jr^-1(d_r), then Exp(d_r)
};
// the member of `jt` that sits on `pose` (-1: none)
MH_HD int window_joint_member(const WindowJoint & jt, int pose)
{
  for (int m = 0; m < jt.n; ++m)
    if (jt.pose[m] == pose) return m;
  return -1;
}

// One row per queued iteration, published as flagged words.
enum WindowRow
{
  kWRowF = 0,      // the cost at the poses the iteration evaluated: sum of the factors' f, then the between terms
  kWRowStepRot,    // max over the poses of |xi_r|
  kWRowStepTrans,  // ... of |xi_t|
  kWRowBits,       // 4: a pivot of the sweep was not positive (no step, the chain stops) | 8: a factor's sums were missing
  kWRowDegen,      // 2 bits per pose: kAlignRotDegenerate | kAlignTransDegenerate of its factor at this iteration
  kWRowFlags,      // 1 stopped after this step | 2 converged | 4 queued behind the stop: nothing was evaluated
  kWRowIters,
  kWRowPad,
  kWRowPose = 8,  // 12 doubles per pose: R (9), t (3) after the step
};
MH_HD int window_row_words(int W) { return kWRowPose + 12 * W; }

struct WindowWork
{
  double A[kWindowMax][36];  // the diagonal blocks of the system
  double E[kWindowMax][36];  // E[i]: the block in block row i, block column i - 1 (the upper one is its transpose); E[0] unused
  double Baa[kWindowMax][36], ga[kWindowMax][6], gb[kWindowMax][6], cz[kWindowMax];  // between factor i: J_a^T W J_a, J_a^T W r, W r, r^T W r
  double H[kWindowMax][36], b[kWindowMax][6], f[kWindowMax];                         // factor i: H_ss, b_s, f
  double L[kWindowMax][36], Dv[kWindowMax][6];  // S_i = L D L^T (unit lower triangle, strictly lower part stored)
  double G[kWindowMax][36];                     // G[i] = S_{i-1}^-1 E_i^T
  double S[36], z[6];
  double rhs[6 * kWindowMax], x[6 * kWindowMax], y[6 * kWindowMax], r[6 * kWindowMax], d[6 * kWindowMax];
  double Rn[kWindowMax][9], tn[kWindowMax][3], srot[kWindowMax], strans[kWindowMax];
  double cost;
  int degen[2 * kWindowMax];
  int ok;
};

// host: a phase is a loop
struct WindowSerial
{
  template <typename F>
  void each(int n, F && f)
  {
    for (int l = 0; l < n; ++l) f(l);
  }
  void sync() {}
};

// ---- small matrices in the replay's operation order (replay.hpp: matmul, matvec, transpose, hat, so3Log, adjoint) ----------
MH_HD void win_mm(const double * a, const double * b, double * c)
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
MH_HD void win_mv(const double * a, const double * v, double * o)
{
  for (int i = 0; i < 3; ++i) o[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}
MH_HD void win_tr(const double * a, double * o)
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * j + i];
}
MH_HD void window_so3log(const double R[9], double w[3])
{
  double c = (R[0] + R[4] + R[8] - 1.0) / 2.0;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  const double th = acos(c);
  const double s = th < 1e-9 ? 0.5 : th / (2.0 * sin(th));
  w[0] = (R[7] - R[5]) * s;
  w[1] = (R[2] - R[6]) * s;
  w[2] = (R[3] - R[1]) * s;
}
// Ad(R, t) in (rotation, translation) tangent order
MH_HD void window_adjoint(const double R[9], const double t[3], double Ad[36])
{
  const double hat[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
  double hR[9];
  win_mm(hat, R, hR);
  for (int i = 0; i < 36; ++i) Ad[i] = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      Ad[6 * i + j] = R[3 * i + j];
      Ad[6 * (3 + i) + 3 + j] = R[3 * i + j];
      Ad[6 * (3 + i) + j] = hR[3 * i + j];
    }
}

// The between factor Z of poses a = (Ra, ta), b = (Rb, tb): Baa = J_a^T W J_a, Eba = J_b^T W J_a (block row b, block column a),
// ga = J_a^T W r, gb = W r, cost = r^T W r  (replay.hpp:460-489; J_b^T W J_b = diag(W) is added by the assembly)
MH_HD void window_between(const double Ra[9], const double ta[3], const double Rb[9], const double tb[3], const double ZR[9], const double Zt[3],
                          const double Wb[6], double Baa[36], double Eba[36], double ga[6], double gb[6], double & cost)
{
  double Rat[9], abR[9], abt[3];
  win_tr(Ra, Rat);
  win_mm(Rat, Rb, abR);
  const double dt[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
  win_mv(Rat, dt, abt);
  double Rzt[9], Re[9], te[3], lr[3];
  win_tr(ZR, Rzt);
  win_mm(Rzt, abR, Re);
  const double de[3] = {abt[0] - Zt[0], abt[1] - Zt[1], abt[2] - Zt[2]};
  win_mv(Rzt, de, te);  // Z^-1 * between
  window_so3log(Re, lr);
  const double r[6] = {lr[0], lr[1], lr[2], te[0], te[1], te[2]};
  double Rabt[9], tinv[3], Ad[36];
  win_tr(abR, Rabt);
  const double nt[3] = {-abt[0], -abt[1], -abt[2]};
  win_mv(Rabt, nt, tinv);
  window_adjoint(Rabt, tinv, Ad);  // J_a = -Ad(between^-1), J_b = I
  for (int p = 0; p < 6; ++p)
    for (int q = 0; q < 6; ++q) {
      double aa = 0;
      for (int m = 0; m < 6; ++m) aa += Ad[6 * m + p] * Wb[m] * Ad[6 * m + q];
      Baa[6 * p + q] = aa;
      Eba[6 * p + q] = -Wb[p] * Ad[6 * p + q];
    }
  cost = 0.0;
  for (int p = 0; p < 6; ++p) {
    gb[p] = Wb[p] * r[p];
    double g = 0;
    for (int m = 0; m < 6; ++m) g += -Ad[6 * m + p] * Wb[m] * r[m];
    ga[p] = g;
    cost += r[p] * Wb[p] * r[p];
  }
}

// window_between with a dense information matrix Om (row-major, read as given): the same residual and J_a = -Ad(between^-1),
// J_b = I; Baa = J_a^T Om J_a, Eba = Om J_a, ga = J_a^T Om r, gb = Om r, cost = r^T Om r  (J_b^T Om J_b = Om is added by the
// assembly).  Eba and gb are read back while Baa, ga and the cost are formed: they must not alias the other outputs.
MH_HD void window_between_dense(const double Ra[9], const double ta[3], const double Rb[9], const double tb[3], const double ZR[9], const double Zt[3],
                                const double Om[36], double Baa[36], double Eba[36], double ga[6], double gb[6], double & cost)
{
  double Rat[9], abR[9], abt[3];
  win_tr(Ra, Rat);
  win_mm(Rat, Rb, abR);
  const double dt[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
  win_mv(Rat, dt, abt);
  double Rzt[9], Re[9], te[3], lr[3];
  win_tr(ZR, Rzt);
  win_mm(Rzt, abR, Re);
  const double de[3] = {abt[0] - Zt[0], abt[1] - Zt[1], abt[2] - Zt[2]};
  win_mv(Rzt, de, te);  // Z^-1 * between
  window_so3log(Re, lr);
  const double r[6] = {lr[0], lr[1], lr[2], te[0], te[1], te[2]};
  double Rabt[9], tinv[3], Ad[36];
  win_tr(abR, Rabt);
  const double nt[3] = {-abt[0], -abt[1], -abt[2]};
  win_mv(Rabt, nt, tinv);
  window_adjoint(Rabt, tinv, Ad);  // J_a = -Ad(between^-1), J_b = I
  for (int p = 0; p < 6; ++p) {
    for (int q = 0; q < 6; ++q) {
      double s = 0;
      for (int m = 0; m < 6; ++m) s += Om[6 * p + m] * -Ad[6 * m + q];
      Eba[6 * p + q] = s;
    }
    double g = 0;
    for (int m = 0; m < 6; ++m) g += Om[6 * p + m] * r[m];
    gb[p] = g;
  }
  cost = 0.0;
  for (int p = 0; p < 6; ++p) {
    for (int q = 0; q < 6; ++q) {
      double aa = 0;
      for (int m = 0; m < 6; ++m) aa += -Ad[6 * m + p] * Eba[6 * m + q];
      Baa[6 * p + q] = aa;
    }
    double g = 0;
    for (int m = 0; m < 6; ++m) g += -Ad[6 * m + p] * gb[m];
    ga[p] = g;
    cost += r[p] * gb[p];
  }
}

// L D L^T y = r for one factorised 6 x 6 block: the three sweeps of align_solve6
MH_HD void window_solve6(const double L[36], const double D[6], const double * r, double * y)
{
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
}

// ---- relinearization past a pose threshold (mh_icp_window_optimise_relin) ------------------------------------------------------
// the pose (R, t) in the tangent of (LR, Lt) under the chain's retraction R <- R Exp(xi_r), t <- t + R xi_t
MH_HD void window_local(const double LR[9], const double Lt[3], const double R[9], const double t[3], double d[6])
{
  double Lrt[9], Rel[9];
  win_tr(LR, Lrt);
  win_mm(Lrt, R, Rel);
  window_so3log(Rel, d);
  const double dt[3] = {t[0] - Lt[0], t[1] - Lt[1], t[2] - Lt[2]};
  win_mv(Lrt, dt, d + 3);
}
// the inverse right Jacobian of SO(3): I + 1/2 [phi]x + c [phi]x^2, c = 1 / th^2 - (1 + cos th) / (2 th sin th) (its series
// 1/12 + th^2 / 720 + th^4 / 30240 below 1e-2 rad, where the closed form has lost five digits and the series' next term is 1e-18)
MH_HD void window_jrinv(const double phi[3], double J[9])
{
  const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2], th = sqrt(th2);
  const double K[9] = {0, -phi[2], phi[1], phi[2], 0, -phi[0], -phi[1], phi[0], 0};
  const double c = th < 1e-2 ? 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0 : 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double kk = 0;
      for (int m = 0; m < 3; ++m) kk += K[3 * i + m] * K[3 * m + j];
      J[3 * i + j] = (i == j ? 1.0 : 0.0) + 0.5 * K[3 * i + j] + c * kk;
    }
}
// The model f + 2 b^T x + x^T H x of a factor around L, seen from the pose at offset d: a step xi there is x = d + M xi to
// first order, M = blockdiag(Jr^-1(d_r), Exp(d_r)).  Ho = M^T H M, bo = M^T (b + H d), fo = f + 2 b^T d + d^T H d; at d = 0 the
// model itself, untouched.  tmp: 36 doubles of the caller's (H M).
MH_HD void window_transport(const double H[36], const double b[6], double f, const double d[6], double Ho[36], double bo[6], double & fo, double * tmp)
{
  if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0 && d[3] == 0.0 && d[4] == 0.0 && d[5] == 0.0) {
    for (int q = 0; q < 36; ++q) Ho[q] = H[q];
    for (int q = 0; q < 6; ++q) bo[q] = b[q];
    fo = f;
    return;
  }
  double M[18];  // Jr^-1(d_r), then Exp(d_r)
  window_jrinv(d, M);
  align_expmap(d, M + 9);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      const double * blk = M + (c < 3 ? 0 : 9);
      const int h0 = c < 3 ? 0 : 3, cc = c - h0;
      tmp[6 * r + c] = H[6 * r + h0] * blk[cc] + H[6 * r + h0 + 1] * blk[3 + cc] + H[6 * r + h0 + 2] * blk[6 + cc];
    }
  double bd = 0.0, dHd = 0.0;
  for (int r = 0; r < 6; ++r) {
    const double * blk = M + (r < 3 ? 0 : 9);
    const int h0 = r < 3 ? 0 : 3, rr = r - h0;
    for (int c = 0; c < 6; ++c) Ho[6 * r + c] = blk[rr] * tmp[6 * h0 + c] + blk[3 + rr] * tmp[6 * (h0 + 1) + c] + blk[6 + rr] * tmp[6 * (h0 + 2) + c];
    double hd = 0.0;
    for (int m = 0; m < 6; ++m) hd += H[6 * r + m] * d[m];
    bd += b[r] * d[r];
    dHd += d[r] * hd;
  }
  for (int r = 0; r < 6; ++r) {
    const double * blk = M + (r < 3 ? 0 : 9);
    const int h0 = r < 3 ? 0 : 3, rr = r - h0;
    double g = 0.0;
    for (int k = 0; k < 3; ++k) {
      double v = b[h0 + k];
      for (int m = 0; m < 6; ++m) v += H[6 * (h0 + k) + m] * d[m];
      g += blk[3 * k + rr] * v;
    }
    bo[r] = g;
  }
  fo = f + 2.0 * bd + dHd;
}
// ISAM2's vector thresholds: component-wise, strict
MH_HD bool window_relin_decide(const double d[6], double relin_rot, double relin_trans)
{
  return fabs(d[0]) > relin_rot || fabs(d[1]) > relin_rot || fabs(d[2]) > relin_rot || fabs(d[3]) > relin_trans || fabs(d[4]) > relin_trans ||
         fabs(d[5]) > relin_trans;
}

// window_transport for the joint factor: with d_m = window_local(L_m, T_m) per member, M = blockdiag(M_m) and d stacked,
// jw.H = M^T H M block by block (H'_ij = M_i^T H_ij M_j for i <= j, H_ij M_j through 36 doubles of tmp, the lower blocks
// mirrored), jw.b = M^T (b + H d), jw.f = f + 2 b^T d + d^T H d; every d zero: H, b, f untouched.  A factor of one member goes
// through the operations of window_transport, in its order.  tmp: 36 doubles per block of the upper triangle (10 at most).
template <typename Par>
MH_HD void window_joint_transport(const WindowJoint & jt, const WindowState & st, WindowJointWork & jw, double (*tmp)[36], Par & par)
{
  constexpr int S = kWindowJointDim;
  const int n = jt.n, nb = n * (n + 1) / 2;
  par.each(n, [&](int m) {
    const int i = jt.pose[m];
    window_local(jt.LR[m], jt.Lt[m], st.R[i], st.t[i], jw.d[m]);
    window_jrinv(jw.d[m], jw.M[m]);
    align_expmap(jw.d[m], jw.M[m] + 9);
  });
  par.each(nb + 6 * n + 1, [&](int l) {
    bool moved = false;
    for (int m = 0; m < n; ++m)
      for (int q = 0; q < 6; ++q) moved = moved || jw.d[m][q] != 0.0;
    if (l < nb) {
      int i = 0, q = l;
      while (q >= n - i) {
        q -= n - i;
        ++i;
      }
      const int j = i + q;
      const double * H = jt.H + 6 * i * S + 6 * j;
      double * Ho = jw.H + 6 * i * S + 6 * j;
      double * Hm = jw.H + 6 * j * S + 6 * i;  // the mirrored block (j, i)
      double * tm = tmp[l];
      if (moved)
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) {
            const double * blk = jw.M[j] + (c < 3 ? 0 : 9);
            const int h0 = c < 3 ? 0 : 3, cc = c - h0;
            tm[6 * r + c] = H[S * r + h0] * blk[cc] + H[S * r + h0 + 1] * blk[3 + cc] + H[S * r + h0 + 2] * blk[6 + cc];
          }
      for (int r = 0; r < 6; ++r) {
        const double * blk = jw.M[i] + (r < 3 ? 0 : 9);
        const int h0 = r < 3 ? 0 : 3, rr = r - h0;
        for (int c = 0; c < 6; ++c) {
          const double v = moved ? blk[rr] * tm[6 * h0 + c] + blk[3 + rr] * tm[6 * (h0 + 1) + c] + blk[6 + rr] * tm[6 * (h0 + 2) + c] : H[S * r + c];
          Ho[S * r + c] = v;
          if (i != j) Hm[S * c + r] = v;
        }
      }
    } else if (l < nb + 6 * n) {
      const int row = l - nb, m = row / 6, r = row % 6;
      if (!moved) {
        jw.b[row] = jt.b[row];
        return;
      }
      const double * blk = jw.M[m] + (r < 3 ? 0 : 9);
      const int h0 = r < 3 ? 0 : 3, rr = r - h0;
      double g = 0.0;
      for (int k = 0; k < 3; ++k) {
        const int hr = 6 * m + h0 + k;
        double v = jt.b[hr];
        for (int j = 0; j < n; ++j)
          for (int q = 0; q < 6; ++q) v += jt.H[S * hr + 6 * j + q] * jw.d[j][q];
        g += blk[3 * k + rr] * v;
      }
      jw.b[row] = g;
    } else {
      if (!moved) {
        jw.f = jt.f;
        return;
      }
      double bd = 0.0, dHd = 0.0;
      for (int row = 0; row < 6 * n; ++row) {
        double hd = 0.0;
        for (int j = 0; j < n; ++j)
          for (int q = 0; q < 6; ++q) hd += jt.H[S * row + 6 * j + q] * jw.d[j][q];
        bd += jt.b[row] * jw.d[row / 6][row % 6];
        dHd += jw.d[row / 6][row % 6] * hd;
      }
      jw.f = jt.f + 2.0 * bd + dHd;
    }
  });
}

// ew.B over the profile: block (i, k), lo(i) <= k < i, is the has_Z term of the pair (k = i - 1), then its edges in list order;
// a block of the profile that has neither is fill: zero.  A phase of its own: window_solve_profile runs it again behind the
// factorisation, which leaves its updated blocks in ew.B.  JOINT: in front of both, the joint factor's block of two member poses.
template <bool JOINT = false, typename Par>
MH_HD void window_assemble_blocks(int W, const WindowParams & p, const WindowWork & w, const WindowEdges & ed, WindowEdgeWork & ew, Par & par,
                                  const WindowJoint * jt = nullptr, const WindowJointWork * jw = nullptr)
{
  par.each(36 * (W * (W - 1) / 2), [&](int l) {
    const int q = l / 36, e = l % 36;
    int i = 1;
    while (window_pair(i + 1, 0) <= q) ++i;
    const int k = q - window_pair(i, 0);
    if (k < ew.lo[i]) return;
    double a = (k == i - 1 && ((p.has_Z >> i) & 1u)) ? w.E[i][e] : 0.0;
    if (JOINT) {
      const int mi = window_joint_member(*jt, i), mk = window_joint_member(*jt, k);
      if (mi >= 0 && mk >= 0) a = jw->H[(6 * mi + e / 6) * kWindowJointDim + 6 * mk + e % 6] + a;
    }
    for (int j = 0; j < ed.n; ++j)
      if (ed.b[j] == i && ed.a[j] == k) a += ew.Eba[j][e];
    ew.B[q][e] = a;
  });
}

// w.A, w.E, w.rhs, w.cost from the factors' sums at the poses of `st`.  RELIN: the factors of `eval` from their sums (and into
// rl, with the pose), the other non-empty ones from rl.  LIN: the linear factors of `lin` as well, carried to the poses of `st`.
// EDGE: the edges of `ed` as well, and every block below the diagonal into ew->B over the profile ew->lo (w.E keeps the has_Z terms)
// JOINT (with LIN and EDGE): the joint factor `jt` as well, carried to the poses of `st` into jw (lw->tmp is its block scratch)
template <bool RELIN, bool LIN, bool EDGE, bool JOINT = false, typename Par>
MH_HD void window_assemble_impl(const double * sums, const WindowState & st, const WindowParams & p, WindowWork & w, WindowRelin * rl, unsigned int eval,
                                const WindowLinear * lin, WindowLinWork * lw, const WindowEdges * ed, WindowEdgeWork * ew, Par & par,
                                const WindowJoint * jt = nullptr, WindowJointWork * jw = nullptr)
{
  static_assert(!JOINT || (LIN && EDGE), "the joint factor rides on the edges chain");
  const int n_edge = EDGE ? ed->n : 0;
  const int W = p.W;
  const int n_lin = LIN ? lin->n : 0;
  par.each(2 * W, [&](int l) {
    const int i = l >> 1, blk = l & 1;
    if (RELIN && ((p.have >> i) & 1u) && !((eval >> i) & 1u)) {
      w.degen[l] = rl->degen[l];
      return;
    }
    w.degen[l] = ((p.have >> i) & 1u) && align_block_degenerate(sums + 32 * i, blk, blk ? p.thresh_trans[i] : p.thresh_rot[i]) ? 1 : 0;
    if (RELIN) rl->degen[l] = w.degen[l];
  });
  par.each(W, [&](int i) {
    if (RELIN && ((p.have >> i) & 1u) && !((eval >> i) & 1u)) {
      window_transport(rl->H[i], rl->b[i], rl->f[i], rl->d[i], w.H[i], w.b[i], w.f[i], w.A[i]);
    } else if ((p.have >> i) & 1u) {
      AlignParams ap{};
      for (int q = 0; q < 3; ++q) ap.gz[q] = p.gz[q];
      ap.reg_4_dof = static_cast<int>((p.reg_4_dof >> i) & 1u);
      ap.project_on_degeneracy = static_cast<int>((p.project_on_degeneracy >> i) & 1u);
      align_hessian(sums + 32 * i, st.R[i], ap, w.degen[2 * i] != 0, w.degen[2 * i + 1] != 0, w.H[i], w.b[i], w.f[i]);
      if (RELIN) {
        for (int q = 0; q < 36; ++q) rl->H[i][q] = w.H[i][q];
        for (int q = 0; q < 6; ++q) rl->b[i][q] = w.b[i][q];
        rl->f[i] = w.f[i];
        for (int q = 0; q < 9; ++q) rl->LR[i][q] = st.R[i][q];
        for (int q = 0; q < 3; ++q) rl->Lt[i][q] = st.t[i][q];
      }
    } else {
      for (int q = 0; q < 36; ++q) w.H[i][q] = 0.0;
      for (int q = 0; q < 6; ++q) w.b[i][q] = 0.0;
      w.f[i] = 0.0;
    }
    if ((p.has_Z >> i) & 1u) {
      window_between(st.R[i - 1], st.t[i - 1], st.R[i], st.t[i], st.ZR[i], st.Zt[i], p.Wb, w.Baa[i], w.E[i], w.ga[i], w.gb[i], w.cz[i]);
    } else {
      for (int q = 0; q < 36; ++q) w.E[i][q] = 0.0;
    }
  });
  if (LIN)
    par.each(n_lin, [&](int j) {
      const int i = lin->pose[j];
      double d[6];
      window_local(lin->LR[j], lin->Lt[j], st.R[i], st.t[i], d);
      window_transport(lin->H[j], lin->b[j], lin->f[j], d, lw->H[j], lw->b[j], lw->f[j], lw->tmp[j]);
    });
  if (JOINT) window_joint_transport(*jt, st, *jw, lw->tmp, par);
  if (EDGE)
    par.each(n_edge + W, [&](int l) {
      if (l < n_edge) {
        const int a = ed->a[l], b = ed->b[l];
        window_between_dense(st.R[a], st.t[a], st.R[b], st.t[b], ed->ZR[l], ed->Zt[l], ed->Om[l], ew->Baa[l], ew->Eba[l], ew->ga[l], ew->gb[l], ew->cz[l]);
      } else {
        const int i = l - n_edge;
        int lo = ((p.has_Z >> i) & 1u) ? i - 1 : i;
        for (int e = 0; e < n_edge; ++e)
          if (ed->b[e] == i && ed->a[e] < lo) lo = ed->a[e];
        if (JOINT && window_joint_member(*jt, i) > 0 && jt->pose[0] < lo) lo = jt->pose[0];  // a member row reaches down to the smallest member
        ew->lo[i] = lo;
      }
    });
  // per entry in the order optimise() adds: the factor, (the linear factors on its pose in list order,) (the joint factor's
  // block,) the between factors in window order, (the edges in list order,) the prior, the damping
  par.each(36 * W + 6 * W + 1, [&](int l) {
    if (l < 36 * W) {
      const int i = l / 36, e = l % 36, r = e / 6, c = e % 6;
      double a = w.H[i][e];
      if (LIN)
        for (int j = 0; j < n_lin; ++j)
          if (lin->pose[j] == i) a += lw->H[j][e];
      if (JOINT) {
        const int m = window_joint_member(*jt, i);
        if (m >= 0) a += jw->H[(6 * m + r) * kWindowJointDim + 6 * m + c];
      }
      if (r == c && ((p.has_Z >> i) & 1u)) a += p.Wb[r];
      if (i + 1 < W && ((p.has_Z >> (i + 1)) & 1u)) a += w.Baa[i + 1][e];
      if (EDGE)
        for (int j = 0; j < n_edge; ++j) {
          if (ed->b[j] == i) a += ed->Om[j][e];
          if (ed->a[j] == i) a += ew->Baa[j][e];
        }
      if (r == c) {
        if (i == 0) a += p.prior[r];
        a += p.damping;
      }
      w.A[i][e] = a;
    } else if (l < 42 * W) {
      const int q = l - 36 * W, i = q / 6, r = q % 6;
      double g = w.b[i][r];
      if (LIN)
        for (int j = 0; j < n_lin; ++j)
          if (lin->pose[j] == i) g += lw->b[j][r];
      if (JOINT) {
        const int m = window_joint_member(*jt, i);
        if (m >= 0) g += jw->b[6 * m + r];
      }
      if ((p.has_Z >> i) & 1u) g += w.gb[i][r];
      if (i + 1 < W && ((p.has_Z >> (i + 1)) & 1u)) g += w.ga[i + 1][r];
      if (EDGE)
        for (int j = 0; j < n_edge; ++j) {
          if (ed->b[j] == i) g += ew->gb[j][r];
          if (ed->a[j] == i) g += ew->ga[j][r];
        }
      w.rhs[q] = -g;
    } else {
      double cost = 0.0;
      for (int i = 0; i < W; ++i) cost += w.f[i];
      if (LIN)
        for (int j = 0; j < n_lin; ++j) cost += lw->f[j];
      if (JOINT) cost += jw->f;
      for (int i = 1; i < W; ++i)
        if ((p.has_Z >> i) & 1u) cost += w.cz[i];
      if (EDGE)
        for (int j = 0; j < n_edge; ++j) cost += ew->cz[j];
      w.cost = cost;
    }
  });
  if (EDGE) window_assemble_blocks<JOINT>(W, p, w, *ed, *ew, par, jt, jw);
}
template <typename Par>
MH_HD void window_assemble(const double * sums, const WindowState & st, const WindowParams & p, WindowWork & w, Par & par)
{
  window_assemble_impl<false, false, false>(sums, st, p, w, nullptr, 0u, nullptr, nullptr, nullptr, nullptr, par);
}

// the block sweep: S_i = L_i D_i L_i^T and G_{i+1} for every block.  false (w.ok == 0): a pivot is not positive
template <typename Par>
MH_HD bool window_factor(int W, WindowWork & w, Par & par)
{
  par.each(1, [&](int) { w.ok = 1; });
  for (int i = 0; i < W; ++i) {
    par.each(36, [&](int l) {
      const int r = l / 6, c = l % 6;
      double s = w.A[i][l];
      if (i > 0)
        for (int m = 0; m < 6; ++m) s -= w.E[i][6 * r + m] * w.G[i][6 * m + c];
      w.S[l] = s;
    });
    for (int j = 0; j < 6; ++j) {
      // index 0 keeps the pivot, index l the entry (j + l, j) of L; each works the pivot out for itself
      par.each(6 - j, [&](int l) {
        double d = w.S[7 * j];
        for (int k = 0; k < j; ++k) d -= w.L[i][6 * j + k] * w.L[i][6 * j + k] * w.Dv[i][k];
        if (l == 0) {
          w.Dv[i][j] = d;
          if (!(d > 0.0) || !(d < 1e300)) w.ok = 0;
        } else {
          const int row = j + l;
          double s = w.S[6 * row + j];
          for (int k = 0; k < j; ++k) s -= w.L[i][6 * row + k] * w.L[i][6 * j + k] * w.Dv[i][k];
          w.L[i][6 * row + j] = s / d;
        }
      });
      if (!w.ok) return false;
    }
    if (i + 1 < W) {
      par.each(6, [&](int c) {
        double col[6];
        window_solve6(w.L[i], w.Dv[i], &w.E[i + 1][6 * c], col);  // column c of E^T = row c of E
        for (int m = 0; m < 6; ++m) w.G[i + 1][6 * m + c] = col[m];
      });
    }
  }
  return true;
}

// A out = v with the factors of window_factor
template <typename Par>
MH_HD void window_sweep(int W, WindowWork & w, const double * v, double * out, Par & par)
{
  for (int i = 0; i < W; ++i) {
    par.each(6, [&](int r) {
      double s = v[6 * i + r];
      if (i > 0)
        for (int m = 0; m < 6; ++m) s -= w.G[i][6 * m + r] * w.y[6 * (i - 1) + m];
      w.y[6 * i + r] = s;
    });
  }
  for (int i = W - 1; i >= 0; --i) {
    par.each(1, [&](int) { window_solve6(w.L[i], w.Dv[i], &w.y[6 * i], w.z); });
    par.each(6, [&](int r) {
      double s = w.z[r];
      if (i + 1 < W)
        for (int m = 0; m < 6; ++m) s -= w.G[i + 1][6 * r + m] * out[6 * (i + 1) + m];
      out[6 * i + r] = s;
    });
  }
}

// w.x from w.A, w.E, w.rhs.  false: the system is not positive definite to working precision (w.x is then meaningless)
template <typename Par>
MH_HD bool window_solve(int W, WindowWork & w, Par & par)
{
  if (!window_factor(W, w, par)) return false;
  window_sweep(W, w, w.rhs, w.x, par);
  for (int it = 0; it < 2; ++it) {
    par.each(6 * W, [&](int row) {
      const int i = row / 6, r = row % 6;
      double hi = w.rhs[row], lo = 0.0;
      auto term = [&](double a, double xj) {
        const double pr = a * xj, pe = fma(a, xj, -pr);  // a x = pr + pe exactly
        const double s = hi - pr, bv = s - hi;
        lo += ((hi - (s - bv)) + (-pr - bv)) - pe;  // two-sum of hi and -pr
        hi = s;
      };
      if (i > 0)
        for (int m = 0; m < 6; ++m) term(w.E[i][6 * r + m], w.x[6 * (i - 1) + m]);
      for (int m = 0; m < 6; ++m) term(w.A[i][6 * r + m], w.x[6 * i + m]);
      if (i + 1 < W)
        for (int m = 0; m < 6; ++m) term(w.E[i + 1][6 * m + r], w.x[6 * (i + 1) + m]);
      w.r[row] = hi + lo;
    });
    window_sweep(W, w, w.r, w.d, par);
    par.each(6 * W, [&](int row) { w.x[row] += w.d[row]; });
  }
  par.each(1, [&](int) {
    for (int q = 0; q < 6 * W; ++q)
      if (!(fabs(w.x[q]) < 1e300)) w.ok = 0;
  });
  return w.ok != 0;
}

// ---- the solve over a row profile (mh_icp_window_optimise_edges) ----------------------------------------------------------------
// Block L D L^T of the system whose block row i holds blocks in the columns lo(i) .. i: with T_ik = L_ik S_k (the updated
// off-diagonal block) and G_ik = S_k^-1 T_ik^T = L_ik^T,
//   S_k = A_kk - sum_j T_kj G_kj,  T_ik = B_ik - sum_j T_ij G_kj  (j from max(lo(i), lo(k)) to k - 1),
// column by column: S_k is factorised as window_factor factorises it, then every row below with lo(i) <= k takes its T_ik (in
// place, in ew.B) and G_ik.  Fill stays inside [lo(i), i]; rows whose profile starts behind k are not touched.  A tridiagonal
// system goes through the operations of window_factor, in its order.  false (w.ok == 0): a pivot is not positive
template <typename Par>
MH_HD bool window_factor_profile(int W, WindowWork & w, WindowEdgeWork & ew, Par & par)
{
  par.each(1, [&](int) { w.ok = 1; });
  for (int k = 0; k < W; ++k) {
    par.each(36, [&](int l) {
      const int r = l / 6, c = l % 6;
      double s = w.A[k][l];
      for (int j = ew.lo[k]; j < k; ++j) {
        const double *T = ew.B[window_pair(k, j)], *G = ew.G[window_pair(k, j)];
        for (int m = 0; m < 6; ++m) s -= T[6 * r + m] * G[6 * m + c];
      }
      w.S[l] = s;
    });
    for (int j = 0; j < 6; ++j) {
      par.each(6 - j, [&](int l) {
        double d = w.S[7 * j];
        for (int q = 0; q < j; ++q) d -= w.L[k][6 * j + q] * w.L[k][6 * j + q] * w.Dv[k][q];
        if (l == 0) {
          w.Dv[k][j] = d;
          if (!(d > 0.0) || !(d < 1e300)) w.ok = 0;
        } else {
          const int row = j + l;
          double s = w.S[6 * row + j];
          for (int q = 0; q < j; ++q) s -= w.L[k][6 * row + q] * w.L[k][6 * j + q] * w.Dv[k][q];
          w.L[k][6 * row + j] = s / d;
        }
      });
      if (!w.ok) return false;
    }
    par.each(36 * (W - 1 - k), [&](int l) {
      const int i = k + 1 + l / 36, e = l % 36, r = e / 6, c = e % 6;
      if (ew.lo[i] > k) return;
      double s = ew.B[window_pair(i, k)][e];
      for (int j = ew.lo[i] > ew.lo[k] ? ew.lo[i] : ew.lo[k]; j < k; ++j) {
        const double *T = ew.B[window_pair(i, j)], *G = ew.G[window_pair(k, j)];
        for (int m = 0; m < 6; ++m) s -= T[6 * r + m] * G[6 * m + c];
      }
      ew.B[window_pair(i, k)][e] = s;
    });
    par.each(6 * (W - 1 - k), [&](int l) {
      const int i = k + 1 + l / 6, c = l % 6;
      if (ew.lo[i] > k) return;
      double col[6];
      window_solve6(w.L[k], w.Dv[k], &ew.B[window_pair(i, k)][6 * c], col);  // column c of T^T = row c of T
      for (int m = 0; m < 6; ++m) ew.G[window_pair(i, k)][6 * m + c] = col[m];
    });
  }
  return true;
}

// A out = v with the factors of window_factor_profile
template <typename Par>
MH_HD void window_sweep_profile(int W, WindowWork & w, const WindowEdgeWork & ew, const double * v, double * out, Par & par)
{
  for (int i = 0; i < W; ++i) {
    par.each(6, [&](int r) {
      double s = v[6 * i + r];
      for (int k = ew.lo[i]; k < i; ++k) {
        const double * G = ew.G[window_pair(i, k)];
        for (int m = 0; m < 6; ++m) s -= G[6 * m + r] * w.y[6 * k + m];
      }
      w.y[6 * i + r] = s;
    });
  }
  for (int i = W - 1; i >= 0; --i) {
    par.each(1, [&](int) { window_solve6(w.L[i], w.Dv[i], &w.y[6 * i], w.z); });
    par.each(6, [&](int r) {
      double s = w.z[r];
      for (int j = i + 1; j < W; ++j) {
        if (ew.lo[j] > i) continue;
        const double * G = ew.G[window_pair(j, i)];
        for (int m = 0; m < 6; ++m) s -= G[6 * r + m] * out[6 * j + m];
      }
      out[6 * i + r] = s;
    });
  }
}

// window_solve over the profile: w.x from w.A, ew.B, w.rhs.  The factorisation leaves its updated blocks in ew.B, so the
// blocks are assembled again behind it (the same phase, the same digits; a third set of 120 blocks would not fit the LDS a
// workgroup may declare): the refinement's residual is taken with every block of the system as assembled.
template <bool JOINT = false, typename Par>
MH_HD bool window_solve_profile(int W, const WindowParams & p, WindowWork & w, const WindowEdges & ed, WindowEdgeWork & ew, Par & par,
                                const WindowJoint * jt = nullptr, const WindowJointWork * jw = nullptr)
{
  if (!window_factor_profile(W, w, ew, par)) return false;
  window_assemble_blocks<JOINT>(W, p, w, ed, ew, par, jt, jw);
  window_sweep_profile(W, w, ew, w.rhs, w.x, par);
  for (int it = 0; it < 2; ++it) {
    par.each(6 * W, [&](int row) {
      const int i = row / 6, r = row % 6;
      double hi = w.rhs[row], lo = 0.0;
      auto term = [&](double a, double xj) {
        const double pr = a * xj, pe = fma(a, xj, -pr);  // a x = pr + pe exactly
        const double s = hi - pr, bv = s - hi;
        lo += ((hi - (s - bv)) + (-pr - bv)) - pe;  // two-sum of hi and -pr
        hi = s;
      };
      for (int k = ew.lo[i]; k < i; ++k)
        for (int m = 0; m < 6; ++m) term(ew.B[window_pair(i, k)][6 * r + m], w.x[6 * k + m]);
      for (int m = 0; m < 6; ++m) term(w.A[i][6 * r + m], w.x[6 * i + m]);
      for (int j = i + 1; j < W; ++j) {
        if (ew.lo[j] > i) continue;
        for (int m = 0; m < 6; ++m) term(ew.B[window_pair(j, i)][6 * m + r], w.x[6 * j + m]);
      }
      w.r[row] = hi + lo;
    });
    window_sweep_profile(W, w, ew, w.r, w.d, par);
    par.each(6 * W, [&](int row) { w.x[row] += w.d[row]; });
  }
  par.each(1, [&](int) {
    for (int q = 0; q < 6 * W; ++q)
      if (!(fabs(w.x[q]) < 1e300)) w.ok = 0;
  });
  return w.ok != 0;
}

// One queued iteration: the chain's state in, the state and the iteration's row out.  sums: 32 doubles per pose (28 sums +
// 4 counters; ignored where p.have has no bit).  arrived: the words of every factor carry the call's number (they always do; a
// chain that finds otherwise stops).  Returns the row's flags.  Once st.stopped is set the poses are passed on unchanged.
// RELIN: `arrived` speaks of the factors this iteration evaluates (window_relin_mask); behind the step, rl holds every pose's
// offset from its linearization pose and the factors the next iteration evaluates.
// LIN: the system and the cost also hold the linear factors of `lin` (lw: their work arrays); nothing else changes.
// EDGE: ... and the edges of `ed` (ew: their work arrays and the profile); the system is solved by window_solve_profile.
// JOINT: ... and the joint factor `jt` (jw: its work arrays); its off-diagonal blocks widen the profile.
template <bool RELIN, bool LIN, bool EDGE, bool JOINT = false, typename Par>
MH_HD int window_advance_impl(WindowState & st, const double * sums, bool arrived, const WindowParams & p, WindowWork & w, double * row, WindowRelin * rl,
                              const WindowRelinParams * rp, const WindowLinear * lin, WindowLinWork * lw, const WindowEdges * ed, WindowEdgeWork * ew, Par & par,
                              const WindowJoint * jt = nullptr, WindowJointWork * jw = nullptr)
{
  const int W = p.W;
  const bool frozen = st.stopped != 0;
  unsigned int eval = 0u;
  if (RELIN) eval = rp->first ? p.have : rl->eval;
  par.sync();  // (every index has read the state before index 0 changes it)
  bool stepped = false;
  if (!frozen && arrived) {
    window_assemble_impl<RELIN, LIN, EDGE, JOINT>(sums, st, p, w, rl, eval, lin, lw, ed, ew, par, jt, jw);
    if (EDGE)
      stepped = window_solve_profile<JOINT>(W, p, w, *ed, *ew, par, jt, jw);
    else
      stepped = window_solve(W, w, par);
    par.each(W, [&](int i) {
      if (stepped) {
        const double * xi = &w.x[6 * i];
        w.srot[i] = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
        w.strans[i] = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
        align_retract(st.R[i], st.t[i], xi, w.Rn[i], w.tn[i]);
      } else {
        w.srot[i] = w.strans[i] = 0.0;
        for (int q = 0; q < 9; ++q) w.Rn[i][q] = st.R[i][q];
        for (int q = 0; q < 3; ++q) w.tn[i][q] = st.t[i][q];
      }
    });
    par.each(12 * W, [&](int l) {
      const int i = l / 12, q = l % 12;
      if (q < 9)
        st.R[i][q] = w.Rn[i][q];
      else
        st.t[i][q - 9] = w.tn[i][q - 9];
    });
    if (RELIN)
      par.each(W, [&](int i) {
        rl->next[i] = 0;
        if ((p.have >> i) & 1u) {
          window_local(rl->LR[i], rl->Lt[i], st.R[i], st.t[i], rl->d[i]);
          rl->next[i] = window_relin_decide(rl->d[i], rp->relin_rot, rp->relin_trans) ? 1 : 0;
        }
      });
  }
  par.each(12 * W, [&](int l) {
    const int i = l / 12, q = l % 12;
    row[kWRowPose + l] = q < 9 ? st.R[i][q] : st.t[i][q - 9];
  });
  int flags = 0;
  par.each(1, [&](int) {
    for (int q = 0; q < kWRowPose; ++q) row[q] = 0.0;
    if (frozen) {
      flags = 1 | (st.converged ? 2 : 0) | 4;
    } else if (!arrived) {
      st.stopped = 1;
      st.iters += 1;
      row[kWRowBits] = static_cast<double>(kAlignSingular | 8);
      flags = 1;
    } else {
      double mr = 0.0, mt = 0.0, dg = 0.0, sh = 1.0;
      bool conv = stepped;
      for (int i = 0; i < W; ++i) {
        mr = w.srot[i] > mr ? w.srot[i] : mr;
        mt = w.strans[i] > mt ? w.strans[i] : mt;
        conv = conv && w.srot[i] < p.eps_rot && w.strans[i] < p.eps_trans;
        dg += sh * static_cast<double>(w.degen[2 * i] * kAlignRotDegenerate + w.degen[2 * i + 1] * kAlignTransDegenerate);
        sh *= 4.0;
      }
      st.converged = conv ? 1 : 0;
      st.stopped = (conv || !stepped) ? 1 : 0;
      st.iters += 1;
      row[kWRowF] = w.cost;
      row[kWRowStepRot] = mr;
      row[kWRowStepTrans] = mt;
      row[kWRowBits] = stepped ? 0.0 : static_cast<double>(kAlignSingular);
      row[kWRowDegen] = dg;
      flags = st.stopped | (conv ? 2 : 0);
      if (RELIN) {
        unsigned int m = 0u;
        for (int i = 0; i < W; ++i) m |= rl->next[i] ? 1u << i : 0u;
        rl->eval = m;
      }
    }
    row[kWRowFlags] = static_cast<double>(flags);
    row[kWRowIters] = static_cast<double>(st.iters);
  });
  return static_cast<int>(row[kWRowFlags]);
}
template <typename Par>
MH_HD int window_advance(WindowState & st, const double * sums, bool arrived, const WindowParams & p, WindowWork & w, double * row, Par & par)
{
  return window_advance_impl<false, false, false>(st, sums, arrived, p, w, row, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, par);
}
// the factors the iteration about to run evaluates (read before window_advance_relin changes rl)
MH_HD unsigned int window_relin_mask(const WindowRelin & rl, const WindowParams & p, const WindowRelinParams & rp) { return rp.first ? p.have : rl.eval; }
template <typename Par>
MH_HD int window_advance_relin(WindowState & st, WindowRelin & rl, const double * sums, bool arrived, const WindowParams & p, const WindowRelinParams & rp,
                               WindowWork & w, double * row, Par & par)
{
  return window_advance_impl<true, false, false>(st, sums, arrived, p, w, row, &rl, &rp, nullptr, nullptr, nullptr, nullptr, par);
}
// mh_icp_window_optimise_lin: either chain with the linear factors of `lin`.  rl, rp: null for the plain chain
template <typename Par>
MH_HD int window_advance_lin(WindowState & st, WindowRelin * rl, const double * sums, bool arrived, const WindowParams & p, const WindowRelinParams * rp,
                             const WindowLinear & lin, WindowLinWork & lw, WindowWork & w, double * row, Par & par)
{
  if (rl) return window_advance_impl<true, true, false>(st, sums, arrived, p, w, row, rl, rp, &lin, &lw, nullptr, nullptr, par);
  return window_advance_impl<false, true, false>(st, sums, arrived, p, w, row, nullptr, nullptr, &lin, &lw, nullptr, nullptr, par);
}
// mh_icp_window_optimise_edges: window_advance_lin with the edges of `ed` (ed.n may be 0: the same system through the profile solve)
template <typename Par>
MH_HD int window_advance_edges(WindowState & st, WindowRelin * rl, const double * sums, bool arrived, const WindowParams & p, const WindowRelinParams * rp,
                               const WindowLinear & lin, WindowLinWork & lw, const WindowEdges & ed, WindowEdgeWork & ew, WindowWork & w, double * row, Par & par)
{
  if (rl) return window_advance_impl<true, true, true>(st, sums, arrived, p, w, row, rl, rp, &lin, &lw, &ed, &ew, par);
  return window_advance_impl<false, true, true>(st, sums, arrived, p, w, row, nullptr, nullptr, &lin, &lw, &ed, &ew, par);
}

// mh_icp_window_optimise_joint: window_advance_edges with the joint factor `jt`
template <typename Par>
MH_HD int window_advance_joint(WindowState & st, WindowRelin * rl, const double * sums, bool arrived, const WindowParams & p, const WindowRelinParams * rp,
                               const WindowLinear & lin, WindowLinWork & lw, const WindowEdges & ed, WindowEdgeWork & ew, const WindowJoint & jt,
                               WindowJointWork & jw, WindowWork & w, double * row, Par & par)
{
  if (rl) return window_advance_impl<true, true, true, true>(st, sums, arrived, p, w, row, rl, rp, &lin, &lw, &ed, &ew, par, &jt, &jw);
  return window_advance_impl<false, true, true, true>(st, sums, arrived, p, w, row, nullptr, nullptr, &lin, &lw, &ed, &ew, par, &jt, &jw);
}

// ---- the marginal prior of the oldest pose (mh_icp_window_marginalise) ------------------------------------------------------------
// What eliminating pose 0 leaves on pose 1: every term that touches pose 0, at the poses given (nothing is iterated), in the
// assembly's own per-entry order — the ICP factor at T_0, the linear factors on pose 0 in list order carried to T_0, the has_Z[1]
// tie, the edges on (0, 1) in list order, the prior, the damping — accumulated into
//   A00 = H_u + sum Baa + prior + damping,  g0 = b_u + sum ga,  A10 = sum E,  A11' = sum Omega,  g1' = sum gb,  c = f_u + sum cz
// and eliminated: A00 = L D L^T as window_factor factorises a pivot block, with its pivot test, then
//   H_m = A11' - A10 A00^-1 A10^T,  b_m = g1' - A10 A00^-1 g0,  f_m = c - g0^T A00^-1 g0,
// the model f + 2 b^T x + x^T H x in the tangent of L = T_1.  Factors on pose 1 alone, ties and edges that do not touch pose 0
// contribute nothing: they stay in the window.  An edge (0, b), b > 1, is the caller's to refuse.
constexpr int kWindowTieMax = kWindowEdgeMax + 1;  // the has_Z[1] tie (slot 0), then edge e in slot 1 + e
struct WindowMarginalWork
{
  double H[36], b[6], f;  // the ICP factor of pose 0: H_ss, b_s, f
  double Baa[kWindowTieMax][36], E[kWindowTieMax][36], ga[kWindowTieMax][6], gb[kWindowTieMax][6], cz[kWindowTieMax];
  double A00[36], A10[36], A11[36], g0[6], g1[6], c;
  double L[36], Dv[6];  // A00 = L D L^T (unit lower triangle, strictly lower part stored)
  double X[7][6];       // A00^-1 times column c of A10^T (c < 6), times g0 (c == 6)
  int degen[2];
  int ok, pad;
};
struct WindowMarginalOut
{
  double H[36], b[6], f;
  int valid, n_ties;
  int degen[2];  // the degeneracy bits of pose 0's factor
};

// sums: the 32 words of factor 0 at T_0 (ignored without bit 0 of p.have).  Of p: has_Z bit 1, have / reg_4_dof /
// project_on_degeneracy bit 0, thresh_*[0], gz, Wb, prior, damping.  Of st: R, t of poses 0 and 1, ZR[1], Zt[1].
template <typename Par>
MH_HD void window_marginal_impl(const double * sums, const WindowState & st, const WindowParams & p, const WindowLinear & lin, WindowLinWork & lw,
                                const WindowEdges & ed, WindowMarginalWork & w, WindowMarginalOut & out, Par & par)
{
  const int n_lin = lin.n, n_edge = ed.n;
  const bool have = (p.have & 1u) != 0, tie = ((p.has_Z >> 1) & 1u) != 0;
  auto on01 = [&](int e) { return ed.a[e] == 0 && ed.b[e] == 1; };
  par.each(2, [&](int blk) { w.degen[blk] = have && align_block_degenerate(sums, blk, blk ? p.thresh_trans[0] : p.thresh_rot[0]) ? 1 : 0; });
  par.each(1 + n_lin + kWindowTieMax, [&](int l) {
    if (l == 0) {
      if (have) {
        AlignParams ap{};
        for (int q = 0; q < 3; ++q) ap.gz[q] = p.gz[q];
        ap.reg_4_dof = static_cast<int>(p.reg_4_dof & 1u);
        ap.project_on_degeneracy = static_cast<int>(p.project_on_degeneracy & 1u);
        align_hessian(sums, st.R[0], ap, w.degen[0] != 0, w.degen[1] != 0, w.H, w.b, w.f);
      } else {
        for (int q = 0; q < 36; ++q) w.H[q] = 0.0;
        for (int q = 0; q < 6; ++q) w.b[q] = 0.0;
        w.f = 0.0;
      }
    } else if (l <= n_lin) {
      const int j = l - 1;
      if (lin.pose[j] != 0) return;
      double d[6];
      window_local(lin.LR[j], lin.Lt[j], st.R[0], st.t[0], d);
      window_transport(lin.H[j], lin.b[j], lin.f[j], d, lw.H[j], lw.b[j], lw.f[j], lw.tmp[j]);
    } else if (l == n_lin + 1) {
      if (tie) window_between(st.R[0], st.t[0], st.R[1], st.t[1], st.ZR[1], st.Zt[1], p.Wb, w.Baa[0], w.E[0], w.ga[0], w.gb[0], w.cz[0]);
    } else {
      const int e = l - n_lin - 2;
      if (e < n_edge && on01(e))
        window_between_dense(st.R[0], st.t[0], st.R[1], st.t[1], ed.ZR[e], ed.Zt[e], ed.Om[e], w.Baa[1 + e], w.E[1 + e], w.ga[1 + e], w.gb[1 + e], w.cz[1 + e]);
    }
  });
  par.each(36 * 3 + 6 * 2 + 1, [&](int l) {
    if (l < 36) {
      const int r = l / 6, c = l % 6;
      double a = w.H[l];
      for (int j = 0; j < n_lin; ++j)
        if (lin.pose[j] == 0) a += lw.H[j][l];
      if (tie) a += w.Baa[0][l];
      for (int e = 0; e < n_edge; ++e)
        if (on01(e)) a += w.Baa[1 + e][l];
      if (r == c) {
        a += p.prior[r];
        a += p.damping;
      }
      w.A00[l] = a;
    } else if (l < 72) {
      const int q = l - 36;
      double a = tie ? w.E[0][q] : 0.0;
      for (int e = 0; e < n_edge; ++e)
        if (on01(e)) a += w.E[1 + e][q];
      w.A10[q] = a;
    } else if (l < 108) {
      const int q = l - 72;
      double a = (tie && q / 6 == q % 6) ? p.Wb[q / 6] : 0.0;
      for (int e = 0; e < n_edge; ++e)
        if (on01(e)) a += ed.Om[e][q];
      w.A11[q] = a;
    } else if (l < 114) {
      const int r = l - 108;
      double g = w.b[r];
      for (int j = 0; j < n_lin; ++j)
        if (lin.pose[j] == 0) g += lw.b[j][r];
      if (tie) g += w.ga[0][r];
      for (int e = 0; e < n_edge; ++e)
        if (on01(e)) g += w.ga[1 + e][r];
      w.g0[r] = g;
    } else if (l < 120) {
      const int r = l - 114;
      double g = tie ? w.gb[0][r] : 0.0;
      for (int e = 0; e < n_edge; ++e)
        if (on01(e)) g += w.gb[1 + e][r];
      w.g1[r] = g;
    } else {
      double c = w.f;
      for (int j = 0; j < n_lin; ++j)
        if (lin.pose[j] == 0) c += lw.f[j];
      if (tie) c += w.cz[0];
      int n = tie ? 1 : 0;
      for (int e = 0; e < n_edge; ++e)
        if (on01(e)) {
          c += w.cz[1 + e];
          n += 1;
        }
      w.c = c;
      w.ok = 1;
      out.n_ties = n;
      out.degen[0] = w.degen[0];
      out.degen[1] = w.degen[1];
    }
  });
  // A00 = L D L^T: the columns of window_factor, its pivot test
  for (int j = 0; j < 6 && w.ok; ++j) {
    par.each(6 - j, [&](int l) {
      double d = w.A00[7 * j];
      for (int k = 0; k < j; ++k) d -= w.L[6 * j + k] * w.L[6 * j + k] * w.Dv[k];
      if (l == 0) {
        w.Dv[j] = d;
        if (!(d > 0.0) || !(d < 1e300)) w.ok = 0;
      } else {
        const int row = j + l;
        double s = w.A00[6 * row + j];
        for (int k = 0; k < j; ++k) s -= w.L[6 * row + k] * w.L[6 * j + k] * w.Dv[k];
        w.L[6 * row + j] = s / d;
      }
    });
  }
  if (!w.ok) {
    par.each(36 + 6 + 1, [&](int l) {
      if (l < 36)
        out.H[l] = 0.0;
      else if (l < 42)
        out.b[l - 36] = 0.0;
      else {
        out.f = 0.0;
        out.valid = 0;
      }
    });
    return;
  }
  par.each(7, [&](int c) { window_solve6(w.L, w.Dv, c < 6 ? &w.A10[6 * c] : w.g0, w.X[c]); });  // column c of A10^T = row c of A10
  // the upper triangle of H_m, mirrored
  par.each(21 + 6 + 1, [&](int l) {
    if (l < 21) {
      int r = 0, q = l;
      while (q >= 6 - r) {
        q -= 6 - r;
        ++r;
      }
      const int c = r + q;
      double s = w.A11[6 * r + c];
      for (int m = 0; m < 6; ++m) s -= w.A10[6 * r + m] * w.X[c][m];
      out.H[6 * r + c] = s;
      out.H[6 * c + r] = s;
    } else if (l < 27) {
      const int r = l - 21;
      double s = w.g1[r];
      for (int m = 0; m < 6; ++m) s -= w.A10[6 * r + m] * w.X[6][m];
      out.b[r] = s;
    } else {
      double s = w.c;
      for (int m = 0; m < 6; ++m) s -= w.g0[m] * w.X[6][m];
      out.f = s;
      out.valid = 1;
    }
  });
}

// ---- the joint marginal of the oldest pose (mh_icp_window_marginalise_joint) -------------------------------------------------------
// window_marginal_impl for a pose 0 that is tied beyond pose 1.  The separator S: pose 1 (always), the far pose of every edge
// (0, b), the members of the joint factor other than pose 0 — sorted, at most kWindowJointMax poses (more: the caller's to
// refuse).  Every term on pose 0 in the assembly's per-entry order — the ICP factor, the linear factors on pose 0, the joint
// factor carried to the current poses (it must contain pose 0: member 0), the has_Z[1] tie, the edges (0, b) in list order,
// the prior, the damping — accumulated over {0} + S into A00, g0, A_S0 (6 |S| x 6), A_SS' (row stride kWindowJointDim), g_S', c
// and eliminated as window_marginal_impl eliminates: the same factorisation of A00, its pivot test, then
//   H_m = A_SS' - A_S0 A00^-1 A_S0^T,  b_m = g_S' - A_S0 A00^-1 g0,  f_m = c - g0^T A00^-1 g0.
// With S = {1} and no joint factor every value goes through the operations of window_marginal_impl, in its order.
// Returns |S| (sep: the first kWindowJointMax of them).  jt: null for none
MH_HD int window_joint_separator(const WindowEdges & ed, const WindowJoint * jt, int sep[kWindowJointMax])
{
  unsigned int mask = 2u;
  for (int e = 0; e < ed.n; ++e)
    if (ed.a[e] == 0) mask |= 1u << ed.b[e];
  for (int m = 0; jt && m < jt->n; ++m)
    if (jt->pose[m] != 0) mask |= 1u << jt->pose[m];
  int n = 0;
  for (int i = 1; i < kWindowMax; ++i)
    if ((mask >> i) & 1u) {
      if (n < kWindowJointMax) sep[n] = i;
      ++n;
    }
  return n;
}
struct WindowMarginalJointWork
{
  double H[36], b[6], f;  // the ICP factor of pose 0: H_ss, b_s, f
  double Baa[kWindowTieMax][36], E[kWindowTieMax][36], ga[kWindowTieMax][6], gb[kWindowTieMax][6], cz[kWindowTieMax];
  double A00[36], AS0[kWindowJointDim * 6], ASS[kWindowJointDim * kWindowJointDim], g0[6], gS[kWindowJointDim], c;
  double L[36], Dv[6];               // A00 = L D L^T
  double X[kWindowJointDim + 1][6];  // A00^-1 times column c of A_S0^T (c < 6 |S|), times g0 (the last)
  int degen[2];
  int ok, pad;
};
struct WindowMarginalJointOut
{
  double H[kWindowJointDim * kWindowJointDim], b[kWindowJointDim], f;  // the leading 6 |S|; zero behind
  int valid, n_ties;
  int degen[2];
};

// sums, p, st: as for window_marginal_impl, and R, t of every separator pose.  n_sep, sep: window_joint_separator's (n_sep <= kWindowJointMax).
template <typename Par>
MH_HD void window_marginal_joint_impl(const double * sums, const WindowState & st, const WindowParams & p, const WindowLinear & lin, WindowLinWork & lw,
                                      const WindowEdges & ed, const WindowJoint * jt, WindowJointWork & jw, int n_sep, const int * sep,
                                      WindowMarginalJointWork & w, WindowMarginalJointOut & out, Par & par)
{
  constexpr int S = kWindowJointDim;
  const int n_lin = lin.n, n_edge = ed.n, N = 6 * n_sep;
  const bool have = (p.have & 1u) != 0, tie = ((p.has_Z >> 1) & 1u) != 0;
  auto on0 = [&](int e, int b) { return ed.a[e] == 0 && ed.b[e] == b; };
  auto from0 = [&](int e) { return ed.a[e] == 0; };
  auto member = [&](int pose) { return jt ? window_joint_member(*jt, pose) : -1; };
  par.each(2, [&](int blk) { w.degen[blk] = have && align_block_degenerate(sums, blk, blk ? p.thresh_trans[0] : p.thresh_rot[0]) ? 1 : 0; });
  par.each(1 + n_lin + kWindowTieMax, [&](int l) {
    if (l == 0) {
      if (have) {
        AlignParams ap{};
        for (int q = 0; q < 3; ++q) ap.gz[q] = p.gz[q];
        ap.reg_4_dof = static_cast<int>(p.reg_4_dof & 1u);
        ap.project_on_degeneracy = static_cast<int>(p.project_on_degeneracy & 1u);
        align_hessian(sums, st.R[0], ap, w.degen[0] != 0, w.degen[1] != 0, w.H, w.b, w.f);
      } else {
        for (int q = 0; q < 36; ++q) w.H[q] = 0.0;
        for (int q = 0; q < 6; ++q) w.b[q] = 0.0;
        w.f = 0.0;
      }
    } else if (l <= n_lin) {
      const int j = l - 1;
      if (lin.pose[j] != 0) return;
      double d[6];
      window_local(lin.LR[j], lin.Lt[j], st.R[0], st.t[0], d);
      window_transport(lin.H[j], lin.b[j], lin.f[j], d, lw.H[j], lw.b[j], lw.f[j], lw.tmp[j]);
    } else if (l == n_lin + 1) {
      if (tie) window_between(st.R[0], st.t[0], st.R[1], st.t[1], st.ZR[1], st.Zt[1], p.Wb, w.Baa[0], w.E[0], w.ga[0], w.gb[0], w.cz[0]);
    } else {
      const int e = l - n_lin - 2;
      if (e < n_edge && from0(e)) {
        const int b = ed.b[e];
        window_between_dense(st.R[0], st.t[0], st.R[b], st.t[b], ed.ZR[e], ed.Zt[e], ed.Om[e], w.Baa[1 + e], w.E[1 + e], w.ga[1 + e], w.gb[1 + e], w.cz[1 + e]);
      }
    }
  });
  if (jt) window_joint_transport(*jt, st, jw, lw.tmp, par);  // (behind the linear factors: their scratch is free)
  par.each(36 + 6 * N + N * N + 6 + N + 1, [&](int l) {
    if (l < 36) {
      const int r = l / 6, c = l % 6;
      double a = w.H[l];
      for (int j = 0; j < n_lin; ++j)
        if (lin.pose[j] == 0) a += lw.H[j][l];
      if (jt) a += jw.H[S * r + c];
      if (tie) a += w.Baa[0][l];
      for (int e = 0; e < n_edge; ++e)
        if (from0(e)) a += w.Baa[1 + e][l];
      if (r == c) {
        a += p.prior[r];
        a += p.damping;
      }
      w.A00[l] = a;
      return;
    }
    l -= 36;
    if (l < 6 * N) {
      const int row = l / 6, c = l % 6, pose = sep[row / 6], q = 6 * (row % 6) + c, m = member(pose);
      double a = (tie && pose == 1) ? w.E[0][q] : 0.0;
      if (m >= 0) a = jw.H[S * (6 * m + row % 6) + c] + a;
      for (int e = 0; e < n_edge; ++e)
        if (on0(e, pose)) a += w.E[1 + e][q];
      w.AS0[l] = a;
      return;
    }
    l -= 6 * N;
    if (l < N * N) {
      const int row = l / N, col = l % N, pr = sep[row / 6], pc = sep[col / 6], r = row % 6, c = col % 6, mr = member(pr), mc = member(pc);
      double a = (tie && pr == 1 && pc == 1 && r == c) ? p.Wb[r] : 0.0;
      if (mr >= 0 && mc >= 0) a = jw.H[S * (6 * mr + r) + 6 * mc + c] + a;
      if (pr == pc)
        for (int e = 0; e < n_edge; ++e)
          if (on0(e, pr)) a += ed.Om[e][6 * r + c];
      w.ASS[S * row + col] = a;
      return;
    }
    l -= N * N;
    if (l < 6) {
      const int r = l;
      double g = w.b[r];
      for (int j = 0; j < n_lin; ++j)
        if (lin.pose[j] == 0) g += lw.b[j][r];
      if (jt) g += jw.b[r];
      if (tie) g += w.ga[0][r];
      for (int e = 0; e < n_edge; ++e)
        if (from0(e)) g += w.ga[1 + e][r];
      w.g0[r] = g;
      return;
    }
    l -= 6;
    if (l < N) {
      const int pose = sep[l / 6], r = l % 6, m = member(pose);
      double g = (tie && pose == 1) ? w.gb[0][r] : 0.0;
      if (m >= 0) g = jw.b[6 * m + r] + g;
      for (int e = 0; e < n_edge; ++e)
        if (on0(e, pose)) g += w.gb[1 + e][r];
      w.gS[l] = g;
      return;
    }
    double c = w.f;
    for (int j = 0; j < n_lin; ++j)
      if (lin.pose[j] == 0) c += lw.f[j];
    if (jt) c += jw.f;
    if (tie) c += w.cz[0];
    int n = tie ? 1 : 0;
    for (int e = 0; e < n_edge; ++e)
      if (from0(e)) {
        c += w.cz[1 + e];
        n += 1;
      }
    w.c = c;
    w.ok = 1;
    out.n_ties = n;
    out.degen[0] = w.degen[0];
    out.degen[1] = w.degen[1];
  });
  // A00 = L D L^T: the columns of window_factor, its pivot test
  for (int j = 0; j < 6 && w.ok; ++j) {
    par.each(6 - j, [&](int l) {
      double d = w.A00[7 * j];
      for (int k = 0; k < j; ++k) d -= w.L[6 * j + k] * w.L[6 * j + k] * w.Dv[k];
      if (l == 0) {
        w.Dv[j] = d;
        if (!(d > 0.0) || !(d < 1e300)) w.ok = 0;
      } else {
        const int row = j + l;
        double s = w.A00[6 * row + j];
        for (int k = 0; k < j; ++k) s -= w.L[6 * row + k] * w.L[6 * j + k] * w.Dv[k];
        w.L[6 * row + j] = s / d;
      }
    });
  }
  par.each(S * S + S + 1, [&](int l) {
    if (l < S * S)
      out.H[l] = 0.0;
    else if (l < S * S + S)
      out.b[l - S * S] = 0.0;
    else {
      out.f = 0.0;
      out.valid = 0;
    }
  });
  if (!w.ok) return;
  par.each(N + 1, [&](int c) { window_solve6(w.L, w.Dv, c < N ? &w.AS0[6 * c] : w.g0, w.X[c < N ? c : S]); });  // column c of A_S0^T = row c of A_S0
  // the upper triangle of H_m, mirrored
  par.each(N * (N + 1) / 2 + N + 1, [&](int l) {
    if (l < N * (N + 1) / 2) {
      int r = 0, q = l;
      while (q >= N - r) {
        q -= N - r;
        ++r;
      }
      const int c = r + q;
      double s = w.ASS[S * r + c];
      for (int m = 0; m < 6; ++m) s -= w.AS0[6 * r + m] * w.X[c][m];
      out.H[S * r + c] = s;
      out.H[S * c + r] = s;
    } else if (l < N * (N + 1) / 2 + N) {
      const int r = l - N * (N + 1) / 2;
      double s = w.gS[r];
      for (int m = 0; m < 6; ++m) s -= w.AS0[6 * r + m] * w.X[S][m];
      out.b[r] = s;
    } else {
      double s = w.c;
      for (int m = 0; m < 6; ++m) s -= w.g0[m] * w.X[S][m];
      out.f = s;
      out.valid = 1;
    }
  });
}

}  // namespace mh

#if defined(__HIPCC__)
#include "icp_device.hpp"

namespace mh
{
// window_kernels.hip — one step of an mh_icp_window_optimise chain, launched behind the staged K3 batch launches (tail = 1) of
// one iteration, whose flagged words landed in ll_dev (32 words per pose).  `next`: the argument blocks of the launches queued
// behind this step (device memory the context owns; null behind the last iteration): the step writes R, t into the block of
// every pose that has one (slot[i] >= 0), and n = 0 once the chain has stopped.
struct WindowStepArgs
{
  const uint4 * ll_dev;
  uint4 * ll_host[kWindowMax];  // pose i's factor: this iteration's slot of its pinned ring (sums + counters are forwarded there)
  uint4 * row_host;             // the iteration's row in mapped pinned memory
  IcpArgs * next;
  WindowState * state;
  WindowParams p;
  signed char slot[kWindowMax];  // pose i's argument block within an iteration's blocks (-1: empty factor, none)
  unsigned int seq;              // tags K3's words of this iteration and everything this step publishes
};
hipError_t launch_window_step(const WindowStepArgs & a, hipStream_t stream);

// One step of an mh_icp_window_optimise_relin chain: as above, and the step decides per factor whether the iteration queued
// behind it evaluates it (n left alone in its argument block) or keeps its linearization (n = 0); it expects K3's words of the
// factors the step in front of it chose, forwards those alone, and publishes the iteration's evaluated mask behind the row.
struct WindowRelinStepArgs
{
  WindowStepArgs s;
  WindowRelin * relin;  // device memory the context owns; needs no initialisation (rp.first)
  uint4 * mask_host;    // the iteration's evaluated mask as one flagged word in mapped pinned memory
  WindowRelinParams rp;
};
hipError_t launch_window_relin_step(const WindowRelinStepArgs & a, hipStream_t stream);

// One step of an mh_icp_window_optimise_lin chain (window_lin_kernels.hip): either of the above (relin: with the decisions),
// with the linear factors of `lin`, which the host wrote once per call.
struct WindowLinStepArgs
{
  WindowRelinStepArgs r;     // relin == false: r.relin, r.mask_host, r.rp unused
  const WindowLinear * lin;  // device memory the context owns
};
hipError_t launch_window_lin_step(const WindowLinStepArgs & a, bool relin, hipStream_t stream);

// One step of an mh_icp_window_optimise_edges chain (window_edge_kernels.hip): the lin step with the edges of `edges`, which
// the host wrote once per call, solved over the row profile.
struct WindowEdgeStepArgs
{
  WindowLinStepArgs l;
  const WindowEdges * edges;  // device memory the context owns
};
hipError_t launch_window_edge_step(const WindowEdgeStepArgs & a, bool relin, hipStream_t stream);

// mh_icp_window_marginalise (window_marginal_kernels.hip): launched behind the one staged K3 launch (tail = 1) of the oldest
// factor, whose flagged words landed in ll_dev (32 words; none when the factor is empty).  The kernel forwards them to ll_host,
// runs window_marginal_impl at the poses of `state` and publishes one row of kWMargWords flagged words.
enum WindowMarginalRow
{
  kWMargValid = 0,
  kWMargTies,
  kWMargF,
  kWMargBits,  // 8: the factor's sums were missing (nothing was computed)
  kWMargB = 4,
  kWMargH = 10,
  kWMargWords = 46,
};
struct WindowMarginalArgs
{
  const uint4 * ll_dev;
  uint4 * ll_host;   // slot 0 of the factor's pinned ring (null: empty factor)
  uint4 * row_host;  // the row in mapped pinned memory
  const WindowState * state;
  const WindowLinear * lin;
  const WindowEdges * edges;
  WindowParams p;
  unsigned int seq;
};
hipError_t launch_window_marginal(const WindowMarginalArgs & a, hipStream_t stream);

// One step of an mh_icp_window_optimise_joint chain (window_joint_kernels.hip): the edge step with the joint factor `joint`,
// which the host wrote once per call.
struct WindowJointStepArgs
{
  WindowEdgeStepArgs e;
  const WindowJoint * joint;  // device memory the context owns
};
hipError_t launch_window_joint_step(const WindowJointStepArgs & a, bool relin, hipStream_t stream);

// mh_icp_window_marginalise_joint (window_joint_kernels.hip): as launch_window_marginal, with the joint factor (null: none) and
// the separator the host worked out; the kernel publishes one row of kWJMargWords flagged words.
enum WindowJointMarginalRow
{
  kWJMargValid = 0,
  kWJMargTies,
  kWJMargF,
  kWJMargBits,  // 8: the factor's sums were missing (nothing was computed)
  kWJMargB = 4,
  kWJMargH = kWJMargB + kWindowJointDim,
  kWJMargWords = kWJMargH + kWindowJointDim * kWindowJointDim,
};
struct WindowMarginalJointArgs
{
  WindowMarginalArgs m;
  const WindowJoint * joint;
  int n_sep, sep[kWindowJointMax];
};
hipError_t launch_window_marginal_joint(const WindowMarginalJointArgs & a, hipStream_t stream);
}  // namespace mh
#endif
