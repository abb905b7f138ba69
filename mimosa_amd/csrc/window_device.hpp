// One Gauss-Newton iteration over a fixed-lag window of poses (mh_icp_window_optimise): from the 28 Hessian sums K3 folded for
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

// w.A, w.E, w.rhs, w.cost from the factors' sums at the poses of `st`
template <typename Par>
MH_HD void window_assemble(const double * sums, const WindowState & st, const WindowParams & p, WindowWork & w, Par & par)
{
  const int W = p.W;
  par.each(2 * W, [&](int l) {
    const int i = l >> 1, blk = l & 1;
    w.degen[l] = ((p.have >> i) & 1u) && align_block_degenerate(sums + 32 * i, blk, blk ? p.thresh_trans[i] : p.thresh_rot[i]) ? 1 : 0;
  });
  par.each(W, [&](int i) {
    if ((p.have >> i) & 1u) {
      AlignParams ap{};
      for (int q = 0; q < 3; ++q) ap.gz[q] = p.gz[q];
      ap.reg_4_dof = static_cast<int>((p.reg_4_dof >> i) & 1u);
      ap.project_on_degeneracy = static_cast<int>((p.project_on_degeneracy >> i) & 1u);
      align_hessian(sums + 32 * i, st.R[i], ap, w.degen[2 * i] != 0, w.degen[2 * i + 1] != 0, w.H[i], w.b[i], w.f[i]);
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
  // per entry in the order optimise() adds: the factor, the between factors in window order, the prior, the damping
  par.each(36 * W + 6 * W + 1, [&](int l) {
    if (l < 36 * W) {
      const int i = l / 36, e = l % 36, r = e / 6, c = e % 6;
      double a = w.H[i][e];
      if (r == c && ((p.has_Z >> i) & 1u)) a += p.Wb[r];
      if (i + 1 < W && ((p.has_Z >> (i + 1)) & 1u)) a += w.Baa[i + 1][e];
      if (r == c) {
        if (i == 0) a += p.prior[r];
        a += p.damping;
      }
      w.A[i][e] = a;
    } else if (l < 42 * W) {
      const int q = l - 36 * W, i = q / 6, r = q % 6;
      double g = w.b[i][r];
      if ((p.has_Z >> i) & 1u) g += w.gb[i][r];
      if (i + 1 < W && ((p.has_Z >> (i + 1)) & 1u)) g += w.ga[i + 1][r];
      w.rhs[q] = -g;
    } else {
      double cost = 0.0;
      for (int i = 0; i < W; ++i) cost += w.f[i];
      for (int i = 1; i < W; ++i)
        if ((p.has_Z >> i) & 1u) cost += w.cz[i];
      w.cost = cost;
    }
  });
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

// One queued iteration: the chain's state in, the state and the iteration's row out.  sums: 32 doubles per pose (28 sums +
// 4 counters; ignored where p.have has no bit).  arrived: the words of every factor carry the call's number (they always do; a
// chain that finds otherwise stops).  Returns the row's flags.  Once st.stopped is set the poses are passed on unchanged.
template <typename Par>
MH_HD int window_advance(WindowState & st, const double * sums, bool arrived, const WindowParams & p, WindowWork & w, double * row, Par & par)
{
  const int W = p.W;
  const bool frozen = st.stopped != 0;
  par.sync();  // (every index has read the state before index 0 changes it)
  bool stepped = false;
  if (!frozen && arrived) {
    window_assemble(sums, st, p, w, par);
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
    }
    row[kWRowFlags] = static_cast<double>(flags);
    row[kWRowIters] = static_cast<double>(st.iters);
  });
  return static_cast<int>(row[kWRowFlags]);
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
}  // namespace mh
#endif
