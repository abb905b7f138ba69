// One Gauss-Newton iteration of a pose graph over all keyframes (mh_pose_graph_optimise, pose_graph_api.hip): N poses, E
// relative-pose edges with dense information matrices, some poses held fixed.  The residual, J_a = -Ad(T_ab^-1), J_b = I and
// the retraction are the window chains' (window_device.hpp: window_between_dense, window_so3log, window_adjoint,
// window_solve6, align_retract), used here and not restated.
//
// The edges are split into near ones (pose_b - pose_a == 1) and far ones (>= 2; at most kPgoFarMax, on a
// graph created wide at most its max_far <= kPgoFarLimit: the section "a wide graph" below).  The system is
//   A = T + sum_f W_f^T Om_f W_f,
// T block-tridiagonal (near edges, damping, identity rows of the fixed poses), W_f the 6 x 6N matrix with J_a in block column
// a and I in block column b of far edge f (a block column of a fixed pose zeroed).  It is solved as
//   Y = T^-1 [W^T | rhs]   (6F + 1 columns),   C = blockdiag(Om_f^-1) + W Y[:, :6F],   x = y - Y C^-1 W y,  y = Y[:, 6F],
// T by the block L D L^T of window_factor, C by L D L^T without pivoting, followed by the chains' two refinement steps with
// the residual against A itself accumulated in twice the working precision.  T must be positive definite by itself: a run
// of poses joined by near edges needs a fixed pose or damping.  A pivot of T, of an Om_f or of C that is not positive takes
// no step (bit 4 of the row's flags).
//
// Plain fp64 for the device (pose_graph_kernels.hip) and the host (tests/cpp/pose_graph_step.cpp under g++), both compiled
// without floating-point contraction.  Work that is independent per index is a function of the index (pgo_edge, pgo_gather,
// pgo_sweep_col): the host loops over it, the kernels give an index to a lane.  Work of one workgroup is written as PHASES
// over a `Par` executor, as in window_device.hpp.  Nothing is summed by atomics: a pose's contributions are added in
// edge-list order from its incidence list, the cost is folded as sum_{l < 256} (sum_k c[l + 256 k]), k and l ascending.
//
// Priors and losses (mh_pose_graph_set_priors, mh_pose_graph_set_loss).  Prior p on pose i is term E + p of the edge pass
// (pgo_term): d = window_local(Z, T_i), and window_transport of the model (Om, 0, 0) by d gives M^T Om M, M^T Om d and
// s = d^T Om d, M = blockdiag(Jr^-1(d_r), Exp(d_r)).  Every term has a weight w and a cost rho from its chi^2 s (pgo_loss).  The
// per-term products stay unweighted in memory; w multiplies an entry WHERE IT IS READ into a sum or a matrix — in pgo_gather, in
// pgo_far_info (w_f Om_f is what is factorised and inverted) and in pgo_residual_row — as one product w * entry, rounded, before
// the addition.  With w == 1.0 that product is the entry itself, so a graph without priors and losses keeps its bits.  A pose's
// sums run over its edges in edge-list order, then over its priors in prior-list order, then the damping; the cost fold runs
// over c[j] = rho of term j, j < E + P, edges then priors.
#pragma once

#include <cstddef>

#include "window_device.hpp"

namespace mh
{
constexpr int kPgoMaxPoses = 4096;
constexpr int kPgoMaxEdges = 32768;
constexpr int kPgoFarMax = 32;
constexpr int kPgoFarLimit = 512;  // far edges of a graph created wide (mh_pose_graph_create_wide)
constexpr int kPgoWideNB = 64;     // panel width of the blocked phases of C: diagonal blocks, strips and tiles are NB x NB
constexpr int kPgoWideLd = 65;     // row stride of a block that is read down a column (one block in a workgroup's LDS)
constexpr int kPgoWideSm = 2 * kPgoWideNB * kPgoWideNB;  // doubles a blocked phase shares (the host's buffer, the kernel's LDS: 64 KiB)
constexpr int kPgoFold = 256;   // partial sums of the cost fold (a constant of the rule, not of a launch)
constexpr int kPgoMaxIters = 64;
constexpr int kPgoGather = 78;  // outputs per pose of pgo_gather: 36 of A_ii, 36 of E_i, 6 of the right-hand side

struct PgoParams
{
  double damping, eps_rot, eps_trans;
};
struct PgoRow
{
  double f, step_rot, step_trans;
  int flags, iters;  // flags: 1 stopped after this step | 2 converged | 4 a pivot was not positive (no step)
};
struct PgoState
{
  int stopped, converged, iters, ok;
};

struct PgoGraph
{
  int N, E, F, K;  // K = 6 F + 1: the columns of Y
  double *R, *t;                           // 9 N, 3 N: the poses the chain has reached
  double *ZR, *Zt, *Om;                    // per edge: the measurement and its information matrix
  double *Baa, *Eba, *ga, *gb, *cz, *res;  // per edge: window_between_dense's outputs; the residual (6)
  double *Ja, *OmL, *OmD, *OmInv;          // per far edge: J_a; Om = L D L^T; Om^-1
  double *A, *Eb, *rhs;                    // T's diagonal blocks, its blocks (i, i - 1), the right-hand side -g
  double *L, *Dv, *G;                      // S_i = L D L^T, G_i = S_{i-1}^-1 E_i^T
  double *Y;                               // 6 N x K, row-major
  double *C, *u;                           // 6 F x 6 F (lower: L, diagonal: D, upper: L D), 6 F
  double * v;                              // 6 F: the blocked solve's second vector (pgo_wide_forward / _backward)
  double *x, *r, *y1, *d;                  // 6 N each (d: the step norms of pgo_finish)
  double *fold;                            // 3 x kPgoFold
  PgoRow * rows;                           // kPgoMaxIters
  int *ea, *eb, *eslot;                    // per edge: its poses; its far slot (-1: a near edge)
  int *inc_off, *inc;                      // N + 1; 2 E: pose i's edges in list order, (e << 1) | (i is the edge's b)
  int * far;                               // F: the far edges, in list order
  unsigned char * fixed;                   // N
  PgoState * st;
  // priors and losses; all zero (P, every kind): none
  int P;                                   // priors: the terms E .. E + P of the edge pass
  double *w, *rho, *lparam;                // per edge: the weight and cost pgo_loss gave; the loss's parameter
  int * lkind;                             // per edge: the loss's kind (kPgoLoss*)
  double *pZR, *pZt, *pOm;                 // per prior: the measured pose and its information matrix
  double *pH, *pg, *pres, *pcz;            // per prior: M^T Om M, M^T Om d, d, d^T Om d
  double *pw, *prho, *plparam;             // per prior: as w, rho, lparam
  int *plkind, *ppose;                     // per prior: as lkind; its pose
  int *pinc_off, *pinc;                    // N + 1; P: pose i's priors in list order
};
enum PgoLossKind
{
  kPgoLossNone, kPgoLossHuber, kPgoLossCauchy, kPgoLossDcs
};
constexpr double kPgoMinWeight = 1e-12;  // a smaller w is taken as this: Om_f^-1 / w stays far below the pivot test's 1e300

// Byte offsets of every array in one block for at most maxN poses and maxE edges; returns the block's size.
enum PgoArray
{
  kPgR, kPgT, kPgZR, kPgZt, kPgOm, kPgBaa, kPgEba, kPgGa, kPgGb, kPgCz, kPgRes, kPgJa, kPgOmL, kPgOmD, kPgOmInv, kPgA, kPgEb, kPgRhs, kPgL,
  kPgDv, kPgG, kPgY, kPgC, kPgU, kPgX, kPgRr, kPgY1, kPgD, kPgFold, kPgRows, kPgEa, kPgEbI, kPgSlot, kPgIncOff, kPgInc, kPgFar, kPgFixed, kPgSt,
  kPgW, kPgRho, kPgLParam, kPgLKind, kPgPZR, kPgPZt, kPgPOm, kPgPH, kPgPG, kPgPRes, kPgPCz, kPgPW, kPgPRho, kPgPLParam, kPgPLKind, kPgPPose,
  kPgPIncOff, kPgPInc, kPgV,
  kPgArrays
};
inline size_t pgo_layout(size_t maxN, size_t maxE, size_t off[kPgArrays], size_t maxF = kPgoFarMax)
{
  const size_t F = maxF, K = 6 * F + 1, D = sizeof(double), I = sizeof(int);
  const size_t bytes[kPgArrays] = {9 * maxN * D, 3 * maxN * D, 9 * maxE * D, 3 * maxE * D, 36 * maxE * D, 36 * maxE * D, 36 * maxE * D, 6 * maxE * D,
                                   6 * maxE * D, maxE * D, 6 * maxE * D, 36 * F * D, 36 * F * D, 6 * F * D, 36 * F * D, 36 * maxN * D, 36 * maxN * D,
                                   6 * maxN * D, 36 * maxN * D, 6 * maxN * D, 36 * maxN * D, 6 * maxN * K * D, 36 * F * F * D, 6 * F * D, 6 * maxN * D,
                                   6 * maxN * D, 6 * maxN * D, 6 * maxN * D, 3 * kPgoFold * D, kPgoMaxIters * sizeof(PgoRow), maxE * I, maxE * I, maxE * I,
                                   (maxN + 1) * I, 2 * maxE * I, F * I, maxN, sizeof(PgoState),
                                   maxE * D, maxE * D, maxE * D, maxE * I, 9 * maxN * D, 3 * maxN * D, 36 * maxN * D, 36 * maxN * D, 6 * maxN * D,
                                   6 * maxN * D, maxN * D, maxN * D, maxN * D, maxN * D, maxN * I, maxN * I, (maxN + 1) * I, maxN * I, 6 * F * D};
  size_t at = 0;
  for (int k = 0; k < kPgArrays; ++k) {
    off[k] = at;
    at += (bytes[k] + 15) / 16 * 16;
  }
  return at;
}
inline void pgo_bind(PgoGraph & g, char * base, const size_t off[kPgArrays])
{
  auto dp = [&](int k) { return reinterpret_cast<double *>(base + off[k]); };
  auto ip = [&](int k) { return reinterpret_cast<int *>(base + off[k]); };
  g.R = dp(kPgR), g.t = dp(kPgT), g.ZR = dp(kPgZR), g.Zt = dp(kPgZt), g.Om = dp(kPgOm);
  g.Baa = dp(kPgBaa), g.Eba = dp(kPgEba), g.ga = dp(kPgGa), g.gb = dp(kPgGb), g.cz = dp(kPgCz), g.res = dp(kPgRes);
  g.Ja = dp(kPgJa), g.OmL = dp(kPgOmL), g.OmD = dp(kPgOmD), g.OmInv = dp(kPgOmInv);
  g.A = dp(kPgA), g.Eb = dp(kPgEb), g.rhs = dp(kPgRhs), g.L = dp(kPgL), g.Dv = dp(kPgDv), g.G = dp(kPgG);
  g.Y = dp(kPgY), g.C = dp(kPgC), g.u = dp(kPgU), g.x = dp(kPgX), g.r = dp(kPgRr), g.y1 = dp(kPgY1), g.d = dp(kPgD), g.fold = dp(kPgFold);
  g.rows = reinterpret_cast<PgoRow *>(base + off[kPgRows]);
  g.ea = ip(kPgEa), g.eb = ip(kPgEbI), g.eslot = ip(kPgSlot), g.inc_off = ip(kPgIncOff), g.inc = ip(kPgInc), g.far = ip(kPgFar);
  g.fixed = reinterpret_cast<unsigned char *>(base + off[kPgFixed]);
  g.st = reinterpret_cast<PgoState *>(base + off[kPgSt]);
  g.w = dp(kPgW), g.rho = dp(kPgRho), g.lparam = dp(kPgLParam), g.lkind = ip(kPgLKind);
  g.pZR = dp(kPgPZR), g.pZt = dp(kPgPZt), g.pOm = dp(kPgPOm), g.pH = dp(kPgPH), g.pg = dp(kPgPG), g.pres = dp(kPgPRes), g.pcz = dp(kPgPCz);
  g.pw = dp(kPgPW), g.prho = dp(kPgPRho), g.plparam = dp(kPgPLParam), g.plkind = ip(kPgPLKind), g.ppose = ip(kPgPPose);
  g.pinc_off = ip(kPgPIncOff), g.pinc = ip(kPgPInc);
  g.v = dp(kPgV);
}

// host: the index arrays of an edge list (ea, eb: E entries, 0 <= ea < eb < N) — every edge's far slot (-1: near), the far
// edges in list order, and per pose its incidence list in edge-list order.  Returns the number of far edges; `far` takes
// far_cap entries at most (the caller refuses a list with more before it gets here).
inline int pgo_index_edges(int N, int E, const int * ea, const int * eb, int * eslot, int * inc_off, int * inc, int * far, int far_cap = kPgoFarMax)
{
  int F = 0;
  for (int i = 0; i <= N; ++i) inc_off[i] = 0;
  for (int e = 0; e < E; ++e) {
    eslot[e] = -1;
    if (eb[e] - ea[e] >= 2) {
      if (F < far_cap) far[F] = e;
      eslot[e] = F++;
    }
    ++inc_off[ea[e] + 1];
    ++inc_off[eb[e] + 1];
  }
  for (int i = 0; i < N; ++i) inc_off[i + 1] += inc_off[i];
  // ascending e: every pose's list is in edge-list order (the running fill position of pose i is kept in inc_off[i] and put back)
  for (int e = 0; e < E; ++e) {
    inc[inc_off[ea[e]]++] = e << 1;
    inc[inc_off[eb[e]]++] = (e << 1) | 1;
  }
  for (int i = N; i > 0; --i) inc_off[i] = inc_off[i - 1];
  inc_off[0] = 0;
  return F;
}

// host: per pose its priors in prior-list order (ppose: P entries, 0 <= ppose < N)
inline void pgo_index_priors(int N, int P, const int * ppose, int * pinc_off, int * pinc)
{
  for (int i = 0; i <= N; ++i) pinc_off[i] = 0;
  for (int p = 0; p < P; ++p) ++pinc_off[ppose[p] + 1];
  for (int i = 0; i < N; ++i) pinc_off[i + 1] += pinc_off[i];
  for (int p = 0; p < P; ++p) pinc[pinc_off[ppose[p]]++] = p;
  for (int i = N; i > 0; --i) pinc_off[i] = pinc_off[i - 1];
  pinc_off[0] = 0;
}

// ---- the loss of a term ------------------------------------------------------------------------------------------------------------
// w and rho of a term whose chi^2 is s.  kind 0: w = 1, rho = s as it is.  Huber (k): w = 1, rho = s up to s = k^2, then
// w = k / sqrt(s), rho = 2 k sqrt(s) - k^2.  Cauchy (k): w = 1 / (1 + s / k^2), rho = k^2 log(1 + s / k^2).  DCS (Phi):
// c = min(1, 2 Phi / (Phi + s)), w = c^2, rho = c^2 s + Phi (1 - c)^2.  Kinds 1 .. 3 read an s that is not positive (zero; an
// indefinite info) as 0, which keeps sqrt and log inside their domains; w is not below kPgoMinWeight.
MH_HD void pgo_loss(int kind, double param, double s, double & w, double & rho)
{
  w = 1.0;
  rho = s;
  if (kind == kPgoLossNone) return;
  const double sp = s > 0.0 ? s : 0.0;
  if (kind == kPgoLossHuber) {
    const double k2 = param * param;
    rho = sp;
    if (sp > k2) {
      const double q = sqrt(sp);
      w = param / q;
      rho = 2.0 * param * q - k2;
    }
  } else if (kind == kPgoLossCauchy) {
    const double k2 = param * param, u = 1.0 + sp / k2;
    w = 1.0 / u;
    rho = k2 * log(u);
  } else {
    const double c0 = 2.0 * param / (param + sp), c = c0 < 1.0 ? c0 : 1.0;
    w = c * c;
    rho = w * sp + param * ((1.0 - c) * (1.0 - c));
  }
  if (w < kPgoMinWeight) w = kPgoMinWeight;
}

// ---- per edge --------------------------------------------------------------------------------------------------------------------
// Edge e at the current poses.  A far edge also leaves J_a = -Ad(T_ab^-1) in its slot; want_res: the residual itself into g.res.
MH_HD void pgo_edge(const PgoGraph & g, int e, bool want_res)
{
  const int a = g.ea[e], b = g.eb[e], f = g.eslot[e];
  const double *Ra = g.R + 9 * a, *ta = g.t + 3 * a, *Rb = g.R + 9 * b, *tb = g.t + 3 * b;
  window_between_dense(Ra, ta, Rb, tb, g.ZR + 9 * e, g.Zt + 3 * e, g.Om + 36 * e, g.Baa + 36 * e, g.Eba + 36 * e, g.ga + 6 * e, g.gb + 6 * e, g.cz[e]);
  pgo_loss(g.lkind[e], g.lparam[e], g.cz[e], g.w[e], g.rho[e]);
  if (f < 0 && !want_res) return;
  double Rat[9], abR[9], abt[3];
  win_tr(Ra, Rat);
  win_mm(Rat, Rb, abR);
  const double dt[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
  win_mv(Rat, dt, abt);
  if (f >= 0) {
    double Rabt[9], tinv[3], Ad[36];
    win_tr(abR, Rabt);
    const double nt[3] = {-abt[0], -abt[1], -abt[2]};
    win_mv(Rabt, nt, tinv);
    window_adjoint(Rabt, tinv, Ad);
    for (int q = 0; q < 36; ++q) g.Ja[36 * f + q] = -Ad[q];
  }
  if (want_res) {
    double Rzt[9], Re[9];
    win_tr(g.ZR + 9 * e, Rzt);
    win_mm(Rzt, abR, Re);
    const double de[3] = {abt[0] - g.Zt[3 * e], abt[1] - g.Zt[3 * e + 1], abt[2] - g.Zt[3 * e + 2]};
    window_so3log(Re, g.res + 6 * e);
    win_mv(Rzt, de, g.res + 6 * e + 3);
  }
}

// ---- per prior --------------------------------------------------------------------------------------------------------------------
// Prior p at the current pose of its keyframe: the model (Om, 0, 0) around Z seen from the offset d (window_transport).
MH_HD void pgo_prior(const PgoGraph & g, int p)
{
  const int i = g.ppose[p];
  const double zero[6] = {0, 0, 0, 0, 0, 0};
  double d[6], tmp[36];
  window_local(g.pZR + 9 * p, g.pZt + 3 * p, g.R + 9 * i, g.t + 3 * i, d);
  window_transport(g.pOm + 36 * p, zero, 0.0, d, g.pH + 36 * p, g.pg + 6 * p, g.pcz[p], tmp);
  for (int q = 0; q < 6; ++q) g.pres[6 * p + q] = d[q];
  pgo_loss(g.plkind[p], g.plparam[p], g.pcz[p], g.pw[p], g.prho[p]);
}
// term j of the edge pass: an edge, or prior j - E
MH_HD void pgo_term(const PgoGraph & g, int j, bool want_res)
{
  if (j < g.E)
    pgo_edge(g, j, want_res);
  else
    pgo_prior(g, j - g.E);
}

// ---- per pose: T and the right-hand side ----------------------------------------------------------------------------------------
// Output l % kPgoGather of pose l / kPgoGather, each sum over the pose's incidence list in edge-list order.  A fixed pose: the
// identity block, no off-diagonal block on either side, a zero right-hand side.  Far edges go into the right-hand side only.
// Every entry read is multiplied by its term's weight; the pose's priors follow its edges.
MH_HD void pgo_gather(const PgoGraph & g, const PgoParams & p, int l)
{
  const int i = l / kPgoGather, q = l % kPgoGather;
  const bool fx = g.fixed[i] != 0;
  const int * inc = g.inc + g.inc_off[i];
  const int n = g.inc_off[i + 1] - g.inc_off[i];
  const int * pinc = g.pinc + (g.P > 0 ? g.pinc_off[i] : 0);
  const int np = g.P > 0 ? g.pinc_off[i + 1] - g.pinc_off[i] : 0;
  if (q < 36) {
    double a = 0.0;
    if (fx) {
      a = (q / 6 == q % 6) ? 1.0 : 0.0;
    } else {
      for (int k = 0; k < n; ++k) {
        const int e = inc[k] >> 1;
        if (g.eslot[e] >= 0) continue;
        a += g.w[e] * ((inc[k] & 1) ? g.Om[36 * e + q] : g.Baa[36 * e + q]);
      }
      for (int k = 0; k < np; ++k) a += g.pw[pinc[k]] * g.pH[36 * pinc[k] + q];
      if (q / 6 == q % 6) a += p.damping;
    }
    g.A[36 * i + q] = a;
  } else if (q < 72) {
    const int c = q - 36;
    double a = 0.0;
    if (!fx && i > 0 && !g.fixed[i - 1])
      for (int k = 0; k < n; ++k) {
        const int e = inc[k] >> 1;
        if ((inc[k] & 1) && g.eslot[e] < 0) a += g.w[e] * g.Eba[36 * e + c];
      }
    g.Eb[36 * i + c] = a;
  } else {
    const int r = q - 72;
    double s = 0.0;
    if (!fx) {
      for (int k = 0; k < n; ++k) {
        const int e = inc[k] >> 1;
        s += g.w[e] * ((inc[k] & 1) ? g.gb[6 * e + r] : g.ga[6 * e + r]);
      }
      for (int k = 0; k < np; ++k) s += g.pw[pinc[k]] * g.pg[6 * pinc[k] + r];
    }
    g.rhs[6 * i + r] = fx ? 0.0 : -s;
  }
}

// ---- per far edge: w Om = L D L^T and (w Om)^-1 -----------------------------------------------------------------------------------
MH_HD bool pgo_far_info(const PgoGraph & g, int f)
{
  const double * Sf = g.Om + 36 * g.far[f];
  const double wf = g.w[g.far[f]];
  double S[36];
  for (int q = 0; q < 36; ++q) S[q] = wf * Sf[q];
  double *L = g.OmL + 36 * f, *D = g.OmD + 6 * f;
  for (int q = 0; q < 36; ++q) L[q] = 0.0;
  for (int j = 0; j < 6; ++j) {
    double d = S[7 * j];
    for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k] * D[k];
    D[j] = d;
    if (!(d > 0.0) || !(d < 1e300)) return false;
    for (int row = j + 1; row < 6; ++row) {
      double s = S[6 * row + j];
      for (int k = 0; k < j; ++k) s -= L[6 * row + k] * L[6 * j + k] * D[k];
      L[6 * row + j] = s / d;
    }
  }
  for (int c = 0; c < 6; ++c) {
    double e[6] = {0, 0, 0, 0, 0, 0}, col[6];
    e[c] = 1.0;
    window_solve6(L, D, e, col);
    for (int m = 0; m < 6; ++m) g.OmInv[36 * f + 6 * m + c] = col[m];
  }
  return true;
}

// ---- T = block L D L^T: window_factor over N blocks -----------------------------------------------------------------------------
// sm: 114 doubles the phases share (the host's stack, the kernel's LDS): S, then the current block's L, D and G.
// false (g.st->ok == 0): a pivot is not positive.
template <typename Par>
MH_HD bool pgo_factor(const PgoGraph & g, double * sm, Par & par)
{
  double *S = sm, *Lc = sm + 36, *Dc = sm + 72, *Gc = sm + 78;
  for (int i = 0; i < g.N; ++i) {
    par.each(36, [&](int l) {
      const int r = l / 6, c = l % 6;
      double s = g.A[36 * i + l];
      if (i > 0)
        for (int m = 0; m < 6; ++m) s -= g.Eb[36 * i + 6 * r + m] * Gc[6 * m + c];
      S[l] = s;
      Lc[l] = 0.0;
    });
    for (int j = 0; j < 6; ++j) {
      par.each(6 - j, [&](int l) {
        double d = S[7 * j];
        for (int k = 0; k < j; ++k) d -= Lc[6 * j + k] * Lc[6 * j + k] * Dc[k];
        if (l == 0) {
          Dc[j] = d;
          if (!(d > 0.0) || !(d < 1e300)) g.st->ok = 0;
        } else {
          const int row = j + l;
          double s = S[6 * row + j];
          for (int k = 0; k < j; ++k) s -= Lc[6 * row + k] * Lc[6 * j + k] * Dc[k];
          Lc[6 * row + j] = s / d;
        }
      });
      if (!g.st->ok) return false;
    }
    par.each(42, [&](int l) {
      if (l < 36)
        g.L[36 * i + l] = Lc[l];
      else
        g.Dv[6 * i + l - 36] = Dc[l - 36];
    });
    if (i + 1 < g.N) {
      par.each(6, [&](int c) {
        double col[6];
        window_solve6(Lc, Dc, &g.Eb[36 * (i + 1) + 6 * c], col);  // column c of E^T = row c of E
        for (int m = 0; m < 6; ++m) Gc[6 * m + c] = col[m];
      });
      par.each(36, [&](int l) { g.G[36 * (i + 1) + l] = Gc[l]; });
    }
  }
  return true;
}

// ---- T out = v for one column: window_sweep over N blocks -----------------------------------------------------------------------
// col < 6 F: column col of W^T; col == 6 F: the right-hand side; src != nullptr: that vector instead (`src_stride` doubles
// between its rows; it may be `out` itself); unit >= 0: the unit vector of that row instead.  out has `stride` doubles between
// rows.  One lane per column; L_i, D_i, G_i are the same for every column.
MH_HD void pgo_sweep_col(const PgoGraph & g, int col, const double * src, double * out, int stride, int src_stride = 1, int unit = -1)
{
  const int N = g.N;
  int fa = -1, fb = -1, f = 0, c = 0;
  if (!src && unit < 0 && col < 6 * g.F) {
    f = col / 6, c = col % 6;
    const int e = g.far[f];
    fa = g.fixed[g.ea[e]] ? -1 : g.ea[e];
    fb = g.fixed[g.eb[e]] ? -1 : g.eb[e];
  }
  double y[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < N; ++i) {
    double v[6];
    for (int r = 0; r < 6; ++r) {
      double s;
      if (unit >= 0)
        s = 6 * i + r == unit ? 1.0 : 0.0;
      else if (src)
        s = src[static_cast<size_t>(6 * i + r) * src_stride];
      else if (col == 6 * g.F)
        s = g.rhs[6 * i + r];
      else
        s = i == fa ? g.Ja[36 * f + 6 * c + r] : (i == fb && r == c ? 1.0 : 0.0);
      if (i > 0)
        for (int m = 0; m < 6; ++m) s -= g.G[36 * i + 6 * m + r] * y[m];
      v[r] = s;
    }
    for (int r = 0; r < 6; ++r) {
      y[r] = v[r];
      out[static_cast<size_t>(6 * i + r) * stride] = v[r];
    }
  }
  double xn[6] = {0, 0, 0, 0, 0, 0};
  for (int i = N - 1; i >= 0; --i) {
    double yi[6], z[6];
    for (int r = 0; r < 6; ++r) yi[r] = out[static_cast<size_t>(6 * i + r) * stride];
    window_solve6(g.L + 36 * i, g.Dv + 6 * i, yi, z);
    for (int r = 0; r < 6; ++r) {
      double s = z[r];
      if (i + 1 < N)
        for (int m = 0; m < 6; ++m) s -= g.G[36 * (i + 1) + 6 * r + m] * xn[m];
      yi[r] = s;
    }
    for (int r = 0; r < 6; ++r) {
      xn[r] = yi[r];
      out[static_cast<size_t>(6 * i + r) * stride] = yi[r];
    }
  }
}

// ---- the far edges' correction ----------------------------------------------------------------------------------------------------
// row `row` of W times the vector y (`stride` doubles between its entries)
MH_HD double pgo_W_row(const PgoGraph & g, int row, const double * y, int stride)
{
  const int f = row / 6, p = row % 6, e = g.far[f], a = g.ea[e], b = g.eb[e];
  double s = 0.0;
  if (!g.fixed[a])
    for (int r = 0; r < 6; ++r) s += g.Ja[36 * f + 6 * p + r] * y[static_cast<size_t>(6 * a + r) * stride];
  if (!g.fixed[b]) s += y[static_cast<size_t>(6 * b + p) * stride];
  return s;
}

// C = blockdiag(Om^-1) + W Y, then C = L D L^T in place, column by column: the lower triangle is read, L replaces it, the
// pivots stay on the diagonal, the upper triangle keeps L D.  false (g.st->ok == 0): a pivot is not positive.
template <typename Par>
MH_HD bool pgo_factor_C(const PgoGraph & g, Par & par)
{
  const int n = 6 * g.F, K = g.K;
  par.each(n * n, [&](int l) {
    const int row = l / n, col = l % n;
    double s = pgo_W_row(g, row, g.Y + col, K);
    if (row / 6 == col / 6) s = g.OmInv[36 * (row / 6) + 6 * (row % 6) + col % 6] + s;
    g.C[l] = s;
  });
  for (int j = 0; j < n; ++j) {
    par.each(1, [&](int) {
      const double d = g.C[j * n + j];
      if (!(d > 0.0) || !(d < 1e300)) g.st->ok = 0;
    });
    if (!g.st->ok) return false;
    par.each(n - j - 1, [&](int l) {
      const int i = j + 1 + l;
      const double t = g.C[i * n + j];
      g.C[j * n + i] = t;
      g.C[i * n + j] = t / g.C[j * n + j];
    });
    const int m = n - j - 1;
    par.each(m * m, [&](int l) {
      const int i = j + 1 + l / m, k = j + 1 + l % m;
      if (k > i) return;
      g.C[i * n + k] -= g.C[i * n + j] * g.C[j * n + k];
    });
  }
  return true;
}

// u = C^-1 W y  (y: `stride` doubles between entries), by the factors pgo_factor_C left
template <typename Par>
MH_HD void pgo_solve_C(const PgoGraph & g, const double * y, int stride, Par & par)
{
  const int n = 6 * g.F;
  par.each(n, [&](int row) { g.u[row] = pgo_W_row(g, row, y, stride); });
  for (int j = 0; j + 1 < n; ++j) par.each(n - j - 1, [&](int l) { g.u[j + 1 + l] -= g.C[(j + 1 + l) * n + j] * g.u[j]; });
  par.each(n, [&](int j) { g.u[j] = g.u[j] / g.C[j * n + j]; });
  for (int j = n - 1; j >= 1; --j) par.each(j, [&](int i) { g.u[i] -= g.C[j * n + i] * g.u[j]; });
}

// entry `row` of y - Y u for the entry y of one column and its u (`ustride` doubles between entries)
MH_HD double pgo_apply_value(const PgoGraph & g, double y, const double * u, int ustride, int row)
{
  const int n = 6 * g.F;
  double s = y;
  for (int c = 0; c < n; ++c) s -= g.Y[static_cast<size_t>(row) * g.K + c] * u[static_cast<size_t>(c) * ustride];
  return s;
}
// entry `row` of y - Y u: into x (first) or added to it (a refinement step)
MH_HD void pgo_apply_row(const PgoGraph & g, const double * y, int stride, bool first, int row)
{
  const double s = pgo_apply_value(g, y[static_cast<size_t>(row) * stride], g.u, 1, row);
  g.x[row] = first ? s : g.x[row] + s;
}

// entry `row` of g.r = rhs - A x against the system as assembled (T's blocks, then the pose's far edges in list order, each
// entry times the edge's weight), in twice the working precision as the window chains take it.  The row of a fixed pose is zero.
// pgo_residual_value: the same for any column: its right-hand side entry and its x (`xs` doubles between entries).
MH_HD double pgo_residual_value(const PgoGraph & g, int row, double rhs, const double * x, int xs)
{
  const int i = row / 6, r = row % 6;
  if (g.fixed[i]) return 0.0;
  auto X = [&](int k) { return x[static_cast<size_t>(k) * xs]; };
  double hi = rhs, lo = 0.0;
  auto term = [&](double a, double xj) {
    const double pr = a * xj, pe = fma(a, xj, -pr);  // a x = pr + pe exactly
    const double s = hi - pr, bv = s - hi;
    lo += ((hi - (s - bv)) + (-pr - bv)) - pe;  // two-sum of hi and -pr
    hi = s;
  };
  if (i > 0)
    for (int m = 0; m < 6; ++m) term(g.Eb[36 * i + 6 * r + m], X(6 * (i - 1) + m));
  for (int m = 0; m < 6; ++m) term(g.A[36 * i + 6 * r + m], X(6 * i + m));
  if (i + 1 < g.N)
    for (int m = 0; m < 6; ++m) term(g.Eb[36 * (i + 1) + 6 * m + r], X(6 * (i + 1) + m));
  const int * inc = g.inc + g.inc_off[i];
  const int n = g.inc_off[i + 1] - g.inc_off[i];
  for (int k = 0; k < n; ++k) {
    const int e = inc[k] >> 1;
    if (g.eslot[e] < 0) continue;
    const int a = g.ea[e], b = g.eb[e];
    const double we = g.w[e];
    if (inc[k] & 1) {
      if (!g.fixed[a])
        for (int m = 0; m < 6; ++m) term(we * g.Eba[36 * e + 6 * r + m], X(6 * a + m));
      for (int m = 0; m < 6; ++m) term(we * g.Om[36 * e + 6 * r + m], X(6 * b + m));
    } else {
      for (int m = 0; m < 6; ++m) term(we * g.Baa[36 * e + 6 * r + m], X(6 * a + m));
      if (!g.fixed[b])
        for (int m = 0; m < 6; ++m) term(we * g.Eba[36 * e + 6 * m + r], X(6 * b + m));
    }
  }
  return hi + lo;
}
MH_HD void pgo_residual_row(const PgoGraph & g, int row) { g.r[row] = pgo_residual_value(g, row, g.rhs[row], g.x, 1); }

// ---- the phases of one iteration that one workgroup runs ------------------------------------------------------------------------
// stage 0, behind the sweep of all K columns: C and its factors, u for y = Y[:, 6F]; stage 1, 2, behind the sweep of g.r into
// g.y1: u for y = g.y1.  Behind it, per row and over any number of workgroups: pgo_apply_row, then (a launch of its own: a row
// reads its neighbours' x) pgo_residual_row.
template <typename Par>
MH_HD void pgo_small(const PgoGraph & g, int stage, Par & par)
{
  if (stage == 0) {
    if (!pgo_factor_C(g, par)) return;
    pgo_solve_C(g, g.Y + 6 * g.F, g.K, par);
  } else {
    pgo_solve_C(g, g.y1, 1, par);
  }
}
// the cost (rho of the terms, edges then priors) in its fixed order into g.fold[0 .. kPgoFold), its total into *f
template <typename Par>
MH_HD void pgo_cost(const PgoGraph & g, double * f, Par & par)
{
  par.each(kPgoFold, [&](int l) {
    double s = 0.0;
    for (int e = l; e < g.E + g.P; e += kPgoFold) s += e < g.E ? g.rho[e] : g.prho[e - g.E];
    g.fold[l] = s;
  });
  par.each(1, [&](int) {
    double s = 0.0;
    for (int l = 0; l < kPgoFold; ++l) s += g.fold[l];
    *f = s;
  });
}
// the step, the row of iteration `it`, the stop test.  trace: nullptr, or 12 N doubles for the poses behind the step.
template <typename Par>
MH_HD void pgo_finish(const PgoGraph & g, const PgoParams & p, int it, double * trace, Par & par)
{
  const int N = g.N;
  PgoRow & row = g.rows[it];
  par.each(6 * N, [&](int q) {
    if (g.st->ok && !(fabs(g.x[q]) < 1e300)) g.st->ok = 0;
  });
  const bool stepped = g.st->ok != 0;
  par.sync();
  par.each(N, [&](int i) {
    double sr = 0.0, st = 0.0;
    if (stepped && !g.fixed[i]) {
      const double * xi = g.x + 6 * i;
      double Rn[9], tn[3];
      sr = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
      st = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
      align_retract(g.R + 9 * i, g.t + 3 * i, xi, Rn, tn);
      for (int q = 0; q < 9; ++q) g.R[9 * i + q] = Rn[q];
      for (int q = 0; q < 3; ++q) g.t[3 * i + q] = tn[q];
    }
    g.d[2 * i] = sr;
    g.d[2 * i + 1] = st;
  });
  if (trace)
    par.each(12 * N, [&](int l) {
      const int i = l / 12, q = l % 12;
      trace[l] = q < 9 ? g.R[9 * i + q] : g.t[3 * i + q - 9];
    });
  par.each(kPgoFold, [&](int l) {
    double mr = 0.0, mt = 0.0;
    for (int i = l; i < N; i += kPgoFold) {
      mr = g.d[2 * i] > mr ? g.d[2 * i] : mr;
      mt = g.d[2 * i + 1] > mt ? g.d[2 * i + 1] : mt;
    }
    g.fold[kPgoFold + l] = mr;
    g.fold[2 * kPgoFold + l] = mt;
  });
  pgo_cost(g, &row.f, par);
  par.each(1, [&](int) {
    double mr = 0.0, mt = 0.0;
    for (int l = 0; l < kPgoFold; ++l) {
      mr = g.fold[kPgoFold + l] > mr ? g.fold[kPgoFold + l] : mr;
      mt = g.fold[2 * kPgoFold + l] > mt ? g.fold[2 * kPgoFold + l] : mt;
    }
    const bool conv = stepped && mr < p.eps_rot && mt < p.eps_trans;
    g.st->converged = conv ? 1 : 0;
    g.st->stopped = (conv || !stepped) ? 1 : 0;
    g.st->iters += 1;
    row.step_rot = mr;
    row.step_trans = mt;
    row.flags = g.st->stopped | (conv ? 2 : 0) | (stepped ? 0 : 4);
    row.iters = g.st->iters;
  });
}

// ---- the host's whole iteration (tests/cpp/pose_graph_step.cpp): the kernels' launches as loops ---------------------------------
// sm: 114 doubles.  Returns the row's flags.
inline int pgo_iterate_host(const PgoGraph & g, const PgoParams & p, int it, double * trace, double * sm)
{
  WindowSerial par;
  if (g.st->stopped) return 1;
  for (int j = 0; j < g.E + g.P; ++j) pgo_term(g, j, false);
  for (int l = 0; l < kPgoGather * g.N; ++l) pgo_gather(g, p, l);
  g.st->ok = 1;
  for (int f = 0; f < g.F; ++f)
    if (!pgo_far_info(g, f)) g.st->ok = 0;
  if (g.st->ok && pgo_factor(g, sm, par)) {
    for (int c = 0; c < g.K; ++c) pgo_sweep_col(g, c, nullptr, g.Y + c, g.K);
    for (int stage = 0; stage < 3 && g.st->ok; ++stage) {
      if (stage > 0) pgo_sweep_col(g, 0, g.r, g.y1, 1);
      pgo_small(g, stage, par);
      if (!g.st->ok) break;
      for (int row = 0; row < 6 * g.N; ++row) pgo_apply_row(g, stage ? g.y1 : g.Y + 6 * g.F, stage ? 1 : g.K, stage == 0, row);
      if (stage < 2)
        for (int row = 0; row < 6 * g.N; ++row) pgo_residual_row(g, row);
    }
  }
  pgo_finish(g, p, it, trace, par);
  return g.rows[it].flags;
}

// ---- a wide graph (mh_pose_graph_create_wide): C built, factorised and solved in blocks ------------------------------------------
// The arithmetic is pgo_factor_C's and pgo_solve_C's, entry by entry: entry (i, k), i >= k, of C starts as pgo_factor_C forms it
// (pgo_W_row in its order, the OmInv entry added in front on the diagonal blocks); for j ascending D_j = C[j][j] under the pivot
// test, U[j][i] = C[i][j] and L[i][j] = C[i][j] / D_j for i > j, and C[i][k] -= L[i][j] * U[j][k] for i >= k > j, the product
// rounded, then subtracted; the solve is u[i] -= L[i][j] * u[j] with j ascending, u[j] /= D_j, u[i] -= L[j][i] * u[j] with j
// descending.  Every entry's operations come in an order of their own, and a schedule that keeps that order per entry gives
// the same bits.  The schedule here: panels of NB = kPgoWideNB columns.  Panel p takes its diagonal block (pgo_wide_diag: the
// steps j of the panel on the block itself), then the strip of rows under it (pgo_wide_strip: the same steps on those rows, which
// leaves their U and L), then every tile behind it (pgo_wide_trail: the panel's NB products of an entry, j ascending).  An entry
// has then seen every j of panels 0 .. p in ascending order when panel p + 1 begins.  Each of the three is a function of a block,
// strip or tile index; a phase that needs ALL of the phase before it is a launch of its own.  sm: kPgoWideSm doubles.
MH_HD int pgo_wide_blocks(int n) { return (n + kPgoWideNB - 1) / kPgoWideNB; }

// tile (ti, tk), tk <= ti, of C's lower triangle as pgo_factor_C forms it (the upper triangle is not read before U is written)
template <typename Par>
MH_HD void pgo_wide_build(const PgoGraph & g, int ti, int tk, Par & par)
{
  constexpr int NB = kPgoWideNB;
  const int n = 6 * g.F, K = g.K;
  par.each(NB * NB, [&](int l) {
    const int row = ti * NB + l / NB, col = tk * NB + l % NB;
    if (row >= n || col > row) return;
    double s = pgo_W_row(g, row, g.Y + col, K);
    if (row / 6 == col / 6) s = g.OmInv[36 * (row / 6) + 6 * (row % 6) + col % 6] + s;
    g.C[row * n + col] = s;
  });
}

// diagonal block p, one workgroup: pgo_factor_C's steps j = NB p .. on the block itself.  false (g.st->ok == 0): a pivot is not positive.
template <typename Par>
MH_HD bool pgo_wide_diag(const PgoGraph & g, int p, double * sm, Par & par)
{
  constexpr int NB = kPgoWideNB, LD = kPgoWideLd;
  const int n = 6 * g.F, j0 = p * NB, nb = n - j0 < NB ? n - j0 : NB;
  par.each(nb * nb, [&](int l) {
    const int r = l / nb, c = l % nb;
    if (c <= r) sm[r * LD + c] = g.C[(j0 + r) * n + j0 + c];
  });
  for (int j = 0; j < nb; ++j) {
    par.each(1, [&](int) {
      const double d = sm[j * LD + j];
      if (!(d > 0.0) || !(d < 1e300)) g.st->ok = 0;
    });
    if (!g.st->ok) return false;
    par.each(nb - j - 1, [&](int l) {
      const int i = j + 1 + l;
      const double t = sm[i * LD + j];
      sm[j * LD + i] = t;
      sm[i * LD + j] = t / sm[j * LD + j];
    });
    const int m = nb - j - 1;
    par.each(m * m, [&](int l) {
      const int i = j + 1 + l / m, k = j + 1 + l % m;
      if (k > i) return;
      sm[i * LD + k] -= sm[i * LD + j] * sm[j * LD + k];
    });
  }
  par.each(nb * nb, [&](int l) { g.C[(j0 + l / nb) * n + j0 + l % nb] = sm[(l / nb) * LD + l % nb]; });
  return true;
}

// strip s of the rows under diagonal block p (rows NB (p + 1 + s) ..): the panel's steps on those rows.  The strip lives in sm by
// columns (entry (r, c) at [c NB + r]: a step reads and writes down a column), the diagonal block's U and D by rows.
template <typename Par>
MH_HD void pgo_wide_strip(const PgoGraph & g, int p, int s, double * sm, Par & par)
{
  constexpr int NB = kPgoWideNB;
  const int n = 6 * g.F, j0 = p * NB, i0 = j0 + NB * (1 + s), nr = n - i0 < NB ? n - i0 : NB;
  if (nr <= 0) return;
  double *Bd = sm, *St = sm + NB * NB;
  par.each(NB * NB, [&](int l) {
    const int r = l / NB, c = l % NB;
    if (c >= r) Bd[l] = g.C[(j0 + r) * n + j0 + c];
  });
  par.each(nr * NB, [&](int l) { St[(l % NB) * NB + l / NB] = g.C[(i0 + l / NB) * n + j0 + l % NB]; });
  for (int j = 0; j < NB; ++j) {
    par.each(nr, [&](int r) {
      const double t = St[j * NB + r];
      g.C[(j0 + j) * n + i0 + r] = t;
      St[j * NB + r] = t / Bd[j * NB + j];
    });
    par.each(nr * (NB - j - 1), [&](int l) {
      const int r = l % nr, k = j + 1 + l / nr;
      St[k * NB + r] -= St[j * NB + r] * Bd[j * NB + k];
    });
  }
  par.each(nr * NB, [&](int l) { g.C[(i0 + l / NB) * n + j0 + l % NB] = St[(l % NB) * NB + l / NB]; });
}

// tile (ti, tk), tk <= ti, of the blocks behind panel p: every entry takes the panel's NB products, j ascending
template <typename Par>
MH_HD void pgo_wide_trail(const PgoGraph & g, int p, int ti, int tk, double * sm, Par & par)
{
  constexpr int NB = kPgoWideNB;
  const int n = 6 * g.F, j0 = p * NB, i0 = j0 + NB * (1 + ti), k0 = j0 + NB * (1 + tk);
  const int nr = n - i0 < NB ? n - i0 : NB, nc = n - k0 < NB ? n - k0 : NB;
  if (nr <= 0 || nc <= 0 || tk > ti) return;
  double *Lp = sm, *Up = sm + NB * NB;
  par.each(nr * NB, [&](int l) { Lp[l] = g.C[(i0 + l / NB) * n + j0 + l % NB]; });
  par.each(NB * nc, [&](int l) { Up[(l / nc) * NB + l % nc] = g.C[(j0 + l / nc) * n + k0 + l % nc]; });
  par.each(nr * nc, [&](int l) {
    const int r = l / nc, c = l % nc, i = i0 + r, k = k0 + c;
    if (k > i) return;
    double t = g.C[i * n + k];
    for (int j = 0; j < NB; ++j) t -= Lp[r * NB + j] * Up[j * NB + c];
    g.C[i * n + k] = t;
  });
}

// u = C^-1 W y in blocks, pgo_solve_C's sums in its order.  Forward step of panel p: block p's entries have taken every j in front
// of the block; they take the block's own j (every workgroup for itself, in LDS), then strip s of the rows behind the block takes
// the panel's NB products, j ascending.  p == 0 starts from pgo_W_row.  Strip 0 also leaves the block's entries, divided by D_j, in
// g.v: g.u's block is read by every strip of this launch and written by none.
template <typename Par>
MH_HD void pgo_wide_forward(const PgoGraph & g, const double * y, int stride, int p, int s, double * sm, Par & par)
{
  constexpr int NB = kPgoWideNB, LD = kPgoWideLd;
  const int n = 6 * g.F, j0 = p * NB, nb = n - j0 < NB ? n - j0 : NB;
  double *ub = sm, *Ld = sm + NB;
  par.each(nb, [&](int i) { ub[i] = p == 0 ? pgo_W_row(g, j0 + i, y, stride) : g.u[j0 + i]; });
  par.each(nb * nb, [&](int l) {
    const int r = l / nb, c = l % nb;
    if (c <= r) Ld[r * LD + c] = g.C[(j0 + r) * n + j0 + c];
  });
  for (int j = 0; j + 1 < nb; ++j) par.each(nb - j - 1, [&](int l) { ub[j + 1 + l] -= Ld[(j + 1 + l) * LD + j] * ub[j]; });
  if (s == 0) par.each(nb, [&](int i) { g.v[j0 + i] = ub[i] / Ld[i * LD + i]; });
  const int i0 = j0 + NB * (1 + s), nr = n - i0 < NB ? n - i0 : NB;
  if (nr <= 0) return;
  par.each(nr * NB, [&](int l) { Ld[(l / NB) * LD + l % NB] = g.C[(i0 + l / NB) * n + j0 + l % NB]; });
  par.each(nr, [&](int r) {
    double t = p == 0 ? pgo_W_row(g, i0 + r, y, stride) : g.u[i0 + r];
    for (int j = 0; j < NB; ++j) t -= Ld[r * LD + j] * ub[j];
    g.u[i0 + r] = t;
  });
}
// Backward step of panel p (p descending): block p's entries of g.v have taken every j behind the block; they take the block's own
// j, descending, then strip s of the rows in front of the block (rows NB s ..) takes the panel's products, j descending.  Strip
// 0 leaves the block's entries, now final, in g.u.
template <typename Par>
MH_HD void pgo_wide_backward(const PgoGraph & g, int p, int s, double * sm, Par & par)
{
  constexpr int NB = kPgoWideNB, LD = kPgoWideLd;
  const int n = 6 * g.F, j0 = p * NB, nb = n - j0 < NB ? n - j0 : NB;
  double *vb = sm, *Ld = sm + NB;
  par.each(nb, [&](int i) { vb[i] = g.v[j0 + i]; });
  par.each(nb * nb, [&](int l) {
    const int r = l / nb, c = l % nb;
    if (c < r) Ld[r * LD + c] = g.C[(j0 + r) * n + j0 + c];
  });
  for (int j = nb - 1; j >= 1; --j) par.each(j, [&](int i) { vb[i] -= Ld[j * LD + i] * vb[j]; });
  if (s == 0) par.each(nb, [&](int i) { g.u[j0 + i] = vb[i]; });
  const int i0 = NB * s;
  if (i0 >= j0) return;
  par.each(NB, [&](int r) {
    double t = g.v[i0 + r];
    for (int j = nb - 1; j >= 0; --j) t -= g.C[(j0 + j) * n + i0 + r] * vb[j];
    g.v[i0 + r] = t;
  });
}

// the phases of pgo_small on a wide graph as the host runs them (the kernels: one launch per line of a loop over blocks)
inline void pgo_small_wide_host(const PgoGraph & g, int stage, double * sm)
{
  WindowSerial par;
  const int nt = pgo_wide_blocks(6 * g.F);
  if (stage == 0) {
    for (int ti = 0; ti < nt; ++ti)
      for (int tk = 0; tk <= ti; ++tk) pgo_wide_build(g, ti, tk, par);
    for (int p = 0; p < nt; ++p) {
      if (!pgo_wide_diag(g, p, sm, par)) return;
      for (int s = 0; s < nt - p - 1; ++s) pgo_wide_strip(g, p, s, sm, par);
      for (int ti = 0; ti < nt - p - 1; ++ti)
        for (int tk = 0; tk <= ti; ++tk) pgo_wide_trail(g, p, ti, tk, sm, par);
    }
  }
  const double * y = stage == 0 ? g.Y + 6 * g.F : g.y1;
  const int stride = stage == 0 ? g.K : 1;
  for (int p = 0; p < nt; ++p)
    for (int s = 0; s < (nt - p - 1 > 1 ? nt - p - 1 : 1); ++s) pgo_wide_forward(g, y, stride, p, s, sm, par);
  for (int p = nt - 1; p >= 0; --p)
    for (int s = 0; s < (p > 1 ? p : 1); ++s) pgo_wide_backward(g, p, s, sm, par);
}

// the host's whole iteration of a wide graph (tests/cpp/pose_graph_wide_step.cpp): pgo_iterate_host with the blocked phases in
// pgo_small's place whenever the graph holds a far edge; `blocked` false runs pgo_small itself on the same arrays (the parity
// test's other side).  sm: kPgoWideSm doubles.
inline int pgo_iterate_wide_host(const PgoGraph & g, const PgoParams & p, int it, double * trace, double * sm, bool blocked)
{
  WindowSerial par;
  if (g.st->stopped) return 1;
  for (int j = 0; j < g.E + g.P; ++j) pgo_term(g, j, false);
  for (int l = 0; l < kPgoGather * g.N; ++l) pgo_gather(g, p, l);
  g.st->ok = 1;
  for (int f = 0; f < g.F; ++f)
    if (!pgo_far_info(g, f)) g.st->ok = 0;
  if (g.st->ok && pgo_factor(g, sm, par)) {
    for (int c = 0; c < g.K; ++c) pgo_sweep_col(g, c, nullptr, g.Y + c, g.K);
    for (int stage = 0; stage < 3 && g.st->ok; ++stage) {
      if (stage > 0) pgo_sweep_col(g, 0, g.r, g.y1, 1);
      if (blocked && g.F > 0)
        pgo_small_wide_host(g, stage, sm);
      else
        pgo_small(g, stage, par);
      if (!g.st->ok) break;
      for (int row = 0; row < 6 * g.N; ++row) pgo_apply_row(g, stage ? g.y1 : g.Y + 6 * g.F, stage ? 1 : g.K, stage == 0, row);
      if (stage < 2)
        for (int row = 0; row < 6 * g.N; ++row) pgo_residual_row(g, row);
    }
  }
  pgo_finish(g, p, it, trace, par);
  return g.rows[it].flags;
}

// ---- marginal covariances (mh_pose_graph_covariances) ---------------------------------------------------------------------------
// Sigma = A^-1 at the stored poses, from what an iteration leaves behind its stage-0 pgo_small: T = L D L^T (g.L, g.Dv, g.G),
// Y = T^-1 W^T and C = L_C D_C L_C^T.  By the Woodbury identity A^-1 = T^-1 - Y C^-1 Y^T:
//   P_i = (T^-1)_ii     the backward recursion P_{N-1} = S_{N-1}^-1, P_i = S_i^-1 + G_{i+1} P_{i+1} G_{i+1}^T (pgo_cov_chain)
//   Sigma_ii            P_i - U_i^T D_C^-1 U_i, U_i = L_C^-1 Y_i^T (pgo_cov_correct: six right-hand sides side by side)
//   Sigma_ij, i < j     block row i of the six columns X = A^-1 E_j: Z = T^-1 E_j (pgo_sweep_col, unit source), X = Z - Y C^-1 W Z,
//                       then the chains' two refinement steps against A (pgo_residual_value, pgo_apply_value)
// The arrays are a block of their own (PgoCov), not pgo_layout's: a graph that never asks for covariances does not pay for them.
// A column lives at stride `ncols` (6 per pair): entry `row` of column q is at [row * ncols + q], one lane per column.
constexpr int kPgoCovPairsMax = 64;
constexpr int kPgoCovPanel = 8;     // rows of C's factor staged at a time by pgo_cov_correct
constexpr int kPgoCovChainSm = 108; // doubles pgo_cov_chain shares: S_i^-1, M = G P, the current P
struct PgoCov
{
  int n_pairs, ncols;  // ncols = 6 n_pairs
  double *P, *S;       // 36 N each: (T^-1)_ii; Sigma_ii (symmetric to the bit, zero for a fixed pose)
  double *X, *Z;       // 6 N x ncols each: the columns; T^-1 of the unit source, then of each residual
  double * U;          // 6 F x ncols: C^-1 W z per column
  double * joint;      // 144 n_pairs
  int * pairs;         // 2 n_pairs: i < j
};
// doubles pgo_cov_correct shares for a graph of F far edges: U (6F x 6), then a panel of kPgoCovPanel rows of C
MH_HD int pgo_cov_correct_sm(int F) { return 6 * F * (6 + kPgoCovPanel); }

// One step of the recursion at block i, two phases.  Lb, Db: L_i, D_i; Gn: G_{i+1}; Pn: P_{i+1} (`last`: i == N - 1, neither is read).
// phase 1, index l < 42: column l of S_i^-1 by window_solve6 (l < 6), else entry l - 6 of M = G_{i+1} P_{i+1}
MH_HD void pgo_cov_step1(const double * Lb, const double * Db, const double * Gn, const double * Pn, bool last, double * Si, double * M, int l)
{
  if (l < 6) {
    double e[6] = {0, 0, 0, 0, 0, 0}, col[6];
    e[l] = 1.0;
    window_solve6(Lb, Db, e, col);
    for (int m = 0; m < 6; ++m) Si[6 * m + l] = col[m];
  } else if (!last) {
    const int a = (l - 6) / 6, m = (l - 6) % 6;
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += Gn[6 * a + k] * Pn[6 * k + m];
    M[l - 6] = s;
  }
}
// phase 2, index l < 36: entry (a, b), a >= b, of P_i = S_i^-1 + M G_{i+1}^T, written to both triangles of Pc (the next step's
// P_{i+1}) and of out
MH_HD void pgo_cov_step2(const double * Gn, const double * Si, const double * M, bool last, double * Pc, double * out, int l)
{
  const int a = l / 6, b = l % 6;
  if (b > a) return;
  double s = Si[6 * a + b];
  if (!last)
    for (int m = 0; m < 6; ++m) s += M[6 * a + m] * Gn[6 * b + m];
  Pc[6 * a + b] = Pc[6 * b + a] = s;
  out[6 * a + b] = out[6 * b + a] = s;
}
// the recursion over all blocks as the host runs it (the kernel walks the same two phases with block i - 1 prefetched)
template <typename Par>
MH_HD void pgo_cov_chain(const PgoGraph & g, const PgoCov & cov, double * sm, Par & par)
{
  double *Si = sm, *M = sm + 36, *Pc = sm + 72;
  for (int i = g.N - 1; i >= 0; --i) {
    const bool last = i == g.N - 1;
    const double * Gn = last ? g.G : g.G + 36 * (i + 1);
    par.each(42, [&](int l) { pgo_cov_step1(g.L + 36 * i, g.Dv + 6 * i, Gn, Pc, last, Si, M, l); });
    par.each(36, [&](int l) { pgo_cov_step2(Gn, Si, M, last, Pc, cov.P + 36 * i, l); });
  }
}

// Sigma_ii of pose i by one workgroup.  U = Y_i^T (6F x 6) is forward-substituted through L_C in place: row k takes
// U[k] -= L_C[k][j] U[j] for j ascending, every product rounded and subtracted by itself; C's factor is staged kPgoCovPanel rows
// at a time (the part left of the panel first, then the panel's own triangle row by row).  Then entry (a, b), a >= b:
// P_i[a][b] - sum_k (U[k][a] U[k][b]) / D_C[k], k ascending, mirrored.  A fixed pose: zeros.  F == 0: P_i's lower triangle, mirrored.
template <typename Par>
MH_HD void pgo_cov_correct(const PgoGraph & g, const PgoCov & cov, int i, double * sm, Par & par)
{
  const int n = 6 * g.F, K = g.K;
  double * S = cov.S + 36 * i;
  const double * P = cov.P + 36 * i;
  if (g.fixed[i]) {
    par.each(36, [&](int l) { S[l] = 0.0; });
    return;
  }
  double *U = sm, *Lp = sm + 6 * n;
  par.each(6 * n, [&](int l) { U[l] = g.Y[static_cast<size_t>(6 * i + l % 6) * K + l / 6]; });
  for (int r0 = 0; r0 < n; r0 += kPgoCovPanel) {
    const int nb = n - r0 < kPgoCovPanel ? n - r0 : kPgoCovPanel, wd = r0 + nb;
    par.each(nb * wd, [&](int l) { Lp[(l / wd) * n + l % wd] = g.C[(r0 + l / wd) * n + l % wd]; });
    par.each(nb * 6, [&](int l) {
      const int il = l / 6, c = l % 6;
      double s = U[6 * (r0 + il) + c];
      for (int j = 0; j < r0; ++j) s -= Lp[il * n + j] * U[6 * j + c];
      U[6 * (r0 + il) + c] = s;
    });
    for (int jl = 0; jl + 1 < nb; ++jl)
      par.each((nb - jl - 1) * 6, [&](int l) {
        const int il = jl + 1 + l / 6, c = l % 6;
        U[6 * (r0 + il) + c] -= Lp[il * n + r0 + jl] * U[6 * (r0 + jl) + c];
      });
  }
  par.each(36, [&](int l) {
    const int a = l / 6, b = l % 6;
    if (b > a) return;
    double s = P[6 * a + b];
    for (int k = 0; k < n; ++k) s -= (U[6 * k + a] * U[6 * k + b]) / g.C[k * n + k];
    S[6 * a + b] = S[6 * b + a] = s;
  });
}

// ---- a pair's columns, one lane per column q (pair q / 6, column q % 6 of E_j) ---------------------------------------------------
MH_HD int pgo_cov_unit(const PgoCov & cov, int q) { return 6 * cov.pairs[2 * (q / 6) + 1] + q % 6; }
// Z = T^-1 E_j (first), or Z = T^-1 Z in place for a residual
MH_HD void pgo_cov_sweep(const PgoGraph & g, const PgoCov & cov, int q, bool first)
{
  pgo_sweep_col(g, 0, cov.Z + q, cov.Z + q, cov.ncols, cov.ncols, first ? pgo_cov_unit(cov, q) : -1);
}
// u = C^-1 W z for column q: pgo_solve_C's sums in its order (forward j ascending, backward j descending), one lane running them
MH_HD void pgo_cov_solve(const PgoGraph & g, const PgoCov & cov, int q)
{
  const int n = 6 * g.F;
  const size_t us = static_cast<size_t>(cov.ncols);
  double * u = cov.U + q;
  for (int row = 0; row < n; ++row) u[row * us] = pgo_W_row(g, row, cov.Z + q, cov.ncols);
  for (int i = 1; i < n; ++i) {
    double s = u[i * us];
    for (int j = 0; j < i; ++j) s -= g.C[i * n + j] * u[j * us];
    u[i * us] = s;
  }
  for (int j = 0; j < n; ++j) u[j * us] = u[j * us] / g.C[j * n + j];
  for (int i = n - 2; i >= 0; --i) {
    double s = u[i * us];
    for (int j = n - 1; j > i; --j) s -= g.C[j * n + i] * u[j * us];
    u[i * us] = s;
  }
}
// entry l = row * ncols + q: X = Z - Y u (first) or X += Z - Y u; with F == 0 there is no u and X = Z or X += Z
MH_HD void pgo_cov_apply(const PgoGraph & g, const PgoCov & cov, bool first, size_t l)
{
  const int row = static_cast<int>(l / cov.ncols), q = static_cast<int>(l % cov.ncols);
  const double s = pgo_apply_value(g, cov.Z[l], cov.U + q, cov.ncols, row);
  cov.X[l] = first ? s : cov.X[l] + s;
}
// entry l of the residual E_j - A X into Z
MH_HD void pgo_cov_residual(const PgoGraph & g, const PgoCov & cov, size_t l)
{
  const int row = static_cast<int>(l / cov.ncols), q = static_cast<int>(l % cov.ncols);
  cov.Z[l] = pgo_residual_value(g, row, row == pgo_cov_unit(cov, q) ? 1.0 : 0.0, cov.X + q, cov.ncols);
}
// entry l < 144 n_pairs of joint: [[S_ii, S_ij], [S_ij^T, S_jj]], the diagonal blocks cov's bits, S_ij block row i of the pair's
// columns (zero when either pose is fixed)
MH_HD void pgo_cov_joint(const PgoGraph & g, const PgoCov & cov, int l)
{
  const int p = l / 144, r = (l % 144) / 12, c = l % 12, i = cov.pairs[2 * p], j = cov.pairs[2 * p + 1];
  double v;
  if (r < 6 && c < 6)
    v = cov.S[36 * i + 6 * r + c];
  else if (r >= 6 && c >= 6)
    v = cov.S[36 * j + 6 * (r - 6) + c - 6];
  else if (g.fixed[i] || g.fixed[j])
    v = 0.0;
  else if (r < 6)
    v = cov.X[static_cast<size_t>(6 * i + r) * cov.ncols + 6 * p + c - 6];
  else
    v = cov.X[static_cast<size_t>(6 * i + c) * cov.ncols + 6 * p + r - 6];
  cov.joint[l] = v;
}
// the columns of every pair as the host runs them (the kernels: one launch per line)
inline void pgo_cov_column(const PgoGraph & g, const PgoCov & cov)
{
  const size_t entries = static_cast<size_t>(6 * g.N) * cov.ncols;
  for (int step = 0; step < 3; ++step) {
    if (step > 0)
      for (size_t l = 0; l < entries; ++l) pgo_cov_residual(g, cov, l);
    for (int q = 0; q < cov.ncols; ++q) pgo_cov_sweep(g, cov, q, step == 0);
    if (g.F > 0)
      for (int q = 0; q < cov.ncols; ++q) pgo_cov_solve(g, cov, q);
    for (size_t l = 0; l < entries; ++l) pgo_cov_apply(g, cov, step == 0, l);
  }
}

// ---- the host's whole covariance call (tests/cpp/pose_graph_cov_step.cpp): the kernels' launches as loops -------------------------
// The system as pgo_iterate_host assembles it, up to C's factor; then the chain, the correction, the pairs.  sm: the larger of
// 114, kPgoCovChainSm and pgo_cov_correct_sm(F) doubles.  Returns 0, or 4: a pivot was not positive (cov's arrays are not written).
inline int pgo_cov_host(const PgoGraph & g, const PgoParams & p, const PgoCov & cov, double * sm)
{
  WindowSerial par;
  g.st->stopped = 0;
  for (int j = 0; j < g.E + g.P; ++j) pgo_term(g, j, false);
  for (int l = 0; l < kPgoGather * g.N; ++l) pgo_gather(g, p, l);
  g.st->ok = 1;
  for (int f = 0; f < g.F; ++f)
    if (!pgo_far_info(g, f)) g.st->ok = 0;
  if (!g.st->ok || !pgo_factor(g, sm, par)) return 4;
  for (int c = 0; c < g.K; ++c) pgo_sweep_col(g, c, nullptr, g.Y + c, g.K);
  if (g.F > 0) pgo_small(g, 0, par);
  if (!g.st->ok) return 4;
  pgo_cov_chain(g, cov, sm, par);
  for (int i = 0; i < g.N; ++i) pgo_cov_correct(g, cov, i, sm, par);
  if (cov.n_pairs > 0) {
    pgo_cov_column(g, cov);
    for (int l = 0; l < 144 * cov.n_pairs; ++l) pgo_cov_joint(g, cov, l);
  }
  return 0;
}

}  // namespace mh
