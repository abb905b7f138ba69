// Drives the joint-factor phases of mh_icp_window_optimise_joint and mh_icp_window_marginalise_joint (mimosa_amd/csrc/window_device.hpp,
// the header the kernels are built from) on the CPU for tests/test_icp_window_joint_cpu.py.  stdin: the number of cases; per case
//   mode (0: the chain, 1: the marginal),
//   n_poses of the joint factor (0: none), per member pose, L (R[9], t[3]), then H (6 n x 6 n, row-major), b (6 n), f,
//   mode 0: a case of tests/cpp/window_edge_step.cpp;  mode 1: a case of tests/cpp/window_marginal_step.cpp
// -> mode 0: what window_edge_step.cpp prints;  mode 1: the separator, H_m, b_m (the leading 6 |S|, packed), f_m, valid, n_ties
//    and the accumulated A00, A_S0, A_SS' (packed), g0, g_S', c
// stdout: JSON, one entry per case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "window_device.hpp"

static double rd()
{
  double v = 0;
  if (std::scanf("%lf", &v) != 1) std::exit(2);
  return v;
}
static void arr(const char * name, const double * v, int n, bool comma = true)
{
  std::printf("\"%s\": [", name);
  for (int i = 0; i < n; ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s", comma ? ", " : "");
}
// the leading n x n of a matrix of row stride kWindowJointDim
static void packed(const char * name, const double * v, int n)
{
  std::vector<double> m(static_cast<size_t>(n) * n);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) m[static_cast<size_t>(r) * n + c] = v[mh::kWindowJointDim * r + c];
  arr(name, m.data(), n * n);
}

int main()
{
  const int n_cases = static_cast<int>(rd());
  auto wp = std::make_unique<mh::WindowWork>();
  auto rlp = std::make_unique<mh::WindowRelin>();
  auto linp = std::make_unique<mh::WindowLinear>();
  auto lwp = std::make_unique<mh::WindowLinWork>();
  auto edp = std::make_unique<mh::WindowEdges>();
  auto ewp = std::make_unique<mh::WindowEdgeWork>();
  auto jtp = std::make_unique<mh::WindowJoint>();
  auto jwp = std::make_unique<mh::WindowJointWork>();
  auto mwp = std::make_unique<mh::WindowMarginalJointWork>();
  auto mop = std::make_unique<mh::WindowMarginalJointOut>();
  mh::WindowEdges & ed = *edp;
  mh::WindowWork & w = *wp;
  mh::WindowLinear & lin = *linp;
  mh::WindowJoint & jt = *jtp;
  std::printf("[");
  for (int c = 0; c < n_cases; ++c) {
    std::printf("%s", c ? ", " : "");
    const int mode = static_cast<int>(rd());
    std::memset(static_cast<void *>(&jt), 0, sizeof(jt));
    jt.n = static_cast<int>(rd());
    if (jt.n < 0 || jt.n > mh::kWindowJointMax) return 3;
    for (int m = 0; m < jt.n; ++m) {
      jt.pose[m] = static_cast<int>(rd());
      for (double & v : jt.LR[m]) v = rd();
      for (double & v : jt.Lt[m]) v = rd();
    }
    for (int r = 0; r < 6 * jt.n; ++r)
      for (int q = 0; q < 6 * jt.n; ++q) jt.H[mh::kWindowJointDim * r + q] = rd();
    for (int r = 0; r < 6 * jt.n; ++r) jt.b[r] = rd();
    if (jt.n) jt.f = rd();
    bool use_relin = false;
    mh::WindowRelinParams rp{};
    if (mode == 0) {
      use_relin = rd() != 0.0;
      rp.relin_rot = rd();
      rp.relin_trans = rd();
    }
    std::memset(static_cast<void *>(&lin), 0, sizeof(lin));
    lin.n = static_cast<int>(rd());
    if (lin.n < 0 || lin.n > mh::kWindowLinMax) return 3;
    for (int j = 0; j < lin.n; ++j) {
      lin.pose[j] = static_cast<int>(rd());
      for (double & v : lin.LR[j]) v = rd();
      for (double & v : lin.Lt[j]) v = rd();
      for (double & v : lin.H[j]) v = rd();
      for (double & v : lin.b[j]) v = rd();
      lin.f[j] = rd();
    }
    std::memset(static_cast<void *>(&ed), 0, sizeof(ed));
    ed.n = static_cast<int>(rd());
    if (ed.n < 0 || ed.n > mh::kWindowEdgeMax) return 3;
    for (int e = 0; e < ed.n; ++e) {
      ed.a[e] = static_cast<int>(rd());
      ed.b[e] = static_cast<int>(rd());
      for (double & v : ed.ZR[e]) v = rd();
      for (double & v : ed.Zt[e]) v = rd();
      for (double & v : ed.Om[e]) v = rd();
    }
    mh::WindowParams p{};
    p.W = static_cast<int>(rd());
    if (p.W < (mode ? 2 : 1) || p.W > mh::kWindowMax) return 3;
    const int W = p.W;
    for (int j = 0; j < lin.n; ++j)
      if (lin.pose[j] < 0 || lin.pose[j] >= W) return 3;
    for (int e = 0; e < ed.n; ++e)
      if (ed.a[e] < 0 || ed.a[e] >= ed.b[e] || ed.b[e] >= W) return 3;
    for (int m = 0; m < jt.n; ++m)
      if (jt.pose[m] < 0 || jt.pose[m] >= W || (m > 0 && jt.pose[m] <= jt.pose[m - 1])) return 3;
    p.has_Z = static_cast<unsigned int>(rd());
    p.have = static_cast<unsigned int>(rd());
    p.reg_4_dof = static_cast<unsigned int>(rd());
    p.project_on_degeneracy = static_cast<unsigned int>(rd());
    for (double & v : p.gz) v = rd();
    for (double & v : p.Wb) v = rd();
    for (double & v : p.prior) v = rd();
    p.damping = rd();
    if (mode == 0) {
      p.eps_rot = rd();
      p.eps_trans = rd();
      for (int i = 0; i < W; ++i) p.thresh_rot[i] = rd();
      for (int i = 0; i < W; ++i) p.thresh_trans[i] = rd();
    } else {
      p.thresh_rot[0] = rd();
      p.thresh_trans[0] = rd();
    }
    mh::WindowState st{};
    for (int i = 0; i < W; ++i) {
      for (double & v : st.R[i]) v = rd();
      for (double & v : st.t[i]) v = rd();
    }
    for (int i = 0; i < W; ++i) {
      for (double & v : st.ZR[i]) v = rd();
      for (double & v : st.Zt[i]) v = rd();
    }
    std::memset(static_cast<void *>(rlp.get()), 0x41, sizeof(mh::WindowRelin));
    std::memset(static_cast<void *>(lwp.get()), 0x41, sizeof(mh::WindowLinWork));
    std::memset(static_cast<void *>(ewp.get()), 0x41, sizeof(mh::WindowEdgeWork));
    std::memset(static_cast<void *>(jwp.get()), 0x41, sizeof(mh::WindowJointWork));
    if (mode == 1) {
      double sums[32];
      for (double & s : sums) s = rd();
      if (jt.n && jt.pose[0] != 0) return 3;
      int sep[mh::kWindowJointMax] = {0, 0, 0, 0};
      const int ns = mh::window_joint_separator(ed, jt.n ? &jt : nullptr, sep);
      if (ns > mh::kWindowJointMax) return 3;
      std::memset(static_cast<void *>(mwp.get()), 0x41, sizeof(mh::WindowMarginalJointWork));
      std::memset(static_cast<void *>(mop.get()), 0x41, sizeof(mh::WindowMarginalJointOut));
      mh::WindowSerial par;
      mh::window_marginal_joint_impl(sums, st, p, lin, *lwp, ed, jt.n ? &jt : nullptr, *jwp, ns, sep, *mwp, *mop, par);
      // everything behind the leading 6 |S| is zero
      int stray = 0;
      for (int r = 0; r < mh::kWindowJointDim; ++r) {
        if (r >= 6 * ns && mop->b[r] != 0.0) ++stray;
        for (int q = 0; q < mh::kWindowJointDim; ++q)
          if ((r >= 6 * ns || q >= 6 * ns) && mop->H[mh::kWindowJointDim * r + q] != 0.0) ++stray;
      }
      std::printf("{\"sep\": [");
      for (int k = 0; k < ns; ++k) std::printf("%s%d", k ? ", " : "", sep[k]);
      std::printf("], ");
      packed("H", mop->H, 6 * ns);
      arr("b", mop->b, 6 * ns);
      arr("A00", mwp->A00, 36);
      arr("AS0", mwp->AS0, 36 * ns);
      packed("ASS", mwp->ASS, 6 * ns);
      arr("g0", mwp->g0, 6);
      arr("gS", mwp->gS, 6 * ns);
      std::printf("\"c\": %.17g, \"f\": %.17g, \"valid\": %d, \"n_ties\": %d, \"stray\": %d}", mwp->c, mop->f, mop->valid, mop->n_ties, stray);
      continue;
    }
    const int n_it = static_cast<int>(rd());
    std::printf("[");
    for (int it = 0; it < n_it; ++it) {
      std::vector<double> sums(32 * static_cast<size_t>(W));
      for (double & s : sums) s = rd();
      std::printf("%s{", it ? ", " : "");
      const bool evaluated = !st.stopped;
      rp.first = it == 0 ? 1 : 0;
      const unsigned int eval = use_relin ? mh::window_relin_mask(*rlp, p, rp) : p.have;
      if (use_relin)  // a kept factor's sums never reach the step
        for (int i = 0; i < W; ++i)
          if (!((eval >> i) & 1u))
            for (int q = 0; q < 32; ++q) sums[32 * static_cast<size_t>(i) + q] = 1e300;
      std::vector<double> row(static_cast<size_t>(mh::window_row_words(W)));
      mh::WindowSerial par;
      int flags;
      if (jt.n)
        flags = mh::window_advance_joint(st, use_relin ? rlp.get() : nullptr, sums.data(), true, p, use_relin ? &rp : nullptr, lin, *lwp, ed, *ewp, jt, *jwp, w, row.data(), par);
      else
        flags = mh::window_advance_edges(st, use_relin ? rlp.get() : nullptr, sums.data(), true, p, use_relin ? &rp : nullptr, lin, *lwp, ed, *ewp, w, row.data(), par);
      if (evaluated) {
        arr("xi", w.x, 6 * W);
        arr("H", &w.H[0][0], 36 * W);
        std::printf("\"cost\": %.17g, \"ok\": %d, \"lo\": [", w.cost, w.ok);
        for (int i = 0; i < W; ++i) std::printf("%s%d", i ? ", " : "", ewp->lo[i]);
        std::printf("], ");
        if (use_relin) std::printf("\"eval\": %u, \"next\": %u, ", eval, rlp->eval);
      }
      std::printf("\"flags\": %d, ", flags);
      arr("row", row.data(), mh::window_row_words(W), false);
      std::printf("}");
    }
    std::printf("]");
  }
  std::printf("]\n");
  return 0;
}
