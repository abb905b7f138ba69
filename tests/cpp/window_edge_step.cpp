// Drives the edge phases and the profile solve of mh_icp_window_optimise_edges (mimosa_amd/csrc/window_device.hpp, the header the
// step kernel is built from) on the CPU for tests/test_icp_window_edges_cpu.py.  stdin: the number of cases; per case
//   use_relin, relin_rot, relin_trans, n_lin, per linear factor pose, L (R[9], t[3]), H[36], b[6], f, n_edges, per edge pose_a,
//   pose_b, Z (R[9], t[3]), info[36], then a case of tests/cpp/window_step.cpp
// -> per queued iteration the row, the flags and, for an evaluated iteration, the step, the ICP factors' H, the cost and the
//    profile (with relin: the evaluated mask and the next one, as tests/cpp/window_relin_step.cpp prints them)
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

int main()
{
  const int n_cases = static_cast<int>(rd());
  auto wp = std::make_unique<mh::WindowWork>();
  auto rlp = std::make_unique<mh::WindowRelin>();
  auto linp = std::make_unique<mh::WindowLinear>();
  auto lwp = std::make_unique<mh::WindowLinWork>();
  auto edp = std::make_unique<mh::WindowEdges>();
  auto ewp = std::make_unique<mh::WindowEdgeWork>();
  mh::WindowEdges & ed = *edp;
  mh::WindowWork & w = *wp;
  mh::WindowLinear & lin = *linp;
  std::printf("[");
  for (int c = 0; c < n_cases; ++c) {
    std::printf("%s", c ? ", " : "");
    const bool use_relin = rd() != 0.0;
    mh::WindowRelinParams rp{};
    rp.relin_rot = rd();
    rp.relin_trans = rd();
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
    if (p.W < 1 || p.W > mh::kWindowMax) return 3;
    const int W = p.W;
    for (int j = 0; j < lin.n; ++j)
      if (lin.pose[j] < 0 || lin.pose[j] >= W) return 3;
    for (int e = 0; e < ed.n; ++e)
      if (ed.a[e] < 0 || ed.a[e] >= ed.b[e] || ed.b[e] >= W) return 3;
    p.has_Z = static_cast<unsigned int>(rd());
    p.have = static_cast<unsigned int>(rd());
    p.reg_4_dof = static_cast<unsigned int>(rd());
    p.project_on_degeneracy = static_cast<unsigned int>(rd());
    for (double & v : p.gz) v = rd();
    for (double & v : p.Wb) v = rd();
    for (double & v : p.prior) v = rd();
    p.damping = rd();
    p.eps_rot = rd();
    p.eps_trans = rd();
    for (int i = 0; i < W; ++i) p.thresh_rot[i] = rd();
    for (int i = 0; i < W; ++i) p.thresh_trans[i] = rd();
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
      const int flags = mh::window_advance_edges(st, use_relin ? rlp.get() : nullptr, sums.data(), true, p, use_relin ? &rp : nullptr, lin, *lwp, ed, *ewp, w, row.data(), par);
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
