// Drives the phases of mh_icp_window_marginalise (mimosa_amd/csrc/window_device.hpp: window_marginal_impl, the header the
// kernel is built from) on the CPU for tests/test_icp_window_marginal_cpu.py.  stdin: the number of cases; per case
//   n_lin, per linear factor pose, L (R[9], t[3]), H[36], b[6], f, n_edges, per edge pose_a, pose_b, Z (R[9], t[3]), info[36],
//   W, has_Z, have, reg_4_dof, project_on_degeneracy (masks), gz[3], Wb[6], prior[6], damping, thresh_rot, thresh_trans of pose 0,
//   per pose R[9], t[3], per pose ZR[9], Zt[3], the 32 words of factor 0
// -> H_m, b_m, f_m, valid, n_ties and the accumulated A00, A10, A11', g0, g1', c
// stdout: JSON, one entry per case.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "window_device.hpp"

static double rd()
{
  double v = 0;
  if (std::scanf("%lf", &v) != 1) std::exit(2);
  return v;
}
static void arr(const char * name, const double * v, int n)
{
  std::printf("\"%s\": [", name);
  for (int i = 0; i < n; ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("], ");
}

int main()
{
  const int n_cases = static_cast<int>(rd());
  auto linp = std::make_unique<mh::WindowLinear>();
  auto lwp = std::make_unique<mh::WindowLinWork>();
  auto edp = std::make_unique<mh::WindowEdges>();
  auto wp = std::make_unique<mh::WindowMarginalWork>();
  mh::WindowLinear & lin = *linp;
  mh::WindowEdges & ed = *edp;
  std::printf("[");
  for (int c = 0; c < n_cases; ++c) {
    std::printf("%s{", c ? ", " : "");
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
    if (p.W < 2 || p.W > mh::kWindowMax) return 3;
    const int W = p.W;
    for (int j = 0; j < lin.n; ++j)
      if (lin.pose[j] < 0 || lin.pose[j] >= W) return 3;
    for (int e = 0; e < ed.n; ++e)
      if (ed.a[e] < 0 || ed.a[e] >= ed.b[e] || ed.b[e] >= W || (ed.a[e] == 0 && ed.b[e] > 1)) return 3;
    p.has_Z = static_cast<unsigned int>(rd());
    p.have = static_cast<unsigned int>(rd());
    p.reg_4_dof = static_cast<unsigned int>(rd());
    p.project_on_degeneracy = static_cast<unsigned int>(rd());
    for (double & v : p.gz) v = rd();
    for (double & v : p.Wb) v = rd();
    for (double & v : p.prior) v = rd();
    p.damping = rd();
    p.thresh_rot[0] = rd();
    p.thresh_trans[0] = rd();
    mh::WindowState st{};
    for (int i = 0; i < W; ++i) {
      for (double & v : st.R[i]) v = rd();
      for (double & v : st.t[i]) v = rd();
    }
    for (int i = 0; i < W; ++i) {
      for (double & v : st.ZR[i]) v = rd();
      for (double & v : st.Zt[i]) v = rd();
    }
    double sums[32];
    for (double & s : sums) s = rd();
    std::memset(static_cast<void *>(lwp.get()), 0x41, sizeof(mh::WindowLinWork));
    std::memset(static_cast<void *>(wp.get()), 0x41, sizeof(mh::WindowMarginalWork));
    mh::WindowMarginalOut out;
    std::memset(static_cast<void *>(&out), 0x41, sizeof(out));
    mh::WindowSerial par;
    mh::window_marginal_impl(sums, st, p, lin, *lwp, ed, *wp, out, par);
    arr("H", out.H, 36);
    arr("b", out.b, 6);
    arr("A00", wp->A00, 36);
    arr("A10", wp->A10, 36);
    arr("A11", wp->A11, 36);
    arr("g0", wp->g0, 6);
    arr("g1", wp->g1, 6);
    std::printf("\"c\": %.17g, \"f\": %.17g, \"valid\": %d, \"n_ties\": %d}", wp->c, out.f, out.valid, out.n_ties);
  }
  std::printf("]\n");
  return 0;
}
