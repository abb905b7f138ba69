// Drives the step arithmetic of mh_icp_window_optimise (mimosa_amd/csrc/window_device.hpp, the header the step kernel is built
// from) on the CPU for tests/test_icp_window_cpu.py.  stdin: the number of cases; per case W, the masks has_Z, have, reg_4_dof,
// project_on_degeneracy, gz[3], between_info[6], prior_info[6], damping, eps_rot, eps_trans, thresh_rot[W], thresh_trans[W],
// (R[9], t[3]) x W, (Z_R[9], Z_t[3]) x W, the number of queued iterations and 32 W doubles (28 sums + 4 counters per pose) for
// each.  stdout: JSON, per case one entry per queued iteration with the row the kernel would publish and, for an evaluated
// iteration, the assembled blocks, the right-hand side and the step; a window of one pose also reports align_step's answer.
#include <cstdio>
#include <cstdlib>
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
  mh::WindowWork & w = *wp;
  std::printf("[");
  for (int c = 0; c < n_cases; ++c) {
    mh::WindowParams p{};
    p.W = static_cast<int>(rd());
    if (p.W < 1 || p.W > mh::kWindowMax) return 3;
    const int W = p.W;
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
    const int n_it = static_cast<int>(rd());
    std::printf("%s[", c ? ", " : "");
    for (int it = 0; it < n_it; ++it) {
      std::vector<double> sums(32 * static_cast<size_t>(W));
      for (double & s : sums) s = rd();
      std::printf("%s{", it ? ", " : "");
      const bool evaluated = !st.stopped;
      if (evaluated && W == 1 && !(p.has_Z & 2u)) {  // the same iteration through align_step
        mh::AlignParams ap{};
        for (int q = 0; q < 3; ++q) ap.gz[q] = p.gz[q];
        ap.eps_rot = p.eps_rot;
        ap.eps_trans = p.eps_trans;
        ap.damping = p.damping;
        ap.prior_rot = p.prior[0];
        ap.prior_trans = p.prior[3];
        ap.thresh_rot = p.thresh_rot[0];
        ap.thresh_trans = p.thresh_trans[0];
        ap.reg_4_dof = static_cast<int>(p.reg_4_dof & 1u);
        ap.project_on_degeneracy = static_cast<int>(p.project_on_degeneracy & 1u);
        mh::AlignStep o;
        mh::align_step(sums.data(), st.R[0], st.t[0], ap, mh::align_block_degenerate(sums.data(), 0, ap.thresh_rot),
                       mh::align_block_degenerate(sums.data(), 1, ap.thresh_trans), o);
        arr("align_xi", o.xi, 6);
        arr("align_R", o.R, 9);
        arr("align_t", o.t, 3);
        std::printf("\"align_bits\": %d, \"align_converged\": %d, ", o.bits, o.converged);
      }
      std::vector<double> row(static_cast<size_t>(mh::window_row_words(W)));
      mh::WindowSerial par;
      const int flags = mh::window_advance(st, sums.data(), true, p, w, row.data(), par);
      if (evaluated) {
        arr("A", &w.A[0][0], 36 * W);
        arr("E", &w.E[0][0], 36 * W);
        arr("rhs", w.rhs, 6 * W);
        arr("xi", w.x, 6 * W);
        arr("H", &w.H[0][0], 36 * W);
        std::printf("\"cost\": %.17g, \"ok\": %d, ", w.cost, w.ok);
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
