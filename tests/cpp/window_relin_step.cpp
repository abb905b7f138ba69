// Drives the relinearization phases of mh_icp_window_optimise_relin (mimosa_amd/csrc/window_device.hpp, the header the step
// kernel is built from) on the CPU for tests/test_icp_window_relin_cpu.py.  stdin: the number of cases; per case its kind:
//   0  transport: H[36], b[6], f, d[6]                          -> Jr^-1(d_r), Exp(d_r), the transported H, b, f
//   1  decide: d[6], relin_rot, relin_trans                     -> window_relin_decide
//   2  local: L (R[9], t[3]), T (R[9], t[3])                    -> window_local
//   3  chain: relin_rot, relin_trans, then a case of tests/cpp/window_step.cpp -> per queued iteration the row, the flags, the
//      mask of the factors the iteration evaluated and, for an evaluated iteration, the step and every pose's offset behind it
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
  mh::WindowWork & w = *wp;
  std::printf("[");
  for (int c = 0; c < n_cases; ++c) {
    const int kind = static_cast<int>(rd());
    std::printf("%s", c ? ", " : "");
    if (kind == 0) {
      double H[36], b[6], f, d[6], Ho[36], bo[6], fo, tmp[36], J[9], E[9];
      for (double & v : H) v = rd();
      for (double & v : b) v = rd();
      f = rd();
      for (double & v : d) v = rd();
      mh::window_jrinv(d, J);
      mh::align_expmap(d, E);
      mh::window_transport(H, b, f, d, Ho, bo, fo, tmp);
      std::printf("{");
      arr("J", J, 9);
      arr("E", E, 9);
      arr("H", Ho, 36);
      arr("b", bo, 6);
      std::printf("\"f\": %.17g}", fo);
    } else if (kind == 1) {
      double d[6];
      for (double & v : d) v = rd();
      const double rr = rd(), rt = rd();
      std::printf("{\"evaluate\": %d}", mh::window_relin_decide(d, rr, rt) ? 1 : 0);
    } else if (kind == 2) {
      double LR[9], Lt[3], R[9], t[3], d[6];
      for (double & v : LR) v = rd();
      for (double & v : Lt) v = rd();
      for (double & v : R) v = rd();
      for (double & v : t) v = rd();
      mh::window_local(LR, Lt, R, t, d);
      std::printf("{");
      arr("d", d, 6, false);
      std::printf("}");
    } else {
      mh::WindowRelinParams rp{};
      rp.relin_rot = rd();
      rp.relin_trans = rd();
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
      // (the step needs nothing from WindowRelin in the first iteration: garbage there must not matter)
      std::memset(static_cast<void *>(rlp.get()), 0x41, sizeof(mh::WindowRelin));
      const int n_it = static_cast<int>(rd());
      std::printf("[");
      for (int it = 0; it < n_it; ++it) {
        std::vector<double> sums(32 * static_cast<size_t>(W));
        for (double & s : sums) s = rd();
        std::printf("%s{", it ? ", " : "");
        const bool evaluated = !st.stopped;
        rp.first = it == 0 ? 1 : 0;
        const unsigned int eval = mh::window_relin_mask(*rlp, p, rp);
        // a kept factor's sums never reach the step: what is fed here for it must not matter
        for (int i = 0; i < W; ++i)
          if (!((eval >> i) & 1u))
            for (int q = 0; q < 32; ++q) sums[32 * static_cast<size_t>(i) + q] = 1e300;
        std::vector<double> row(static_cast<size_t>(mh::window_row_words(W)));
        mh::WindowSerial par;
        const int flags = mh::window_advance_relin(st, *rlp, sums.data(), true, p, rp, w, row.data(), par);
        if (evaluated) {
          arr("xi", w.x, 6 * W);
          arr("H", &w.H[0][0], 36 * W);
          arr("b", &w.b[0][0], 6 * W);
          arr("d", &rlp->d[0][0], 6 * mh::kWindowMax);
          std::printf("\"cost\": %.17g, \"ok\": %d, \"eval\": %u, \"next\": %u, ", w.cost, w.ok, eval, rlp->eval);
        }
        std::printf("\"flags\": %d, ", flags);
        arr("row", row.data(), mh::window_row_words(W), false);
        std::printf("}");
      }
      std::printf("]");
    }
  }
  std::printf("]\n");
  return 0;
}
