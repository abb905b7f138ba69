// Drives the step arithmetic of mh_icp_align (mimosa_amd/csrc/align_device.hpp, the header the step kernel is built from)
// on the CPU for tests/test_icp_align_cpu.py.  stdin: the number of cases; per case 12 parameters (gz[3], eps_rot, eps_trans,
// damping, prior_rot, prior_trans, thresh_rot, thresh_trans, reg_4_dof, project_on_degeneracy), R[9], t[3], the number of
// queued iterations and 32 doubles (28 sums + 4 counters) for each.  stdout: JSON, per case one entry per queued iteration
// with the row the kernel would publish and, for an evaluated iteration, H, b, xi of its step.
#include <cstdio>
#include <cstdlib>

#include "align_device.hpp"

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
  std::printf("[");
  for (int c = 0; c < n_cases; ++c) {
    mh::AlignParams p;
    for (int i = 0; i < 3; ++i) p.gz[i] = rd();
    p.eps_rot = rd();
    p.eps_trans = rd();
    p.damping = rd();
    p.prior_rot = rd();
    p.prior_trans = rd();
    p.thresh_rot = rd();
    p.thresh_trans = rd();
    p.reg_4_dof = static_cast<int>(rd());
    p.project_on_degeneracy = static_cast<int>(rd());
    mh::AlignState st{};
    for (int i = 0; i < 9; ++i) st.R[i] = rd();
    for (int i = 0; i < 3; ++i) st.t[i] = rd();
    const int n_it = static_cast<int>(rd());
    std::printf("%s[", c ? ", " : "");
    for (int it = 0; it < n_it; ++it) {
      double sums[32];
      for (double & s : sums) s = rd();
      const bool rdg = mh::align_block_degenerate(sums, 0, p.thresh_rot), tdg = mh::align_block_degenerate(sums, 1, p.thresh_trans);
      std::printf("%s{", it ? ", " : "");
      if (!st.stopped) {
        mh::AlignStep o;
        mh::align_step(sums, st.R, st.t, p, rdg, tdg, o);
        arr("H", o.H, 36);
        arr("b", o.b, 6);
        arr("xi", o.xi, 6);
      }
      double row[mh::kRowWords];
      const int flags = mh::align_advance(st, sums, true, p, rdg, tdg, row);
      std::printf("\"flags\": %d, \"rot_degen\": %d, \"trans_degen\": %d, ", flags, rdg ? 1 : 0, tdg ? 1 : 0);
      arr("row", row, mh::kRowWords, false);
      std::printf("}");
    }
    std::printf("]");
  }
  std::printf("]\n");
  return 0;
}
