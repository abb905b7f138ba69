// Drives the rule of map carving (mimosa_amd/csrc/carve_device.hpp, the header carve_kernels.hip is built from) on the CPU for
// tests/test_map_carve_cpu.py.  Numbers travel as C hexadecimal floating-point literals, so nothing is rounded on the way.
// stdin: commands, one after another, until the end of input:
//   cells N k          then k vectors (s0 s1 s2)                            -> per vector [cell, face, i, j] (cell -1: none; then face = i = j = -1)
//   params N ring range_min range_max margin_abs margin_rel R[9] t[3] origin[3]   sets the parameters of the commands below -> []
//   observe k          then k points (x y z, rounded to f32 here)           -> per point [cell, "r2"] (cell -1: not used; r2 only when used)
//   image h            then h pairs (cell value); every other cell not hit  -> []
//   decide k           then k points (x y z, rounded to f32 here)           -> per point 0 untested, 1 kept, 2 seen through
// stdout: one JSON list per command, one per line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "carve_device.hpp"

static double need()
{
  double v = 0;
  if (std::scanf("%lf", &v) != 1) std::exit(2);
  return v;
}

int main()
{
  mh::CarveParams P{};
  P.N = 4;
  std::vector<double> img;
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    const std::string_view c(cmd);
    std::printf("[");
    if (c == "cells") {
      const int N = static_cast<int>(need()), k = static_cast<int>(need());
      for (int n = 0; n < k; ++n) {
        const double s[3] = {need(), need(), need()};
        int face = -1, i = -1, j = -1;
        const int cell = mh::carve_cell(s, N, &face, &i, &j);
        std::printf("%s[%d, %d, %d, %d]", n ? ", " : "", cell, face, i, j);
      }
    } else if (c == "params") {
      P.N = static_cast<int>(need());
      P.ring = static_cast<int>(need());
      const double rmin = need(), rmax = need();
      P.range_min2 = rmin * rmin;
      P.range_max2 = rmax * rmax;
      P.margin_abs = need();
      P.margin_rel = need();
      for (double & v : P.R) v = need();
      for (double & v : P.t) v = need();
      for (double & v : P.origin) v = need();
      if (P.N < mh::kCarveGridMin || P.N > mh::kCarveGridMax || P.ring < 0 || P.ring > mh::kCarveRingMax) return 3;
      img.assign(static_cast<size_t>(6) * P.N * P.N, HUGE_VAL);
    } else if (c == "observe") {
      const int k = static_cast<int>(need());
      for (int n = 0; n < k; ++n) {
        const float x = static_cast<float>(need()), y = static_cast<float>(need()), z = static_cast<float>(need());
        double r2 = 0;
        const int cell = mh::carve_observe(P, x, y, z, r2);
        if (cell >= 0)
          std::printf("%s[%d, \"%a\"]", n ? ", " : "", cell, r2);
        else
          std::printf("%s[-1]", n ? ", " : "");
      }
    } else if (c == "image") {
      img.assign(static_cast<size_t>(6) * P.N * P.N, HUGE_VAL);
      const int h = static_cast<int>(need());
      for (int n = 0; n < h; ++n) {
        const long cell = static_cast<long>(need());
        const double v = need();
        if (cell < 0 || cell >= static_cast<long>(img.size())) return 3;
        img[static_cast<size_t>(cell)] = v;
      }
    } else if (c == "decide") {
      const int k = static_cast<int>(need());
      if (img.empty()) return 3;
      for (int n = 0; n < k; ++n) {
        const float x = static_cast<float>(need()), y = static_cast<float>(need()), z = static_cast<float>(need());
        std::printf("%s%d", n ? ", " : "", mh::carve_decide(P, img.data(), x, y, z));
      }
    } else {
      return 2;
    }
    std::printf("]\n");
  }
  return 0;
}
