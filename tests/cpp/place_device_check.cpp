// Drives the place-recognition rule (mimosa_amd/csrc/place_device.hpp, the header place_kernels.hip is built from) on the CPU for
// tests/test_place_cpu.py.  Numbers travel as C hexadecimal floating-point literals, so nothing is rounded on the way.
// stdin: commands, one after another, until the end of input:
//   table                                                   -> [[cos j as %.17g strings], [sin j likewise]], j = 0 .. 14
//   params r_min r_max z_min z_max R[9]                     sets the parameters of the commands below -> the 21 ring boundaries b2 as "%a" strings
//   cells k          then k points (x y z, rounded to f32 here)     -> per point [cell, bits of the value] (cell -1: does not count; bits 0 then)
//   describe k       then k points                                  -> the 1 200 cells as the bits of their floats
//   distance min_overlap m   then the query's 1 200 values and m x 1 200 candidate values (rounded to f32 here)
//                                                           -> per candidate ["D as %a", shift]
//   rank top_k m     then m values of D                      -> the top_k indices as the select kernel's rounds find them with 256 lanes
// stdout: one JSON list per command, one per line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <vector>

#include "place_device.hpp"

static double need()
{
  double v = 0;
  if (std::scanf("%lf", &v) != 1) std::exit(2);
  return v;
}

static unsigned bits_of(float v)
{
  unsigned b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}

int main()
{
  mh::PlaceParams P{};
  bool have_params = false;
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    const std::string_view c(cmd);
    std::printf("[");
    if (c == "table") {
      for (int t = 0; t < 2; ++t) {
        std::printf("%s[", t ? ", " : "");
        for (int j = 0; j < mh::kPlaceQuadSectors; ++j)
          std::printf("%s\"%.17g\"", j ? ", " : "", t ? mh::place_sector_sin(j) : mh::place_sector_cos(j));
        std::printf("]");
      }
    } else if (c == "params") {
      const double r_min = need(), r_max = need();
      P.r_min2 = r_min * r_min;
      P.z_min = need();
      P.z_max = need();
      for (double & v : P.R) v = need();
      mh::place_ring_table(r_max, P.b2);
      have_params = true;
      for (int i = 0; i <= mh::kPlaceRings; ++i) std::printf("%s\"%a\"", i ? ", " : "", P.b2[i]);
    } else if (c == "cells" || c == "describe") {
      if (!have_params) return 3;
      const int k = static_cast<int>(need());
      std::vector<float> desc(mh::kPlaceCells, 0.0f);
      for (int n = 0; n < k; ++n) {
        const float x = static_cast<float>(need()), y = static_cast<float>(need()), z = static_cast<float>(need());
        float value = 0.0f;
        const int cell = mh::place_cell(P, x, y, z, value);
        if (cell >= mh::kPlaceCells) return 3;
        if (cell >= 0 && bits_of(value) > bits_of(desc[static_cast<size_t>(cell)])) desc[static_cast<size_t>(cell)] = value;  // (as the kernel: on the bits)
        if (c == "cells") std::printf("%s[%d, %u]", n ? ", " : "", cell, cell >= 0 ? bits_of(value) : 0u);
      }
      if (c == "describe")
        for (int i = 0; i < mh::kPlaceCells; ++i) std::printf("%s%u", i ? ", " : "", bits_of(desc[static_cast<size_t>(i)]));
    } else if (c == "distance") {
      const int min_overlap = static_cast<int>(need()), m = static_cast<int>(need());
      if (m < 0) return 3;
      std::vector<float> q(mh::kPlaceCells), cd(mh::kPlaceCells);
      double nq[mh::kPlaceSectors], nc[mh::kPlaceSectors];
      for (float & v : q) v = static_cast<float>(need());
      for (int j = 0; j < mh::kPlaceSectors; ++j) nq[j] = mh::place_column_norm(q.data(), j);
      for (int e = 0; e < m; ++e) {
        for (float & v : cd) v = static_cast<float>(need());
        for (int j = 0; j < mh::kPlaceSectors; ++j) nc[j] = mh::place_column_norm(cd.data(), j);
        const mh::PlaceScore s = mh::place_distance(q.data(), nq, cd.data(), nc, min_overlap);
        std::printf("%s[\"%a\", %d]", e ? ", " : "", s.dist, s.shift);
      }
    } else if (c == "rank") {
      const int top_k = static_cast<int>(need()), m = static_cast<int>(need());
      if (m < 0 || top_k < 1 || top_k > mh::kPlaceMaxHits) return 3;
      std::vector<mh::PlaceScore> scores(static_cast<size_t>(m));
      for (mh::PlaceScore & s : scores) {
        s.dist = need();
        s.shift = s.reserved = 0;
      }
      constexpr int kLanes = 256;
      mh::PlaceKey prev = mh::place_no_key();
      std::vector<mh::PlaceKey> keys(kLanes);
      for (int r = 0; r < top_k; ++r) {
        for (int lane = 0; lane < kLanes; ++lane) keys[static_cast<size_t>(lane)] = mh::place_select_lane(scores.data(), m, lane, kLanes, prev);
        const mh::PlaceKey w = mh::place_best_of(keys.data(), kLanes);
        if (w.index >= 0) prev = w;
        std::printf("%s%d", r ? ", " : "", w.index);
      }
    } else {
      return 2;
    }
    std::printf("]\n");
  }
  return 0;
}
