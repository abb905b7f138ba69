// Map carving (mh_map_carve*): the direction cell of a vector and the seen-through predicate of a map point.  Plain functions
// for the device (carve_kernels.hip) and the host (tests/cpp/map_carve_cells.cpp under g++); both are compiled without
// floating-point contraction, so both give the same digits.  The rule is stated word for word in include/mimosa_hip.h; every
// expression below is written in the order given there.
#pragma once

#include <cmath>
#include <cstdint>

#include "math3.hpp"

namespace mh
{
constexpr int kCarveGridMin = 4, kCarveGridMax = 512, kCarveRingMax = 2;
// "not hit": the bit pattern of +infinity, above the pattern of every finite non-negative double, so that an unsigned 64-bit
// minimum over bit patterns is the minimum over values
constexpr unsigned long long kCarveNotHit = 0x7FF0000000000000ull;

// decisions of carve_decide
constexpr int kCarveUntested = 0, kCarveKept = 1, kCarveSeenThrough = 2;

struct CarveParams
{
  double R[9], t[3];     // pose of F in the map frame (row-major R)
  double origin[3];      // sensor origin in F
  double range_min2, range_max2;  // range_min * range_min, range_max * range_max
  double margin_abs, margin_rel;
  int N, ring;
};

MH_HD bool carve_finite(double v) { return v - v == 0.0; }

// the cell of s, or -1; face / i / j of it where the caller wants them
MH_HD int carve_cell(const double s[3], int N, int * face_out = nullptr, int * i_out = nullptr, int * j_out = nullptr)
{
#pragma clang fp contract(off)
  const double a0 = std::fabs(s[0]), a1 = std::fabs(s[1]), a2 = std::fabs(s[2]);
  const int f = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
  const double m = f == 0 ? a0 : (f == 1 ? a1 : a2);
  // the zero vector; an overflowed difference; a NaN component (one on the major axis makes m NaN or 0, another fails a_k <= m)
  if (!(m > 0.0) || !carve_finite(m) || !(a0 <= m) || !(a1 <= m) || !(a2 <= m)) return -1;
  const double sf = f == 0 ? s[0] : (f == 1 ? s[1] : s[2]);
  const double su = f == 0 ? s[1] : (f == 1 ? s[2] : s[0]);
  const double sv = f == 0 ? s[2] : (f == 1 ? s[0] : s[1]);
  const int face = 2 * f + (sf < 0.0 ? 1 : 0);
  const double u = su / m, v = sv / m;  // in [-1, 1]: |su|, |sv| <= m
  const double half = 0.5 * static_cast<double>(N);
  int i = static_cast<int>(std::floor((u + 1.0) * half));  // in [0, N]
  int j = static_cast<int>(std::floor((v + 1.0) * half));
  i = i < N - 1 ? i : N - 1;
  j = j < N - 1 ? j : N - 1;
  if (face_out) *face_out = face;
  if (i_out) *i_out = i;
  if (j_out) *j_out = j;
  return (face * N + j) * N + i;
}

MH_HD double carve_r2(const double s[3])
{
#pragma clang fp contract(off)
  const double p0 = s[0] * s[0], p1 = s[1] * s[1], p2 = s[2] * s[2];
  const double s01 = p0 + p1;
  return s01 + p2;
}

// an observation point: its cell and r2 when it enters the image, else -1
MH_HD int carve_observe(const CarveParams & P, float xf, float yf, float zf, double & r2)
{
#pragma clang fp contract(off)
  const double x = static_cast<double>(xf), y = static_cast<double>(yf), z = static_cast<double>(zf);
  if (!carve_finite(x) || !carve_finite(y) || !carve_finite(z)) return -1;
  const double s[3] = {x - P.origin[0], y - P.origin[1], z - P.origin[2]};
  r2 = carve_r2(s);
  if (!(r2 >= P.range_min2)) return -1;
  return carve_cell(s, P.N);
}

// a map point in F, sensor-relative: s = R^T (p - t) - origin
MH_HD void carve_map_vector(const CarveParams & P, float xf, float yf, float zf, double s[3])
{
#pragma clang fp contract(off)
  const double d0 = static_cast<double>(xf) - P.t[0], d1 = static_cast<double>(yf) - P.t[1], d2 = static_cast<double>(zf) - P.t[2];
  for (int a = 0; a < 3; ++a) {
    const double p0 = P.R[a] * d0, p1 = P.R[3 + a] * d1, p2 = P.R[6 + a] * d2;
    const double s01 = p0 + p1;
    const double s012 = s01 + p2;
    s[a] = s012 - P.origin[a];
  }
}

// img: the 6 N^2 cells as doubles ("not hit" reads as +infinity)
MH_HD int carve_decide(const CarveParams & P, const double * img, float xf, float yf, float zf)
{
#pragma clang fp contract(off)
  double s[3];
  carve_map_vector(P, xf, yf, zf, s);
  const double r2 = carve_r2(s);
  if (!(r2 >= P.range_min2 && r2 <= P.range_max2)) return kCarveUntested;
  int face, ci, cj;
  if (carve_cell(s, P.N, &face, &ci, &cj) < 0) return kCarveUntested;
  const double r = std::sqrt(r2);
  const double inf = HUGE_VAL;
  double q = inf;
  for (int dj = -P.ring; dj <= P.ring; ++dj) {
    const int j = cj + dj;
    if (j < 0 || j >= P.N) continue;
    for (int di = -P.ring; di <= P.ring; ++di) {
      const int i = ci + di;
      if (i < 0 || i >= P.N) continue;
      const double c = img[(face * P.N + j) * P.N + i];
      if (!(c < inf)) return kCarveKept;  // a cell that is not hit
      q = c < q ? c : q;
    }
  }
  const double mr = P.margin_rel * r;
  const double mg = P.margin_abs + mr;
  const double lim = r + mg;
  return lim * lim < q ? kCarveSeenThrough : kCarveKept;
}

}  // namespace mh
