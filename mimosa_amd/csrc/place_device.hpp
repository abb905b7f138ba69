// Place recognition (mh_place_*): the cell of a point in the ring x sector height image, the column norms of an image, the
// distance of two images over every column shift, and the ranking of the hits.  Plain functions for the device
// (place_kernels.hip) and the host (tests/cpp/place_device_check.cpp under g++); both are compiled without floating-point
// contraction, so both give the same digits.  The rule is stated word for word in include/mimosa_hip.h; every expression below
// is written in the order given there.
#pragma once

#include <cmath>
#include <cstdint>

#include "math3.hpp"

namespace mh
{
constexpr int kPlaceRings = 20, kPlaceSectors = 60, kPlaceCells = kPlaceRings * kPlaceSectors;  // MH_PLACE_RINGS, MH_PLACE_SECTORS
constexpr int kPlaceQuadSectors = kPlaceSectors / 4;
constexpr int kPlaceMaxHits = 16;          // MH_PLACE_MAX_HITS
constexpr int kPlaceMaxEntries = 65536;
constexpr double kPlaceNoMatch = 2.0;      // d(s) of a shift with fewer than min_overlap valid columns; D of an entry without an admissible shift

// cos and sin of 6 degrees * j, j = 0 .. 14, as 17-digit literals: the sector rule compares against these numbers, not against
// what a library's cos would give
MH_HD double place_sector_cos(int j)
{
  const double C[kPlaceQuadSectors] = {1.0,
                                       0.9945218953682733,
                                       0.9781476007338057,
                                       0.9510565162951535,
                                       0.9135454576426009,
                                       0.8660254037844386,
                                       0.8090169943749475,
                                       0.7431448254773942,
                                       0.6691306063588582,
                                       0.5877852522924731,
                                       0.5,
                                       0.4067366430758002,
                                       0.30901699437494745,
                                       0.20791169081775934,
                                       0.10452846326765347};
  return C[j];
}
MH_HD double place_sector_sin(int j)
{
  const double S[kPlaceQuadSectors] = {0.0,
                                       0.10452846326765347,
                                       0.20791169081775934,
                                       0.30901699437494745,
                                       0.4067366430758002,
                                       0.5,
                                       0.5877852522924731,
                                       0.6691306063588582,
                                       0.7431448254773942,
                                       0.8090169943749475,
                                       0.8660254037844386,
                                       0.9135454576426009,
                                       0.9510565162951535,
                                       0.9781476007338057,
                                       0.9945218953682733};
  return S[j];
}

struct PlaceParams
{
  double R[9];                  // R_G_F, row-major
  double r_min2;                // r_min * r_min
  double z_min, z_max;
  double b2[kPlaceRings + 1];   // b2[i] = (i * w) * (i * w), w = r_max / 20: place_ring_table
};

// the ring boundaries, squared: computed once (on the host) and handed to the kernel and to the restatement as numbers
inline void place_ring_table(double r_max, double b2[kPlaceRings + 1])
{
#pragma clang fp contract(off)
  const double w = r_max / static_cast<double>(kPlaceRings);
  for (int i = 0; i <= kPlaceRings; ++i) {
    const double e = static_cast<double>(i) * w;
    b2[i] = e * e;
  }
}

// the cell (ring * 60 + sector) of a point and its value, or -1 when the point does not count
MH_HD int place_cell(const PlaceParams & P, float xf, float yf, float zf, float & value)
{
#pragma clang fp contract(off)
  const double x = static_cast<double>(xf), y = static_cast<double>(yf), z = static_cast<double>(zf);
  double p[3];
  for (int a = 0; a < 3; ++a) {
    const double p0 = P.R[3 * a] * x, p1 = P.R[3 * a + 1] * y, p2 = P.R[3 * a + 2] * z;
    const double s01 = p0 + p1;
    p[a] = s01 + p2;
  }
  const double xx = p[0] * p[0], yy = p[1] * p[1];
  const double r2 = xx + yy;
  // (written so that a NaN fails)
  if (!(r2 >= P.r_min2 && r2 < P.b2[kPlaceRings] && p[2] > P.z_min && p[2] < P.z_max)) return -1;
  int ring = 0;
  for (int i = 1; i < kPlaceRings; ++i) ring += r2 >= P.b2[i] ? 1 : 0;
  const double xp = p[0], yp = p[1];
  const int q = (xp > 0.0 && yp >= 0.0) ? 0 : ((xp <= 0.0 && yp > 0.0) ? 1 : ((xp < 0.0 && yp <= 0.0) ? 2 : 3));
  const double u = q == 0 ? xp : (q == 1 ? yp : (q == 2 ? -xp : -yp));
  const double v = q == 0 ? yp : (q == 1 ? -xp : (q == 2 ? -yp : xp));
  int m = 0;
  for (int j = 1; j < kPlaceQuadSectors; ++j) {
    const double vc = v * place_sector_cos(j), us = u * place_sector_sin(j);
    m += vc >= us ? 1 : 0;
  }
  value = static_cast<float>(p[2] - P.z_min);
  return ring * kPlaceSectors + (kPlaceQuadSectors * q + m);
}

// n[j] = sqrt(sum over the rings, ascending, of X[i][j]^2) of column j
MH_HD double place_column_norm(const float * X, int j)
{
#pragma clang fp contract(off)
  double s = 0.0;
  for (int i = 0; i < kPlaceRings; ++i) {
    const double v = static_cast<double>(X[i * kPlaceSectors + j]);
    const double vv = v * v;
    s = s + vv;
  }
  return std::sqrt(s);
}

// d(s) of query Q (norms nq) against candidate Cd (norms nc)
MH_HD double place_shift_distance(const float * Q, const double * nq, const float * Cd, const double * nc, int s, int min_overlap)
{
#pragma clang fp contract(off)
  double acc = 0.0;
  int n_valid = 0;
  int k = s;  // (j + s) % 60
  for (int j = 0; j < kPlaceSectors; ++j) {
    if (nq[j] > 0.0 && nc[k] > 0.0) {
      double dot = 0.0;
      for (int i = 0; i < kPlaceRings; ++i) {
        const double pr = static_cast<double>(Q[i * kPlaceSectors + j]) * static_cast<double>(Cd[i * kPlaceSectors + k]);
        dot = dot + pr;
      }
      const double den = nq[j] * nc[k];
      const double c = dot / den;
      acc = acc + c;
      ++n_valid;
    }
    k = k + 1 == kPlaceSectors ? 0 : k + 1;
  }
  if (n_valid < min_overlap) return kPlaceNoMatch;
  const double mean = acc / static_cast<double>(n_valid);
  return 1.0 - mean;
}

// {D, shift} of an entry; the layout of mh_place_score
struct PlaceScore
{
  double dist;
  int32_t shift, reserved;
};
static_assert(sizeof(PlaceScore) == 16, "place recognition: score layout");

// D = min over s of d[s], shift = the smallest s that attains it; no admissible shift: {2.0, 0}
MH_HD PlaceScore place_best_shift(const double * d)
{
  PlaceScore r;
  r.dist = kPlaceNoMatch;
  r.shift = 0;
  r.reserved = 0;
  for (int s = 0; s < kPlaceSectors; ++s)
    if (d[s] < r.dist) {
      r.dist = d[s];
      r.shift = s;
    }
  return r;
}

// the whole comparison on one thread (the host check; the kernel gives a lane one shift each)
inline PlaceScore place_distance(const float * Q, const double * nq, const float * Cd, const double * nc, int min_overlap)
{
  double d[kPlaceSectors];
  for (int s = 0; s < kPlaceSectors; ++s) d[s] = place_shift_distance(Q, nq, Cd, nc, s, min_overlap);
  return place_best_shift(d);
}

// ---- ranking ----------------------------------------------------------------------------------------------------------------
// D ascending (the doubles compared as they are), then database index ascending; an entry with D == 2.0 is never a hit.
// index < 0: no entry — behind every entry.
struct PlaceKey
{
  double dist;
  int32_t index, shift;
};
MH_HD PlaceKey place_no_key()
{
  PlaceKey k;
  k.dist = kPlaceNoMatch;
  k.index = -1;
  k.shift = 0;
  return k;
}
MH_HD PlaceKey place_key_of(const PlaceScore & s, int index)
{
  PlaceKey k;
  k.dist = s.dist;
  k.index = (index >= 0 && s.dist < kPlaceNoMatch) ? index : -1;
  k.shift = s.shift;
  return k;
}
// a ranks strictly before b
MH_HD bool place_before(const PlaceKey & a, const PlaceKey & b)
{
  if (a.index < 0) return false;
  if (b.index < 0) return true;
  if (a.dist < b.dist) return true;
  if (b.dist < a.dist) return false;
  return a.index < b.index;
}
// Top-K selection, one round (as reloc_select_lane): the best key among entries lane, lane + n_lanes, ... that ranks strictly
// behind `prev` (prev.index < 0 in the first round: every entry qualifies)
MH_HD PlaceKey place_select_lane(const PlaceScore * scores, int n, int lane, int n_lanes, const PlaceKey & prev)
{
  PlaceKey best = place_no_key();
  // four entries per trip, their loads issued together (a walk of one dependent load per entry is most of the kernel); a slot
  // past the last entry re-reads the trip's first entry under index -1, which never ranks before anything
  constexpr int U = 4;
  for (int i0 = lane; i0 < n; i0 += U * n_lanes) {
    PlaceKey k[U];
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * n_lanes;
      const bool valid = i < n;
      k[u] = place_key_of(scores[valid ? i : i0], valid ? i : -1);
    }
    for (int u = 0; u < U; ++u)
      if ((prev.index < 0 || place_before(prev, k[u])) && place_before(k[u], best)) best = k[u];
  }
  return best;
}
MH_HD PlaceKey place_best_of(const PlaceKey * keys, int n)
{
  PlaceKey best = place_no_key();
  for (int i = 0; i < n; ++i)
    if (place_before(keys[i], best)) best = keys[i];
  return best;
}
}  // namespace mh

#if defined(__HIPCC__)
// ---- the launches (place_kernels.hip) -------------------------------------------------------------------------------------
#include <hip/hip_runtime.h>

namespace mh
{
constexpr int kPlaceThreads = 256;       // lanes of a describe workgroup, of a query workgroup (one entry per wave) and of the select workgroup
constexpr int kPlaceChunk = 1024;        // points one describe workgroup folds into its LDS image before it merges
constexpr int kPlaceQueryMaxGrid = 2048; // query workgroups; each takes entries 4 * (block + k * grid) + wave, k = 0, 1, ...

// what the select kernel leaves: the top_k entries in rank order, index -1 behind the last real hit
struct PlaceBest
{
  int32_t index[kPlaceMaxHits];
  int32_t shift[kPlaceMaxHits];
  double dist[kPlaceMaxHits];
};
static_assert(sizeof(PlaceBest) == 256, "place recognition: layout of the hits' block");

// desc (1 200 floats, cleared by this call) = the image of n points at src (stride floats apart)
hipError_t launch_place_describe(const float * src, uint32_t n, uint32_t stride, const PlaceParams & P, float * desc, hipStream_t stream);
// norms[60] of desc
hipError_t launch_place_norms(const float * desc, double * norms, hipStream_t stream);
// scores[e] = {D, shift} of the query against entry e, e < n_entries
hipError_t launch_place_query(const float * q_desc, const double * q_norms, const float * db_desc, const double * db_norms, int n_entries, int min_overlap,
                              PlaceScore * scores, hipStream_t stream);
hipError_t launch_place_select(const PlaceScore * scores, int n_entries, int top_k, PlaceBest * out, hipStream_t stream);
}  // namespace mh
#endif
