// Relocalisation (mh_icp_score_poses, mh_icp_relocalise): everything of the score of a candidate pose that is not a map lookup.
// Plain functions for the device (reloc_kernels.hip) and the host (tests/cpp/reloc_select.cpp under g++); both are compiled
// without floating-point contraction, so both give the same digits.
//
// Score of one pose (R, t) with gate g and stride s over a factor's points i, i % s == 0, i counting in the order the points
// were given to mh_icp_create*:
//   q        = reloc_transform(R, t, x, y, z)                  fp64, the additions in the order written there
//   c        = reloc_voxel(q * inv_leaf)                       a point with any |q_a * inv_leaf| not below 2^20 (or not finite)
//                                                              indexes nothing: not occupied, not an inlier
//   occupied   the cell of c holds at least one point
//   d2       = min over the map's neighbour voxels of reloc_sq_dist(point - q)
//   inlier     a nearest point exists and d2 <= g * g
// and mh_pose_score = {points looked at, occupied, inliers, 0, sum of d2 over the inliers}.
//
// The squared distance is the one mh_map_knn reports in sq_dists: knn_query's exact tier (icp_kernels.hip) ranks its survivors
// with sq_dist3(c.x - q0, c.y - q1, c.z - q2) = (dx * dx + dz * dz) + dy * dy, d = map point - query, every product and sum
// rounded on its own — Eigen's SSE2 Vector4d reduction order, NOT dx * dx + (dy * dy + dz * dz).  reloc_sq_dist is that
// expression, so the minimum found here is mh_map_knn's sq_dists[0] for k = 1 bit for bit (a minimum does not depend on the
// order the candidates are visited in, and ties give the same value whichever candidate wins).
#pragma once

#include <cmath>
#include <cstdint>

#include "math3.hpp"
#include "voxel_map.hpp"

namespace mh
{
constexpr int kRelocChunk = 1024;      // points of the (strided) cloud one workgroup of the score kernel serves; independent of n_poses
constexpr int kRelocThreads = 256;     // its lanes: lane l takes points chunk_base + l, + 256, + 512, + 768 in that order
constexpr int kRelocSelThreads = 256;  // the lanes of the select kernel's one workgroup
constexpr int kRelocMaxRefine = 8;     // MH_RELOC_MAX_REFINE
constexpr double kRelocCoordLimit = 1048576.0;  // 2^20 voxels (map_device.hpp: kVoxCoordBits = 21)

// one workgroup's share of a pose's score, and a pose's score (the layout of mh_pose_score)
struct RelocPartial
{
  int32_t n_occupied, n_inliers;
  double sum_sq;
};
struct RelocScore
{
  int32_t n_points, n_occupied, n_inliers, reserved;
  double sum_sq;
};
static_assert(sizeof(RelocPartial) == 16 && sizeof(RelocScore) == 24, "relocalisation: score layout");

// points of an n-point cloud with i % stride == 0, and the workgroups a pose is split over
MH_HD int reloc_sub_count(int n, int stride) { return n > 0 ? (n - 1) / stride + 1 : 0; }
MH_HD int reloc_chunks(int m) { return m > 0 ? (m + kRelocChunk - 1) / kRelocChunk : 1; }

// q_a = ((R[3a] x + R[3a+1] y) + R[3a+2] z) + t[a]
MH_HD void reloc_transform(const double * R, const double * t, float xf, float yf, float zf, double q[3])
{
#pragma clang fp contract(off)
  const double x = static_cast<double>(xf), y = static_cast<double>(yf), z = static_cast<double>(zf);
  for (int a = 0; a < 3; ++a) {
    const double p0 = R[3 * a] * x, p1 = R[3 * a + 1] * y, p2 = R[3 * a + 2] * z;
    const double s01 = p0 + p1;
    const double s012 = s01 + p2;
    q[a] = s012 + t[a];
  }
}

// voxel coordinate of u = q * inv_leaf; false: outside +-2^20 voxels or not finite — c is not written and nothing may be indexed
MH_HD bool reloc_voxel(const double u[3], int c[3])
{
  if (!(std::fabs(u[0]) < kRelocCoordLimit) || !(std::fabs(u[1]) < kRelocCoordLimit) || !(std::fabs(u[2]) < kRelocCoordLimit)) return false;
  c[0] = fast_floor(u[0]);
  c[1] = fast_floor(u[1]);
  c[2] = fast_floor(u[2]);
  return true;
}

// d = map point - query (see the head of the file)
MH_HD double reloc_sq_dist(double dx, double dy, double dz)
{
#pragma clang fp contract(off)
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double xz = xx + zz;
  return xz + yy;
}

// Squared distance (voxel units) from u to the box of the voxel c + (ox, oy, oz), c the voxel of u; shrunk by a millionth of a
// voxel per axis, so that a point the map filed under that voxel by its own rounding is never farther than its box.
MH_HD double reloc_box_sq(const double u[3], const int c[3], int ox, int oy, int oz)
{
  const int o[3] = {ox, oy, oz};
  double s = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double f = u[a] - static_cast<double>(c[a]);  // in [0, 1]
    double d = o[a] < 0 ? f : (o[a] > 0 ? 1.0 - f : 0.0);
    d = d > 1e-6 ? d - 1e-6 : 0.0;
    s += d * d;
  }
  return s;
}

// ---- fixed-order folds ----------------------------------------------------------------------------------------------------
// a lane's points in index order, the lanes of a wave by the DPP sums of wave_dpp.hpp, then:
// the waves of a workgroup in wave order
MH_HD RelocPartial reloc_fold_waves(const RelocPartial * w, int n_waves)
{
  RelocPartial r = w[0];
  for (int i = 1; i < n_waves; ++i) {
    r.n_occupied += w[i].n_occupied;
    r.n_inliers += w[i].n_inliers;
    r.sum_sq += w[i].sum_sq;
  }
  return r;
}
// the workgroups of a pose in chunk order
MH_HD RelocScore reloc_fold_chunks(const RelocPartial * p, int n_chunks, int n_points)
{
  RelocScore s;
  s.n_points = n_points;
  s.n_occupied = p[0].n_occupied;
  s.n_inliers = p[0].n_inliers;
  s.reserved = 0;
  s.sum_sq = p[0].sum_sq;
  for (int i = 1; i < n_chunks; ++i) {
    s.n_occupied += p[i].n_occupied;
    s.n_inliers += p[i].n_inliers;
    s.sum_sq += p[i].sum_sq;
  }
  return s;
}

// ---- ranking ----------------------------------------------------------------------------------------------------------------
// n_inliers descending, then sum_sq ascending (the doubles compared as they are), then pose index ascending.  index < 0: no
// pose — behind every pose.
struct RelocKey
{
  int32_t n_inliers;
  int32_t index;
  double sum_sq;
};
MH_HD RelocKey reloc_no_key()
{
  RelocKey k;
  k.n_inliers = 0;
  k.index = -1;
  k.sum_sq = 0.0;
  return k;
}
MH_HD RelocKey reloc_key_of(const RelocScore & s, int index)
{
  RelocKey k;
  k.n_inliers = s.n_inliers;
  k.index = index;
  k.sum_sq = s.sum_sq;
  return k;
}
// a ranks strictly before b
MH_HD bool reloc_before(const RelocKey & a, const RelocKey & b)
{
  if (a.index < 0) return false;
  if (b.index < 0) return true;
  if (a.n_inliers != b.n_inliers) return a.n_inliers > b.n_inliers;
  if (a.sum_sq < b.sum_sq) return true;
  if (b.sum_sq < a.sum_sq) return false;
  return a.index < b.index;
}

// Top-K selection, one round: the best key among poses lane, lane + n_lanes, ... that ranks strictly behind `prev` (prev.index
// < 0 in the first round: every pose qualifies).  K rounds, each followed by reloc_best_of over the lanes' answers, give the K
// best in order: the keys are distinct (the index is part of them), so "strictly behind the last winner" never repeats one.
MH_HD RelocKey reloc_select_lane(const RelocScore * scores, int n_poses, int lane, int n_lanes, const RelocKey & prev)
{
  RelocKey best = reloc_no_key();
  // four poses per trip, their loads issued together (a walk of one dependent load per pose was most of the select kernel); a
  // slot past the last pose re-reads the trip's first pose under index -1, which never ranks before anything
  constexpr int U = 4;
  for (int i0 = lane; i0 < n_poses; i0 += U * n_lanes) {
    RelocKey k[U];
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * n_lanes;
      const bool valid = i < n_poses;
      k[u] = reloc_key_of(scores[valid ? i : i0], valid ? i : -1);
    }
    for (int u = 0; u < U; ++u) {
      const bool take = (prev.index < 0 || reloc_before(prev, k[u])) && reloc_before(k[u], best);
      if (take) best = k[u];
    }
  }
  return best;
}
MH_HD RelocKey reloc_best_of(const RelocKey * keys, int n)
{
  RelocKey best = reloc_no_key();
  for (int i = 0; i < n; ++i)
    if (reloc_before(keys[i], best)) best = keys[i];
  return best;
}
}  // namespace mh

#if defined(__HIPCC__)
// ---- the launch chain (reloc_kernels.hip) ---------------------------------------------------------------------------------
#include "icp_device.hpp"

namespace mh
{
// what the select kernel leaves in mapped pinned memory: the top_k pose indices in rank order (-1 behind the last pose) and
// their scores
struct RelocBest
{
  int32_t index[kRelocMaxRefine];
  RelocScore score[kRelocMaxRefine];
};
static_assert(sizeof(RelocBest) == 224, "relocalisation: layout of the winners' block");

struct RelocScoreArgs
{
  MapView map;
  const float4 * sub;       // the factor's points i with i % stride == 0, point i at i / stride (m of them)
  int m, n_chunks, n_poses;
  const double * poses;     // 12 doubles per pose: R row-major, t
  double gate2;             // g * g
  RelocPartial * partials;  // [n_poses][n_chunks]
};

// sub[o / stride] = src[i] for every point whose index o = perm[i] (perm == nullptr: o = i) in the caller's order has o % stride == 0
hipError_t launch_reloc_gather(const float4 * src, const uint32_t * perm, int n, int stride, float4 * sub, hipStream_t stream);
hipError_t launch_reloc_score(const RelocScoreArgs & a, hipStream_t stream);
hipError_t launch_reloc_fold(const RelocPartial * partials, int n_poses, int n_chunks, int m, RelocScore * scores, hipStream_t stream);
hipError_t launch_reloc_select(const RelocScore * scores, int n_poses, int top_k, RelocBest * out, hipStream_t stream);
}  // namespace mh
#endif
