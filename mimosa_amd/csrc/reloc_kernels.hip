// Relocalisation: score candidate poses of a factor's cloud against its map, and rank them (mh_icp_score_poses,
// mh_icp_relocalise; the arithmetic that is not a map lookup: reloc_device.hpp).  Compiled without floating-point contraction.
//
// The chain of one call: gather (the strided cloud in the caller's point order) -> score (one workgroup per pose and chunk of
// kRelocChunk points) -> fold (one lane per pose: its chunks in chunk order) -> select (one workgroup: the top_k poses).
// No floating-point atomics anywhere: a lane adds its points in index order, a wave its lanes by the DPP pattern of
// wave_dpp.hpp, a workgroup its waves in wave order, a pose its workgroups in chunk order.  The chunk size is a constant, so a
// pose's score has the same bits alone, at any position of any batch and on every repeat.
//
// The score kernel brings its own lookup over the layout of voxel_map.hpp — one block-hash probe, the halo'd 6 x 6 x 6 cell
// table of the query's block, the float4 buckets — and reads nothing of the coarse (packed) tier: it wants ONE nearest
// distance per query, not a k-NN list, and most queries of a global search end at the probe (no table: nothing lies in the
// block or its halo).  A workgroup is 256 lanes: the kernel is a chain of dependent gathers per lane, what hides it is waves
// per SIMD, and a 1 024-point cloud (the usual stride-subsampled scan) is one workgroup per pose with four points per lane —
// 1 024 lanes per workgroup would leave a pose's lanes one point each and a barrier four times as wide for nothing.  The
// strided cloud (16 KiB at 1 024 points) is read straight from L2, which every pose's workgroup hits: a lane reads each of its
// points once, so staging them in LDS would add a copy and no reuse.
#include <hip/hip_runtime.h>

#include "map_device.hpp"
#include "reloc_device.hpp"
#include "wave_dpp.hpp"

namespace mh
{
namespace
{
constexpr double kRelocInf = 1.7976931348623157e308;

__global__ __launch_bounds__(256) void reloc_gather_kernel(const float4 * src, const uint32_t * perm, int n, int stride, float4 * sub)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = perm ? perm[i] : static_cast<uint32_t>(i);
  if (o < static_cast<uint32_t>(n) && o % static_cast<uint32_t>(stride) == 0u) sub[o / static_cast<uint32_t>(stride)] = src[i];
}

// the nearest squared distance among the cnt points of voxel vid, folded into best
__device__ __forceinline__ void reloc_scan_voxel(const float4 * buckets, uint32_t word, const double q[3], double & best)
{
  const uint32_t cnt = min(word & 31u, static_cast<uint32_t>(kBucketStride));
  const float4 * b = buckets + static_cast<size_t>(word >> 5) * kBucketStride;
  for (uint32_t s = 0; s < cnt; ++s) {
    const float4 c = b[s];
    const double d = reloc_sq_dist(static_cast<double>(c.x) - q[0], static_cast<double>(c.y) - q[1], static_cast<double>(c.z) - q[2]);
    if (d < best) best = d;
  }
}

// one point of one pose: occupied / inlier / d2 (valid where inlier)
template <int NOFF>
__device__ __forceinline__ void reloc_score_point(const MapView & map, const double * R, const double * t, const float4 p, double gate2,
                                                  double leaf2, uint32_t & occupied, uint32_t & inlier, double & d2)
{
  occupied = inlier = 0u;
  d2 = 0.0;
  double q[3];
  reloc_transform(R, t, p.x, p.y, p.z, q);
  const double u[3] = {q[0] * map.inv_leaf, q[1] * map.inv_leaf, q[2] * map.inv_leaf};
  int c[3];
  if (!reloc_voxel(u, c)) return;  // outside +-2^20 voxels, or not finite: indexes nothing
  // one hash probe: table entry = {key lo, key hi, block id, -}; hi word -1 = empty slot (|c| < 2^20: the block coordinate fits the key)
  const int bx = c[0] >> kBlockLog2, by = c[1] >> kBlockLog2, bz = c[2] >> kBlockLog2;
  const uint64_t key = pack_coord_key(bx, by, bz);
  const int klo = static_cast<int>(static_cast<uint32_t>(key)), khi = static_cast<int>(static_cast<uint32_t>(key >> 32));
  uint32_t h = block_hash(bx, by, bz) & map.mask;
  int4 e = map.table[h];
  while (e.y != -1 && !(e.x == klo && e.y == khi)) {  // collision: linear probe (load <= 0.5, so an empty slot ends it)
    h = (h + 1) & map.mask;
    e = map.table[h];
  }
  if (e.y == -1) return;  // no table: nothing lies in the block or its halo
  constexpr int m = kBlockDim - 1;
  const uint32_t * tab = map.cells + static_cast<size_t>(e.z) * kCellsPerBlock + halo_index(c[0] & m, c[1] & m, c[2] & m);
  const uint32_t centre = tab[0];
  occupied = (centre & 31u) ? 1u : 0u;
  double best = kRelocInf;
  reloc_scan_voxel(map.buckets, centre, q, best);
  // the other neighbour voxels of the map's mode.  The minimum does not depend on the order they are visited in; a voxel
  // whose box is farther than the best so far — or than the gate: such a point is no inlier whatever its distance — is passed over.
#pragma unroll
  for (int i = -1; i <= 1; ++i)
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
      for (int k = -1; k <= 1; ++k) {
        const int nz = (i != 0) + (j != 0) + (k != 0);
        if (nz == 0 || NOFF == 1 || (NOFF == 7 && nz != 1) || (NOFF == 19 && nz == 3)) continue;
        const uint32_t word = tab[(i * kHaloDim + j) * kHaloDim + k];
        if ((word & 31u) == 0u) continue;
        const double box = reloc_box_sq(u, c, i, j, k) * leaf2;
        if (box > best || box > gate2) continue;
        reloc_scan_voxel(map.buckets, word, q, best);
      }
  if (best <= gate2) {  // (best == kRelocInf: no nearest point; the gate is finite)
    inlier = 1u;
    d2 = best;
  }
}

template <int NOFF>
__global__ __launch_bounds__(kRelocThreads) void reloc_score_kernel(const RelocScoreArgs a)
{
  __shared__ RelocPartial s_wave[kRelocThreads / 64];
  const int pose = static_cast<int>(blockIdx.x) / a.n_chunks, chunk = static_cast<int>(blockIdx.x) - pose * a.n_chunks;
  double R[9], t[3];
  {
    const double * P = a.poses + static_cast<size_t>(pose) * 12;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = P[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = P[9 + i];
  }
  const double leaf = 1.0 / a.map.inv_leaf, leaf2 = leaf * leaf;
  uint32_t cnt[2] = {0u, 0u};
  double sum[1] = {0.0};
  constexpr int kPerLane = kRelocChunk / kRelocThreads;
  for (int r = 0; r < kPerLane; ++r) {  // the lane's points in index order
    const int i = chunk * kRelocChunk + r * kRelocThreads + static_cast<int>(threadIdx.x);
    if (i < a.m) {
      uint32_t occ, inl;
      double d2;
      reloc_score_point<NOFF>(a.map, R, t, a.sub[i], a.gate2, leaf2, occ, inl, d2);
      cnt[0] += occ;
      cnt[1] += inl;
      if (inl) sum[0] += d2;
    }
  }
  // lanes (all 64 active again here), then waves in wave order
  wave_sum_to_lane63_u32<2>(cnt);
  wave_sum_to_lane63_f64<1>(sum);
  if ((threadIdx.x & 63u) == 63u) {
    RelocPartial w;
    w.n_occupied = static_cast<int32_t>(cnt[0]);
    w.n_inliers = static_cast<int32_t>(cnt[1]);
    w.sum_sq = sum[0];
    s_wave[threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) a.partials[static_cast<size_t>(pose) * a.n_chunks + chunk] = reloc_fold_waves(s_wave, kRelocThreads / 64);
}

__global__ __launch_bounds__(256) void reloc_fold_kernel(const RelocPartial * partials, int n_poses, int n_chunks, int m, RelocScore * scores)
{
  const int pose = blockIdx.x * 256 + threadIdx.x;
  if (pose >= n_poses) return;
  scores[pose] = reloc_fold_chunks(partials + static_cast<size_t>(pose) * n_chunks, n_chunks, m);
}

// One workgroup.  top_k rounds: every lane's best pose behind the last winner, the lanes' answers four at a time, those four at a
// time, then all sixteen.  The winners are kept in LDS; the block in mapped pinned memory is written once at the end, one lane
// per winner (a store across PCIe in front of every round's barrier cost more than the round).
__global__ __launch_bounds__(kRelocSelThreads) void reloc_select_kernel(const RelocScore * scores, int n_poses, int top_k, RelocBest * out)
{
  __shared__ RelocKey s_key[kRelocSelThreads];
  __shared__ RelocKey s_key4[kRelocSelThreads / 4];
  __shared__ RelocKey s_key16[kRelocSelThreads / 16];
  __shared__ RelocKey s_prev;
  __shared__ int32_t s_index[kRelocMaxRefine];
  const int lane = static_cast<int>(threadIdx.x);
  if (lane == 0) s_prev = reloc_no_key();
  if (lane < kRelocMaxRefine) s_index[lane] = -1;
  __syncthreads();
  for (int r = 0; r < top_k && r < kRelocMaxRefine; ++r) {  // (uniform)
    s_key[lane] = reloc_select_lane(scores, n_poses, lane, kRelocSelThreads, s_prev);
    __syncthreads();
    if (lane < kRelocSelThreads / 4) s_key4[lane] = reloc_best_of(s_key + 4 * lane, 4);
    __syncthreads();
    if (lane < kRelocSelThreads / 16) s_key16[lane] = reloc_best_of(s_key4 + 4 * lane, 4);
    __syncthreads();
    if (lane == 0) {
      const RelocKey w = reloc_best_of(s_key16, kRelocSelThreads / 16);
      // behind the last pose (w.index < 0): s_prev stays the last winner, so every later round finds none either
      if (w.index >= 0) {
        s_prev = w;
        s_index[r] = w.index;
      }
    }
    __syncthreads();
  }
  if (lane < kRelocMaxRefine) {
    const int32_t idx = s_index[lane];
    RelocScore sc;
    sc.n_points = sc.n_occupied = sc.n_inliers = sc.reserved = 0;
    sc.sum_sq = 0.0;
    if (idx >= 0) sc = scores[idx];
    out->index[lane] = idx;
    out->score[lane] = sc;
  }
}
}  // namespace

hipError_t launch_reloc_gather(const float4 * src, const uint32_t * perm, int n, int stride, float4 * sub, hipStream_t stream)
{
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(reloc_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, perm, n, stride, sub);
  return hipGetLastError();
}

hipError_t launch_reloc_score(const RelocScoreArgs & a, hipStream_t stream)
{
  const dim3 grid(static_cast<unsigned int>(a.n_poses) * static_cast<unsigned int>(a.n_chunks)), block(kRelocThreads);
  if (a.map.n_off <= 1)
    hipLaunchKernelGGL(reloc_score_kernel<1>, grid, block, 0, stream, a);
  else if (a.map.n_off == 7)
    hipLaunchKernelGGL(reloc_score_kernel<7>, grid, block, 0, stream, a);
  else if (a.map.n_off == 19)
    hipLaunchKernelGGL(reloc_score_kernel<19>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(reloc_score_kernel<27>, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_reloc_fold(const RelocPartial * partials, int n_poses, int n_chunks, int m, RelocScore * scores, hipStream_t stream)
{
  hipLaunchKernelGGL(reloc_fold_kernel, dim3((n_poses + 255) / 256), dim3(256), 0, stream, partials, n_poses, n_chunks, m, scores);
  return hipGetLastError();
}

hipError_t launch_reloc_select(const RelocScore * scores, int n_poses, int top_k, RelocBest * out, hipStream_t stream)
{
  hipLaunchKernelGGL(reloc_select_kernel, dim3(1), dim3(kRelocSelThreads), 0, stream, scores, n_poses, top_k, out);
  return hipGetLastError();
}

}  // namespace mh
