// HIP kernels of map carving (mh_map_carve*, include/mimosa_hip.h): the observation image of a scan on a cube-map direction
// grid, the seen-through test of every map point against it with the in-bucket compaction of the survivors, and the totals.
// The rule itself is carve_device.hpp; voxels a carve empties are erased by the LRU purge's compaction (map_api.hip).
// Compiled with -ffp-contract=off: every decision is a threshold test on products the restatement (tests/map_carve_ref.py)
// evaluates without FMA.
#include <hip/hip_runtime.h>

#include "carve_device.hpp"
#include "map_device.hpp"

namespace mh
{
namespace
{
constexpr int kT = 256;

// the image to "not hit", the call's observation counter to zero
__global__ __launch_bounds__(kT) void carve_clear_kernel(unsigned long long * img, uint32_t cells, unsigned long long * n_obs_used)
{
  for (uint32_t c = blockIdx.x * kT + threadIdx.x; c < cells; c += gridDim.x * kT) img[c] = kCarveNotHit;
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_obs_used = 0ull;
}

// r2 >= 0 and finite-or-infinite: its bit pattern orders as its value, so an unsigned 64-bit atomic minimum is the minimum
__global__ __launch_bounds__(kT) void carve_splat_kernel(const float * __restrict__ src, uint32_t n, uint32_t stride, const CarveParams P,
                                                          unsigned long long * img, unsigned long long * n_obs_used)
{
  uint32_t used = 0;
  for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
    const float * p = src + static_cast<size_t>(i) * stride;
    double r2;
    const int cell = carve_observe(P, p[0], p[1], p[2], r2);
    if (cell < 0) continue;
    atomicMin(&img[cell], static_cast<unsigned long long>(__double_as_longlong(r2)));
    ++used;
  }
  // one atomic per wave, not per thread
#pragma unroll
  for (int mk = 32; mk >= 1; mk >>= 1) used += __shfl_xor(used, mk, 64);
  if ((threadIdx.x & 63u) == 0u && used) atomicAdd(n_obs_used, static_cast<unsigned long long>(used));
}

// One wave per voxel, lane j holds the j-th point of the bucket (map_insert_points_kernel's layout).  per_voxel[v] = removed |
// tested << 8 | emptied << 16; keep[v] = the voxel is not emptied.  APPLY: the survivors move to the front in order (every lane has read its
// point before any lane writes), lane 0 writes the count, lanes 0 .. 7 the cell words.  !APPLY stores nothing of the map.
template <bool APPLY>
__global__ __launch_bounds__(kT) void carve_test_kernel(const MapArrays m, uint32_t n_voxels, const CarveParams P, const double * __restrict__ img,
                                                         double leaf, double sx, double sy, double sz, double skip_dist2, uint32_t * per_voxel,
                                                         uint32_t * keep)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * kT + threadIdx.x) >> 6, n_waves = (gridDim.x * kT) >> 6;
  for (uint32_t v = wave; v < n_voxels; v += n_waves) {
    const int4 vx = m.vox[v];
    const uint32_t count = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(vx.w));
    // wave-uniform early-out: no point of a voxel whose centre is farther than range_max + half the voxel diagonal (+ 1e-6 of
    // that for the roundings of this test itself) from the sensor can pass the range_max gate
    const double cx = (static_cast<double>(vx.x) + 0.5) * leaf - sx, cy = (static_cast<double>(vx.y) + 0.5) * leaf - sy,
                 cz = (static_cast<double>(vx.z) + 0.5) * leaf - sz;
    if ((cx * cx + cy * cy) + cz * cz > skip_dist2) {
      if (lane == 0) {
        per_voxel[v] = 0u;
        keep[v] = 1u;
      }
      continue;
    }
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t qb = 0u;
    int decision = kCarveUntested;
    if (lane < count) {
      b = m.buckets[static_cast<size_t>(v) * kBucketStride + lane];
      if (APPLY) qb = m.qbuckets[static_cast<size_t>(v) * kBucketStride + lane];
      decision = carve_decide(P, img, b.x, b.y, b.z);
    }
    const uint64_t gone = __ballot(decision == kCarveSeenThrough);
    const uint64_t tested = __ballot(decision != kCarveUntested);
    const uint64_t stay = __ballot(lane < count && decision != kCarveSeenThrough);
    const uint32_t n_gone = static_cast<uint32_t>(__popcll(gone)), n_stay = static_cast<uint32_t>(__popcll(stay));
    if (lane == 0) {
      per_voxel[v] = n_gone | (static_cast<uint32_t>(__popcll(tested)) << 8) | ((n_gone != 0u && n_stay == 0u) ? (1u << 16) : 0u);
      keep[v] = (n_gone != 0u && n_stay == 0u) ? 0u : 1u;
    }
    if (!APPLY || n_gone == 0u) continue;
    if ((stay >> lane) & 1ull) {
      const uint32_t slot = static_cast<uint32_t>(__popcll(stay & ((1ull << lane) - 1ull)));
      if (slot != lane) {
        m.buckets[static_cast<size_t>(v) * kBucketStride + slot] = b;
        m.qbuckets[static_cast<size_t>(v) * kBucketStride + slot] = qb;
      }
    }
    if (lane == 0) m.vox[v] = make_int4(vx.x, vx.y, vx.z, static_cast<int>(n_stay));
    if (n_stay != 0u && lane < 8u) {  // an emptied voxel is erased with its words by the compaction that follows
      int bx, by, bz;
      if (voxel_block(vx.x, vx.y, vx.z, static_cast<int>(lane), bx, by, bz)) {
        const int blk = find_block(m, bx, by, bz);
        if (blk >= 0)
          m.cells[static_cast<size_t>(blk) * kCellsPerBlock + halo_index(vx.x - bx * kBlockDim, vx.y - by * kBlockDim, vx.z - bz * kBlockDim)] =
            (v << 5) | n_stay;
      }
    }
  }
}

// One workgroup: the six counters into the state block; APPLY takes the removed points off n_points.
__global__ __launch_bounds__(1024) void carve_totals_kernel(MapState * st, const uint32_t * per_voxel, uint32_t n_voxels, const double * img, uint32_t cells,
                                                            const unsigned long long * n_obs_used, int apply)
{
  __shared__ unsigned long long s_w[5][16];
  unsigned long long t[5] = {0ull, 0ull, 0ull, 0ull, 0ull};  // cells hit, tested, removed, touched, emptied
  for (uint32_t c = threadIdx.x; c < cells; c += 1024u) t[0] += img[c] < HUGE_VAL ? 1ull : 0ull;
  for (uint32_t v = threadIdx.x; v < n_voxels; v += 1024u) {
    const uint32_t w = per_voxel[v];
    const uint32_t gone = w & 0xFFu;
    t[1] += (w >> 8) & 0xFFu;
    t[2] += gone;
    t[3] += gone ? 1ull : 0ull;
    t[4] += (w >> 16) & 1u;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) t[k] += __shfl_xor(t[k], mk, 64);
    if ((threadIdx.x & 63u) == 0u) s_w[k][threadIdx.x >> 6] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    unsigned long long tot = 0;
    for (int w = 0; w < 16; ++w) tot += s_w[threadIdx.x][w];
    st->carve[1 + threadIdx.x] = tot;
    if (threadIdx.x == 2 && apply) st->n_points -= tot;
  }
  if (threadIdx.x == 5) st->carve[0] = *n_obs_used;
}
}  // namespace

size_t carve_image_bytes(int N) { return (static_cast<size_t>(6) * N * N + 1) * sizeof(unsigned long long); }

hipError_t launch_carve_image(const float * src, uint32_t n, uint32_t stride_floats, const CarveParams & P, void * image, hipStream_t stream)
{
  const uint32_t cells = 6u * static_cast<uint32_t>(P.N) * static_cast<uint32_t>(P.N);
  unsigned long long * img = static_cast<unsigned long long *>(image);
  hipLaunchKernelGGL(carve_clear_kernel, dim3((cells + kT - 1) / kT), dim3(kT), 0, stream, img, cells, img + cells);
  if (n) hipLaunchKernelGGL(carve_splat_kernel, dim3(max(1u, min((n + kT - 1) / kT, 8192u))), dim3(kT), 0, stream, src, n, stride_floats, P, img, img + cells);
  return hipGetLastError();
}

hipError_t launch_carve_test(const MapArrays & m, uint32_t n_voxels, const CarveParams & P, const void * image, double leaf, const double sensor_W[3],
                             double range_max, bool apply, uint32_t * per_voxel, uint32_t * keep, hipStream_t stream)
{
  const uint32_t cells = 6u * static_cast<uint32_t>(P.N) * static_cast<uint32_t>(P.N);
  const double * img = static_cast<const double *>(image);
  const double bound = (range_max + 0.5 * std::sqrt(3.0) * leaf) * (1.0 + 1e-6);
  if (n_voxels) {
    const int grid = static_cast<int>(std::min<size_t>((static_cast<size_t>(n_voxels) * 64 + kT - 1) / kT, 16384));
    if (apply)
      hipLaunchKernelGGL(carve_test_kernel<true>, dim3(grid), dim3(kT), 0, stream, m, n_voxels, P, img, leaf, sensor_W[0], sensor_W[1], sensor_W[2],
                         bound * bound, per_voxel, keep);
    else
      hipLaunchKernelGGL(carve_test_kernel<false>, dim3(grid), dim3(kT), 0, stream, m, n_voxels, P, img, leaf, sensor_W[0], sensor_W[1], sensor_W[2],
                         bound * bound, per_voxel, keep);
  }
  hipLaunchKernelGGL(carve_totals_kernel, dim3(1), dim3(1024), 0, stream, m.state, per_voxel, n_voxels, img, cells,
                     static_cast<const unsigned long long *>(image) + cells, apply ? 1 : 0);
  return hipGetLastError();
}

}  // namespace mh
