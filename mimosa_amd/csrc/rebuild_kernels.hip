// HIP kernels of mh_map_rebuild_from_keyframes and of the keyframe cloud store (mh_keyframes_*): a chunk of keyframes — their clouds
// laid end to end, each under its own pose — as ONE insert of the device-resident voxel map (map_kernels.hip).
//
// The insert's rule couples only the points of one voxel, in input order, and numbers voxels in first-seen order, so the insert of
// the concatenation builds the buckets and voxel ids of one insert per keyframe.  What the concatenation loses is which INSERT
// touched a voxel last — the LRU stamp; map_rebuild_stamp_kernel puts it back from the largest point index of every segment.
//   map_rebuild_assign_kernel   phase A.1 of the chunk: point -> its keyframe (binary search over the chunk's prefix offsets, bounded
//                               by the workgroup's first and last point) -> arena load -> that keyframe's f32 pose
//                               (map_world_point, the expression map_assign_kernel uses) -> pts, key, bad_coord, vg::voxel_assign
//   phases A.2 to C             the insert's own launches (launch_map_insert_group, launch_map_create_voxels,
//                               launch_map_insert_points), untouched
//   map_rebuild_stamp_kernel    one wave per segment: max of its point indices (shuffle reduction, no atomics) -> keyframe ordinal j
//                               -> lru[voxel] = counter at chunk start + j.  A voxel is stamped by every insert one of whose points
//                               fell into it, kept or not: map_insert_points_kernel's rule.
// Compiled with -ffp-contract=off, like map_kernels.hip: the transform feeds voxel assignment.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "map_device.hpp"
#include "voxel_group.hpp"

namespace mh
{
namespace
{
constexpr int kT = 256;

// the keyframe of point i: the largest j in [lo, hi) with rel[j] <= i.  rel[lo] <= i, and rel[j] > i for every j >= hi.  Keyframes of
// 0 points repeat an offset; the largest j is the one that holds the point.
__device__ __forceinline__ uint32_t keyframe_of(const uint32_t * __restrict__ rel, uint32_t lo, uint32_t hi, uint32_t i)
{
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (rel[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kT) void map_rebuild_assign_kernel(const float4 * __restrict__ arena, const RebuildKeyframe * __restrict__ kf,
                                                                 const uint32_t * __restrict__ rel, uint32_t kc, uint32_t n, double inv_leaf,
                                                                 float4 * pts, VoxelHash h, uint32_t * slot_of, MapState * st)
{
  __shared__ uint32_t s_j[2];  // the keyframes of the workgroup's first and last point: every point's search runs between them
  const uint32_t i0 = blockIdx.x * kT, i = i0 + threadIdx.x;
  if (threadIdx.x < 2u) s_j[threadIdx.x] = keyframe_of(rel, 0u, kc, threadIdx.x == 0u ? i0 : min(i0 + kT - 1u, n - 1u));
  __syncthreads();
  const bool valid = i < n;
  uint64_t key = vg::kEmpty64;
  if (valid) {
    const uint32_t j = keyframe_of(rel, s_j[0], s_j[1] + 1u, i);
    const RebuildKeyframe & k = kf[j];
    const float4 p = arena[k.src + (i - rel[j])];
    float x, y, z;
    map_world_point(k.Rt12, p.x, p.y, p.z, x, y, z);
    pts[i] = make_float4(x, y, z, 1.0f);
    key = map_point_key(x, y, z, inv_leaf, st);
  }
  const uint32_t slot = vg::voxel_assign(h, valid, key, i);
  if (valid) slot_of[i] = slot;
}

__global__ __launch_bounds__(kT) void map_rebuild_stamp_kernel(const MapArrays m, const uint32_t * __restrict__ idx_unsorted, const uint2 * __restrict__ seg,
                                                                const uint32_t * __restrict__ seg_vid, const uint32_t * __restrict__ rel, uint32_t kc,
                                                                unsigned long long counter_start)
{
  const uint32_t ns = m.state->n_segments;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * kT + threadIdx.x) >> 6, n_waves = (gridDim.x * kT) >> 6;
  for (uint32_t s = wave; s < ns; s += n_waves) {
    const uint2 sg = seg[s];
    const uint32_t s0 = __builtin_amdgcn_readfirstlane(sg.x), s1 = s0 + __builtin_amdgcn_readfirstlane(sg.y);
    uint32_t last = 0u;  // a segment holds at least one point
    for (uint32_t p = s0 + lane; p < s1; p += 64u) last = max(last, idx_unsorted[p]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) last = max(last, static_cast<uint32_t>(__shfl_xor(static_cast<int>(last), d)));
    if (lane == 0u) m.lru[seg_vid[s]] = counter_start + keyframe_of(rel, 0u, kc, last);
  }
}

__global__ __launch_bounds__(kT) void keyframes_pack_kernel(const float * __restrict__ src, uint32_t n, uint32_t stride, float4 * __restrict__ dst,
                                                             unsigned long long * offsets, unsigned long long end)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) offsets[1] = end;
  for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
    const float * p = src + static_cast<size_t>(i) * stride;
    dst[i] = make_float4(p[0], p[1], p[2], 1.0f);
  }
}
}  // namespace

hipError_t launch_map_rebuild_assign(const MapArrays & m, const float4 * arena, const RebuildKeyframe * kf, const uint32_t * rel, uint32_t kc,
                                     uint32_t n, double inv_leaf, const InsertScratch & s, hipStream_t stream)
{
  if (!n || !kc) return hipErrorInvalidValue;
  const vg::Layout L = vg::layout(n);
  const vg::Buffers B = vg::carve(s.group, n);
  const hipError_t e = hipMemsetAsync(s.group, 0xFF, L.clear_bytes, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(map_rebuild_assign_kernel, dim3((n + kT - 1) / kT), dim3(kT), 0, stream, arena, kf, rel, kc, n, inv_leaf, s.pts, B.h, B.slot_of,
                     m.state);
  return hipGetLastError();
}

hipError_t launch_map_rebuild_stamp(const MapArrays & m, const uint32_t * rel, uint32_t kc, uint32_t n, unsigned long long counter_start,
                                    const InsertScratch & s, hipStream_t stream)
{
  if (!n || !kc) return hipErrorInvalidValue;
  const vg::Buffers B = vg::carve(s.group, n);
  const size_t grid = std::min<size_t>((static_cast<size_t>(n) * 64 + kT - 1) / kT, 16384);  // <= one wave per point, as phase C
  hipLaunchKernelGGL(map_rebuild_stamp_kernel, dim3(static_cast<uint32_t>(grid)), dim3(kT), 0, stream, m, B.idx_unsorted, B.seg, s.seg_vid, rel, kc,
                     counter_start);
  return hipGetLastError();
}

hipError_t launch_keyframes_pack(const float * src, uint32_t n, uint32_t stride_floats, float4 * dst, unsigned long long * offsets,
                                 unsigned long long end, hipStream_t stream)
{
  const uint32_t grid = std::max(1u, std::min((n + kT - 1) / kT, 8192u));
  hipLaunchKernelGGL(keyframes_pack_kernel, dim3(grid), dim3(kT), 0, stream, src, n, stride_floats, dst, offsets, end);
  return hipGetLastError();
}

}  // namespace mh
