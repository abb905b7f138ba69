// Place recognition (mh_place_*): the ring x sector height image of a cloud, its column norms, the distance of a query image
// to every entry of a keyframe database over every column shift, and the top_k entries (the arithmetic: place_device.hpp).
// Compiled without floating-point contraction.
//
// describe: a workgroup folds kPlaceChunk points into a 1 200-cell image in LDS with an unsigned maximum on the float bits (the
// values are >= 0, so the bits order like the values), then merges its occupied cells into the global image with one vector
// atomic each.  The global image is cleared by a fill in front of the kernel.  A maximum does not depend on the order of its
// operands, so the image has the same bits whatever the launch shape.
//
// query: one entry per wave, four per workgroup.  The query image and its norms are staged in LDS once per workgroup, an entry's
// image and norms once per wave; lane s < 60 computes d(s) — 60 columns, each a 20-term dot product, in the order the header
// states — so at every step the wave reads ONE query word (a broadcast) and 60 consecutive entry words (no bank conflict).
// Lane 0 then takes the minimum over the shifts in shift order.  Nothing is summed across lanes, waves or workgroups: an
// entry's {D, shift} has the same bits alone, at any database size, at any position and on every repeat.
//
// select: one workgroup, top_k rounds, as reloc_select_kernel.
#include <hip/hip_runtime.h>

#include "place_device.hpp"

namespace mh
{
namespace
{
__global__ __launch_bounds__(kPlaceThreads) void place_describe_kernel(const float * src, uint32_t n, uint32_t stride, const PlaceParams P,
                                                                        unsigned int * desc)
{
  __shared__ unsigned int s_img[kPlaceCells];
  for (int c = static_cast<int>(threadIdx.x); c < kPlaceCells; c += kPlaceThreads) s_img[c] = 0u;
  __syncthreads();
  const uint32_t base = blockIdx.x * static_cast<uint32_t>(kPlaceChunk);
  for (int r = 0; r < kPlaceChunk / kPlaceThreads; ++r) {
    const uint32_t i = base + static_cast<uint32_t>(r) * kPlaceThreads + threadIdx.x;
    if (i < n) {
      const float * p = src + static_cast<size_t>(i) * stride;
      float value;
      const int cell = place_cell(P, p[0], p[1], p[2], value);
      if (cell >= 0) atomicMax(&s_img[cell], __float_as_uint(value));
    }
  }
  __syncthreads();
  for (int c = static_cast<int>(threadIdx.x); c < kPlaceCells; c += kPlaceThreads) {
    const unsigned int v = s_img[c];
    if (v != 0u) atomicMax(&desc[c], v);
  }
}

__global__ __launch_bounds__(64) void place_norms_kernel(const float * desc, double * norms)
{
  const int j = static_cast<int>(threadIdx.x);
  if (j < kPlaceSectors) norms[j] = place_column_norm(desc, j);
}

constexpr int kPlaceWaves = kPlaceThreads / 64;

__global__ __launch_bounds__(kPlaceThreads) void place_query_kernel(const float * q_desc, const double * q_norms, const float * db_desc,
                                                                     const double * db_norms, int n_entries, int min_overlap, PlaceScore * scores)
{
  __shared__ float s_q[kPlaceCells];
  __shared__ double s_qn[kPlaceSectors];
  __shared__ float s_c[kPlaceWaves][kPlaceCells];
  __shared__ double s_cn[kPlaceWaves][kPlaceSectors];
  __shared__ double s_d[kPlaceWaves][64];
  const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63;
  for (int c = tid; c < kPlaceCells; c += kPlaceThreads) s_q[c] = q_desc[c];
  if (tid < kPlaceSectors) s_qn[tid] = q_norms[tid];
  // (every wave of the workgroup makes the same number of trips: the barriers are uniform)
  for (int first = static_cast<int>(blockIdx.x) * kPlaceWaves; first < n_entries; first += static_cast<int>(gridDim.x) * kPlaceWaves) {
    const int e = first + wave;
    const bool live = e < n_entries;
    __syncthreads();  // the last trip's reads of s_c / s_d are over (first trip: nothing to wait for but the query's stores)
    if (live) {
      const float * X = db_desc + static_cast<size_t>(e) * kPlaceCells;
      for (int c = lane; c < kPlaceCells; c += 64) s_c[wave][c] = X[c];
      if (lane < kPlaceSectors) s_cn[wave][lane] = db_norms[static_cast<size_t>(e) * kPlaceSectors + lane];
    }
    __syncthreads();
    if (live && lane < kPlaceSectors) s_d[wave][lane] = place_shift_distance(s_q, s_qn, s_c[wave], s_cn[wave], lane, min_overlap);
    __syncthreads();
    if (live && lane == 0) scores[e] = place_best_shift(s_d[wave]);
  }
}

__global__ __launch_bounds__(kPlaceThreads) void place_select_kernel(const PlaceScore * scores, int n_entries, int top_k, PlaceBest * out)
{
  __shared__ PlaceKey s_key[kPlaceThreads];
  __shared__ PlaceKey s_key16[kPlaceThreads / 16];
  __shared__ PlaceKey s_prev;
  __shared__ PlaceKey s_hit[kPlaceMaxHits];
  const int lane = static_cast<int>(threadIdx.x);
  if (lane == 0) s_prev = place_no_key();
  if (lane < kPlaceMaxHits) s_hit[lane] = place_no_key();
  __syncthreads();
  for (int r = 0; r < top_k && r < kPlaceMaxHits; ++r) {  // (uniform)
    s_key[lane] = place_select_lane(scores, n_entries, lane, kPlaceThreads, s_prev);
    __syncthreads();
    if (lane < kPlaceThreads / 16) s_key16[lane] = place_best_of(s_key + 16 * lane, 16);
    __syncthreads();
    if (lane == 0) {
      const PlaceKey w = place_best_of(s_key16, kPlaceThreads / 16);
      // behind the last hit (w.index < 0): s_prev stays the last winner, so every later round finds none either
      if (w.index >= 0) {
        s_prev = w;
        s_hit[r] = w;
      }
    }
    __syncthreads();
  }
  if (lane < kPlaceMaxHits) {
    const PlaceKey h = s_hit[lane];
    out->index[lane] = h.index;
    out->shift[lane] = h.index >= 0 ? h.shift : 0;
    out->dist[lane] = h.dist;
  }
}
}  // namespace

hipError_t launch_place_describe(const float * src, uint32_t n, uint32_t stride, const PlaceParams & P, float * desc, hipStream_t stream)
{
  hipError_t e = hipMemsetAsync(desc, 0, kPlaceCells * sizeof(float), stream);
  if (e != hipSuccess || n == 0) return e;
  const uint32_t grid = (n + kPlaceChunk - 1) / kPlaceChunk;
  hipLaunchKernelGGL(place_describe_kernel, dim3(grid), dim3(kPlaceThreads), 0, stream, src, n, stride, P, reinterpret_cast<unsigned int *>(desc));
  return hipGetLastError();
}

hipError_t launch_place_norms(const float * desc, double * norms, hipStream_t stream)
{
  hipLaunchKernelGGL(place_norms_kernel, dim3(1), dim3(64), 0, stream, desc, norms);
  return hipGetLastError();
}

hipError_t launch_place_query(const float * q_desc, const double * q_norms, const float * db_desc, const double * db_norms, int n_entries, int min_overlap,
                              PlaceScore * scores, hipStream_t stream)
{
  int grid = (n_entries + kPlaceWaves - 1) / kPlaceWaves;
  grid = grid < kPlaceQueryMaxGrid ? grid : kPlaceQueryMaxGrid;
  hipLaunchKernelGGL(place_query_kernel, dim3(grid), dim3(kPlaceThreads), 0, stream, q_desc, q_norms, db_desc, db_norms, n_entries, min_overlap, scores);
  return hipGetLastError();
}

hipError_t launch_place_select(const PlaceScore * scores, int n_entries, int top_k, PlaceBest * out, hipStream_t stream)
{
  hipLaunchKernelGGL(place_select_kernel, dim3(1), dim3(kPlaceThreads), 0, stream, scores, n_entries, top_k, out);
  return hipGetLastError();
}

}  // namespace mh
