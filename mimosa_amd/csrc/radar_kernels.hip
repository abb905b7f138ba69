// HIP kernels of the radar Doppler path (SURVEY.md component #14): the radar front end and DopplerHessianFactor.
//
// Reference:
//   Manager::preprocess            src/radar/manager.cpp:111-181 (rioPoint remap, NaN / intensity / range / azimuth /
//                                  elevation gates, valid_targets_ in input order)
//   TargetData                     include/mimosa/radar/utils.hpp:17-43
//   DopplerHessianFactor           include/mimosa/radar/factor.hpp:98-188 (linearize)
//
// radar_prepare_kernel (ONE workgroup, 1024 lanes): the cloud is walked in chunks of 1024 records; each lane decodes and
// gates one record, a ballot / popcount scan over the 16 waves gives every kept record its place behind the kept records of
// the earlier chunks: a stable compaction in input order, no atomics.  A radar cloud has a few hundred to a few thousand
// points, one workgroup walks 5 000 of them in five chunks; the bound is the launch and the chunk barriers, not bandwidth.
//
// Float conventions.  The reference is a baseline x86-64 build (no FMA) and every gate is a threshold test on f32 values,
// so this file is compiled with -ffp-contract=off.  range = Vector3f::norm() = sqrt((x*x + y*y) + z*z) in f32: the f32
// square root is taken as sqrt in double rounded once to float, which is exact (53 >= 2 * 24 + 2 bits).  atan2f is taken as
// (float)atan2((double)y, (double)x): that is the correctly rounded f32 result except in double-rounding cases, so it can
// differ from the host libm's atan2f by one ulp, which changes the kept set only for a point within about one ulp of an
// angle threshold.  deg2rad<float>(deg) = (deg * float(M_PI)) / 180.f is computed on the host.
//
// radar_linearize_kernel (one 256-lane workgroup per factor, any number of factors in one launch): each target gives the
// 9-vector j = (J1 rotation, J2, J3 gyroscope) and its whitened, weighted residual; a lane accumulates w^2 j j^T (45 unique
// entries), the gradient (9) and f in fp64 registers over targets lane, lane + 256, ...; the 55 sums are reduced by the fp64
// DPP wave sums (wave_dpp.hpp), then across the four waves in LDS in wave order.  No atomics: the summation order depends on
// the factor's target count alone, so a factor gives the same bits alone, in a batch of any composition and on every repeat.
// 32 bytes read and ~230 fp64 operations per target: a window of 64 factors x 1 000 targets is 2 MB and 15 M flops, far
// under a microsecond of HBM or fp64 rate on the whole chip; with one workgroup per factor the kernel runs on 64 CUs and
// its time is the per-lane dependent chain (4 targets per lane) plus the reduction and the launch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "radar_device.hpp"
#include "wave_dpp.hpp"

namespace mh
{
namespace
{
constexpr int kPrepThreads = 1024;
constexpr int kPrepWaves = kPrepThreads / 64;

__device__ __forceinline__ float load_f32(const unsigned char * rec, uint32_t off)
{
  return *reinterpret_cast<const float *>(rec + off);  // offsets and point_step are multiples of 4 (checked on the host)
}

__device__ __forceinline__ double4 bearing_of(double x, double y, double z, double range, double radial_speed)
{
  // factor.hpp:138-139: Point3(t.x, t.y, t.z) / t.range, doppler = t.radial_speed
  return make_double4(x / range, y / range, z / range, radial_speed);
}

__global__ __launch_bounds__(kPrepThreads) void radar_prepare_kernel(const unsigned char * raw, uint32_t n, const RadarFilter f,
                                                                    mh_radar_target * targets, double4 * bd, uint32_t * count)
{
  __shared__ uint32_t wave_counts[kPrepWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t base = 0;  // kept records of the earlier chunks
  for (uint32_t start = 0; start < n; start += kPrepThreads) {
    const uint32_t i = start + threadIdx.x;
    bool keep = false;
    float x = 0.f, y = 0.f, z = 0.f, intensity = 0.f, velocity = 0.f, range = 0.f, azimuth = 0.f, elevation = 0.f;
    if (i < n) {
      const unsigned char * rec = raw + static_cast<size_t>(i) * f.point_step;
      const float rx = load_f32(rec, f.off_x), ry = load_f32(rec, f.off_y);
      z = load_f32(rec, f.off_z);
      intensity = load_f32(rec, f.off_intensity);  // rioPoint: snr_db (noise_db is not read)
      velocity = load_f32(rec, f.off_velocity);    // rioPoint: v_doppler_mps
      x = f.rio ? ry : rx;                          // manager.cpp:126-134
      y = f.rio ? -rx : ry;
      keep = !(isnan(x) || isnan(y) || isnan(z) || isnan(intensity) || isnan(velocity));  // :146-151
      keep = keep && !(intensity < f.filter_min_db);                                     // :153-155
      range = static_cast<float>(sqrt(static_cast<double>(x * x + y * y + z * z)));     // :158 getVector3fMap().norm()
      keep = keep && !(range < f.range_min || range > f.range_max);                      // :159-161
      azimuth = static_cast<float>(atan2(static_cast<double>(y), static_cast<double>(x)));  // :163 atan2(float, float)
      keep = keep && !(fabsf(azimuth) > f.thr_azimuth);                                  // :164-166
      const float rxy = static_cast<float>(sqrt(static_cast<double>(x * x + y * y)));
      elevation = static_cast<float>(atan2(static_cast<double>(z), static_cast<double>(rxy)));  // :168
      keep = keep && !(fabsf(elevation) > f.thr_elevation);                              // :169-171
    }
    const uint64_t ballot = __ballot(keep);
    const uint32_t below = static_cast<uint32_t>(__popcll(ballot & ((lane ? (~0ull >> (64 - lane)) : 0ull))));
    if (lane == 0) wave_counts[wave] = static_cast<uint32_t>(__popcll(ballot));
    __syncthreads();
    uint32_t before = base, total = base;
    for (uint32_t w = 0; w < static_cast<uint32_t>(kPrepWaves); ++w) {
      if (w < wave) before += wave_counts[w];
      total += wave_counts[w];
    }
    if (keep) {
      const uint32_t o = before + below;
      mh_radar_target t;  // :173-174 emplace_back(x, y, z, range, azimuth, elevation, velocity, intensity)
      t.x = x;
      t.y = y;
      t.z = z;
      t.range = range;
      t.azimuth = azimuth;
      t.elevation = elevation;
      t.radial_speed = velocity;
      t.intensity = intensity;
      targets[o] = t;
      bd[o] = bearing_of(t.x, t.y, t.z, t.range, t.radial_speed);
    }
    base = total;
    __syncthreads();  // wave_counts is rewritten by the next chunk
  }
  if (threadIdx.x == 0) *count = base;
}

__global__ __launch_bounds__(256) void radar_bearing_kernel(const mh_radar_target * targets, uint32_t n, double4 * bd)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const mh_radar_target t = targets[i];
  bd[i] = bearing_of(t.x, t.y, t.z, t.range, t.radial_speed);
}

// factor.hpp:137-178 for one target: j = (J1[0:3], J2, J3[3:6]) before whitening, e the raw residual
__device__ __forceinline__ void target_terms(const RadarLinArgs & a, const double4 & t, double (&j)[9], double & e)
{
  e = -(t.x * a.vR[0] + t.y * a.vR[1] + t.z * a.vR[2]) - t.w;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    j[c] = -(t.x * a.A1[c] + t.y * a.A1[3 + c] + t.z * a.A1[6 + c]);
    j[3 + c] = -(t.x * a.A2[c] + t.y * a.A2[3 + c] + t.z * a.A2[6 + c]);
    j[6 + c] = -(t.x * a.A3[c] + t.y * a.A3[3 + c] + t.z * a.A3[6 + c]);
  }
}
// :157-163 whitening by noise_sigma, then the robust weight sqrt(1 / (1 + (e_w / 2.3849)^2))
__device__ __forceinline__ double robust_weight(double e_whitened)
{
  const double q = e_whitened / 2.3849;
  return sqrt(1.0 / (1.0 + q * q));
}

__global__ __launch_bounds__(kRadarThreads) void radar_linearize_kernel(const RadarLinArgs * args, double * out)
{
  __shared__ double part[kRadarThreads / 64][kRadarSums];
  const RadarLinArgs & a = args[blockIdx.x];
  const uint32_t n = a.n;
  const double4 * tg = a.targets;
  double acc[kRadarSums];
#pragma unroll
  for (int k = 0; k < kRadarSums; ++k) acc[k] = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += kRadarThreads) {
    double j[9], e;
    target_terms(a, tg[i], j, e);
    const double ew = e * a.inv_sigma;
    const double w = robust_weight(ew);
    const double s = a.inv_sigma * w;
    double jw[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) jw[k] = j[k] * s;
    const double eww = ew * w;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c) acc[k++] += jw[r] * jw[c];  // :179-184 G_rc += J_r^T J_c
#pragma unroll
    for (int r = 0; r < 9; ++r) acc[45 + r] -= jw[r] * eww;  // :185-187 g_i += -J_i^T e
    acc[54] += eww * eww;                                   // :188 f += e^2
  }
  // fixed-order reduction: DPP wave sums (five chunks of 11 to bound the registers), then the waves in order
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c0 = 0; c0 < kRadarSums; c0 += 11) {
    double v[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) v[k] = acc[c0 + k];
    wave_sum_to_lane63_f64<11>(v);
    if (lane == 63)
#pragma unroll
      for (int k = 0; k < 11; ++k) part[wave][c0 + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < kRadarSums) {
    double s = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRadarThreads / 64; ++w) s += part[w][threadIdx.x];
    out[static_cast<size_t>(blockIdx.x) * kRadarOutStride + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(256) void radar_residuals_kernel(const RadarLinArgs * args, double * e_whitened, double * weight)
{
  const RadarLinArgs & a = args[0];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double j[9], e;
  target_terms(a, a.targets[i], j, e);
  const double ew = e * a.inv_sigma;
  e_whitened[i] = ew;
  weight[i] = robust_weight(ew);
}
}  // namespace

hipError_t launch_radar_prepare(const void * raw, uint32_t n, const RadarFilter & f, mh_radar_target * targets, double4 * bd,
                                uint32_t * count, hipStream_t stream)
{
  radar_prepare_kernel<<<1, kPrepThreads, 0, stream>>>(static_cast<const unsigned char *>(raw), n, f, targets, bd, count);
  return hipGetLastError();
}

hipError_t launch_radar_bearing(const mh_radar_target * targets, uint32_t n, double4 * bd, hipStream_t stream)
{
  if (n == 0) return hipSuccess;
  radar_bearing_kernel<<<(n + 255) / 256, 256, 0, stream>>>(targets, n, bd);
  return hipGetLastError();
}

hipError_t launch_radar_linearize(const RadarLinArgs * args, uint32_t n_factors, double * out, hipStream_t stream)
{
  if (n_factors == 0) return hipSuccess;
  radar_linearize_kernel<<<n_factors, kRadarThreads, 0, stream>>>(args, out);
  return hipGetLastError();
}

hipError_t launch_radar_residuals(const RadarLinArgs * args, uint32_t n, double * e_whitened, double * weight, hipStream_t stream)
{
  if (n == 0) return hipSuccess;
  radar_residuals_kernel<<<(n + 255) / 256, 256, 0, stream>>>(args, e_whitened, weight);
  return hipGetLastError();
}
}  // namespace mh
