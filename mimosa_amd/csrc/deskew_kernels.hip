// HIP kernels for the f32 rigid transforms of the scan (kernels K1 / K2 of SURVEY.md §2.3), and K0: the fp64 per-timestamp pose
// table K1 reads, from the IMU intervals (Manager::deskewPoints' pose part, src/lidar/manager.cpp:455-499; mh_scan_deskew_imu).
//
// Reference: Manager::deskewPoints hot loop src/lidar/manager.cpp:496-509 (per-timestamp-group
// pose, p <- R p + t in float), Geometric::preprocess body transform src/lidar/geometric.cpp:154-161,
// Geometric::updateMap world transform src/lidar/geometric.cpp:483-490.
//
// The reference is built for baseline x86-64 (no FMA) and Eigen evaluates the 3x3 * 3x1 float
// product coefficient-wise as r0*x + (r1*y + r2*z), then adds t.  This file is compiled with
// -ffp-contract=off so the results are bit-identical: a 1-ulp difference is harmless for the ICP
// residual but can move a point across a voxel boundary in the down-sampler / map insert.
// Pure streaming work: 32 B in, 12 B (xyz) out per point; the timestamp -> group lookup is a binary search over the
// <= 4096 distinct timestamps staged in LDS (16 KiB); the group's pose (48 B) comes through L1 / L2 (staging the whole
// pose table per block cost more than it saved: 48 KiB x 512 blocks of extra reads for a 4 MiB cloud).
#include <hip/hip_runtime.h>

#include "icp_device.hpp"
#include "scan_device.hpp"

namespace mh
{
namespace
{
constexpr int kThreads = 256;
constexpr int kMaxGroupsLds = 4096;

__device__ __forceinline__ void xform(const float * P, float & x, float & y, float & z)
{
  const float px = x, py = y, pz = z;
  x = (P[0] * px + (P[1] * py + P[2] * pz)) + P[9];
  y = (P[3] * px + (P[4] * py + P[5] * pz)) + P[10];
  z = (P[6] * px + (P[7] * py + P[8] * pz)) + P[11];
}

// One thread per point.  A point record is two float4: {x,y,z,pad} {intensity,t,idx,range}.
__global__ __launch_bounds__(kThreads) void deskew_kernel(float4 * pts, int n, const uint32_t * unique_ns,
                                                           const float * Rt12, int n_groups, const float * body,
                                                           int use_lds)
{
  __shared__ uint32_t s_ns[kMaxGroupsLds];
  __shared__ float s_body[12];
  if (use_lds)
    for (int i = threadIdx.x; i < n_groups; i += kThreads) s_ns[i] = unique_ns[i];
  if (body && threadIdx.x < 12) s_body[threadIdx.x] = body[threadIdx.x];
  __syncthreads();
  const uint32_t * ns = use_lds ? s_ns : unique_ns;
  const float * poses = Rt12;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    float4 a = pts[2 * i];
    const float4 b = pts[2 * i + 1];
    const uint32_t t = __float_as_uint(b.y);
    // lower_bound(unique_ns, t)
    int lo = 0, hi = n_groups;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ns[mid] < t)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < n_groups && ns[lo] == t) xform(poses + 12 * lo, a.x, a.y, a.z);
    if (body) xform(s_body, a.x, a.y, a.z);
    pts[2 * i] = a;
  }
}

__global__ __launch_bounds__(kThreads) void transform_kernel(float4 * pts, int n, const float * Rt12)
{
  __shared__ float s_p[12];
  if (threadIdx.x < 12) s_p[threadIdx.x] = Rt12[threadIdx.x];
  __syncthreads();
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    float4 a = pts[2 * i];
    xform(s_p, a.x, a.y, a.z);
    pts[2 * i] = a;
  }
}

// mh_point32[n] -> float4 xyz[n] (the 16-byte-per-point source layout the ICP kernel reads)
__global__ __launch_bounds__(kThreads) void pack_xyz_kernel(const float4 * pts, int n, float4 * xyz)
{
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) xyz[i] = pts[2 * i];
}

int grid_for(int n) { return max(1, min((n + kThreads - 1) / kThreads, 2048)); }
// Device-to-device copy of 16-byte words as a kernel: stream-ordered like any launch.  (hipMemcpyAsync device-to-device goes
// through the runtime's copy path; in the pipelined replay — a second thread uploading 4 MiB on a copy stream at the same time —
// that call was seen to BLOCK the calling thread for 0.4 ms in about a third of the processes.)
__global__ __launch_bounds__(256) void copy16_kernel(const uint4 * __restrict__ src, uint4 * __restrict__ dst, size_t n16)
{
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}

// ---- K0: the per-timestamp pose table (Manager::deskewPoints' pose part, lidar/manager.cpp:455-499) ---------------------------
// One lane per distinct timestamp, fp64, in the reference's operation order (no FMA: this file is built with -ffp-contract=off).
// A latency-bound launch of a few waves (1024 timestamps = 4 workgroups): what matters is that it needs no host round trip.
constexpr int kPoseThreads = 256;

__device__ __forceinline__ void mat3_mul(const double * a, const double * b, double * c)
{
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ __forceinline__ void mat3_vec(const double * a, const double * v, double * o)
{
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}
// gtsam::Rot3::Expmap (Rodrigues) with the small-angle branch of the host mirror's so3Expmap
__device__ __forceinline__ void so3_expmap(const double wx, const double wy, const double wz, double * R)
{
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double A, B;
  if (th < 1e-10) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
  } else {
    A = sin(th) / th;
    B = (1.0 - cos(th)) / th2;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double kk = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) kk += K[3 * i + m] * K[3 * m + j];
      R[3 * i + j] = (i == j ? 1.0 : 0.0) + (A * K[3 * i + j] + B * kk);
    }
}

__global__ __launch_bounds__(kPoseThreads) void deskew_pose_kernel(const uint32_t * __restrict__ unique_ns, const int n_groups,
                                                                   const double * __restrict__ block, const int n_seg,
                                                                   uint32_t * __restrict__ table_ns, double * __restrict__ T64,
                                                                   float * __restrict__ T32, uint32_t * flag)
{
  // the fixed part and the intervals in LDS (at most 12 016 bytes): every lane of a wave reads the same one or two intervals
  __shared__ double s_blk[sizeof(DeskewImuBlock) / sizeof(double)];
  const int n_words = n_seg > 0 ? static_cast<int>((offsetof(DeskewImuBlock, seg) + n_seg * sizeof(mh_imu_segment)) / sizeof(double)) : 0;
  for (int i = threadIdx.x; i < n_words; i += kPoseThreads) s_blk[i] = block[i];
  __syncthreads();
  const int g = blockIdx.x * kPoseThreads + threadIdx.x;
  if (g >= n_groups) return;
  const DeskewImuBlock & B = *reinterpret_cast<const DeskewImuBlock *>(s_blk);
  const uint32_t ns = unique_ns[g];
  double T[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
  // the timestamps ascend: if any of them lies behind the last interval, the last one does — every lane sees the same answer,
  // so the whole table stays identity (no point is moved with a made-up pose) and the host learns of it at its next wait
  const bool past_end = n_seg > 0 && B.header_ts + unique_ns[n_groups - 1] * 1.0e-9 > B.seg[n_seg - 1].t1;
  if (past_end && g == 0) *flag = 1u;
  if (n_seg > 0 && !past_end) {
    const double ts = B.header_ts + ns * 1.0e-9;  // globalTs, manager.hpp:94
    // the first interval with ts <= t1 (:469-476): found once for the wave's first timestamp (the same search in every lane:
    // LDS broadcasts), then a forward scan of usually zero or one step
    const double ts0 = B.header_ts + unique_ns[g & ~63] * 1.0e-9;
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ts0 > B.seg[mid].t1)
        lo = mid + 1;
      else
        hi = mid;
    }
    int c = lo;
    while (c < n_seg - 1 && ts > B.seg[c].t1) ++c;
    const mh_imu_segment & S = B.seg[c];
    const double dt = ts - S.t0;
    // :478-489  R = R_c Exp(omega dt),  p = p_c + v_c dt + 1/2 R_c acc dt^2 + 1/2 g dt^2
    double E[9], R[9], Ra[3], p[3];
    so3_expmap(S.omega[0] * dt, S.omega[1] * dt, S.omega[2] * dt, E);
    mat3_mul(S.R, E, R);
    mat3_vec(S.R, S.acc, Ra);
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = S.p[i] + S.v[i] * dt + 0.5 * Ra[i] * dt * dt + 0.5 * B.gravity[i] * dt * dt;
    // :493-499  T_Le_W * T_W_Bt * T_B_S  (Pose3 product: R1 R2, t1 + R1 t2)
    double R1[9], t1[3], t2[3];
    mat3_mul(B.R_Le_W, R, R1);
    mat3_vec(B.R_Le_W, p, t1);
    mat3_mul(R1, B.R_B_S, T);
    mat3_vec(R1, B.t_B_S, t2);
#pragma unroll
    for (int i = 0; i < 3; ++i) T[9 + i] = (B.t_Le_W[i] + t1[i]) + t2[i];
  }
  table_ns[g] = ns;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    T64[12 * static_cast<size_t>(g) + i] = T[i];
    T32[12 * static_cast<size_t>(g) + i] = static_cast<float>(T[i]);  // :504-505 cast<float>()
  }
}
}  // namespace

hipError_t launch_copy16(const void * src, void * dst, size_t bytes, hipStream_t stream)
{
  const size_t n16 = bytes / 16;  // callers copy whole 16-byte records (mh_point32 = 32 bytes)
  if (!n16) return hipSuccess;
  const size_t blocks = (n16 + 255) / 256;
  hipLaunchKernelGGL(copy16_kernel, dim3(static_cast<unsigned int>(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream,
                     static_cast<const uint4 *>(src), static_cast<uint4 *>(dst), n16);
  return hipGetLastError();
}

hipError_t launch_deskew(mh_point32 * pts, int n, const uint32_t * unique_ns, const float * Rt12, int n_groups,
                         const float * body_Rt12, hipStream_t stream)
{
  hipLaunchKernelGGL(deskew_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, reinterpret_cast<float4 *>(pts), n,
                     unique_ns, Rt12, n_groups, body_Rt12, n_groups <= kMaxGroupsLds ? 1 : 0);
  return hipGetLastError();
}
hipError_t launch_deskew_poses(const uint32_t * unique_ns, int n_groups, const DeskewImuBlock * block, int n_seg, void * table,
                               float * Rt12_f32, uint32_t * flag, hipStream_t stream)
{
  if (n_groups <= 0) return hipSuccess;
  if (n_seg < 0 || n_seg > kMaxImuSegments) return hipErrorInvalidValue;
  auto * ns = static_cast<uint32_t *>(table);
  auto * T64 = reinterpret_cast<double *>(static_cast<char *>(table) + pose_table_ns_bytes(static_cast<size_t>(n_groups)));
  hipLaunchKernelGGL(deskew_pose_kernel, dim3((n_groups + kPoseThreads - 1) / kPoseThreads), dim3(kPoseThreads), 0, stream, unique_ns,
                     n_groups, reinterpret_cast<const double *>(block), n_seg, ns, T64, Rt12_f32, flag);
  return hipGetLastError();
}
hipError_t launch_transform(mh_point32 * pts, int n, const float * Rt12, hipStream_t stream)
{
  hipLaunchKernelGGL(transform_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, reinterpret_cast<float4 *>(pts), n,
                     Rt12);
  return hipGetLastError();
}
hipError_t launch_pack_xyz(const mh_point32 * pts, int n, float4 * xyz, hipStream_t stream)
{
  hipLaunchKernelGGL(pack_xyz_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream,
                     reinterpret_cast<const float4 *>(pts), n, xyz);
  return hipGetLastError();
}
}  // namespace mh
