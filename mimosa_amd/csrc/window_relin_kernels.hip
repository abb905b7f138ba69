// icp_window_relin_step_kernel: the step of an mh_icp_window_optimise_relin chain (chain_api.hip) — icp_window_step_kernel
// (window_kernels.hip) with a decision per factor: one workgroup of one wave behind the staged K3 batch launches of an iteration,
// window_device.hpp's phases one index per lane with a barrier behind each, everything fp64, compiled without floating-point
// contraction so that the host build of the header gives the same digits.  A translation unit of its own, so that the plain
// step kernel is compiled exactly as it was.
#include <hip/hip_runtime.h>

#include "icp_device.hpp"
#include "window_device.hpp"

namespace mh
{
namespace
{
constexpr int kWindowLanes = 64;

struct WindowWave
{
  int lane;
  template <typename F>
  __device__ void each(int n, F && f)
  {
    for (int l = lane; l < n; l += kWindowLanes) f(l);
    __syncthreads();
  }
  __device__ void sync() { __syncthreads(); }
};
}  // namespace

// The step of an mh_icp_window_optimise_relin chain: the same phases, with a factor's stored model carried to the current pose
// where the step in front decided to keep its linearization (window_device.hpp: window_advance_relin).
__global__ __launch_bounds__(kWindowLanes) void icp_window_relin_step_kernel(const WindowRelinStepArgs ra)
{
  __shared__ WindowWork s_w;
  __shared__ double s_sum[32 * kWindowMax];
  __shared__ double s_row[kWRowPose + 12 * kWindowMax];
  __shared__ int s_missing;
  const WindowStepArgs & a = ra.s;
  const int lane = static_cast<int>(threadIdx.x);
  const int W = a.p.W;  // 1 .. kWindowMax (checked by the host)

  // what the step in front of this one decided (every lane reads it before window_advance_relin's first barrier)
  const unsigned int eval = window_relin_mask(*ra.relin, a.p, ra.rp);
  if (lane == 0) s_missing = 0;
  __syncthreads();
  // K3's words of the factors this iteration evaluated; a kept factor's launch touched nothing and its slot is not read
  for (int l = lane; l < 32 * W; l += kWindowLanes) {
    const int i = l >> 5;
    double v = 0.0;
    if ((eval >> i) & 1u) {
      const uint4 w = a.ll_dev[l];
      if (w.y != a.seq || w.w != a.seq) s_missing = 1;
      v = __longlong_as_double(static_cast<long long>(static_cast<unsigned long long>(w.x) | (static_cast<unsigned long long>(w.z) << 32)));
    }
    s_sum[l] = v;
  }
  const bool frozen = a.state->stopped != 0;
  __syncthreads();
  const bool missing = s_missing != 0;

  WindowWave par{lane};
  const int flags = window_advance_relin(*a.state, *ra.relin, s_sum, !missing, a.p, ra.rp, s_w, s_row, par);

  // the launches queued behind this step: the new poses, and n = 0 for a factor that keeps its linearization (every factor
  // once the chain has stopped)
  if (a.next) {
    for (int l = lane; l < 12 * W; l += kWindowLanes) {
      const int i = l / 12, q = l % 12, s = a.slot[i];
      if (s < 0) continue;
      if (q < 9)
        a.next[s].R[q] = s_row[kWRowPose + l];
      else
        a.next[s].t[q - 9] = s_row[kWRowPose + l];
    }
    if (lane < W && a.slot[lane] >= 0 && ((flags & 1) || !((ra.relin->eval >> lane) & 1u))) a.next[a.slot[lane]].n = 0;
  }
  if (!frozen && !missing) {
    for (int l = lane; l < 32 * W; l += kWindowLanes) {
      const int i = l >> 5;
      if (((eval >> i) & 1u) && a.ll_host[i]) ll_store(a.ll_host[i] + (l & 31), s_sum[l], a.seq);
    }
    if (lane == 0) ll_store(ra.mask_host, static_cast<double>(eval), a.seq);
  }
  for (int l = lane; l < kWRowPose + 12 * W; l += kWindowLanes) ll_store(a.row_host + l, s_row[l], a.seq);
}

hipError_t launch_window_relin_step(const WindowRelinStepArgs & a, hipStream_t stream)
{
  if (a.s.p.W < 1 || a.s.p.W > kWindowMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(icp_window_relin_step_kernel, dim3(1), dim3(kWindowLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mh
