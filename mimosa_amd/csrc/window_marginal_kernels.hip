// icp_window_marginal_kernel: the kernel of mh_icp_window_marginalise (chain_api.hip) — what eliminating the oldest pose of a
// fixed-lag window leaves on the pose behind it, as one dense Gaussian (window_device.hpp: window_marginal_impl).  Launched
// behind the one K3 launch of the oldest factor: it reads that factor's 28 sums and 4 counters through the flagged words as the
// step kernels do (missing sums are reported, not used), forwards them to the factor's pinned ring, evaluates every term that
// touches pose 0 at the poses given — the ICP factor, the linear factors on pose 0, the has_Z[1] tie, the edges on (0, 1) —
// into LDS, eliminates pose 0 and publishes H_m, b_m, f_m as one row of flagged words.  One workgroup of one wave, a barrier
// behind each phase, everything fp64, compiled without floating-point contraction so that the host build of the header
// (tests/cpp/window_marginal_step.cpp) gives the same digits.  A translation unit of its own, so that the step kernels are
// compiled exactly as they were.
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

__global__ __launch_bounds__(kWindowLanes) void icp_window_marginal_kernel(const WindowMarginalArgs a)
{
  __shared__ WindowMarginalWork s_w;
  __shared__ WindowLinWork s_lw;
  __shared__ WindowMarginalOut s_out;
  __shared__ double s_sum[32];
  __shared__ double s_row[kWMargWords];
  __shared__ int s_missing;
  const int lane = static_cast<int>(threadIdx.x);
  const bool have = (a.p.have & 1u) != 0;

  if (lane == 0) s_missing = 0;
  __syncthreads();
  if (lane < 32) {
    double v = 0.0;
    if (have) {
      const uint4 w = a.ll_dev[lane];
      if (w.y != a.seq || w.w != a.seq) s_missing = 1;
      v = __longlong_as_double(static_cast<long long>(static_cast<unsigned long long>(w.x) | (static_cast<unsigned long long>(w.z) << 32)));
    }
    s_sum[lane] = v;
  }
  __syncthreads();
  const bool missing = s_missing != 0;

  for (int l = lane; l < kWMargWords; l += kWindowLanes) s_row[l] = 0.0;
  __syncthreads();
  if (!missing) {
    WindowWave par{lane};
    window_marginal_impl(s_sum, *a.state, a.p, *a.lin, s_lw, *a.edges, s_w, s_out, par);
    for (int l = lane; l < kWMargWords; l += kWindowLanes) {
      double v = 0.0;
      if (l == kWMargValid)
        v = static_cast<double>(s_out.valid);
      else if (l == kWMargTies)
        v = static_cast<double>(s_out.n_ties);
      else if (l == kWMargF)
        v = s_out.f;
      else if (l >= kWMargH)
        v = s_out.H[l - kWMargH];
      else if (l >= kWMargB)
        v = s_out.b[l - kWMargB];
      s_row[l] = v;
    }
    if (have && a.ll_host && lane < 32) ll_store(a.ll_host + lane, s_sum[lane], a.seq);
  } else if (lane == 0) {
    s_row[kWMargBits] = 8.0;
  }
  __syncthreads();
  for (int l = lane; l < kWMargWords; l += kWindowLanes) ll_store(a.row_host + l, s_row[l], a.seq);
}

hipError_t launch_window_marginal(const WindowMarginalArgs & a, hipStream_t stream)
{
  if (a.p.W < 2 || a.p.W > kWindowMax || !a.state || !a.lin || !a.edges || !a.row_host || !a.ll_dev) return hipErrorInvalidValue;
  hipLaunchKernelGGL(icp_window_marginal_kernel, dim3(1), dim3(kWindowLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mh
