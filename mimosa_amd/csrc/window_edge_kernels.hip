// icp_window_edge_step_kernel: the step of an mh_icp_window_optimise_edges chain (chain_api.hip) — icp_window_lin_step_kernel
// (window_lin_kernels.hip) whose system also holds between factors on any pair of poses, each with a dense information matrix:
// one more phase per iteration evaluates each of them at the current poses (window_device.hpp: window_between_dense), one
// index per edge, into LDS; the assembly adds them behind the has_Z terms.  The system is then no longer block-tridiagonal
// and is solved over its row profile (window_factor_profile): the off-diagonal blocks and the factor's S_k^-1 T^T, up to 120
// blocks of 6 x 6 each, sit in LDS as well — 153 960 B in all, under the 160 KiB one workgroup of gfx950 may declare; one
// workgroup per launch, so occupancy is not a concern.  The edges themselves sit in the context's device block, written once
// per call and only read here.  One workgroup of one wave, a barrier behind each phase, everything fp64, compiled without
// floating-point contraction so that the host build of the header gives the same digits.  A translation unit of its own, so
// that the other step kernels are compiled exactly as they were.
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

template <bool RELIN>
__global__ __launch_bounds__(kWindowLanes) void icp_window_edge_step_kernel(const WindowEdgeStepArgs ea)
{
  __shared__ WindowWork s_w;
  __shared__ WindowLinWork s_lw;
  __shared__ WindowEdgeWork s_ew;
  __shared__ double s_sum[32 * kWindowMax];
  __shared__ double s_row[kWRowPose + 12 * kWindowMax];
  __shared__ int s_missing;
  const WindowLinStepArgs & la = ea.l;
  const WindowRelinStepArgs & ra = la.r;
  const WindowStepArgs & a = ra.s;
  const int lane = static_cast<int>(threadIdx.x);
  const int W = a.p.W;  // 1 .. kWindowMax (checked by the host)

  // the factors this iteration evaluated: all non-empty ones, or what the step in front of this one decided (every lane reads
  // it before window_advance_impl's first barrier)
  const unsigned int eval = RELIN ? window_relin_mask(*ra.relin, a.p, ra.rp) : a.p.have;
  if (lane == 0) s_missing = 0;
  __syncthreads();
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
  const int flags = window_advance_impl<RELIN, true, true>(*a.state, s_sum, !missing, a.p, s_w, s_row, RELIN ? ra.relin : nullptr, RELIN ? &ra.rp : nullptr,
                                                           la.lin, &s_lw, ea.edges, &s_ew, par);

  // the launches queued behind this step: the new poses, and n = 0 once the chain has stopped or (RELIN) for a factor that
  // keeps its linearization
  if (a.next) {
    for (int l = lane; l < 12 * W; l += kWindowLanes) {
      const int i = l / 12, q = l % 12, s = a.slot[i];
      if (s < 0) continue;
      if (q < 9)
        a.next[s].R[q] = s_row[kWRowPose + l];
      else
        a.next[s].t[q - 9] = s_row[kWRowPose + l];
    }
    if (lane < W && a.slot[lane] >= 0) {
      bool skip = (flags & 1) != 0;
      if (RELIN) skip = skip || !((ra.relin->eval >> lane) & 1u);
      if (skip) a.next[a.slot[lane]].n = 0;
    }
  }
  if (!frozen && !missing) {
    for (int l = lane; l < 32 * W; l += kWindowLanes) {
      const int i = l >> 5;
      if (((eval >> i) & 1u) && a.ll_host[i]) ll_store(a.ll_host[i] + (l & 31), s_sum[l], a.seq);
    }
    if (RELIN && lane == 0) ll_store(ra.mask_host, static_cast<double>(eval), a.seq);
  }
  for (int l = lane; l < kWRowPose + 12 * W; l += kWindowLanes) ll_store(a.row_host + l, s_row[l], a.seq);
}

hipError_t launch_window_edge_step(const WindowEdgeStepArgs & a, bool relin, hipStream_t stream)
{
  if (a.l.r.s.p.W < 1 || a.l.r.s.p.W > kWindowMax || !a.l.lin || !a.edges) return hipErrorInvalidValue;
  if (relin)
    hipLaunchKernelGGL(icp_window_edge_step_kernel<true>, dim3(1), dim3(kWindowLanes), 0, stream, a);
  else
    hipLaunchKernelGGL(icp_window_edge_step_kernel<false>, dim3(1), dim3(kWindowLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mh
