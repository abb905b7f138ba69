// icp_window_joint_step_kernel: the step of an mh_icp_window_optimise_joint chain (chain_api.hip) — icp_window_edge_step_kernel
// (window_edge_kernels.hip) whose system also holds ONE dense factor on up to four poses of the window: the joint marginal a
// fixed-lag smoother carries once odometry edges reach from the oldest pose past pose 1.  Two more phases per iteration carry
// it to the current poses of its members (window_device.hpp: window_joint_transport: one index per member for the offsets,
// then one per block of the upper triangle, per gradient row and for the constant), the assembly adds its diagonal blocks and
// gradient behind the linear factors and its off-diagonal blocks into the row profile.  LDS: the edge step's 153 960 B plus
// WindowJointWork (the carried H' of 24 x 24, b', f', the members' offsets and Jacobians: 5 576 B) — 159 536 B of the 163 840 B
// a gfx950 workgroup may declare; WindowLinWork::tmp, free behind the linear-factor phase, is the block scratch.
// icp_window_marginal_joint_kernel: the kernel of mh_icp_window_marginalise_joint — icp_window_marginal_kernel
// (window_marginal_kernels.hip) with the edges (0, b) beyond pose 1 and the carried joint factor, eliminating pose 0 onto a
// separator of up to four poses (window_marginal_joint_impl); its row is kWJMargWords flagged words wide.
// Both: one workgroup of one wave, a barrier behind each phase, no spin waits, everything fp64, compiled without floating-point
// contraction so that the host build of the header (tests/cpp/window_joint_step.cpp) gives the same digits.  A translation unit
// of its own, so that the other kernels are compiled exactly as they were.
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
__global__ __launch_bounds__(kWindowLanes) void icp_window_joint_step_kernel(const WindowJointStepArgs ja)
{
  __shared__ WindowWork s_w;
  __shared__ WindowLinWork s_lw;
  __shared__ WindowEdgeWork s_ew;
  __shared__ WindowJointWork s_jw;
  __shared__ double s_sum[32 * kWindowMax];
  __shared__ double s_row[kWRowPose + 12 * kWindowMax];
  __shared__ int s_missing;
  const WindowEdgeStepArgs & ea = ja.e;
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
  const int flags = window_advance_impl<RELIN, true, true, true>(*a.state, s_sum, !missing, a.p, s_w, s_row, RELIN ? ra.relin : nullptr, RELIN ? &ra.rp : nullptr,
                                                                 la.lin, &s_lw, ea.edges, &s_ew, par, ja.joint, &s_jw);

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

hipError_t launch_window_joint_step(const WindowJointStepArgs & a, bool relin, hipStream_t stream)
{
  const WindowStepArgs & s = a.e.l.r.s;
  if (s.p.W < 1 || s.p.W > kWindowMax || !a.e.l.lin || !a.e.edges || !a.joint) return hipErrorInvalidValue;
  if (relin)
    hipLaunchKernelGGL(icp_window_joint_step_kernel<true>, dim3(1), dim3(kWindowLanes), 0, stream, a);
  else
    hipLaunchKernelGGL(icp_window_joint_step_kernel<false>, dim3(1), dim3(kWindowLanes), 0, stream, a);
  return hipGetLastError();
}

__global__ __launch_bounds__(kWindowLanes) void icp_window_marginal_joint_kernel(const WindowMarginalJointArgs ja)
{
  __shared__ WindowMarginalJointWork s_w;
  __shared__ WindowLinWork s_lw;
  __shared__ WindowJointWork s_jw;
  __shared__ WindowMarginalJointOut s_out;
  __shared__ double s_sum[32];
  __shared__ int s_sep[kWindowJointMax];
  __shared__ int s_missing;
  const WindowMarginalArgs & a = ja.m;
  const int lane = static_cast<int>(threadIdx.x);
  const bool have = (a.p.have & 1u) != 0;

  if (lane == 0) s_missing = 0;
  if (lane < kWindowJointMax) s_sep[lane] = ja.sep[lane];
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

  if (!missing) {
    WindowWave par{lane};
    window_marginal_joint_impl(s_sum, *a.state, a.p, *a.lin, s_lw, *a.edges, ja.joint, s_jw, ja.n_sep, s_sep, s_w, s_out, par);
    if (have && a.ll_host && lane < 32) ll_store(a.ll_host + lane, s_sum[lane], a.seq);
  }
  __syncthreads();
  for (int l = lane; l < kWJMargWords; l += kWindowLanes) {
    double v = 0.0;
    if (missing)
      v = l == kWJMargBits ? 8.0 : 0.0;
    else if (l == kWJMargValid)
      v = static_cast<double>(s_out.valid);
    else if (l == kWJMargTies)
      v = static_cast<double>(s_out.n_ties);
    else if (l == kWJMargF)
      v = s_out.f;
    else if (l >= kWJMargH)
      v = s_out.H[l - kWJMargH];
    else if (l >= kWJMargB)
      v = s_out.b[l - kWJMargB];
    ll_store(a.row_host + l, v, a.seq);
  }
}

hipError_t launch_window_marginal_joint(const WindowMarginalJointArgs & a, hipStream_t stream)
{
  const WindowMarginalArgs & m = a.m;
  if (m.p.W < 2 || m.p.W > kWindowMax || !m.state || !m.lin || !m.edges || !m.row_host || !m.ll_dev) return hipErrorInvalidValue;
  if (a.n_sep < 1 || a.n_sep > kWindowJointMax) return hipErrorInvalidValue;
  for (int k = 0; k < a.n_sep; ++k)
    if (a.sep[k] < 1 || a.sep[k] >= m.p.W || (k > 0 && a.sep[k] <= a.sep[k - 1])) return hipErrorInvalidValue;
  hipLaunchKernelGGL(icp_window_marginal_joint_kernel, dim3(1), dim3(kWindowLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mh
