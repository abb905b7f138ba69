// icp_window_step_kernel: the link between two iterations of an mh_icp_window_optimise chain (chain_api.hip).  One workgroup of
// one wave, launched behind the staged K3 batch launches of an iteration (tail = 1: each factor's last workgroup folds its rows
// and publishes the 28 sums + 4 counters as flagged words — here into device-resident slots, 32 words per pose).  The step
// turns the sums into the next W poses (window_device.hpp), writes them into the argument blocks of the launches queued behind
// it, forwards every factor's sums to its own pinned ring and publishes the iteration's row to the call's slot in mapped
// pinned memory, every double as one self-validating 16-byte store.
//
// Lanes: window_device.hpp's phases, one index per lane with a barrier behind each.  The two 3 x 3 eigen problems of every
// factor (the longest dependent chains in front of the sweep) run on 2 W lanes side by side, the per-pose Hessians and between
// terms on W lanes, the assembly on all 64; the sweep's W block pivots are the critical path: per block 36 lanes form S_i, the
// six columns of its L D L^T take 6 - j lanes each, six lanes solve for the columns of G_{i+1}.  The system, its factors and
// the vectors live in LDS (36 KiB of work arrays; 42 KiB with the sums and the row).  Everything is fp64; the file is compiled
// without floating-point contraction so that the host build of window_device.hpp gives the same digits.
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

__global__ __launch_bounds__(kWindowLanes) void icp_window_step_kernel(const WindowStepArgs a)
{
  __shared__ WindowWork s_w;
  __shared__ double s_sum[32 * kWindowMax];
  __shared__ double s_row[kWRowPose + 12 * kWindowMax];
  __shared__ int s_missing;
  const int lane = static_cast<int>(threadIdx.x);
  const int W = a.p.W;  // 1 .. kWindowMax (checked by the host)

  // K3's words of this iteration (written by the kernels in front of this one on the stream: ordinary loads)
  if (lane == 0) s_missing = 0;
  __syncthreads();
  for (int l = lane; l < 32 * W; l += kWindowLanes) {
    const int i = l >> 5;
    double v = 0.0;
    if ((a.p.have >> i) & 1u) {
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
  const int flags = window_advance(*a.state, s_sum, !missing, a.p, s_w, s_row, par);

  // the launches queued behind this step evaluate at the new poses — or at nothing, once the chain has stopped: with n = 0 K3
  // touches no point, so iterations queued behind the stop leave every factor in the state the last evaluated poses left
  if (a.next) {
    for (int l = lane; l < 12 * W; l += kWindowLanes) {
      const int i = l / 12, q = l % 12, s = a.slot[i];
      if (s < 0) continue;
      if (q < 9)
        a.next[s].R[q] = s_row[kWRowPose + l];
      else
        a.next[s].t[q - 9] = s_row[kWRowPose + l];
    }
    if ((flags & 1) && lane < W && a.slot[lane] >= 0) a.next[a.slot[lane]].n = 0;
  }
  // to the host: the sums + counters of an evaluated iteration to each factor's ring, then the row
  if (!frozen && !missing)
    for (int l = lane; l < 32 * W; l += kWindowLanes) {
      const int i = l >> 5;
      if (((a.p.have >> i) & 1u) && a.ll_host[i]) ll_store(a.ll_host[i] + (l & 31), s_sum[l], a.seq);
    }
  for (int l = lane; l < kWRowPose + 12 * W; l += kWindowLanes) ll_store(a.row_host + l, s_row[l], a.seq);
}

hipError_t launch_window_step(const WindowStepArgs & a, hipStream_t stream)
{
  if (a.p.W < 1 || a.p.W > kWindowMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(icp_window_step_kernel, dim3(1), dim3(kWindowLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mh
