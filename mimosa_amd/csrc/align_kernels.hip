// icp_align_step_kernel: the link between two K3 launches of an alignment chain with one member (chain_api.hip: mh_icp_align,
// a one-member mh_icp_align_batch).  One workgroup of one wave, launched behind each K3 (batch form, tail = 1: its last workgroup
// folds the rows and publishes the 28 sums + 4 counters as flagged words — here into a device-resident slot).  The step turns the sums into the next pose (align_device.hpp), writes it
// into the argument block of the K3 launch queued behind it, and publishes the iteration's sums and its trace row to the
// call's slot in mapped pinned memory, every double as one self-validating 16-byte store.
//
// Lanes: 0 and 1 decompose the rotation and the translation block side by side (the two eigen problems are the longest
// dependent chains of the step), lane 0 solves and retracts, lanes 0..31 forward the words.  Everything is fp64; the file is
// compiled without floating-point contraction so that the host build of align_device.hpp gives the same digits.
//
// icp_align_batch_step_kernel: the same step for the members of a chain with several in one launch, one one-wave workgroup
// per member.  The members share nothing — no barrier across workgroups, no atomics: workgroup m reads and writes
// what member m's arguments point at.
#include <hip/hip_runtime.h>

#include "align_device.hpp"
#include "icp_device.hpp"

namespace mh
{
// one wave, one chain: what both kernels run
__device__ __forceinline__ void align_step_wave(const AlignStepArgs & a, double * s_sum, double * s_row, int * s_stop)
{
  const int lane = static_cast<int>(threadIdx.x);

  // K3's words of this iteration (written by the kernel in front of this one on the stream: ordinary loads)
  bool arrived = true;
  if (lane < 32) {
    const uint4 w = a.ll_dev[lane];
    arrived = w.y == a.seq && w.w == a.seq;
    s_sum[lane] = __longlong_as_double(static_cast<long long>(static_cast<unsigned long long>(w.x) | (static_cast<unsigned long long>(w.z) << 32)));
  }
  const bool frozen = a.state->stopped != 0;  // (read before lane 0 updates it: the barrier below is the first)
  const bool missing = __ballot(!arrived) != 0ull;
  __syncthreads();

  bool degen = false;
  if (lane < 2 && !frozen && !missing) degen = align_block_degenerate(s_sum, lane, lane == 0 ? a.p.thresh_rot : a.p.thresh_trans);
  const unsigned long long dm = __ballot(degen);

  if (lane == 0) {
    AlignState st = *a.state;
    *s_stop = align_advance(st, s_sum, !missing, a.p, (dm & 1ull) != 0, (dm & 2ull) != 0, s_row) & 1;
    *a.state = st;
  }
  __syncthreads();

  // the launch queued behind this step evaluates at the new pose — or at nothing, once the chain has stopped: with n = 0 K3
  // touches no point, so iterations queued behind the stop leave the factor in the state the last evaluated pose left
  if (a.next) {
    if (lane < 9) a.next->R[lane] = s_row[kRowR + lane];
    if (lane >= 16 && lane < 19) a.next->t[lane - 16] = s_row[kRowT + lane - 16];
    if (lane == 32 && *s_stop) a.next->n = 0;
  }
  // to the host: the sums + counters of an evaluated iteration, then the row
  if (lane < 32 && !frozen && !missing) ll_store(a.ll_host + lane, s_sum[lane], a.seq);
  if (lane < kRowWords) ll_store(a.ll_host + kLlSums + lane, s_row[lane], a.seq);
}

__global__ __launch_bounds__(64) void icp_align_step_kernel(const AlignStepArgs a)
{
  __shared__ double s_sum[32];
  __shared__ double s_row[kRowWords];
  __shared__ int s_stop;
  align_step_wave(a, s_sum, s_row, &s_stop);
}

__global__ __launch_bounds__(64) void icp_align_batch_step_kernel(const AlignBatchStepArgs b)
{
  __shared__ double s_sum[32];
  __shared__ double s_row[kRowWords];
  __shared__ int s_stop;
  align_step_wave(b.m[blockIdx.x], s_sum, s_row, &s_stop);  // (the grid is the number of members: launch_align_chain_step)
}

hipError_t launch_align_chain_step(const AlignBatchStepArgs & a, int n_members, hipStream_t stream)
{
  if (n_members < 1 || n_members > kAlignBatchMax) return hipErrorInvalidValue;
  if (n_members == 1)  // (the small kernel-argument segment of one member's arguments)
    hipLaunchKernelGGL(icp_align_step_kernel, dim3(1), dim3(64), 0, stream, a.m[0]);
  else
    hipLaunchKernelGGL(icp_align_batch_step_kernel, dim3(n_members), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace mh
