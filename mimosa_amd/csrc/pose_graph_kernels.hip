// The kernels of an mh_pose_graph_optimise chain (pose_graph_api.hip); the arithmetic is pose_graph_device.hpp.  One iteration
// is a fixed run of launches on the context's stream, each phase that needs ALL of the phase before it a launch of its own (no
// rendezvous between workgroups inside a kernel):
//   pgo_edge_kernel      one lane per term: an edge (window_between_dense into per-edge rows; J_a of a far edge) or, behind the
//                        edges, a prior (window_local, window_transport into per-prior rows); its weight and cost (pgo_loss)
//   pgo_gather_kernel    one lane per output of a pose (78): T's blocks and the right-hand side from the incidence list
//   pgo_factor_kernel    one wave: Om_f = L D L^T and Om_f^-1 per far edge, then T's block L D L^T, N dependent 6 x 6 steps
//   pgo_sweep_kernel     one lane per column of [W^T | rhs] (6 F + 1), forward and back over the N blocks
//   then three times (stage 0, and the two refinement steps; from the second on behind a pgo_sweep_kernel of the residual's one column):
//     pgo_small_kernel     one workgroup: (stage 0: C and its L D L^T,) u = C^-1 W y
//     pgo_apply_kernel     one lane per row: x = y - Y u, or x += y - Y u
//     pgo_residual_kernel  one lane per row: rhs - A x (not behind the last step)
//   pgo_finish_kernel    one workgroup: retraction, the cost, the trace row, the stop test
// 15 launches.  Every kernel returns at once when the chain has stopped (PgoState::stopped) and, behind the factor kernel, when
// a pivot was not positive (PgoState::ok == 0): only pgo_finish_kernel then runs, to write the row.  Everything fp64, compiled
// without floating-point contraction so that the host build of the header gives the same digits.
#include <hip/hip_runtime.h>

#include "flagged_word.hpp"
#include "pose_graph_device.hpp"

namespace mh
{
namespace
{
constexpr int kPgoLanes = 256;

template <int LANES>
struct PgoGroup
{
  int lane;
  template <typename F>
  __device__ void each(int n, F && f)
  {
    for (int l = lane; l < n; l += LANES) f(l);
    __syncthreads();
  }
  __device__ void sync() { __syncthreads(); }
};
}  // namespace

__global__ __launch_bounds__(kPgoLanes) void pgo_edge_kernel(const PgoGraph g, const int want_res)
{
  if (g.st->stopped) return;
  const int e = static_cast<int>(blockIdx.x) * kPgoLanes + static_cast<int>(threadIdx.x);
  if (e < g.E + g.P) pgo_term(g, e, want_res != 0);
}

__global__ __launch_bounds__(kPgoLanes) void pgo_gather_kernel(const PgoGraph g, const PgoParams p)
{
  if (g.st->stopped) return;
  const int l = static_cast<int>(blockIdx.x) * kPgoLanes + static_cast<int>(threadIdx.x);
  if (l < kPgoGather * g.N) pgo_gather(g, p, l);
}

__global__ __launch_bounds__(64) void pgo_factor_kernel(const PgoGraph g)
{
  __shared__ double s_m[114];
  if (g.st->stopped) return;
  const int lane = static_cast<int>(threadIdx.x);
  PgoGroup<64> par{lane};
  if (lane == 0) g.st->ok = 1;
  __syncthreads();
  if (lane < g.F && !pgo_far_info(g, lane)) g.st->ok = 0;
  __syncthreads();
  if (!g.st->ok) return;
  pgo_factor(g, s_m, par);
}

// src: nullptr for the K columns of [W^T | rhs] into Y, else the one column g.r into g.y1
__global__ __launch_bounds__(64) void pgo_sweep_kernel(const PgoGraph g, const int refine)
{
  if (g.st->stopped || !g.st->ok) return;
  const int col = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);
  if (refine) {
    if (col == 0) pgo_sweep_col(g, 0, g.r, g.y1, 1);
  } else if (col < g.K) {
    pgo_sweep_col(g, col, nullptr, g.Y + col, g.K);
  }
}

// stage 0 / 1 / 2 as in the file comment: one workgroup
__global__ __launch_bounds__(kPgoLanes) void pgo_small_kernel(const PgoGraph g, const int stage)
{
  if (g.st->stopped || !g.st->ok) return;
  PgoGroup<kPgoLanes> par{static_cast<int>(threadIdx.x)};
  pgo_small(g, stage, par);
}

// one lane per row of x: x = y - Y u (stage 0) or x += y1 - Y u
__global__ __launch_bounds__(kPgoLanes) void pgo_apply_kernel(const PgoGraph g, const int stage)
{
  if (g.st->stopped || !g.st->ok) return;
  const int row = static_cast<int>(blockIdx.x) * kPgoLanes + static_cast<int>(threadIdx.x);
  if (row < 6 * g.N) pgo_apply_row(g, stage ? g.y1 : g.Y + 6 * g.F, stage ? 1 : g.K, stage == 0, row);
}

// one lane per row of the residual rhs - A x
__global__ __launch_bounds__(kPgoLanes) void pgo_residual_kernel(const PgoGraph g)
{
  if (g.st->stopped || !g.st->ok) return;
  const int row = static_cast<int>(blockIdx.x) * kPgoLanes + static_cast<int>(threadIdx.x);
  if (row < 6 * g.N) pgo_residual_row(g, row);
}

// one workgroup: the step, the row of iteration `it`, the stop test.  trace: nullptr or the row of iteration `it` in the device's
// pose trace.  word: the iteration's flagged word in mapped pinned memory (the row's flags; 5 for an iteration queued behind
// the stop).
__global__ __launch_bounds__(kPgoLanes) void pgo_finish_kernel(const PgoGraph g, const PgoParams p, const int it, double * trace, uint4 * word,
                                                                const unsigned int seq)
{
  const int lane = static_cast<int>(threadIdx.x);
  if (g.st->stopped) {
    if (lane == 0) ll_store(word, 5.0, seq);
    return;
  }
  PgoGroup<kPgoLanes> par{lane};
  pgo_finish(g, p, it, trace, par);
  if (lane == 0) ll_store(word, static_cast<double>(g.rows[it].flags), seq);
}

// the cost of the terms pgo_edge_kernel evaluated, into rows[0].f.  chi2 != 0 (mh_pose_graph_residuals): the sum of the edges'
// chi^2 instead, whatever their losses
__global__ __launch_bounds__(kPgoLanes) void pgo_cost_kernel(const PgoGraph g, const int chi2)
{
  PgoGroup<kPgoLanes> par{static_cast<int>(threadIdx.x)};
  PgoGraph h = g;
  if (chi2) {
    h.rho = g.cz;
    h.P = 0;
  }
  pgo_cost(h, &g.rows[0].f, par);
}

hipError_t launch_pgo_edges(const PgoGraph & g, bool want_res, hipStream_t stream)
{
  if (g.E < 0 || g.E > kPgoMaxEdges || g.P < 0 || g.P > kPgoMaxPoses) return hipErrorInvalidValue;
  if (g.E + g.P == 0) return hipSuccess;
  hipLaunchKernelGGL(pgo_edge_kernel, dim3((g.E + g.P + kPgoLanes - 1) / kPgoLanes), dim3(kPgoLanes), 0, stream, g, want_res ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_pgo_cost(const PgoGraph & g, bool chi2, hipStream_t stream)
{
  hipLaunchKernelGGL(pgo_cost_kernel, dim3(1), dim3(kPgoLanes), 0, stream, g, chi2 ? 1 : 0);
  return hipGetLastError();
}

// one iteration behind whatever is on the stream
hipError_t launch_pgo_iteration(const PgoGraph & g, const PgoParams & p, int it, double * trace, uint4 * word, unsigned int seq, hipStream_t stream)
{
  if (g.N < 1 || g.N > kPgoMaxPoses || g.E < 0 || g.E > kPgoMaxEdges || g.P < 0 || g.P > kPgoMaxPoses || g.F < 0 || g.F > kPgoFarMax || g.K != 6 * g.F + 1 || it < 0 || it >= kPgoMaxIters)
    return hipErrorInvalidValue;
  hipError_t e = launch_pgo_edges(g, false, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pgo_gather_kernel, dim3((kPgoGather * g.N + kPgoLanes - 1) / kPgoLanes), dim3(kPgoLanes), 0, stream, g, p);
  hipLaunchKernelGGL(pgo_factor_kernel, dim3(1), dim3(64), 0, stream, g);
  hipLaunchKernelGGL(pgo_sweep_kernel, dim3((g.K + 63) / 64), dim3(64), 0, stream, g, 0);
  const dim3 rows((6 * g.N + kPgoLanes - 1) / kPgoLanes);
  for (int stage = 0; stage < 3; ++stage) {
    if (stage > 0) hipLaunchKernelGGL(pgo_sweep_kernel, dim3(1), dim3(64), 0, stream, g, 1);
    hipLaunchKernelGGL(pgo_small_kernel, dim3(1), dim3(kPgoLanes), 0, stream, g, stage);
    hipLaunchKernelGGL(pgo_apply_kernel, rows, dim3(kPgoLanes), 0, stream, g, stage);
    if (stage < 2) hipLaunchKernelGGL(pgo_residual_kernel, rows, dim3(kPgoLanes), 0, stream, g);
  }
  hipLaunchKernelGGL(pgo_finish_kernel, dim3(1), dim3(kPgoLanes), 0, stream, g, p, it, trace, word, seq);
  return hipGetLastError();
}

}  // namespace mh
