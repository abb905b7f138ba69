// The kernels of an mh_pose_graph_optimise chain (pose_graph_api.hip); the arithmetic is pose_graph_device.hpp.  One iteration
// is a fixed run of launches on the context's stream, each phase that needs ALL of the phase before it a launch of its own (no
// rendezvous between workgroups inside a kernel):
//   pgo_edge_kernel      one lane per term: an edge (window_between_dense into per-edge rows; J_a of a far edge) or, behind the
//                        edges, a prior (window_local, window_transport into per-prior rows); its weight and cost (pgo_loss)
//   pgo_gather_kernel    one lane per output of a pose (78): T's blocks and the right-hand side from the incidence list
//   pgo_factor_kernel    one wave: Om_f = L D L^T and Om_f^-1 per far edge (lane l: f = l, l + 64, ...), then T's block L D L^T, N dependent 6 x 6 steps
//   pgo_sweep_kernel     one lane per column of [W^T | rhs] (6 F + 1), forward and back over the N blocks
//   then three times (stage 0, and the two refinement steps; from the second on behind a pgo_sweep_kernel of the residual's one column):
//     pgo_small_kernel     one workgroup: (stage 0: C and its L D L^T,) u = C^-1 W y
//     pgo_apply_kernel     one lane per row: x = y - Y u, or x += y - Y u
//     pgo_residual_kernel  one lane per row: rhs - A x (not behind the last step)
//   pgo_finish_kernel    one workgroup: retraction, the cost, the trace row, the stop test
// 15 launches; a graph created wide runs pgo_small_kernel's work in blocks over many workgroups (below: pgo_wide_*).  Every kernel returns at once when the chain has stopped (PgoState::stopped) and, behind the factor kernel, when
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
  for (int f = lane; f < g.F; f += 64)
    if (!pgo_far_info(g, f)) g.st->ok = 0;
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

// ---- a wide graph: pgo_small_kernel's work in blocks (pose_graph_device.hpp: pgo_wide_*) ------------------------------------------
// In pgo_small_kernel's place, with nt = ceil(6 F / NB) panels:
//   stage 0:  pgo_wide_build_kernel   a workgroup per NB x NB tile of C's lower triangle, a lane per entry (adjacent lanes adjacent in col)
//             per panel p:  pgo_wide_diag_kernel   one workgroup: the diagonal block in LDS, the pivot test
//                           pgo_wide_strip_kernel  a workgroup per NB rows under the block: their U and L, the block's factors in LDS
//                           pgo_wide_trail_kernel  a workgroup per tile behind the panel, the panel's L and U operands in LDS
//   every stage:  per panel p ascending  pgo_wide_forward_kernel   a wave per NB rows behind the block (one at least), u's block in LDS
//                 per panel p descending pgo_wide_backward_kernel  a wave per NB rows in front of the block (one at least)
// 1 + 3 nt - 2 launches for the factor (the last panel has neither strip nor tile), 2 nt per solve.  The work of a launch is at most
// NB^2 steps in one workgroup, whatever F is.
__global__ __launch_bounds__(kPgoLanes) void pgo_wide_build_kernel(const PgoGraph g)
{
  if (g.st->stopped || !g.st->ok || blockIdx.x > blockIdx.y) return;
  PgoGroup<kPgoLanes> par{static_cast<int>(threadIdx.x)};
  pgo_wide_build(g, static_cast<int>(blockIdx.y), static_cast<int>(blockIdx.x), par);
}

__global__ __launch_bounds__(kPgoLanes) void pgo_wide_diag_kernel(const PgoGraph g, const int p)
{
  __shared__ double s_m[kPgoWideNB * kPgoWideLd];
  if (g.st->stopped || !g.st->ok) return;
  PgoGroup<kPgoLanes> par{static_cast<int>(threadIdx.x)};
  pgo_wide_diag(g, p, s_m, par);
}

__global__ __launch_bounds__(kPgoLanes) void pgo_wide_strip_kernel(const PgoGraph g, const int p)
{
  __shared__ double s_m[kPgoWideSm];
  if (g.st->stopped || !g.st->ok) return;
  PgoGroup<kPgoLanes> par{static_cast<int>(threadIdx.x)};
  pgo_wide_strip(g, p, static_cast<int>(blockIdx.x), s_m, par);
}

__global__ __launch_bounds__(kPgoLanes) void pgo_wide_trail_kernel(const PgoGraph g, const int p)
{
  __shared__ double s_m[kPgoWideSm];
  if (g.st->stopped || !g.st->ok || blockIdx.x > blockIdx.y) return;
  PgoGroup<kPgoLanes> par{static_cast<int>(threadIdx.x)};
  pgo_wide_trail(g, p, static_cast<int>(blockIdx.y), static_cast<int>(blockIdx.x), s_m, par);
}

__global__ __launch_bounds__(64) void pgo_wide_forward_kernel(const PgoGraph g, const int stage, const int p)
{
  __shared__ double s_m[kPgoWideNB + kPgoWideNB * kPgoWideLd];
  if (g.st->stopped || !g.st->ok) return;
  PgoGroup<64> par{static_cast<int>(threadIdx.x)};
  pgo_wide_forward(g, stage ? g.y1 : g.Y + 6 * g.F, stage ? 1 : g.K, p, static_cast<int>(blockIdx.x), s_m, par);
}

__global__ __launch_bounds__(64) void pgo_wide_backward_kernel(const PgoGraph g, const int p)
{
  __shared__ double s_m[kPgoWideNB + kPgoWideNB * kPgoWideLd];
  if (g.st->stopped || !g.st->ok) return;
  PgoGroup<64> par{static_cast<int>(threadIdx.x)};
  pgo_wide_backward(g, p, static_cast<int>(blockIdx.x), s_m, par);
}

// pgo_small_kernel's stage on a wide graph that holds a far edge
static void launch_pgo_small_wide(const PgoGraph & g, int stage, hipStream_t stream)
{
  const int nt = pgo_wide_blocks(6 * g.F);
  if (stage == 0) {
    hipLaunchKernelGGL(pgo_wide_build_kernel, dim3(nt, nt), dim3(kPgoLanes), 0, stream, g);
    for (int p = 0; p < nt; ++p) {
      const int behind = nt - p - 1;
      hipLaunchKernelGGL(pgo_wide_diag_kernel, dim3(1), dim3(kPgoLanes), 0, stream, g, p);
      if (behind > 0) {
        hipLaunchKernelGGL(pgo_wide_strip_kernel, dim3(behind), dim3(kPgoLanes), 0, stream, g, p);
        hipLaunchKernelGGL(pgo_wide_trail_kernel, dim3(behind, behind), dim3(kPgoLanes), 0, stream, g, p);
      }
    }
  }
  for (int p = 0; p < nt; ++p) hipLaunchKernelGGL(pgo_wide_forward_kernel, dim3(nt - p - 1 > 1 ? nt - p - 1 : 1), dim3(64), 0, stream, g, stage, p);
  for (int p = nt - 1; p >= 0; --p) hipLaunchKernelGGL(pgo_wide_backward_kernel, dim3(p > 1 ? p : 1), dim3(64), 0, stream, g, p);
}

// one iteration behind whatever is on the stream.  far_cap: the far edges the graph's arrays were laid out for; wide: a graph created
// wide, which runs the blocked launches in pgo_small_kernel's place whenever it holds a far edge
hipError_t launch_pgo_iteration(const PgoGraph & g, const PgoParams & p, int it, double * trace, uint4 * word, unsigned int seq, hipStream_t stream, int far_cap,
                                bool wide)
{
  if (g.N < 1 || g.N > kPgoMaxPoses || g.E < 0 || g.E > kPgoMaxEdges || g.P < 0 || g.P > kPgoMaxPoses || g.F < 0 || g.F > far_cap ||
      far_cap > (wide ? kPgoFarLimit : kPgoFarMax) || g.K != 6 * g.F + 1 || it < 0 || it >= kPgoMaxIters)
    return hipErrorInvalidValue;
  hipError_t e = launch_pgo_edges(g, false, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pgo_gather_kernel, dim3((kPgoGather * g.N + kPgoLanes - 1) / kPgoLanes), dim3(kPgoLanes), 0, stream, g, p);
  hipLaunchKernelGGL(pgo_factor_kernel, dim3(1), dim3(64), 0, stream, g);
  hipLaunchKernelGGL(pgo_sweep_kernel, dim3((g.K + 63) / 64), dim3(64), 0, stream, g, 0);
  const dim3 rows((6 * g.N + kPgoLanes - 1) / kPgoLanes);
  for (int stage = 0; stage < 3; ++stage) {
    if (stage > 0) hipLaunchKernelGGL(pgo_sweep_kernel, dim3(1), dim3(64), 0, stream, g, 1);
    if (wide && g.F > 0)
      launch_pgo_small_wide(g, stage, stream);
    else
      hipLaunchKernelGGL(pgo_small_kernel, dim3(1), dim3(kPgoLanes), 0, stream, g, stage);
    hipLaunchKernelGGL(pgo_apply_kernel, rows, dim3(kPgoLanes), 0, stream, g, stage);
    if (stage < 2) hipLaunchKernelGGL(pgo_residual_kernel, rows, dim3(kPgoLanes), 0, stream, g);
  }
  hipLaunchKernelGGL(pgo_finish_kernel, dim3(1), dim3(kPgoLanes), 0, stream, g, p, it, trace, word, seq);
  return hipGetLastError();
}

// ---- mh_pose_graph_covariances -------------------------------------------------------------------------------------------------------
// Behind an iteration's launches up to the stage-0 pgo_small_kernel (T's factors, Y, C's factor):
//   pgo_cov_chain_kernel    one wave: P_i = (T^-1)_ii, N dependent 6 x 6 steps backwards.  Block i - 1's L, D and G_i (78 doubles)
//                           are loaded into registers before the arithmetic of block i and put into LDS behind it, so that no
//                           step waits for global memory; P_{i+1} stays in LDS.
//   pgo_cov_correct_kernel  one wave per pose: Sigma_ii = P_i - U^T D_C^-1 U; U and a panel of C's factor in LDS
//   per pair column (one lane per column, or per entry of the columns):
//     pgo_cov_sweep_kernel, pgo_cov_solve_kernel (F > 0), pgo_cov_apply_kernel, then twice pgo_cov_residual_kernel and the three again
//   pgo_cov_joint_kernel    one lane per entry of joint
// Every kernel returns at once when a pivot was not positive (PgoState::ok == 0).
__global__ __launch_bounds__(64) void pgo_cov_chain_kernel(const PgoGraph g, const PgoCov cov)
{
  __shared__ double s_m[kPgoCovChainSm];
  __shared__ double s_blk[2][78];  // L_i (36), D_i (6), G_{i+1} (36) of the current block and of the next one
  if (!g.st->ok) return;
  const int lane = static_cast<int>(threadIdx.x), N = g.N;
  double *Si = s_m, *M = s_m + 36, *Pc = s_m + 72;
  // entry k < 78 of block i: L_i, D_i, G_{i+1} (behind the last block: G_{N-1}, which pgo_cov_step1/2 do not read).  ONE load from
  // a selected address per lane: three loads under three lane masks into one register would each wait for the one before.
  auto load = [&](int i, int k) -> double {
    const double * p = k < 36 ? g.L + 36 * i + k : (k < 42 ? g.Dv + 6 * i + (k - 36) : g.G + 36 * (i + 1 < N ? i + 1 : i) + (k - 42));
    return *p;
  };
  s_blk[0][lane] = load(N - 1, lane);
  if (lane < 14) s_blk[0][64 + lane] = load(N - 1, 64 + lane);
  __syncthreads();
  int cur = 0;
  for (int i = N - 1; i >= 0; --i) {
    const bool last = i == N - 1;
    double n0 = 0.0, n1 = 0.0;
    if (i > 0) {
      n0 = load(i - 1, lane);
      if (lane < 14) n1 = load(i - 1, 64 + lane);
    }
    const double *Lb = s_blk[cur], *Db = s_blk[cur] + 36, *Gn = s_blk[cur] + 42;
    if (lane < 42) pgo_cov_step1(Lb, Db, Gn, Pc, last, Si, M, lane);
    __syncthreads();
    // (before phase 2: the wait for the prefetch then stands in front of phase 2's stores of P_i, not behind them)
    s_blk[cur ^ 1][lane] = n0;
    if (lane < 14) s_blk[cur ^ 1][64 + lane] = n1;
    if (lane < 36) pgo_cov_step2(Gn, Si, M, last, Pc, cov.P + 36 * i, lane);
    __syncthreads();
    cur ^= 1;
  }
}

__global__ __launch_bounds__(64) void pgo_cov_correct_kernel(const PgoGraph g, const PgoCov cov)
{
  __shared__ double s_m[6 * kPgoFarMax * (6 + kPgoCovPanel)];
  if (!g.st->ok) return;
  PgoGroup<64> par{static_cast<int>(threadIdx.x)};
  pgo_cov_correct(g, cov, static_cast<int>(blockIdx.x), s_m, par);
}

__global__ __launch_bounds__(64) void pgo_cov_sweep_kernel(const PgoGraph g, const PgoCov cov, const int first)
{
  if (!g.st->ok) return;
  const int q = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);
  if (q < cov.ncols) pgo_cov_sweep(g, cov, q, first != 0);
}

__global__ __launch_bounds__(64) void pgo_cov_solve_kernel(const PgoGraph g, const PgoCov cov)
{
  if (!g.st->ok) return;
  const int q = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);
  if (q < cov.ncols) pgo_cov_solve(g, cov, q);
}

__global__ __launch_bounds__(kPgoLanes) void pgo_cov_apply_kernel(const PgoGraph g, const PgoCov cov, const int first)
{
  if (!g.st->ok) return;
  const size_t l = static_cast<size_t>(blockIdx.x) * kPgoLanes + threadIdx.x;
  if (l < static_cast<size_t>(6 * g.N) * cov.ncols) pgo_cov_apply(g, cov, first != 0, l);
}

__global__ __launch_bounds__(kPgoLanes) void pgo_cov_residual_kernel(const PgoGraph g, const PgoCov cov)
{
  if (!g.st->ok) return;
  const size_t l = static_cast<size_t>(blockIdx.x) * kPgoLanes + threadIdx.x;
  if (l < static_cast<size_t>(6 * g.N) * cov.ncols) pgo_cov_residual(g, cov, l);
}

__global__ __launch_bounds__(kPgoLanes) void pgo_cov_joint_kernel(const PgoGraph g, const PgoCov cov)
{
  if (!g.st->ok) return;
  const int l = static_cast<int>(blockIdx.x) * kPgoLanes + static_cast<int>(threadIdx.x);
  if (l < 144 * cov.n_pairs) pgo_cov_joint(g, cov, l);
}

// the whole chain of a covariance call behind whatever is on the stream (g.st zeroed by the caller)
hipError_t launch_pgo_covariances(const PgoGraph & g, const PgoParams & p, const PgoCov & cov, hipStream_t stream)
{
  if (g.N < 1 || g.N > kPgoMaxPoses || g.E < 0 || g.E > kPgoMaxEdges || g.P < 0 || g.P > kPgoMaxPoses || g.F < 0 || g.F > kPgoFarMax || g.K != 6 * g.F + 1 ||
      cov.n_pairs < 0 || cov.n_pairs > kPgoCovPairsMax || cov.ncols != 6 * cov.n_pairs)
    return hipErrorInvalidValue;
  hipError_t e = launch_pgo_edges(g, false, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pgo_gather_kernel, dim3((kPgoGather * g.N + kPgoLanes - 1) / kPgoLanes), dim3(kPgoLanes), 0, stream, g, p);
  hipLaunchKernelGGL(pgo_factor_kernel, dim3(1), dim3(64), 0, stream, g);
  hipLaunchKernelGGL(pgo_sweep_kernel, dim3((g.K + 63) / 64), dim3(64), 0, stream, g, 0);
  if (g.F > 0) hipLaunchKernelGGL(pgo_small_kernel, dim3(1), dim3(kPgoLanes), 0, stream, g, 0);
  hipLaunchKernelGGL(pgo_cov_chain_kernel, dim3(1), dim3(64), 0, stream, g, cov);
  hipLaunchKernelGGL(pgo_cov_correct_kernel, dim3(g.N), dim3(64), 0, stream, g, cov);
  if (cov.n_pairs > 0) {
    const dim3 cols((cov.ncols + 63) / 64);
    const dim3 entries(static_cast<unsigned>((static_cast<size_t>(6 * g.N) * cov.ncols + kPgoLanes - 1) / kPgoLanes));
    for (int step = 0; step < 3; ++step) {
      if (step > 0) hipLaunchKernelGGL(pgo_cov_residual_kernel, entries, dim3(kPgoLanes), 0, stream, g, cov);
      hipLaunchKernelGGL(pgo_cov_sweep_kernel, cols, dim3(64), 0, stream, g, cov, step == 0 ? 1 : 0);
      if (g.F > 0) hipLaunchKernelGGL(pgo_cov_solve_kernel, cols, dim3(64), 0, stream, g, cov);
      hipLaunchKernelGGL(pgo_cov_apply_kernel, entries, dim3(kPgoLanes), 0, stream, g, cov, step == 0 ? 1 : 0);
    }
    hipLaunchKernelGGL(pgo_cov_joint_kernel, dim3((144 * cov.n_pairs + kPgoLanes - 1) / kPgoLanes), dim3(kPgoLanes), 0, stream, g, cov);
  }
  return hipGetLastError();
}

}  // namespace mh
