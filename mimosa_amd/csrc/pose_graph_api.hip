// Pose-graph entry points of the C ABI (include/mimosa_hip.h): mh_pose_graph_*.  The kernels are pose_graph_kernels.hip, the
// arithmetic pose_graph_device.hpp.  Everything runs on the context's stream; mh_pose_graph_optimise queues its iterations
// (all of them, or check_every at a time, looking at the last queued iteration's flagged word in between) and ends in one wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "flagged_word.hpp"
#include "mh_internal.hpp"
#include "pose_graph_device.hpp"

static_assert(sizeof(mh_pose_graph_config) == 32 && sizeof(mh_pose_graph_trace) == 32 && sizeof(mh_pose_graph_result) == 32 + 64 * 32, "mh_pose_graph_* layout");
static_assert(sizeof(mh_pose_prior) == 392 && sizeof(mh_pose_graph_loss) == 16, "mh_pose_prior, mh_pose_graph_loss layout");
static_assert(MH_PGO_LOSS_NONE == mh::kPgoLossNone && MH_PGO_LOSS_HUBER == mh::kPgoLossHuber && MH_PGO_LOSS_CAUCHY == mh::kPgoLossCauchy &&
                MH_PGO_LOSS_DCS == mh::kPgoLossDcs,
              "MH_PGO_LOSS_*");
static_assert(sizeof(mh_pose_graph_cov_info) == 16 && MH_PGO_COV_PAIRS_MAX == mh::kPgoCovPairsMax, "mh_pose_graph_cov_info layout");
static_assert(MH_PGO_MAX_POSES == mh::kPgoMaxPoses && MH_PGO_MAX_EDGES == mh::kPgoMaxEdges && MH_PGO_FAR_MAX == mh::kPgoFarMax && MH_PGO_FAR_LIMIT == mh::kPgoFarLimit &&
                mh::kPgoMaxIters == 64,
              "mh_pose_graph_* constants");

namespace mh
{
hipError_t launch_pgo_edges(const PgoGraph & g, bool want_res, hipStream_t stream);
hipError_t launch_pgo_cost(const PgoGraph & g, bool chi2, hipStream_t stream);
hipError_t launch_pgo_iteration(const PgoGraph & g, const PgoParams & p, int it, double * trace, uint4 * word, unsigned int seq, hipStream_t stream, int far_cap,
                                bool wide);
hipError_t launch_pgo_covariances(const PgoGraph & g, const PgoParams & p, const PgoCov & cov, hipStream_t stream);
}  // namespace mh

struct mh_pose_graph final : CtxOwned
{
  size_t max_poses = 0, max_edges = 0;
  size_t max_far = MH_PGO_FAR_MAX;  // far edges the arrays are laid out for
  bool wide = false;                // mh_pose_graph_create_wide: C in blocks (launch_pgo_iteration)
  size_t n = 0, n_edges = 0, n_far = 0, n_priors = 0;
  size_t off[mh::kPgArrays] = {};
  mh::PgoGraph g{};          // device pointers into mem.block
  // what goes back when the context does
  struct Memory
  {
    DevBuf block;     // every array of mh::PgoGraph (pgo_layout)
    DevBuf trace;     // double, iters x n x 12: the poses behind every step (grown on demand)
    DevBuf cov;       // mh_pose_graph_covariances (allocated at its first call): P and Sigma_ii (36 max_poses each), joint, pairs
    DevBuf cov_cols;  // ... the pairs' columns X, Z (6 n x 6 n_pairs each) and U (6 F x 6 n_pairs), grown on demand
    PinnedBuf h_out;  // pinned staging of whatever a call hands to the host (grown on demand)
  } mem;
  uint4 * h_words = nullptr;  // one flagged word per iteration (mapped pinned, zeroed at create) and its device-side address
  uint4 * d_words = nullptr;
  unsigned int seq = 0;
  char * h_out() const { return mem.h_out.as<char>(); }
  void ctx_gone() override
  {
    mem = Memory{};
    if (h_words) (void)hipHostFree(h_words);
    h_words = d_words = nullptr;
    n = n_edges = n_far = n_priors = 0;
  }
  ~mh_pose_graph() { ctx_gone(); }
};

namespace
{
// every entry point but destroy: a graph whose context was shut down
int pgo_alive(const mh_pose_graph * pg, const char * who) { return ctx_alive(pg, who, "graph"); }

// (every call that used the block has waited)
int pgo_host(mh_pose_graph * pg, size_t bytes)
{
  MH_HIP(pg->ctx, pg->mem.h_out.reserve(bytes));
  return MH_OK;
}

// host -> device behind everything on the stream, through the pinned block at `at`
template <typename T>
hipError_t pgo_up(mh_pose_graph * pg, size_t & at, T * dst, const T * src, size_t count)
{
  if (!count) return hipSuccess;
  std::memcpy(pg->h_out() + at, src, count * sizeof(T));
  const hipError_t e = hipMemcpyAsync(dst, pg->h_out() + at, count * sizeof(T), hipMemcpyHostToDevice, pg->ctx->stream);
  at += (count * sizeof(T) + 15) / 16 * 16;
  return e;
}

int pgo_create(mh_ctx * ctx, size_t max_poses, size_t max_edges, size_t max_far, bool wide, mh_pose_graph ** out)
{
  MH_HIP(ctx, mh_enter(ctx));
  mh_pose_graph * pg = new mh_pose_graph;
  pg->max_poses = max_poses;
  pg->max_edges = max_edges;
  pg->max_far = max_far;
  pg->wide = wide;
  const size_t bytes = mh::pgo_layout(max_poses, std::max<size_t>(max_edges, 1), pg->off, max_far);
  hipError_t e = pg->mem.block.alloc(bytes);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&pg->h_words), mh::kPgoMaxIters * sizeof(uint4), hipHostMallocMapped);
  if (e == hipSuccess) {
    std::memset(pg->h_words, 0, mh::kPgoMaxIters * sizeof(uint4));
    e = hipHostGetDevicePointer(reinterpret_cast<void **>(&pg->d_words), pg->h_words, 0);
  }
  mh::pgo_bind(pg->g, pg->mem.block.as<char>(), pg->off);
  // no loss on any term until mh_pose_graph_set_loss says otherwise
  if (e == hipSuccess) e = hipMemsetAsync(pg->g.lkind, 0, std::max<size_t>(max_edges, 1) * sizeof(int), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(pg->g.plkind, 0, max_poses * sizeof(int), ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    delete pg;
    return hip_fail(ctx, e, wide ? "mh_pose_graph_create_wide" : "mh_pose_graph_create");
  }
  ctx_register(pg, ctx);
  *out = pg;
  return MH_OK;
}

// the graph without edges: every pose's incidence list empty
int pgo_drop_edges(mh_pose_graph * pg)
{
  pg->n_edges = pg->n_far = 0;
  MH_HIP(pg->ctx, hipMemsetAsync(pg->g.inc_off, 0, (pg->n + 1) * sizeof(int), pg->ctx->stream));
  return MH_OK;
}

int pgo_check_edges(const mh_pose_graph * pg, const mh_window_edge * edges, size_t n_edges, size_t & n_far)
{
  const mh_ctx * ctx = pg->ctx;
  if (n_edges > pg->max_edges) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_edges: more edges than the graph was created for");
  n_far = 0;
  for (size_t e = 0; e < n_edges; ++e) {
    const mh_window_edge & q = edges[e];
    if (q.pose_a < 0 || q.pose_a >= q.pose_b || static_cast<size_t>(q.pose_b) >= pg->n)
      return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_edges: edge " + std::to_string(e) + " needs 0 <= pose_a < pose_b < n");
    if (!window_edge_finite(q)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_edges: edge " + std::to_string(e) + " has an entry that is not finite");
    if (!exactly_symmetric(q.info, 6, 6)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_edges: an edge's info is not symmetric");
    if (q.pose_b - q.pose_a >= 2) ++n_far;
  }
  if (!pg->wide && n_far > MH_PGO_FAR_MAX)
    return fail(ctx, MH_ERR_UNSUPPORTED, "mh_pose_graph_set_edges: more than MH_PGO_FAR_MAX edges with pose_b - pose_a >= 2");
  if (n_far > pg->max_far)
    return fail(ctx, MH_ERR_UNSUPPORTED, "mh_pose_graph_set_edges: more than max_far (" + std::to_string(pg->max_far) + ") edges with pose_b - pose_a >= 2");
  return MH_OK;
}

int pgo_set_edges(mh_pose_graph * pg, const mh_window_edge * edges, size_t E, size_t n_far)
{
  mh_ctx * ctx = pg->ctx;
  const size_t N = pg->n;
  std::vector<int> ea(E), eb(E), slot(E), inc_off(N + 1, 0), inc(2 * E), far(n_far);
  std::vector<double> ZR(9 * E), Zt(3 * E), Om(36 * E);
  for (size_t e = 0; e < E; ++e) {
    const mh_window_edge & q = edges[e];
    ea[e] = q.pose_a;
    eb[e] = q.pose_b;
    std::memcpy(&ZR[9 * e], q.Z_R, sizeof(q.Z_R));
    std::memcpy(&Zt[3 * e], q.Z_t, sizeof(q.Z_t));
    std::memcpy(&Om[36 * e], q.info, sizeof(q.info));
  }
  far.resize(pg->max_far);
  (void)mh::pgo_index_edges(static_cast<int>(N), static_cast<int>(E), ea.data(), eb.data(), slot.data(), inc_off.data(), inc.data(), far.data(),
                            static_cast<int>(pg->max_far));
  MH_HIP(ctx, mh_enter(ctx));
  const int rc = pgo_host(pg, (48 * E + 5 * E + N + 1 + n_far) * 8 + 16 * 16);
  if (rc != MH_OK) return rc;
  size_t at = 0;
  const mh::PgoGraph & g = pg->g;
  hipError_t e = hipMemsetAsync(g.lkind, 0, std::max<size_t>(E, 1) * sizeof(int), ctx->stream);  // the edges' losses go with the list
  if (e == hipSuccess) e = pgo_up(pg, at, g.ea, ea.data(), E);
  if (e == hipSuccess) e = pgo_up(pg, at, g.eb, eb.data(), E);
  if (e == hipSuccess) e = pgo_up(pg, at, g.eslot, slot.data(), E);
  if (e == hipSuccess) e = pgo_up(pg, at, g.inc_off, inc_off.data(), N + 1);
  if (e == hipSuccess) e = pgo_up(pg, at, g.inc, inc.data(), 2 * E);
  if (e == hipSuccess) e = pgo_up(pg, at, g.far, far.data(), n_far);
  if (e == hipSuccess) e = pgo_up(pg, at, g.ZR, ZR.data(), 9 * E);
  if (e == hipSuccess) e = pgo_up(pg, at, g.Zt, Zt.data(), 3 * E);
  if (e == hipSuccess) e = pgo_up(pg, at, g.Om, Om.data(), 36 * E);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // (the pinned block is the next call's too)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    pg->n_edges = pg->n_far = 0;  // what is on the device is not a graph any more
    return hip_fail(ctx, e, "mh_pose_graph_set_edges");
  }
  pg->n_edges = E;
  pg->n_far = n_far;
  return MH_OK;
}

mh::PgoGraph pgo_graph(const mh_pose_graph * pg)
{
  mh::PgoGraph g = pg->g;
  g.N = static_cast<int>(pg->n);
  g.E = static_cast<int>(pg->n_edges);
  g.F = static_cast<int>(pg->n_far);
  g.K = 6 * g.F + 1;
  g.P = static_cast<int>(pg->n_priors);
  return g;
}

// the word of iteration `it`: its flags once they have arrived
bool pgo_read_word(const mh_pose_graph * pg, int it, unsigned int seq, long spin_ns, int & flags)
{
  double v = 0.0;
  if (!mh::spin_until([&] { return mh::ll_read(reinterpret_cast<const uint64_t *>(pg->h_words + it), seq, v); }, spin_ns)) return false;
  flags = static_cast<int>(v);
  return true;
}

int pgo_optimise(mh_pose_graph * pg, const mh_pose_graph_config * cfg, mh_pose_graph_result * out, double * trace_poses)
{
  mh_ctx * ctx = pg->ctx;
  const size_t N = pg->n;
  const int iters = cfg->iters, chunk = cfg->check_every > 0 ? cfg->check_every : iters;
  MH_HIP(ctx, mh_enter(ctx));
  const size_t pose_bytes = 12 * N * sizeof(double), head = sizeof(mh::PgoState) + mh::kPgoMaxIters * sizeof(mh::PgoRow);
  const size_t trace_bytes = trace_poses ? static_cast<size_t>(iters) * pose_bytes : 0;
  int rc = pgo_host(pg, head + trace_bytes);
  if (rc != MH_OK) return rc;
  if (trace_bytes > pg->mem.trace.cap) MH_HIP(ctx, pg->mem.trace.alloc(trace_bytes));
  double * const d_trace = pg->mem.trace.as<double>();
  const mh::PgoGraph g = pgo_graph(pg);
  const mh::PgoParams p{cfg->damping, cfg->eps_rot, cfg->eps_trans};
  unsigned int seq[mh::kPgoMaxIters];
  for (int i = 0; i < iters; ++i) {
    if (++pg->seq == 0u) ++pg->seq;
    seq[i] = pg->seq;
  }
  hipError_t e = hipMemsetAsync(g.st, 0, sizeof(mh::PgoState), ctx->stream);
  int queued = 0, flags = 0;
  while (e == hipSuccess && queued < iters && !(flags & 1)) {
    const int upto = std::min(queued + chunk, iters);
    for (; e == hipSuccess && queued < upto; ++queued)
      e = mh::launch_pgo_iteration(g, p, queued, trace_poses ? d_trace + static_cast<size_t>(queued) * 12 * N : nullptr, pg->d_words + queued,
                                   seq[queued], ctx->stream, static_cast<int>(pg->max_far), pg->wide);
    if (e != hipSuccess || queued == iters) break;
    // the last queued iteration's word: the value itself, then the stream behind it
    if (!pgo_read_word(pg, queued - 1, seq[queued - 1], 50000000L, flags)) {
      e = hipStreamSynchronize(ctx->stream);
      if (e == hipSuccess && !pgo_read_word(pg, queued - 1, seq[queued - 1], 2000000L, flags)) {
        return fail(ctx, MH_ERR_HIP, "mh_pose_graph_optimise: the stream drained without the chain's results");
      }
    }
  }
  if (e == hipSuccess) e = hipMemcpyAsync(pg->h_out(), g.st, sizeof(mh::PgoState), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(pg->h_out() + sizeof(mh::PgoState), g.rows, mh::kPgoMaxIters * sizeof(mh::PgoRow), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && trace_poses)
    e = hipMemcpyAsync(pg->h_out() + head, d_trace, static_cast<size_t>(queued) * pose_bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return hip_fail(ctx, e, "mh_pose_graph_optimise");
  }
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mh::PgoState st;
  std::memcpy(&st, pg->h_out(), sizeof(st));
  const mh::PgoRow * rows = reinterpret_cast<const mh::PgoRow *>(pg->h_out() + sizeof(mh::PgoState));
  if (st.iters < 1 || st.iters > queued) return fail(ctx, MH_ERR_HIP, "mh_pose_graph_optimise: the chain left no result");
  std::memset(out, 0, sizeof(*out));
  out->iters = st.iters;
  out->converged = st.converged;
  out->n_poses = static_cast<int32_t>(N);
  out->n_far = static_cast<int32_t>(pg->n_far);
  for (int i = 0; i < st.iters; ++i) {
    out->trace[i].f = rows[i].f;
    out->trace[i].step_rot = rows[i].step_rot;
    out->trace[i].step_trans = rows[i].step_trans;
    out->trace[i].flags = rows[i].flags & 4;
  }
  out->f_first = rows[0].f;
  out->f_last = rows[st.iters - 1].f;
  if (trace_poses) std::memcpy(trace_poses, pg->h_out() + head, static_cast<size_t>(st.iters) * pose_bytes);
  return MH_OK;
}

int pgo_residuals(mh_pose_graph * pg, double * r, double * chi2, double * f)
{
  mh_ctx * ctx = pg->ctx;
  const size_t E = pg->n_edges;
  MH_HIP(ctx, mh_enter(ctx));
  const int rc = pgo_host(pg, 16 + 7 * E * sizeof(double));
  if (rc != MH_OK) return rc;
  mh::PgoGraph g = pgo_graph(pg);
  g.P = 0;  // the edges alone
  hipError_t e = hipMemsetAsync(g.st, 0, sizeof(mh::PgoState), ctx->stream);
  if (e == hipSuccess) e = mh::launch_pgo_edges(g, true, ctx->stream);
  if (e == hipSuccess) e = mh::launch_pgo_cost(g, true, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(pg->h_out(), &g.rows[0].f, sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && E) e = hipMemcpyAsync(pg->h_out() + 16, g.res, 6 * E * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && E) e = hipMemcpyAsync(pg->h_out() + 16 + 6 * E * sizeof(double), g.cz, E * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return hip_fail(ctx, e, "mh_pose_graph_residuals");
  }
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (f) std::memcpy(f, pg->h_out(), sizeof(double));
  if (r && E) std::memcpy(r, pg->h_out() + 16, 6 * E * sizeof(double));
  if (chi2 && E) std::memcpy(chi2, pg->h_out() + 16 + 6 * E * sizeof(double), E * sizeof(double));
  return MH_OK;
}

// rule 10: the system as an iteration assembles it, up to C's factor; the chain, the correction, the pairs' columns; one wait
int pgo_covariances(mh_pose_graph * pg, double damping, double * cov, const int32_t * pairs, size_t n_pairs, double * joint, mh_pose_graph_cov_info * info)
{
  mh_ctx * ctx = pg->ctx;
  const size_t N = pg->n, D = sizeof(double), ncols = 6 * n_pairs;
  MH_HIP(ctx, mh_enter(ctx));
  const size_t at_pairs = 16, at_cov = at_pairs + 2 * mh::kPgoCovPairsMax * sizeof(int), at_joint = at_cov + 36 * N * D;
  const int rc = pgo_host(pg, at_joint + 144 * n_pairs * D);
  if (rc != MH_OK) return rc;
  // the fixed part: P, Sigma_ii, joint, pairs
  const size_t off_S = 36 * pg->max_poses * D, off_joint = 2 * off_S, off_pairs = off_joint + 144 * mh::kPgoCovPairsMax * D;
  if (!pg->mem.cov.p) MH_HIP(ctx, pg->mem.cov.alloc(off_pairs + 2 * mh::kPgoCovPairsMax * sizeof(int)));
  const size_t col = 6 * N * ncols * D, ucol = 6 * pg->n_far * ncols * D;
  if (n_pairs) MH_HIP(ctx, pg->mem.cov_cols.reserve(2 * col + ucol, ctx->stream, false));
  const mh::PgoGraph g = pgo_graph(pg);
  const mh::PgoParams p{damping, 0.0, 0.0};
  char * const base = pg->mem.cov.as<char>();
  mh::PgoCov c{};
  c.n_pairs = static_cast<int>(n_pairs);
  c.ncols = static_cast<int>(ncols);
  c.P = reinterpret_cast<double *>(base);
  c.S = reinterpret_cast<double *>(base + off_S);
  c.joint = reinterpret_cast<double *>(base + off_joint);
  c.pairs = reinterpret_cast<int *>(base + off_pairs);
  if (n_pairs) {
    c.X = pg->mem.cov_cols.as<double>();
    c.Z = c.X + 6 * N * ncols;
    c.U = c.Z + 6 * N * ncols;
  }
  hipError_t e = hipMemsetAsync(g.st, 0, sizeof(mh::PgoState), ctx->stream);
  size_t at = at_pairs;
  if (e == hipSuccess && n_pairs) e = pgo_up(pg, at, c.pairs, pairs, 2 * n_pairs);
  if (e == hipSuccess) e = mh::launch_pgo_covariances(g, p, c, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(pg->h_out(), g.st, sizeof(mh::PgoState), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(pg->h_out() + at_cov, c.S, 36 * N * D, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && n_pairs) e = hipMemcpyAsync(pg->h_out() + at_joint, c.joint, 144 * n_pairs * D, hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return hip_fail(ctx, e, "mh_pose_graph_covariances");
  }
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mh::PgoState st;
  std::memcpy(&st, pg->h_out(), sizeof(st));
  info->n_poses = static_cast<int32_t>(N);
  info->n_far = static_cast<int32_t>(pg->n_far);
  info->n_pairs = static_cast<int32_t>(n_pairs);
  info->flags = st.ok ? 0 : 4;
  if (!st.ok) return MH_OK;  // (what the kernels behind the failed pivot left on the device is not a result: nothing is handed out)
  if (cov) std::memcpy(cov, pg->h_out() + at_cov, 36 * N * D);
  if (joint && n_pairs) std::memcpy(joint, pg->h_out() + at_joint, 144 * n_pairs * D);
  return MH_OK;
}

bool pgo_prior_finite(const mh_pose_prior & q)
{
  for (double v : q.Z_R)
    if (!std::isfinite(v)) return false;
  for (double v : q.Z_t)
    if (!std::isfinite(v)) return false;
  for (double v : q.info)
    if (!std::isfinite(v)) return false;
  return true;
}

int pgo_check_priors(const mh_pose_graph * pg, const mh_pose_prior * priors, size_t P)
{
  const mh_ctx * ctx = pg->ctx;
  if (P > pg->max_poses) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_priors: more priors than max_poses");
  for (size_t p = 0; p < P; ++p) {
    const mh_pose_prior & q = priors[p];
    if (q.pose < 0 || static_cast<size_t>(q.pose) >= pg->n)
      return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_priors: prior " + std::to_string(p) + " needs 0 <= pose < n");
    if (!pgo_prior_finite(q)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_priors: prior " + std::to_string(p) + " has an entry that is not finite");
    if (!exactly_symmetric(q.info, 6, 6)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_priors: a prior's info is not symmetric");
  }
  return MH_OK;
}

int pgo_set_priors(mh_pose_graph * pg, const mh_pose_prior * priors, size_t P)
{
  mh_ctx * ctx = pg->ctx;
  const size_t N = pg->n;
  std::vector<int> pose(P), pinc_off(N + 1, 0), pinc(P);
  std::vector<double> ZR(9 * P), Zt(3 * P), Om(36 * P);
  for (size_t p = 0; p < P; ++p) {
    const mh_pose_prior & q = priors[p];
    pose[p] = q.pose;
    std::memcpy(&ZR[9 * p], q.Z_R, sizeof(q.Z_R));
    std::memcpy(&Zt[3 * p], q.Z_t, sizeof(q.Z_t));
    std::memcpy(&Om[36 * p], q.info, sizeof(q.info));
  }
  mh::pgo_index_priors(static_cast<int>(N), static_cast<int>(P), pose.data(), pinc_off.data(), pinc.data());
  MH_HIP(ctx, mh_enter(ctx));
  const int rc = pgo_host(pg, (48 * P + P + N + 1) * 8 + 8 * 16);
  if (rc != MH_OK) return rc;
  size_t at = 0;
  const mh::PgoGraph & g = pg->g;
  hipError_t e = hipMemsetAsync(g.plkind, 0, pg->max_poses * sizeof(int), ctx->stream);  // the priors' losses go with the list
  if (e == hipSuccess) e = pgo_up(pg, at, g.ppose, pose.data(), P);
  if (e == hipSuccess) e = pgo_up(pg, at, g.pinc_off, pinc_off.data(), N + 1);
  if (e == hipSuccess) e = pgo_up(pg, at, g.pinc, pinc.data(), P);
  if (e == hipSuccess) e = pgo_up(pg, at, g.pZR, ZR.data(), 9 * P);
  if (e == hipSuccess) e = pgo_up(pg, at, g.pZt, Zt.data(), 3 * P);
  if (e == hipSuccess) e = pgo_up(pg, at, g.pOm, Om.data(), 36 * P);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // (the pinned block is the next call's too)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    pg->n_priors = 0;  // what is on the device is not a prior list any more
    return hip_fail(ctx, e, "mh_pose_graph_set_priors");
  }
  pg->n_priors = P;
  return MH_OK;
}

int pgo_check_loss(const mh_ctx * ctx, const mh_pose_graph_loss * loss, size_t n, const char * what)
{
  for (size_t k = 0; loss && k < n; ++k) {
    if (loss[k].kind < MH_PGO_LOSS_NONE || loss[k].kind > MH_PGO_LOSS_DCS)
      return fail(ctx, MH_ERR_INVALID_ARG, std::string("mh_pose_graph_set_loss: ") + what + " " + std::to_string(k) + " has a kind outside 0 .. 3");
    if (loss[k].kind != MH_PGO_LOSS_NONE && !(std::isfinite(loss[k].param) && loss[k].param > 0.0))
      return fail(ctx, MH_ERR_INVALID_ARG, std::string("mh_pose_graph_set_loss: ") + what + " " + std::to_string(k) + " needs a finite param > 0");
  }
  return MH_OK;
}

// one list of losses: kinds and params of n terms, or no loss on any of them
hipError_t pgo_up_loss(mh_pose_graph * pg, size_t & at, const mh_pose_graph_loss * loss, size_t n, int * kind, double * param)
{
  if (!loss || !n) return hipMemsetAsync(kind, 0, std::max<size_t>(n, 1) * sizeof(int), pg->ctx->stream);
  std::vector<int> k(n);
  std::vector<double> v(n);
  for (size_t i = 0; i < n; ++i) {
    k[i] = loss[i].kind;
    v[i] = loss[i].kind != MH_PGO_LOSS_NONE ? loss[i].param : 1.0;
  }
  hipError_t e = pgo_up(pg, at, kind, k.data(), n);
  if (e == hipSuccess) e = pgo_up(pg, at, param, v.data(), n);
  return e;
}

int pgo_set_loss(mh_pose_graph * pg, const mh_pose_graph_loss * edges, const mh_pose_graph_loss * priors)
{
  mh_ctx * ctx = pg->ctx;
  MH_HIP(ctx, mh_enter(ctx));
  const int rc = pgo_host(pg, (pg->n_edges + pg->n_priors) * 16 + 4 * 16);
  if (rc != MH_OK) return rc;
  size_t at = 0;
  hipError_t e = pgo_up_loss(pg, at, edges, pg->n_edges, pg->g.lkind, pg->g.lparam);
  if (e == hipSuccess) e = pgo_up_loss(pg, at, priors, pg->n_priors, pg->g.plkind, pg->g.plparam);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_fail(ctx, e, "mh_pose_graph_set_loss");
  return MH_OK;
}

// every term at the stored poses, for mh_pose_graph_prior_residuals (d, chi2) and mh_pose_graph_weights (w_edges, w_priors, f)
int pgo_evaluate(mh_pose_graph * pg, const char * who, double * d, double * chi2, double * w_edges, double * w_priors, double * f)
{
  mh_ctx * ctx = pg->ctx;
  const size_t E = pg->n_edges, P = pg->n_priors, D = sizeof(double);
  MH_HIP(ctx, mh_enter(ctx));
  const int rc = pgo_host(pg, 16 + (E + 8 * P) * D);
  if (rc != MH_OK) return rc;
  const mh::PgoGraph g = pgo_graph(pg);
  char * const h_w = pg->h_out() + 16, * const h_pw = h_w + E * D, * const h_d = h_pw + P * D, * const h_c = h_d + 6 * P * D;
  hipError_t e = hipMemsetAsync(g.st, 0, sizeof(mh::PgoState), ctx->stream);
  if (e == hipSuccess) e = mh::launch_pgo_edges(g, false, ctx->stream);
  if (e == hipSuccess) e = mh::launch_pgo_cost(g, false, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(pg->h_out(), &g.rows[0].f, D, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && E) e = hipMemcpyAsync(h_w, g.w, E * D, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && P) e = hipMemcpyAsync(h_pw, g.pw, P * D, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && P) e = hipMemcpyAsync(h_d, g.pres, 6 * P * D, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && P) e = hipMemcpyAsync(h_c, g.pcz, P * D, hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return hip_fail(ctx, e, who);
  }
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (f) std::memcpy(f, pg->h_out(), D);
  if (w_edges && E) std::memcpy(w_edges, h_w, E * D);
  if (w_priors && P) std::memcpy(w_priors, h_pw, P * D);
  if (d && P) std::memcpy(d, h_d, 6 * P * D);
  if (chi2 && P) std::memcpy(chi2, h_c, P * D);
  return MH_OK;
}
}  // namespace

extern "C" {

int mh_pose_graph_create(mh_ctx * ctx, size_t max_poses, size_t max_edges, mh_pose_graph ** out)
{
  if (out) *out = nullptr;
  if (!out) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create: NULL argument");
  return guarded(ctx, "mh_pose_graph_create", [&]() -> int {
    // (before the context is looked at: sizes are refused the same way with and without one)
    if (max_poses < 1 || max_poses > MH_PGO_MAX_POSES) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create: max_poses must be in 1..4096");
    if (max_edges > MH_PGO_MAX_EDGES) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create: max_edges must be in 0..32768");
    if (!ctx) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create: NULL argument");
    return pgo_create(ctx, max_poses, max_edges, MH_PGO_FAR_MAX, false, out);
  });
}

int mh_pose_graph_create_wide(mh_ctx * ctx, size_t max_poses, size_t max_edges, size_t max_far, mh_pose_graph ** out)
{
  if (out) *out = nullptr;
  if (!out) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create_wide: NULL argument");
  return guarded(ctx, "mh_pose_graph_create_wide", [&]() -> int {
    if (max_poses < 1 || max_poses > MH_PGO_MAX_POSES) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create_wide: max_poses must be in 1..4096");
    if (max_edges > MH_PGO_MAX_EDGES) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create_wide: max_edges must be in 0..32768");
    if (max_far < 1 || max_far > MH_PGO_FAR_LIMIT) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create_wide: max_far must be in 1..512");
    if (!ctx) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_create_wide: NULL argument");
    return pgo_create(ctx, max_poses, max_edges, max_far, true, out);
  });
}

void mh_pose_graph_destroy(mh_pose_graph * pg)
{
  if (!pg) return;
  if (mh_ctx * ctx = pg->ctx) {
    (void)mh_enter(ctx);
    (void)hipStreamSynchronize(ctx->stream);  // the pinned blocks go back: nothing may still be copying into them
    ctx_unregister(pg);
  }
  delete pg;
}

int mh_pose_graph_set_poses(mh_pose_graph * pg, const double * R, const double * t, size_t n)
{
  if (!pg || !R || !t) return fail(pg ? pg->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_set_poses: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_set_poses", [&]() -> int {
    int rc = pgo_alive(pg, "mh_pose_graph_set_poses");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = pg->ctx;
    if (n < 1 || n > pg->max_poses) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_poses: n must be in 1..max_poses");
    for (size_t i = 0; i < 9 * n; ++i)
      if (!std::isfinite(R[i])) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_poses: R of pose " + std::to_string(i / 9) + " has an entry that is not finite");
    for (size_t i = 0; i < 3 * n; ++i)
      if (!std::isfinite(t[i])) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_poses: t of pose " + std::to_string(i / 3) + " has an entry that is not finite");
    MH_HIP(ctx, mh_enter(ctx));
    if ((rc = pgo_host(pg, 12 * n * sizeof(double) + 32)) != MH_OK) return rc;
    size_t at = 0;
    MH_HIP(ctx, pgo_up(pg, at, pg->g.R, R, 9 * n));
    MH_HIP(ctx, pgo_up(pg, at, pg->g.t, t, 3 * n));
    if (n != pg->n) {  // another graph: its edges, fixed poses, priors and losses are the caller's to set again
      pg->n = n;
      pg->n_priors = 0;
      MH_HIP(ctx, hipMemsetAsync(pg->g.fixed, 0, n, ctx->stream));
      if ((rc = pgo_drop_edges(pg)) != MH_OK) return rc;
    }
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the pinned block is the next call's too)
    return MH_OK;
  });
}

int mh_pose_graph_set_fixed(mh_pose_graph * pg, const uint8_t * fixed)
{
  if (!pg) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_set_fixed: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_set_fixed", [&]() -> int {
    int rc = pgo_alive(pg, "mh_pose_graph_set_fixed");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = pg->ctx;
    if (pg->n == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_fixed: no poses have been set");
    MH_HIP(ctx, mh_enter(ctx));
    if (!fixed) {
      MH_HIP(ctx, hipMemsetAsync(pg->g.fixed, 0, pg->n, ctx->stream));
      return MH_OK;
    }
    if ((rc = pgo_host(pg, pg->n + 16)) != MH_OK) return rc;
    std::vector<unsigned char> f(pg->n);
    for (size_t i = 0; i < pg->n; ++i) f[i] = fixed[i] ? 1 : 0;
    size_t at = 0;
    MH_HIP(ctx, pgo_up(pg, at, pg->g.fixed, f.data(), pg->n));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MH_OK;
  });
}

int mh_pose_graph_set_edges(mh_pose_graph * pg, const mh_window_edge * edges, size_t n_edges)
{
  if (!pg || (!edges && n_edges)) return fail(pg ? pg->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_set_edges: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_set_edges", [&]() -> int {
    int rc = pgo_alive(pg, "mh_pose_graph_set_edges");
    if (rc != MH_OK) return rc;
    if (pg->n == 0) return fail(pg->ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_edges: no poses have been set");
    size_t n_far = 0;
    if ((rc = pgo_check_edges(pg, edges, n_edges, n_far)) != MH_OK) return rc;
    return pgo_set_edges(pg, edges, n_edges, n_far);
  });
}

int mh_pose_graph_set_priors(mh_pose_graph * pg, const mh_pose_prior * priors, size_t n)
{
  if (!pg || (!priors && n)) return fail(pg ? pg->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_set_priors: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_set_priors", [&]() -> int {
    int rc = pgo_alive(pg, "mh_pose_graph_set_priors");
    if (rc != MH_OK) return rc;
    if (pg->n == 0) return fail(pg->ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_priors: no poses have been set");
    if ((rc = pgo_check_priors(pg, priors, n)) != MH_OK) return rc;
    return pgo_set_priors(pg, priors, n);
  });
}

int mh_pose_graph_set_loss(mh_pose_graph * pg, const mh_pose_graph_loss * edges, const mh_pose_graph_loss * priors)
{
  if (!pg) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_set_loss: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_set_loss", [&]() -> int {
    int rc = pgo_alive(pg, "mh_pose_graph_set_loss");
    if (rc != MH_OK) return rc;
    const mh_ctx * ctx = pg->ctx;
    if (pg->n == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_loss: no poses have been set");
    if (edges && pg->n_edges == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_set_loss: no edges have been set");
    if ((rc = pgo_check_loss(ctx, edges, pg->n_edges, "edge")) != MH_OK) return rc;
    if ((rc = pgo_check_loss(ctx, priors, pg->n_priors, "prior")) != MH_OK) return rc;
    return pgo_set_loss(pg, edges, priors);
  });
}

int mh_pose_graph_prior_residuals(mh_pose_graph * pg, double * d, double * chi2)
{
  if (!pg) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_prior_residuals: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_prior_residuals", [&]() -> int {
    const int rc = pgo_alive(pg, "mh_pose_graph_prior_residuals");
    if (rc != MH_OK) return rc;
    if (pg->n == 0) return fail(pg->ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_prior_residuals: no poses have been set");
    return pgo_evaluate(pg, "mh_pose_graph_prior_residuals", d, chi2, nullptr, nullptr, nullptr);
  });
}

int mh_pose_graph_weights(mh_pose_graph * pg, double * w_edges, double * w_priors, double * f)
{
  if (!pg) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_weights: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_weights", [&]() -> int {
    const int rc = pgo_alive(pg, "mh_pose_graph_weights");
    if (rc != MH_OK) return rc;
    if (pg->n == 0) return fail(pg->ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_weights: no poses have been set");
    return pgo_evaluate(pg, "mh_pose_graph_weights", nullptr, nullptr, w_edges, w_priors, f);
  });
}

int mh_pose_graph_get_poses(mh_pose_graph * pg, double * R, double * t, size_t capacity, size_t * n_out)
{
  if (!pg) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_get_poses: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_get_poses", [&]() -> int {
    int rc = pgo_alive(pg, "mh_pose_graph_get_poses");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = pg->ctx;
    const size_t n = pg->n;
    if (n_out) *n_out = n;
    if (!R && !t) return MH_OK;
    if (capacity < n) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_get_poses: capacity is below the pose count");
    if (n == 0) return MH_OK;
    MH_HIP(ctx, mh_enter(ctx));
    if ((rc = pgo_host(pg, 12 * n * sizeof(double))) != MH_OK) return rc;
    MH_HIP(ctx, hipMemcpyAsync(pg->h_out(), pg->g.R, 9 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(pg->h_out() + 9 * n * sizeof(double), pg->g.t, 3 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (R) std::memcpy(R, pg->h_out(), 9 * n * sizeof(double));
    if (t) std::memcpy(t, pg->h_out() + 9 * n * sizeof(double), 3 * n * sizeof(double));
    return MH_OK;
  });
}

int mh_pose_graph_residuals(mh_pose_graph * pg, double * r, double * chi2, double * f)
{
  if (!pg) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_residuals: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_residuals", [&]() -> int {
    const int rc = pgo_alive(pg, "mh_pose_graph_residuals");
    if (rc != MH_OK) return rc;
    if (pg->n == 0) return fail(pg->ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_residuals: no poses have been set");
    return pgo_residuals(pg, r, chi2, f);
  });
}

int mh_pose_graph_covariances(mh_pose_graph * pg, double damping, double * cov, const int32_t * pairs, size_t n_pairs, double * joint,
                              mh_pose_graph_cov_info * info)
{
  if (!pg || !info) return fail(pg ? pg->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_covariances: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_covariances", [&]() -> int {
    const int rc = pgo_alive(pg, "mh_pose_graph_covariances");
    if (rc != MH_OK) return rc;
    const mh_ctx * ctx = pg->ctx;
    if (!cov && !joint) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_covariances: cov and joint are both NULL");
    if (n_pairs > MH_PGO_COV_PAIRS_MAX) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_covariances: n_pairs must be in 0..64");
    if (n_pairs && (!pairs || !joint)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_covariances: pairs and joint must be given with n_pairs > 0");
    if (!(damping >= 0.0) || !std::isfinite(damping)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_covariances: damping must be >= 0 and finite");
    if (pg->n == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_covariances: no poses have been set");
    if (pg->n_far > MH_PGO_FAR_MAX)
      return fail(ctx, MH_ERR_UNSUPPORTED, "mh_pose_graph_covariances: the graph holds more than MH_PGO_FAR_MAX edges with pose_b - pose_a >= 2");
    for (size_t p = 0; p < n_pairs; ++p)
      if (pairs[2 * p] < 0 || pairs[2 * p] >= pairs[2 * p + 1] || static_cast<size_t>(pairs[2 * p + 1]) >= pg->n)
        return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_covariances: pair " + std::to_string(p) + " needs 0 <= i < j < n");
    return pgo_covariances(pg, damping, cov, pairs, n_pairs, joint, info);
  });
}

int mh_pose_graph_optimise(mh_pose_graph * pg, const mh_pose_graph_config * cfg, mh_pose_graph_result * out, double * trace_poses)
{
  if (!pg || !cfg || !out) return fail(pg ? pg->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_pose_graph_optimise: NULL argument");
  return guarded(pg->ctx, "mh_pose_graph_optimise", [&]() -> int {
    const int rc = pgo_alive(pg, "mh_pose_graph_optimise");
    if (rc != MH_OK) return rc;
    const mh_ctx * ctx = pg->ctx;
    if (cfg->iters < 1 || cfg->iters > mh::kPgoMaxIters) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_optimise: iters must be in 1..64");
    const bool ok = cfg->damping >= 0.0 && cfg->eps_rot >= 0.0 && cfg->eps_trans >= 0.0 && cfg->check_every >= 0 && std::isfinite(cfg->damping) &&
                    std::isfinite(cfg->eps_rot) && std::isfinite(cfg->eps_trans);
    if (!ok) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_optimise: eps, damping and check_every must be >= 0 and finite");
    if (pg->n == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_pose_graph_optimise: no poses have been set");
    return pgo_optimise(pg, cfg, out, trace_poses);
  });
}

}  // extern "C"
