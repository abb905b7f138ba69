// The device-chain drivers of the C ABI (include/mimosa_hip.h): mh_icp_align[_async], mh_icp_align_batch[_async|_wait],
// mh_icp_window_optimise[_async], mh_icp_window_optimise_relin[_async], mh_icp_window_optimise_lin[_async],
// mh_icp_window_optimise_edges[_async], mh_icp_window_marginalise[_async], mh_icp_window_optimise_joint[_async],
// mh_icp_window_marginalise_joint[_async] and mh_icp_window_wait.  A chain is K3 (icp_kernels.hip), a step kernel
// (align_kernels.hip, window_kernels.hip, window_relin_kernels.hip, window_lin_kernels.hip, window_edge_kernels.hip,
// window_joint_kernels.hip; window_marginal_kernels.hip and window_joint_kernels.hip for the marginals),
// K3, step ... on the context's stream with one wait at its
// end; every step publishes a row of flagged words the host reads.  There are two families: the alignment chains (mh_icp_align
// is the chain of one member on the factor's own record and storage, mh_icp_align_batch the chain of up to 16 on the context's:
// one record, one layout, one driver) and the window calls.  What the two share is written once at the top; staging layout,
// the step launch and the decoding of a row are each family's own, argument checks each entry point's.  A factor in a chain is
// held (mh_internal.hpp: hold / let_go) until the chain is collected or abandoned.  The factor handle, linearize and the
// flagged words of a call live in mh_api.hip (mh_internal.hpp: mhi); what a window entry point was given and the checks of it
// that need no device in window_request.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "mh_internal.hpp"

// (The block of an alignment chain, a function of its capacity, stands with its record: AlignChain in mh_internal.hpp.)
// mh_icp_window_optimise's block of device memory (mh_ctx::d_window) and the pinned staging of its first part (h_window):
// [grid prefixes, 256 B | WindowState | iters x n_slots argument blocks | 256 B that load_uniform may read past the last block |
//  one landing slot of 32 flagged words per pose for K3's sums and counters (every iteration's words carry its own number) |
//  WindowRelin, which the steps of an mh_icp_window_optimise_relin chain keep among themselves |
//  WindowLinear, the linear factors of an mh_icp_window_optimise_lin call (staged behind the first part in h_window) |
//  WindowEdges, the edges of an mh_icp_window_optimise_edges call (staged behind WindowLinear) |
//  WindowJoint, the joint factor of an mh_icp_window_optimise_joint / mh_icp_window_marginalise_joint call (staged behind WindowEdges)]
constexpr size_t kWinStateAt = 256;
constexpr size_t kWinBlocksAt = 3584;
constexpr size_t kWinStageBytes = kWinBlocksAt + sizeof(mh::IcpArgs) * mh::kWindowMax * kMaxPending;
constexpr size_t kWinLlAt = (kWinStageBytes + 256 + 255) & ~size_t(255);
constexpr size_t kWinRelinAt = kWinLlAt + 32 * sizeof(uint4) * mh::kWindowMax;
constexpr size_t kWinLinAt = kWinRelinAt + ((sizeof(mh::WindowRelin) + 255) & ~size_t(255));
constexpr size_t kWinEdgeAt = kWinLinAt + ((sizeof(mh::WindowLinear) + 255) & ~size_t(255));
constexpr size_t kWinJointAt = kWinEdgeAt + ((sizeof(mh::WindowEdges) + 255) & ~size_t(255));
constexpr size_t kWinBytes = kWinJointAt + ((sizeof(mh::WindowJoint) + 255) & ~size_t(255));
constexpr size_t kWinStageEdgeAt = kWinStageBytes + ((sizeof(mh::WindowLinear) + 255) & ~size_t(255));  // in h_window
constexpr size_t kWinStageJointAt = kWinStageEdgeAt + ((sizeof(mh::WindowEdges) + 255) & ~size_t(255));
static_assert(MH_WINDOW_JOINT_POSES == mh::kWindowJointMax && kWinJointAt % 16 == 0 && kWinStageJointAt % 16 == 0 &&
                mh::kWJMargWords <= static_cast<int>(256 * kMaxPending), "mh_icp_window_optimise_joint layout");
static_assert(MH_WINDOW_EDGE_MAX == mh::kWindowEdgeMax && kWinEdgeAt % 16 == 0 && kWinStageEdgeAt % 16 == 0, "mh_icp_window_optimise_edges layout");
static_assert(MH_WINDOW_LINEAR_MAX == mh::kWindowLinMax && kWinLinAt % 16 == 0, "mh_icp_window_optimise_lin layout");
constexpr size_t kWinRowWords = 256;  // flagged words per iteration's row in h_window_rows
constexpr size_t kWinMaskWord = kWinRowWords - 1;  // of which the last: the evaluated mask of an mh_icp_window_optimise_relin iteration
static_assert(mh::kWRowPose + 12 * mh::kWindowMax <= static_cast<int>(kWinMaskWord) && kWinRelinAt % 16 == 0, "mh_icp_window_optimise_relin layout");
static_assert(kWinStateAt + sizeof(mh::WindowState) <= kWinBlocksAt && mh::kWRowPose + 12 * mh::kWindowMax <= static_cast<int>(kWinRowWords) &&
                MH_WINDOW_MAX == mh::kWindowMax, "mh_icp_window_optimise layout");

// Launch groups of a window: the factors that share a kernel instantiation — workgroup size (256 threads up to 65 536 points,
// 512 above: so every factor reduces in exactly the order of a separate call), k == 5 or the generic k <= 8 path, neighbour
// mode, unary / binary.  Shared by mh_icp_linearize_batch and mh_icp_window_optimise, which therefore run a window's factors
// in the same classes.
std::vector<LaunchGroup> mhi::window_launch_groups(mh_icp * const * icps, size_t n_factors)
{
  std::vector<LaunchGroup> groups;
  long long total_points = 0;  // the class of a small cloud depends on how full the machine is: the whole window's points
  for (size_t f = 0; f < n_factors; ++f) total_points += static_cast<long long>(icps[f]->n);
  // (more factors than ride in the kernel-argument segment: the staged launch form has the one-lane-per-point classes only)
  const bool maybe_staged = n_factors > static_cast<size_t>(mh::kBatchInline);
  for (size_t f = 0; f < n_factors; ++f) {
    const mh_icp * c = icps[f];
    if (c->n == 0) continue;
    const int k = c->cfg.num_corres_points == 5 ? 5 : 8, n_off = c->map->n_off;
    int tpb = mh::linearize_class(static_cast<int>(c->n), static_cast<int>(c->cfg.num_corres_points), false, total_points);
    if (maybe_staged && tpb < 256) tpb = 256;
    LaunchGroup * g = nullptr;
    for (LaunchGroup & q : groups)
      if (q.tpb == tpb && q.k == k && q.n_off == n_off && q.binary == c->binary) g = &q;
    if (!g) {
      groups.push_back(LaunchGroup{tpb, k, n_off, c->binary, {}});
      g = &groups.back();
    }
    g->members.push_back(f);
  }
  return groups;
}

// ---- what the two families share ------------------------------------------------------------------------------------------
// Where a chain's rows arrive in mapped pinned memory: iteration i's row is `words` flagged words at base + i * stride, each
// tagged seq[i].
struct ChainRows
{
  const uint4 * base;
  size_t stride;
  int words;
  const unsigned int * seq;
};

static bool chain_read_row(const ChainRows & r, int i, long spin_ns, double * row)
{
  const uint4 * base = r.base + static_cast<size_t>(i) * r.stride;
  mh::SpinBudget spin(spin_ns);  // one budget for the whole row
  for (int w = r.words - 1; w >= 0; --w)  // the word that is written last first
    if (!spin.until([&] { return mh::ll_read(reinterpret_cast<const uint64_t *>(base + w), r.seq[i], row[w]); })) return false;
  return true;
}

// wait for the row of iteration i (the last one queued so far): the values themselves, the stream behind them
static int chain_wait_row(mh_ctx * ctx, const ChainRows & r, int i, double * row, const char * what)
{
  if (chain_read_row(r, i, 50000000L, row)) return MH_OK;  // 50 ms: 64 iterations of a large cloud are a few
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (chain_read_row(r, i, 2000000L, row)) return MH_OK;
  return fail(ctx, MH_ERR_HIP, std::string(what) + ": the stream drained without the chain's results");
}

// Every iteration's copy of the K3 argument block `a` (mhi::chain_k3_block), iteration i's at blocks[i * stride]: cold only
// where the factor was, and in iteration 0; the iteration's number; its landing slot ll_step words behind the one before.
static void chain_fill_blocks(const mh::IcpArgs & a, bool cold0, int iters, const unsigned int * seq, mh::IcpArgs * blocks, size_t stride, size_t ll_step)
{
  for (int i = 0; i < iters; ++i) {
    mh::IcpArgs b = a;
    b.cold = (i == 0 && cold0) ? 1 : 0;
    b.seq = seq[i];
    b.ll = a.ll + static_cast<size_t>(i) * ll_step;
    blocks[static_cast<size_t>(i) * stride] = b;
  }
}

// What a chain with several factors asks of each of them, in this order; the words are the entry point's (empty == nullptr: a
// factor without points is welcome).  None of icps[0 .. n) is NULL.
struct FactorWords
{
  const char * contexts, * unary, * sharded, * in_flight, * empty, * twice;
};

static Refusal chain_check_factors(const mh_ctx * ctx, mh_icp * const * icps, size_t n, const FactorWords & w)
{
  for (size_t f = 0; f < n; ++f) {
    const mh_icp * c = icps[f];
    if (c->ctx != ctx) return {MH_ERR_INVALID_ARG, w.contexts};
    if (c->binary) return {MH_ERR_UNSUPPORTED, w.unary};
    if (c->no_order || c->cap_n > c->n) return {MH_ERR_UNSUPPORTED, w.sharded};
    if (c->n_pending) return {MH_ERR_INVALID_ARG, w.in_flight};
    if (w.empty && c->n == 0) return {MH_ERR_INVALID_ARG, w.empty};
    for (size_t g = 0; g < f; ++g)
      if (icps[g] == c) return {MH_ERR_INVALID_ARG, w.twice};
  }
  return {};
}

// Launch groups in slot order, as mh_icp_linearize_batch lays the same factors out: one staged K3 launch per group, member m's
// argument block at slot[m] of an iteration (a factor in no group keeps what slot[] held).  Returns the slots per iteration.
static int chain_plan_launches(const std::vector<LaunchGroup> & groups, int * slot, std::vector<WindowLaunch> & launches)
{
  launches.clear();
  int n_slots = 0;
  for (const LaunchGroup & g : groups) {
    launches.push_back(WindowLaunch{g.tpb, g.k, g.n_off, n_slots, static_cast<int>(g.members.size()), 0});
    for (size_t m : g.members) slot[m] = n_slots++;
  }
  return n_slots;
}

// The grid prefix of every launch (where each member's workgroups start, and their sum: the launch's grid) from the first
// iteration's argument blocks.  Launch gi has n + 1 entries, so its prefix starts gi entries behind its first slot — where
// chain_launch_k3 looks for it.
static void chain_fill_prefix(int * prefix, std::vector<WindowLaunch> & launches, const mh::IcpArgs * blocks)
{
  for (size_t gi = 0; gi < launches.size(); ++gi) {
    WindowLaunch & wl = launches[gi];
    int * start = prefix + wl.first + static_cast<int>(gi);
    int acc = 0;
    for (int i = 0; i < wl.n; ++i) {
      start[i] = acc;
      acc += mh::class_grid(blocks[wl.first + i].n, wl.tpb);
    }
    start[wl.n] = acc;
    wl.grid = acc;
  }
}

// ... and the K3 launches of one iteration whose argument blocks start at `blocks` (device), prefix as chain_fill_prefix left it
static hipError_t chain_launch_k3(const std::vector<WindowLaunch> & launches, mh::IcpArgs * blocks, const int * prefix, hipStream_t stream)
{
  hipError_t e = hipSuccess;
  for (size_t gi = 0; gi < launches.size() && e == hipSuccess; ++gi) {
    const WindowLaunch & wl = launches[gi];
    e = mh::launch_linearize_batch(blocks + wl.first, prefix + wl.first + static_cast<int>(gi), wl.n, wl.grid, wl.tpb, wl.k, wl.n_off, false, stream);
  }
  return e;
}

// the step's parameters of an alignment of icp under cfg, gz = -g_unit
static mh::AlignParams align_params(const mh_icp_align_config & cfg, const mh_icp * icp, const double gz[3])
{
  mh::AlignParams p;
  for (int i = 0; i < 3; ++i) p.gz[i] = gz[i];
  p.eps_rot = cfg.eps_rot;
  p.eps_trans = cfg.eps_trans;
  p.damping = cfg.damping;
  p.prior_rot = cfg.prior_sigma_rot > 0.0 ? 1.0 / (cfg.prior_sigma_rot * cfg.prior_sigma_rot) : 0.0;
  p.prior_trans = cfg.prior_sigma_trans > 0.0 ? 1.0 / (cfg.prior_sigma_trans * cfg.prior_sigma_trans) : 0.0;
  p.thresh_rot = icp->cfg.degen_thresh_rot;
  p.thresh_trans = icp->cfg.degen_thresh_trans;
  p.reg_4_dof = icp->cfg.reg_4_dof;
  p.project_on_degeneracy = icp->cfg.project_on_degneneracy;
  return p;
}

// The loop of a blocking call (chunk > 0: queue that many iterations, wait for the last row queued, and again until all are
// queued or a row says the chain has stopped, bit 1 of its flags word) and the wait of a call that did not block (chunk == 0:
// everything is queued, wait for its last row); then the result.  enqueue(upto) puts the iterations up to `upto` on the stream
// and moves `queued`; it has abandoned the call when it fails.
template <typename Enqueue, typename WaitRow, typename Abandon, typename Finish>
static int chain_drive(const int & queued, int iters, int chunk, int flags_word, Enqueue enqueue, WaitRow wait_row, Abandon abandon, Finish finish)
{
  static_assert(mh::kRowWords <= static_cast<int>(kWinRowWords), "no family's row is longer than the window's");
  double row[kWinRowWords];
  do {
    int rc = chunk > 0 ? enqueue(std::min(queued + chunk, iters)) : MH_OK;
    if (rc != MH_OK) return rc;
    if (queued > 0 && (rc = wait_row(queued - 1, row)) != MH_OK) {
      abandon();
      return rc;
    }
  } while (chunk > 0 && queued < iters && !(static_cast<int>(row[flags_word]) & 1));
  return finish();
}

// The rows of the queued iterations in order, iteration i's into buf + i * buf_stride, up to the first that was queued behind
// the stop (bit 4 of its flags word: nothing was evaluated, there or later); decode(i, row) takes each evaluated one.  iters:
// how many were evaluated — 0 is the caller's error to word (the first queued iteration is always evaluated: its row never
// carries the bit); converged: bit 2 of the last of them.
template <typename Decode>
static int chain_trace(mh_ctx * ctx, const ChainRows & r, int queued, int flags_word, const char * what, double * buf, size_t buf_stride,
                       Decode decode, int & iters, int & converged)
{
  iters = converged = 0;
  for (int i = 0; i < queued; ++i) {
    double * row = buf + static_cast<size_t>(i) * buf_stride;
    const int rc = chain_wait_row(ctx, r, i, row, what);
    if (rc != MH_OK) return rc;
    const int flags = static_cast<int>(row[flags_word]);
    if (flags & 4) break;
    decode(i, row);
    iters = i + 1;
    converged = (flags & 2) ? 1 : 0;
  }
  return MH_OK;
}

// first / last of a result: the host epilogue of linearize() on the sums K3 folded in iteration `it` of the chain, at the pose
// R_at, as call number linearize_count of the factor.  false: the sums did not arrive (the caller words the error).
static bool chain_epilogue(const mh_icp * icp, int it, const double R_at[9], const double gz[3], int linearize_count, unsigned int seq,
                           mh_icp_result * out)
{
  PendingCall pc{};
  pc.out = nullptr;
  std::memcpy(pc.R, R_at, sizeof(pc.R));
  std::memcpy(pc.gz, gz, sizeof(pc.gz));
  pc.linearize_count = linearize_count;
  pc.seq = seq;
  pc.components = false;
  pc.ev[0] = pc.ev[1] = pc.ev[2] = nullptr;
  mh::DeviceResult dres;
  if (!mhi::collect_call(icp, it, pc, 2000000L, dres)) return false;
  mhi::finish(icp, dres, pc, out);
  out->gpu_ms_linearize = out->gpu_ms_localizability = -1.0f;
  return true;
}

// ---- alignment chains: [K3 batch launches, one step launch] x iters on the context's stream, one wait ----------------------
// mh_icp_align is the chain of one member on the factor's own record and storage, mh_icp_align_batch the chain of up to
// MH_ALIGN_BATCH_MAX members on the context's (AlignChain, mh_internal.hpp); one driver serves both.  The argument blocks of
// every iteration sit in the chain's device block, filled here except R, t of the iterations after the first, which the step in
// front of each writes (align_kernels.hip).  K3 runs as in a window call (staged batch form, one launch per launch group, tail =
// 1 — for one member the class a call of its own would get), its flagged words landing in the member's device slot; the step
// launch has one workgroup per member, which forwards that member's words and its own row to the iteration's slot of the
// member's pinned ring.  So a member of a batch is collected like a call of its own (align_collect).
static mh_ctx * batch_ctx(mh_icp * const * icps, size_t B) { return (icps && B && icps[0]) ? icps[0]->ctx : nullptr; }

static void align_abandon(AlignChain & c)
{
  (void)hipStreamSynchronize(c.icps[0]->ctx->stream);
  let_go(c.icps, c.n);
  c.n = 0;
}

// What mh_icp_align refuses of a config, for every entry point that takes one (each words the two messages with its own prefix).
int mhi::align_check_config(const mh_ctx * ctx, const mh_icp_align_config & cfg, const char * iters_prefix, const char * ranges_prefix)
{
  if (cfg.max_iters < 1 || cfg.max_iters > kMaxPending) return fail(ctx, MH_ERR_INVALID_ARG, std::string(iters_prefix) + "max_iters must be in 1..64");
  if (!(cfg.eps_rot >= 0.0) || !(cfg.eps_trans >= 0.0) || !(cfg.damping >= 0.0) || !(cfg.prior_sigma_rot >= 0.0) || !(cfg.prior_sigma_trans >= 0.0) ||
      cfg.check_every < 0)
    return fail(ctx, MH_ERR_INVALID_ARG, std::string(ranges_prefix) + "eps, damping, prior sigmas and check_every must be >= 0");
  return MH_OK;
}

// The call is staged and its members are held: the entry point `what` has checked its arguments and c.h, c.d are allocated
// (the context is entered).  A failure half way returns with nothing held.
static int align_begin(AlignChain & c, const char * what, Held as, mh_icp * const * icps, size_t B, const double * R0, const double * t0,
                       const double g_unit[3], const mh_icp_align_config * cfg, mh_icp_align_result * out)
{
  mh_ctx * ctx = icps[0]->ctx;
  const int iters = cfg->max_iters;
  c.what = what;
  c.cfg = *cfg;
  c.queued = 0;
  c.out = out;
  for (int i = 0; i < 3; ++i) c.gz[i] = -g_unit[i];
  c.n_slots = chain_plan_launches(mhi::window_launch_groups(icps, B), c.slot, c.launches);  // as mh_icp_window_optimise lays the same factors out

  char * h = static_cast<char *>(c.h);
  char * d = static_cast<char *>(c.d);
  auto * blocks = reinterpret_cast<mh::IcpArgs *>(h + align_blocks_at(c.capacity));
  for (int it = 0; it < iters; ++it) c.seq[it] = mhi::next_call_seq();
  for (size_t m = 0; m < B; ++m) {
    mh_icp * icp = icps[m];
    c.icps[m] = icp;
    c.count0[m] = icp->linearize_count;
    std::memcpy(c.R0[m], R0 + 9 * m, sizeof(c.R0[m]));
    mh::IcpArgs a;
    const int rc = mhi::chain_k3_block(icp, R0 + 9 * m, t0 + 3 * m, g_unit, a);
    if (rc != MH_OK) return rc;
    a.ll = reinterpret_cast<uint4 *>(d + align_ll_at(c.capacity)) + kAlignLlWords * m;
    mh::AlignState st;
    std::memset(&st, 0, sizeof(st));
    std::memcpy(st.R, a.R, sizeof(st.R));
    std::memcpy(st.t, a.t, sizeof(st.t));
    std::memcpy(h + kAlignStateAt + kAlignStateStride * m, &st, sizeof(st));
    chain_fill_blocks(a, icp->cold, iters, c.seq, blocks + c.slot[m], static_cast<size_t>(c.n_slots), 0);
    c.p[m] = align_params(*cfg, icp, c.gz);
  }
  chain_fill_prefix(reinterpret_cast<int *>(h), c.launches, blocks);
  MH_HIP(ctx, hipMemcpyAsync(d, h, align_blocks_at(c.capacity) + sizeof(mh::IcpArgs) * static_cast<size_t>(c.n_slots) * static_cast<size_t>(iters),
                             hipMemcpyHostToDevice, ctx->stream));
  c.n = static_cast<int>(B);
  for (size_t m = 0; m < B; ++m) hold(icps[m], as);
  return MH_OK;
}

// iterations [queued, upto) onto the stream
static int align_enqueue(AlignChain & c, int upto)
{
  mh_ctx * ctx = c.icps[0]->ctx;
  char * d = static_cast<char *>(c.d);
  auto * blocks = reinterpret_cast<mh::IcpArgs *>(d + align_blocks_at(c.capacity));
  const int * prefix = reinterpret_cast<const int *>(d);
  for (int it = c.queued; it < upto; ++it) {
    hipError_t e = chain_launch_k3(c.launches, blocks + static_cast<size_t>(it) * c.n_slots, prefix, ctx->stream);
    if (e == hipSuccess) {
      mh::AlignBatchStepArgs s;
      std::memset(static_cast<void *>(&s), 0, sizeof(s));
      for (int m = 0; m < c.n; ++m) {
        mh::AlignStepArgs & a = s.m[m];
        a.ll_dev = reinterpret_cast<const uint4 *>(d + align_ll_at(c.capacity)) + kAlignLlWords * m;
        a.ll_host = c.icps[m]->d_h_ll + static_cast<size_t>(it) * c.icps[m]->ll_words;
        a.next = it + 1 < c.cfg.max_iters ? blocks + static_cast<size_t>(it + 1) * c.n_slots + c.slot[m] : nullptr;
        a.state = reinterpret_cast<mh::AlignState *>(d + kAlignStateAt + kAlignStateStride * m);
        a.p = c.p[m];
        a.seq = c.seq[it];
      }
      e = mh::launch_align_chain_step(s, c.n, ctx->stream);
    }
    if (e != hipSuccess) {
      align_abandon(c);
      return hip_fail(ctx, e, (std::string(c.what) + ": launch").c_str());
    }
    c.queued = it + 1;
  }
  return MH_OK;
}

// The result of one member whose queued iterations have run: the factor's rows (tagged seq[i]) decoded into *out, first /
// last from the host epilogue.  lost: a row did not arrive or no iteration was evaluated — the caller abandons its call;
// otherwise the caller moves the handle's books by out->iters.
static int align_collect(mh_icp * icp, const unsigned int * seq, int queued, const double R0[9], const double gz[3], int count0, mh_icp_align_result * out,
                         const char * what, bool & lost)
{
  mh_ctx * ctx = icp->ctx;
  std::memset(static_cast<void *>(out), 0, sizeof(*out));
  int iters = 0, converged = 0;
  double row_buf[mh::kRowWords];
  const ChainRows rows{icp->h_ll.as<uint4>() + mh::kLlSums, icp->ll_words, mh::kRowWords, seq};
  const int rc = chain_trace(ctx, rows, queued, mh::kRowFlags, what, row_buf, 0, [&](int i, const double * row) {
    mh_icp_align_trace & tr = out->trace[i];
    tr.f = row[mh::kRowF];
    tr.step_rot = row[mh::kRowStepRot];
    tr.step_trans = row[mh::kRowStepTrans];
    tr.n_knn = static_cast<int64_t>(row[mh::kRowKnn]);
    tr.degenerate = static_cast<int32_t>(row[mh::kRowBits]);
    std::memcpy(tr.R, row + mh::kRowR, sizeof(tr.R));
    std::memcpy(tr.t, row + mh::kRowT, sizeof(tr.t));
  }, iters, converged);
  lost = rc != MH_OK || iters == 0;
  if (lost) return rc != MH_OK ? rc : fail(ctx, MH_ERR_HIP, std::string(what) + ": no iteration was evaluated");
  int rc_all = MH_OK;
  if (out->trace[iters - 1].degenerate & 8) rc_all = fail(ctx, MH_ERR_HIP, std::string(what) + ": a step did not find its K3's sums");
  out->iters = iters;
  out->converged = converged;
  std::memcpy(out->R, out->trace[iters - 1].R, sizeof(out->R));
  std::memcpy(out->t, out->trace[iters - 1].t, sizeof(out->t));
  // first / last: at the initial and at the last evaluated pose
  for (int which = 0; which < 2 && rc_all == MH_OK; ++which) {
    const int i = which == 0 ? 0 : iters - 1;
    if (!chain_epilogue(icp, i, i == 0 ? R0 : out->trace[i - 1].R, gz, count0 + i + 1, seq[i], which == 0 ? &out->first : &out->last))
      rc_all = fail(ctx, MH_ERR_HIP, std::string(what) + ": an iteration's sums did not arrive");
  }
  return rc_all;
}

// every queued iteration has run (the caller waited for every member's last row): the results, and the handles' books
static int align_finish(AlignChain & c)
{
  int rc_all = MH_OK;
  for (int m = 0; m < c.n; ++m) {
    bool lost = false;
    const int rc = align_collect(c.icps[m], c.seq, c.queued, c.R0[m], c.gz, c.count0[m], &c.out[m], c.what, lost);
    if (lost) {  // the members collected so far keep their books; the call is over for all
      align_abandon(c);
      return rc;
    }
    c.icps[m]->linearize_count = c.count0[m] + c.out[m].iters;
    c.icps[m]->cold = false;
    if (rc_all == MH_OK) rc_all = rc;
  }
  let_go(c.icps, c.n);
  c.n = 0;
  return rc_all;
}

// The row of iteration i as chain_drive looks at it: every member's row has arrived, and the stop bit is set when every
// member's is.
static int align_wait_row(const AlignChain & c, int i, double * row)
{
  int all = 1;
  for (int m = 0; m < c.n; ++m) {
    const mh_icp * icp = c.icps[m];
    const int rc = chain_wait_row(icp->ctx, ChainRows{icp->h_ll.as<uint4>() + mh::kLlSums, icp->ll_words, mh::kRowWords, c.seq}, i, row, c.what);
    if (rc != MH_OK) return rc;
    all &= static_cast<int>(row[mh::kRowFlags]);
  }
  row[mh::kRowFlags] = static_cast<double>(all & 1);
  return MH_OK;
}

// the call after align_begin: everything queued and left in flight, or driven to its result
static int align_run(AlignChain & c, int chunk)
{
  return chain_drive(c.queued, c.cfg.max_iters, chunk, mh::kRowFlags, [&c](int upto) { return align_enqueue(c, upto); },
                     [&c](int i, double * row) { return align_wait_row(c, i, row); }, [&c] { align_abandon(c); }, [&c] { return align_finish(c); });
}

static int align_start(AlignChain & c, bool blocking)
{
  const mh_icp_align_config & cfg = c.cfg;
  if (!blocking) return align_enqueue(c, cfg.max_iters);
  return align_run(c, cfg.check_every > 0 ? cfg.check_every : cfg.max_iters);
}

int mhi::align_wait(mh_icp * icp)
{
  MH_HIP(icp->ctx, mh_enter(icp->ctx));
  return align_run(icp->align, 0);
}

static int mh_icp_align_impl(mh_icp * icp, const double R0[9], const double t0[3], const double g_unit[3], const mh_icp_align_config * cfg,
                             mh_icp_align_result * out, bool blocking)
{
  if (!icp || !R0 || !t0 || !g_unit || !cfg || !out) return fail(icp ? icp->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_icp_align: NULL argument");
  mh_ctx * ctx = icp->ctx;
  if (icp->binary) return fail(ctx, MH_ERR_UNSUPPORTED, "mh_icp_align: unary factors only");
  if (icp->n_pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_align: the factor has calls in flight");
  if (const int rc = mhi::align_check_config(ctx, *cfg, "mh_icp_align: ", "mh_icp_align: ")) return rc;
  if (icp->no_order || icp->cap_n > icp->n) return fail(ctx, MH_ERR_UNSUPPORTED, "mh_icp_align: not for the factors of the map-sharded path");
  if (icp->n == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_align: the factor has no points");
  MH_HIP(ctx, mh_enter(ctx));
  AlignChain & c = icp->align;
  MH_HIP(ctx, icp->d_align.reserve(align_bytes(1), ctx->stream, false));
  MH_HIP(ctx, icp->h_align.reserve(align_stage_bytes(1), align_stage_bytes(1)));
  c.h = icp->h_align.p;
  c.d = icp->d_align.p;
  const int rc = align_begin(c, "mh_icp_align", Held::align, &icp, 1, R0, t0, g_unit, cfg, out);
  return rc != MH_OK ? rc : align_start(c, blocking);
}

static int mh_icp_align_batch_impl(mh_icp * const * icps, size_t B, const double * R0, const double * t0, const double g_unit[3],
                                   const mh_icp_align_config * cfg, mh_icp_align_result * out, bool blocking)
{
  mh_ctx * ctx = batch_ctx(icps, B);
  if (!icps || !R0 || !t0 || !g_unit || !cfg || !out) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_align_batch: NULL argument");
  if (B < 1 || B > static_cast<size_t>(MH_ALIGN_BATCH_MAX)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_align_batch: B must be in 1..16");
  for (size_t m = 0; m < B; ++m)
    if (!icps[m]) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_align_batch: NULL member");
  ctx = icps[0]->ctx;
  AlignChain & c = ctx->align_batch;
  if (c.n) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_align_batch: the context has a batch call in flight");
  static constexpr FactorWords words{"mh_icp_align_batch: factors of different contexts", "mh_icp_align_batch: unary factors only",
                                     "mh_icp_align_batch: not for the factors of the map-sharded path", "mh_icp_align_batch: a member has calls in flight",
                                     "mh_icp_align_batch: a member has no points", "mh_icp_align_batch: the same factor twice"};
  if (const Refusal no = chain_check_factors(ctx, icps, B, words)) return fail(ctx, no.code, no.message);
  if (const int rc = mhi::align_check_config(ctx, *cfg, "mh_icp_align_batch: ", "mh_icp_align_batch: ")) return rc;
  MH_HIP(ctx, mh_enter(ctx));
  if (!c.h) MH_HIP(ctx, hipHostMalloc(&c.h, align_stage_bytes(c.capacity), hipHostMallocDefault));
  if (!c.d) MH_HIP(ctx, hipMalloc(&c.d, align_bytes(c.capacity)));
  const int rc = align_begin(c, "mh_icp_align_batch", Held::align_batch, icps, B, R0, t0, g_unit, cfg, out);
  return rc != MH_OK ? rc : align_start(c, blocking);
}

int mhi::align_batch(mh_icp * const * icps, size_t B, const double * R0, const double * t0, const double g_unit[3], const mh_icp_align_config * cfg,
                     mh_icp_align_result * out)
{
  return mh_icp_align_batch_impl(icps, B, R0, t0, g_unit, cfg, out, true);
}

static int mh_icp_align_batch_wait_impl(mh_ctx * ctx)
{
  if (!ctx) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_icp_align_batch_wait: ctx is NULL");
  if (!ctx->align_batch.n) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_align_batch_wait: no batch call in flight");
  MH_HIP(ctx, mh_enter(ctx));
  return align_run(ctx->align_batch, 0);
}

// ---- fixed-lag window: [K3 batch launches, step] x iters on the context's stream, one wait --------------------------------
// The argument blocks of every iteration sit in device memory the context owns (d_window), filled here except R, t of the
// iterations after the first, which the step kernel in front of each writes (window_kernels.hip).  K3 runs in the staged batch
// form, one launch per launch group, tail = 1, its flagged words landing in a device slot per pose; the step forwards them to
// the iteration's slot of each factor's pinned ring and publishes its own row to the context's rows.
static ChainRows window_rows(const mh_ctx * ctx) { return {ctx->h_window_rows, kWinRowWords, mh::window_row_words(ctx->window.W), ctx->window.seq}; }

// the context of a window's factors (where a message goes: mh_last_error(ctx) as well as mh_last_error(NULL))
static mh_ctx * window_ctx(mh_icp * const * icps, size_t W) { return (icps && W && icps[0]) ? icps[0]->ctx : nullptr; }

// the window call on ctx is over (collected, or abandoned behind a drained stream): its factors are free again
static void window_release(mh_ctx * ctx)
{
  let_go(ctx->window.icps, ctx->window.W);
  ctx->window.active = false;
}

static void window_abandon(mh_ctx * ctx)
{
  (void)hipStreamSynchronize(ctx->stream);
  window_release(ctx);
}

// ---- the start of a window call: window_begin and its stages ---------------------------------------------------------------
// What is asked of the factors themselves, where the order of the checks has it (window_request.hpp: behind the arguments,
// before the config).
static Refusal window_check_factors(const WindowRequest & q)
{
  static_assert(kWindowItersMax == kMaxPending, "the chain holds a factor's whole ring: one pending slot per iteration");
  const mh_ctx * ctx = q.icps[0]->ctx;
  if (ctx->window.active) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise: the context has a window call in flight"};
  static constexpr FactorWords words{"mh_icp_window_optimise: factors of different contexts", "mh_icp_window_optimise: unary factors only",
                                     "mh_icp_window_optimise: not for the factors of the map-sharded path", "mh_icp_window_optimise: a factor has calls in flight",
                                     nullptr, "mh_icp_window_optimise: the same factor twice"};
  return chain_check_factors(ctx, q.icps, q.W, words);
}

// The shape of the call: its iterations, and which factor's K3 runs in which launch from which slot.  A marginal is ONE queued
// "iteration" in which only icps[0] runs K3, in the class of a call of its own (as mh_icp_align runs it), and the marginal
// kernel stands in for the step.
static void window_plan(WindowCall & c, const WindowRequest & q)
{
  const bool marginal = q.kind != WindowKind::optimise;
  c.W = static_cast<int>(q.W);
  c.iters = marginal ? 1 : q.cfg->iters;
  std::vector<LaunchGroup> groups;
  if (!marginal)
    groups = mhi::window_launch_groups(q.icps, q.W);
  else if (const mh_icp * icp = q.icps[0]; icp->n)
    groups.push_back(LaunchGroup{mh::linearize_class(static_cast<int>(icp->n), static_cast<int>(icp->cfg.num_corres_points), false),
                                 icp->cfg.num_corres_points == 5 ? 5 : 8, icp->map->n_off, false, {0}});
  for (size_t f = 0; f < q.W; ++f) c.slot[f] = -1;
  c.n_slots = chain_plan_launches(groups, c.slot, c.launches);
}

// the context's three blocks, on first use
static int window_alloc(mh_ctx * ctx)
{
  if (!ctx->h_window) MH_HIP(ctx, hipHostMalloc(&ctx->h_window, kWinStageJointAt + sizeof(mh::WindowJoint), hipHostMallocDefault));
  if (!ctx->d_window) MH_HIP(ctx, hipMalloc(&ctx->d_window, kWinBytes));
  if (!ctx->h_window_rows) {
    MH_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_window_rows), kWinRowWords * sizeof(uint4) * kMaxPending, hipHostMallocMapped));
    std::memset(ctx->h_window_rows, 0, kWinRowWords * sizeof(uint4) * kMaxPending);
    MH_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->d_window_rows), ctx->h_window_rows, 0));
  }
  return MH_OK;
}

// The first part of h_window: WindowState, per factor the argument blocks of a components-off linearize at its pose in every
// iteration, the grid prefixes.  c.R0 keeps the caller's R for the epilogue of `first`; the chain starts from a.R, which for a
// unary factor is the same matrix.
static int window_stage_blocks(mh_ctx * ctx, const WindowRequest & q, unsigned int zmask)
{
  WindowCall & c = ctx->window;
  char * h = static_cast<char *>(ctx->h_window);
  auto * blocks = reinterpret_cast<mh::IcpArgs *>(h + kWinBlocksAt);
  mh::WindowState st;
  std::memset(&st, 0, sizeof(st));
  for (size_t f = 0; f < q.W; ++f) {
    mh_icp * icp = q.icps[f];
    c.icps[f] = icp;
    c.count0[f] = icp->linearize_count;
    std::memcpy(c.R0[f], q.R + 9 * f, sizeof(c.R0[f]));
    std::memcpy(st.R[f], q.R + 9 * f, sizeof(st.R[f]));
    std::memcpy(st.t[f], q.t + 3 * f, sizeof(st.t[f]));
    if ((zmask >> f) & 1u) {
      std::memcpy(st.ZR[f], q.Z_R + 9 * f, sizeof(st.ZR[f]));
      std::memcpy(st.Zt[f], q.Z_t + 3 * f, sizeof(st.Zt[f]));
    }
    if (c.slot[f] < 0) continue;  // an empty factor, or one a marginal leaves alone
    mh::IcpArgs a;
    const int rc = mhi::chain_k3_block(icp, q.R + 9 * f, q.t + 3 * f, q.g_unit, a);
    if (rc != MH_OK) return rc;
    a.ll = reinterpret_cast<uint4 *>(static_cast<char *>(ctx->d_window) + kWinLlAt) + 32 * f;
    std::memcpy(st.R[f], a.R, sizeof(st.R[f]));
    std::memcpy(st.t[f], a.t, sizeof(st.t[f]));
    chain_fill_blocks(a, icp->cold, c.iters, c.seq, blocks + c.slot[f], static_cast<size_t>(c.n_slots), 0);
  }
  chain_fill_prefix(reinterpret_cast<int *>(h), c.launches, blocks);
  std::memcpy(h + kWinStateAt, &st, sizeof(st));
  return MH_OK;
}

static void window_fill_params(mh::WindowParams & p, const WindowRequest & q, unsigned int zmask, const double gz[3])
{
  std::memset(&p, 0, sizeof(p));
  p.W = static_cast<int>(q.W);
  p.has_Z = zmask;
  for (size_t f = 0; f < q.W; ++f) {
    const mh_icp * icp = q.icps[f];
    if (icp->n) p.have |= 1u << f;
    if (icp->cfg.reg_4_dof) p.reg_4_dof |= 1u << f;
    if (icp->cfg.project_on_degneneracy) p.project_on_degeneracy |= 1u << f;
    p.thresh_rot[f] = icp->cfg.degen_thresh_rot;
    p.thresh_trans[f] = icp->cfg.degen_thresh_trans;
  }
  for (int i = 0; i < 3; ++i) p.gz[i] = gz[i];
  for (int i = 0; i < 6; ++i) {
    p.Wb[i] = q.cfg->between_info[i];
    p.prior[i] = q.cfg->prior_info[i];
  }
  p.damping = q.cfg->damping;
  p.eps_rot = q.cfg->eps_rot;
  p.eps_trans = q.cfg->eps_trans;
}

// the linear factors, once per call: the header and the factors in use
static int stage_linear(mh_ctx * ctx, const mh_window_linear_factor * lin, size_t n_lin)
{
  auto * wl = reinterpret_cast<mh::WindowLinear *>(static_cast<char *>(ctx->h_window) + kWinStageBytes);
  wl->n = static_cast<int>(n_lin);
  wl->pad = 0;
  for (size_t j = 0; j < static_cast<size_t>(mh::kWindowLinMax); ++j) wl->pose[j] = j < n_lin ? lin[j].pose : 0;
  for (size_t j = 0; j < n_lin; ++j) {
    std::memcpy(wl->LR[j], lin[j].L_R, sizeof(wl->LR[j]));
    std::memcpy(wl->Lt[j], lin[j].L_t, sizeof(wl->Lt[j]));
    std::memcpy(wl->H[j], lin[j].H, sizeof(wl->H[j]));
    std::memcpy(wl->b[j], lin[j].b, sizeof(wl->b[j]));
    wl->f[j] = lin[j].f;
  }
  MH_HIP(ctx, hipMemcpyAsync(static_cast<char *>(ctx->d_window) + kWinLinAt, wl, sizeof(mh::WindowLinear), hipMemcpyHostToDevice, ctx->stream));
  return MH_OK;
}

// the edges, once per call; the slots behind the last keep a valid pair, which nothing reads
static int stage_edges(mh_ctx * ctx, const mh_window_edge * edges, size_t n_edges)
{
  auto * we = reinterpret_cast<mh::WindowEdges *>(static_cast<char *>(ctx->h_window) + kWinStageEdgeAt);
  std::memset(static_cast<void *>(we), 0, sizeof(*we));
  we->n = static_cast<int>(n_edges);
  for (size_t e = 0; e < n_edges; ++e) {
    we->a[e] = edges[e].pose_a;
    we->b[e] = edges[e].pose_b;
    std::memcpy(we->ZR[e], edges[e].Z_R, sizeof(we->ZR[e]));
    std::memcpy(we->Zt[e], edges[e].Z_t, sizeof(we->Zt[e]));
    std::memcpy(we->Om[e], edges[e].info, sizeof(we->Om[e]));
  }
  MH_HIP(ctx, hipMemcpyAsync(static_cast<char *>(ctx->d_window) + kWinEdgeAt, we, sizeof(mh::WindowEdges), hipMemcpyHostToDevice, ctx->stream));
  return MH_OK;
}

// the joint factor, once per call: the members in use, everything behind them zero
static int stage_joint(mh_ctx * ctx, const mh_window_joint_factor & joint)
{
  auto * wj = reinterpret_cast<mh::WindowJoint *>(static_cast<char *>(ctx->h_window) + kWinStageJointAt);
  std::memset(static_cast<void *>(wj), 0, sizeof(*wj));
  const int n = joint.n_poses;
  wj->n = n;
  for (int m = 0; m < n; ++m) {
    wj->pose[m] = joint.pose[m];
    std::memcpy(wj->LR[m], joint.L_R + 9 * m, sizeof(wj->LR[m]));
    std::memcpy(wj->Lt[m], joint.L_t + 3 * m, sizeof(wj->Lt[m]));
  }
  for (int r = 0; r < 6 * n; ++r) {
    std::memcpy(wj->H + mh::kWindowJointDim * r, joint.H + 24 * r, sizeof(double) * 6 * n);
    wj->b[r] = joint.b[r];
  }
  wj->f = joint.f;
  MH_HIP(ctx, hipMemcpyAsync(static_cast<char *>(ctx->d_window) + kWinJointAt, wj, sizeof(mh::WindowJoint), hipMemcpyHostToDevice, ctx->stream));
  return MH_OK;
}

// Everything the chain reads, staged in pinned memory and sent: the first part in one copy, then each payload in its own.  A
// failure (of chain_k3_block half way, of a copy) returns with nothing marked in flight.
static int window_stage(mh_ctx * ctx, const WindowRequest & q, const WindowChecked & k)
{
  MH_HIP(ctx, mh_enter(ctx));
  int rc = window_alloc(ctx);
  if (rc != MH_OK) return rc;
  WindowCall & c = ctx->window;
  for (int i = 0; i < 3; ++i) c.gz[i] = -q.g_unit[i];
  for (int it = 0; it < c.iters; ++it) c.seq[it] = mhi::next_call_seq();
  if ((rc = window_stage_blocks(ctx, q, k.zmask)) != MH_OK) return rc;
  window_fill_params(c.p, q, k.zmask, c.gz);
  MH_HIP(ctx, hipMemcpyAsync(ctx->d_window, ctx->h_window, kWinBlocksAt + sizeof(mh::IcpArgs) * static_cast<size_t>(c.n_slots) * static_cast<size_t>(c.iters),
                             hipMemcpyHostToDevice, ctx->stream));
  if (q.lin_call && (rc = stage_linear(ctx, q.lin, q.n_lin)) != MH_OK) return rc;
  // (the marginal kernels and the joint step read the header of an empty list of edges)
  if ((q.n_edges || q.kind != WindowKind::optimise || q.joint) && (rc = stage_edges(ctx, q.edges, q.n_edges)) != MH_OK) return rc;
  if (q.joint && (rc = stage_joint(ctx, *q.joint)) != MH_OK) return rc;
  return MH_OK;
}

// The call is in flight: what its enqueue and its collectors need of the request, and the factors' books.
static void window_claim(mh_ctx * ctx, const WindowRequest & q, const WindowChecked & k)
{
  WindowCall & c = ctx->window;
  c.kind = q.kind;
  c.outputs = q.outputs;
  c.has_joint = q.joint != nullptr;
  c.relin = q.relin != nullptr;
  c.relin_rot = q.relin ? q.relin->relin_rot : 0.0;
  c.relin_trans = q.relin ? q.relin->relin_trans : 0.0;
  c.lin = q.lin_call;
  c.edges = q.n_edges > 0;
  if (q.kind != WindowKind::optimise) {
    std::memcpy(c.L1R, q.R + 9, sizeof(c.L1R));
    std::memcpy(c.L1t, q.t + 3, sizeof(c.L1t));
  }
  c.n_sep = k.n_sep;
  for (int s = 0; s < MH_WINDOW_JOINT_POSES; ++s) {
    c.sep[s] = k.sep[s];
    if (s < k.n_sep) {  // (W >= 2 and every separator pose inside the window: the edges' and the joint factor's checks)
      std::memcpy(c.LSR[s], q.R + 9 * k.sep[s], sizeof(c.LSR[s]));
      std::memcpy(c.LSt[s], q.t + 3 * k.sep[s], sizeof(c.LSt[s]));
    }
  }
  c.queued = 0;
  c.active = true;
  for (size_t f = 0; f < q.W; ++f) hold(q.icps[f], Held::window);
}

static int window_begin(const WindowRequest & q)
{
  WindowChecked k;
  if (const Refusal no = window_check_request(q, k, [&q] { return window_check_factors(q); })) return fail(window_ctx(q.icps, q.W), no.code, no.message);
  mh_ctx * ctx = q.icps[0]->ctx;
  window_plan(ctx->window, q);
  const int rc = window_stage(ctx, q, k);
  if (rc != MH_OK) return rc;
  window_claim(ctx, q, k);
  return MH_OK;
}

// iterations [queued, upto) onto the stream
static int window_enqueue(mh_ctx * ctx, int upto)
{
  WindowCall & c = ctx->window;
  char * d = static_cast<char *>(ctx->d_window);
  auto * blocks = reinterpret_cast<mh::IcpArgs *>(d + kWinBlocksAt);
  const int * prefix = reinterpret_cast<const int *>(d);
  // the step kernel of the call.  The argument structs nest in this order (window_device.hpp), each kernel taking the one of
  // its name with everything inside it: joint { edge { lin { relin { plain } } } }
  enum class Step { plain, relin, lin, edge, joint };
  const Step step = !(c.relin || c.lin) ? Step::plain : c.has_joint ? Step::joint : c.edges ? Step::edge : c.lin ? Step::lin : Step::relin;
  for (int it = c.queued; it < upto; ++it) {
    hipError_t e = chain_launch_k3(c.launches, blocks + static_cast<size_t>(it) * c.n_slots, prefix, ctx->stream);
    if (e == hipSuccess) {
      mh::WindowJointStepArgs ja;
      std::memset(static_cast<void *>(&ja), 0, sizeof(ja));
      mh::WindowEdgeStepArgs & ea = ja.e;
      mh::WindowLinStepArgs & la = ea.l;
      mh::WindowRelinStepArgs & ra = la.r;
      mh::WindowStepArgs & s = ra.s;
      s.ll_dev = reinterpret_cast<const uint4 *>(d + kWinLlAt);
      for (int i = 0; i < c.W; ++i) {
        s.ll_host[i] = c.icps[i]->n ? c.icps[i]->d_h_ll + static_cast<size_t>(it) * c.icps[i]->ll_words : nullptr;
        s.slot[i] = static_cast<signed char>(c.slot[i]);
      }
      s.row_host = ctx->d_window_rows + static_cast<size_t>(it) * kWinRowWords;
      s.next = it + 1 < c.iters ? blocks + static_cast<size_t>(it + 1) * c.n_slots : nullptr;
      s.state = reinterpret_cast<mh::WindowState *>(d + kWinStateAt);
      s.p = c.p;
      s.seq = c.seq[it];
      if (c.relin) {
        ra.relin = reinterpret_cast<mh::WindowRelin *>(d + kWinRelinAt);
        ra.mask_host = s.row_host + kWinMaskWord;
        ra.rp.relin_rot = c.relin_rot;
        ra.rp.relin_trans = c.relin_trans;
        ra.rp.first = it == 0 ? 1 : 0;
      }
      la.lin = reinterpret_cast<const mh::WindowLinear *>(d + kWinLinAt);
      ea.edges = reinterpret_cast<const mh::WindowEdges *>(d + kWinEdgeAt);
      ja.joint = reinterpret_cast<const mh::WindowJoint *>(d + kWinJointAt);
      switch (step) {
        case Step::plain: e = mh::launch_window_step(s, ctx->stream); break;
        case Step::relin: e = mh::launch_window_relin_step(ra, ctx->stream); break;
        case Step::lin: e = mh::launch_window_lin_step(la, c.relin, ctx->stream); break;
        case Step::edge: e = mh::launch_window_edge_step(ea, c.relin, ctx->stream); break;
        case Step::joint: e = mh::launch_window_joint_step(ja, c.relin, ctx->stream); break;
      }
    }
    if (e != hipSuccess) {
      window_abandon(ctx);
      return hip_fail(ctx, e, "mh_icp_window_optimise: launch");
    }
    c.queued = it + 1;
  }
  return MH_OK;
}

// every queued iteration has run (the caller waited for the last row): the result, and the handles' books
static int window_finish(mh_ctx * ctx)
{
  WindowCall & c = ctx->window;
  mh_icp_window_result * out = c.outputs.out;
  std::memset(static_cast<void *>(out), 0, sizeof(*out));
  const int W = c.W, words = mh::window_row_words(W);
  std::vector<double> rows(static_cast<size_t>(c.queued) * words);
  int iters = 0, converged = 0;
  bool lost = false;
  const int rc = chain_trace(ctx, window_rows(ctx), c.queued, mh::kWRowFlags, "mh_icp_window_optimise", rows.data(), static_cast<size_t>(words),
                             [&](int it, const double * row) {
    mh_icp_window_trace & tr = out->trace[it];
    tr.f = row[mh::kWRowF];
    tr.step_rot = row[mh::kWRowStepRot];
    tr.step_trans = row[mh::kWRowStepTrans];
    tr.flags = static_cast<int32_t>(row[mh::kWRowBits]) & mh::kAlignSingular;
    tr.degenerate = static_cast<uint32_t>(row[mh::kWRowDegen]);
    lost = lost || (static_cast<int>(row[mh::kWRowBits]) & 8);
    if (c.outputs.trace_poses) std::memcpy(c.outputs.trace_poses + static_cast<size_t>(it) * W * 12, row + mh::kWRowPose, sizeof(double) * 12 * W);
  }, iters, converged);
  if (rc != MH_OK || iters == 0) {
    window_abandon(ctx);
    return rc != MH_OK ? rc : fail(ctx, MH_ERR_HIP, "mh_icp_window_optimise: no iteration was evaluated");
  }
  int rc_all = MH_OK;
  if (lost) rc_all = fail(ctx, MH_ERR_HIP, "mh_icp_window_optimise: a step did not find its K3's sums");
  out->iters = iters;
  out->converged = converged;
  out->n_poses = W;
  const double * last_row = rows.data() + static_cast<size_t>(iters - 1) * words;
  for (int i = 0; i < W; ++i) {
    std::memcpy(out->R + 9 * i, last_row + mh::kWRowPose + 12 * i, sizeof(double) * 9);
    std::memcpy(out->t + 3 * i, last_row + mh::kWRowPose + 12 * i + 9, sizeof(double) * 3);
  }
  // which factors ran K3 in which iteration: all of them, unless the chain's steps decided (the word behind each row).  An
  // empty factor has no evaluation; its books move with the iterations, as they always did.
  uint32_t masks[kMaxPending];
  for (int it = 0; it < iters; ++it) masks[it] = c.p.have;
  for (int it = 0; it < iters && c.relin && rc_all == MH_OK; ++it) {
    double m = 0.0;
    const uint4 * word = ctx->h_window_rows + static_cast<size_t>(it) * kWinRowWords + kWinMaskWord;
    mh::SpinBudget spin(2000000L);
    if (!spin.until([&] { return mh::ll_read(reinterpret_cast<const uint64_t *>(word), c.seq[it], m); })) {
      rc_all = fail(ctx, MH_ERR_HIP, "mh_icp_window_optimise_relin: an iteration's evaluated mask did not arrive");
      break;
    }
    masks[it] = static_cast<uint32_t>(m);
    if (c.outputs.evaluated_mask) c.outputs.evaluated_mask[it] = masks[it];
  }
  int last_it[mh::kWindowMax], n_eval[mh::kWindowMax];
  for (int i = 0; i < W; ++i) {
    last_it[i] = c.icps[i]->n ? 0 : iters - 1;
    n_eval[i] = c.icps[i]->n ? 0 : iters;
    for (int it = 0; it < iters && c.icps[i]->n; ++it)
      if ((masks[it] >> i) & 1u) {
        last_it[i] = it;
        n_eval[i] += 1;
      }
  }
  // first / last: at the initial and at the last evaluated poses
  for (int i = 0; i < W && rc_all == MH_OK; ++i) {
    const mh_icp * icp = c.icps[i];
    for (int which = 0; which < 2 && rc_all == MH_OK; ++which) {
      const int it = which == 0 ? 0 : last_it[i];
      const double * R_at = it == 0 ? c.R0[i] : rows.data() + static_cast<size_t>(it - 1) * words + mh::kWRowPose + 12 * i;
      if (!chain_epilogue(icp, it, R_at, c.gz, c.count0[i] + (which == 0 ? 1 : n_eval[i]), icp->n ? c.seq[it] : 0, which == 0 ? &out->first[i] : &out->last[i]))
        rc_all = fail(ctx, MH_ERR_HIP, "mh_icp_window_optimise: an iteration's sums did not arrive");
    }
  }
  for (int i = 0; i < W; ++i) {
    c.icps[i]->linearize_count = c.count0[i] + n_eval[i];
    c.icps[i]->cold = false;
  }
  window_release(ctx);
  return rc_all;
}

static int window_run(mh_ctx * ctx, int chunk)
{
  return chain_drive(ctx->window.queued, ctx->window.iters, chunk, mh::kWRowFlags, [ctx](int upto) { return window_enqueue(ctx, upto); },
                     [ctx](int it, double * row) { return chain_wait_row(ctx, window_rows(ctx), it, row, "mh_icp_window_optimise"); },
                     [ctx] { window_abandon(ctx); }, [ctx] { return window_finish(ctx); });
}

// ---- the marginal prior of the oldest pose: K3 of icps[0], the marginal kernel, one wait ------------------------------------------
// window_begin staged the call as a window call of one queued iteration whose only argument block is the oldest factor's.
static int marginal_enqueue(mh_ctx * ctx)
{
  WindowCall & c = ctx->window;
  char * d = static_cast<char *>(ctx->d_window);
  hipError_t e = chain_launch_k3(c.launches, reinterpret_cast<mh::IcpArgs *>(d + kWinBlocksAt), reinterpret_cast<const int *>(d), ctx->stream);
  if (e == hipSuccess) {
    mh::WindowMarginalArgs a;
    std::memset(static_cast<void *>(&a), 0, sizeof(a));
    a.ll_dev = reinterpret_cast<const uint4 *>(d + kWinLlAt);
    a.ll_host = c.icps[0]->n ? c.icps[0]->d_h_ll : nullptr;
    a.row_host = ctx->d_window_rows;
    a.state = reinterpret_cast<const mh::WindowState *>(d + kWinStateAt);
    a.lin = reinterpret_cast<const mh::WindowLinear *>(d + kWinLinAt);
    a.edges = reinterpret_cast<const mh::WindowEdges *>(d + kWinEdgeAt);
    a.p = c.p;
    a.seq = c.seq[0];
    if (c.kind == WindowKind::marginal_joint) {
      mh::WindowMarginalJointArgs ja;
      std::memset(static_cast<void *>(&ja), 0, sizeof(ja));
      ja.m = a;
      ja.joint = c.has_joint ? reinterpret_cast<const mh::WindowJoint *>(d + kWinJointAt) : nullptr;
      ja.n_sep = c.n_sep;
      for (int k = 0; k < MH_WINDOW_JOINT_POSES; ++k) ja.sep[k] = c.sep[k];
      e = mh::launch_window_marginal_joint(ja, ctx->stream);
    } else {
      e = mh::launch_window_marginal(a, ctx->stream);
    }
  }
  if (e != hipSuccess) {
    window_abandon(ctx);
    return hip_fail(ctx, e, "mh_icp_window_marginalise: launch");
  }
  c.queued = 1;
  return MH_OK;
}

// What the two marginal calls share behind their kernel's row: wait for the row (`words` flagged words, the bits word at
// `bits_word`), clear *out, let `decode` take the row unless the kernel reports missing sums, `oldest` from the host epilogue of icps[0]'s K3, the
// oldest factor's books and the release of the window.
template <typename Decode>
static int marginal_collect(mh_ctx * ctx, int words, int bits_word, const char * what, void * out, size_t out_bytes, mh_icp_result * oldest, Decode decode)
{
  WindowCall & c = ctx->window;
  std::vector<double> row(static_cast<size_t>(words));
  const ChainRows rows{ctx->h_window_rows, kWinRowWords, words, c.seq};
  const int rc = chain_wait_row(ctx, rows, 0, row.data(), what);
  if (rc != MH_OK) {
    window_abandon(ctx);
    return rc;
  }
  std::memset(out, 0, out_bytes);
  int rc_all = MH_OK;
  if (static_cast<int>(row[bits_word]) & 8) rc_all = fail(ctx, MH_ERR_HIP, std::string(what) + ": the kernel did not find its K3's sums");
  mh_icp * icp = c.icps[0];
  if (rc_all == MH_OK) {
    decode(row.data());
    if (!chain_epilogue(icp, 0, c.R0[0], c.gz, c.count0[0] + 1, icp->n ? c.seq[0] : 0, oldest))
      rc_all = fail(ctx, MH_ERR_HIP, std::string(what) + ": the oldest factor's sums did not arrive");
  }
  icp->linearize_count = c.count0[0] + 1;
  icp->cold = false;
  window_release(ctx);
  return rc_all;
}

// mh_icp_window_marginalise_joint: the wide row
static int marginal_joint_finish(mh_ctx * ctx)
{
  WindowCall & c = ctx->window;
  mh_window_joint_marginal * out = c.outputs.jmarg;
  return marginal_collect(ctx, mh::kWJMargWords, mh::kWJMargBits, "mh_icp_window_marginalise_joint", out, sizeof(*out), &out->oldest, [&](const double * row) {
    out->prior.n_poses = c.n_sep;  // the separator and its poses are reported whether or not A00 had a positive pivot
    for (int k = 0; k < c.n_sep; ++k) {
      out->prior.pose[k] = c.sep[k];
      std::memcpy(out->prior.L_R + 9 * k, c.LSR[k], sizeof(c.LSR[k]));
      std::memcpy(out->prior.L_t + 3 * k, c.LSt[k], sizeof(c.LSt[k]));
    }
    std::memcpy(out->prior.H, row + mh::kWJMargH, sizeof(out->prior.H));
    std::memcpy(out->prior.b, row + mh::kWJMargB, sizeof(out->prior.b));
    out->prior.f = row[mh::kWJMargF];
    out->valid = static_cast<int32_t>(row[mh::kWJMargValid]);
    out->n_ties = static_cast<int32_t>(row[mh::kWJMargTies]);
  });
}

// wait for the kernel's row, then the result and the oldest factor's books
static int marginal_finish(mh_ctx * ctx)
{
  static_assert(mh::kWMargWords <= static_cast<int>(kWinRowWords) && mh::kWMargH + 36 == mh::kWMargWords, "mh_icp_window_marginalise layout");
  WindowCall & c = ctx->window;
  if (c.kind == WindowKind::marginal_joint) return marginal_joint_finish(ctx);
  mh_window_marginal * out = c.outputs.marg;
  return marginal_collect(ctx, mh::kWMargWords, mh::kWMargBits, "mh_icp_window_marginalise", out, sizeof(*out), &out->oldest, [&](const double * row) {
    out->prior.pose = 1;
    std::memcpy(out->prior.L_R, c.L1R, sizeof(c.L1R));
    std::memcpy(out->prior.L_t, c.L1t, sizeof(c.L1t));
    std::memcpy(out->prior.H, row + mh::kWMargH, sizeof(out->prior.H));
    std::memcpy(out->prior.b, row + mh::kWMargB, sizeof(out->prior.b));
    out->prior.f = row[mh::kWMargF];
    out->valid = static_cast<int32_t>(row[mh::kWMargValid]);
    out->n_ties = static_cast<int32_t>(row[mh::kWMargTies]);
  });
}

static int mh_icp_window_wait_impl(mh_ctx * ctx)
{
  if (!ctx) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_icp_window_wait: ctx is NULL");
  if (!ctx->window.active) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_window_wait: no window call in flight");
  MH_HIP(ctx, mh_enter(ctx));
  if (ctx->window.kind != WindowKind::optimise) return marginal_finish(ctx);
  return window_run(ctx, 0);
}

static int mh_icp_window_marginalise_impl(const WindowRequest & q)
{
  int rc = window_begin(q);
  if (rc != MH_OK) return rc;
  mh_ctx * ctx = q.icps[0]->ctx;
  rc = marginal_enqueue(ctx);
  if (rc != MH_OK || !q.blocking) return rc;
  return marginal_finish(ctx);
}

static int mh_icp_window_optimise_impl(const WindowRequest & q)
{
  const int rc = window_begin(q);
  if (rc != MH_OK) return rc;
  mh_ctx * ctx = q.icps[0]->ctx;
  if (!q.blocking) return window_enqueue(ctx, q.cfg->iters);
  return window_run(ctx, q.cfg->check_every > 0 ? q.cfg->check_every : q.cfg->iters);
}

extern "C" {

int mh_icp_align(mh_icp * icp, const double R0[9], const double t0[3], const double g_unit[3], const mh_icp_align_config * cfg,
                 mh_icp_align_result * out)
{
  return guarded(icp ? icp->ctx : nullptr, "mh_icp_align", [&]() -> int { return mh_icp_align_impl(icp, R0, t0, g_unit, cfg, out, true); });
}
int mh_icp_align_async(mh_icp * icp, const double R0[9], const double t0[3], const double g_unit[3], const mh_icp_align_config * cfg,
                       mh_icp_align_result * out)
{
  return guarded(icp ? icp->ctx : nullptr, "mh_icp_align_async", [&]() -> int { return mh_icp_align_impl(icp, R0, t0, g_unit, cfg, out, false); });
}
int mh_icp_align_batch(mh_icp * const * icps, size_t B, const double * R0, const double * t0, const double g_unit[3], const mh_icp_align_config * cfg,
                       mh_icp_align_result * out)
{
  return guarded(batch_ctx(icps, B), "mh_icp_align_batch", [&]() -> int { return mh_icp_align_batch_impl(icps, B, R0, t0, g_unit, cfg, out, true); });
}
int mh_icp_align_batch_async(mh_icp * const * icps, size_t B, const double * R0, const double * t0, const double g_unit[3], const mh_icp_align_config * cfg,
                             mh_icp_align_result * out)
{
  return guarded(batch_ctx(icps, B), "mh_icp_align_batch_async", [&]() -> int { return mh_icp_align_batch_impl(icps, B, R0, t0, g_unit, cfg, out, false); });
}
int mh_icp_align_batch_wait(mh_ctx * ctx)
{
  return guarded(ctx, "mh_icp_align_batch_wait", [&]() -> int { return mh_icp_align_batch_wait_impl(ctx); });
}

// The window family: every entry point writes down what it was given (window_request.hpp) and hands that on.
int mh_icp_window_optimise(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                           const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, mh_icp_window_result * out, double * trace_poses)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = true, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .outputs = {.out = out, .trace_poses = trace_poses}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_optimise_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                 const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, mh_icp_window_result * out, double * trace_poses)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = false, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .outputs = {.out = out, .trace_poses = trace_poses}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_async", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_optimise_relin(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                 const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                 mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = true, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .relin_required = true,
                        .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_relin", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_optimise_relin_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                       const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                       mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = false, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .relin_required = true,
                        .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_relin_async", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_optimise_lin(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                               const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                               const mh_window_linear_factor * lin, size_t n_lin, mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = true, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .lin_call = true, .lin = lin, .n_lin = n_lin,
                        .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_lin", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_optimise_lin_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                     const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                     const mh_window_linear_factor * lin, size_t n_lin, mh_icp_window_result * out, double * trace_poses,
                                     uint32_t * evaluated_mask)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = false, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .lin_call = true, .lin = lin, .n_lin = n_lin,
                        .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_lin_async", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
// n_edges == 0: the lin call's own step kernels
int mh_icp_window_optimise_edges(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                 const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                 const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges, size_t n_edges, mh_icp_window_result * out,
                                 double * trace_poses, uint32_t * evaluated_mask)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = true, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges,
                        .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_edges", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_optimise_edges_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                       const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                       const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges, size_t n_edges,
                                       mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = false, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges,
                        .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_edges_async", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_marginalise(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                              const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_window_linear_factor * lin, size_t n_lin,
                              const mh_window_edge * edges, size_t n_edges, mh_window_marginal * out)
{
  const WindowRequest q{.kind = WindowKind::marginal, .blocking = true, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges, .outputs = {.marg = out}};
  return guarded(window_ctx(icps, W), "mh_icp_window_marginalise", [&]() -> int { return mh_icp_window_marginalise_impl(q); });
}
int mh_icp_window_marginalise_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                    const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_window_linear_factor * lin,
                                    size_t n_lin, const mh_window_edge * edges, size_t n_edges, mh_window_marginal * out)
{
  const WindowRequest q{.kind = WindowKind::marginal, .blocking = false, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges, .outputs = {.marg = out}};
  return guarded(window_ctx(icps, W), "mh_icp_window_marginalise_async", [&]() -> int { return mh_icp_window_marginalise_impl(q); });
}
// joint == NULL: mh_icp_window_optimise_edges, its kernels
int mh_icp_window_optimise_joint(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                 const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                 const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges, size_t n_edges, mh_icp_window_result * out,
                                 double * trace_poses, uint32_t * evaluated_mask, const mh_window_joint_factor * joint)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = true, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges,
                        .joint = joint, .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_joint", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_optimise_joint_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                       const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                       const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges, size_t n_edges,
                                       mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask, const mh_window_joint_factor * joint)
{
  const WindowRequest q{.kind = WindowKind::optimise, .blocking = false, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .relin = relin, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges,
                        .joint = joint, .outputs = {.out = out, .trace_poses = trace_poses, .evaluated_mask = evaluated_mask}};
  return guarded(window_ctx(icps, W), "mh_icp_window_optimise_joint_async", [&]() -> int { return mh_icp_window_optimise_impl(q); });
}
int mh_icp_window_marginalise_joint(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                    const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_window_linear_factor * lin,
                                    size_t n_lin, const mh_window_edge * edges, size_t n_edges, const mh_window_joint_factor * joint,
                                    mh_window_joint_marginal * out)
{
  const WindowRequest q{.kind = WindowKind::marginal_joint, .blocking = true, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges, .joint = joint,
                        .outputs = {.jmarg = out}};
  return guarded(window_ctx(icps, W), "mh_icp_window_marginalise_joint", [&]() -> int { return mh_icp_window_marginalise_impl(q); });
}
int mh_icp_window_marginalise_joint_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z, const double * Z_R,
                                          const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg, const mh_window_linear_factor * lin,
                                          size_t n_lin, const mh_window_edge * edges, size_t n_edges, const mh_window_joint_factor * joint,
                                          mh_window_joint_marginal * out)
{
  const WindowRequest q{.kind = WindowKind::marginal_joint, .blocking = false, .icps = icps, .W = W, .R = R, .t = t, .has_Z = has_Z, .Z_R = Z_R, .Z_t = Z_t,
                        .g_unit = g_unit, .cfg = cfg, .lin_call = true, .lin = lin, .n_lin = n_lin, .edges = edges, .n_edges = n_edges, .joint = joint,
                        .outputs = {.jmarg = out}};
  return guarded(window_ctx(icps, W), "mh_icp_window_marginalise_joint_async", [&]() -> int { return mh_icp_window_marginalise_impl(q); });
}
int mh_icp_window_wait(mh_ctx * ctx)
{
  return guarded(ctx, "mh_icp_window_wait", [&]() -> int { return mh_icp_window_wait_impl(ctx); });
}

}  // extern "C"
