// Relocalisation entry points of the C ABI (include/mimosa_hip.h): mh_icp_score_poses[_async], mh_icp_relocalise and
// mh_icp_relocalise_batch.  The kernels are reloc_kernels.hip, the arithmetic reloc_device.hpp; the refinement of a candidate is
// mh_icp_align, of all candidates at once mh_icp_align_batch (chain_api.hip), called as a caller would call them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>

#include "mh_internal.hpp"
#include "reloc_device.hpp"

static_assert(sizeof(mh_pose_score) == sizeof(mh::RelocScore) && MH_RELOC_MAX_REFINE == mh::kRelocMaxRefine, "mh_pose_score layout");

// the factor's mapped pinned block: [winners, 256 B | poses, 96 B each | scores, 24 B each]
constexpr size_t kRelocPosesAt = 256;
static_assert(sizeof(mh::RelocBest) <= kRelocPosesAt, "mh_icp_score_poses layout");
static size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

static int score_begin(mh_icp * icp, const double * R, const double * t, size_t n_poses, const mh_icp_score_config * cfg, mh_pose_score * scores,
                       int32_t * best)
{
  if (!icp || !R || !t || !cfg) return fail(icp ? icp->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_icp_score_poses: NULL argument");
  mh_ctx * ctx = icp->ctx;
  if (icp->binary) return fail(ctx, MH_ERR_UNSUPPORTED, "mh_icp_score_poses: unary factors only");
  if (icp->n_pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: the factor has calls in flight");
  if (n_poses < 1 || n_poses > static_cast<size_t>(MH_RELOC_MAX_POSES)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: n_poses must be in 1..65536");
  if (!(std::isfinite(cfg->gate) && cfg->gate > 0.0)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: the gate must be finite and > 0");
  if (cfg->stride < 1) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: stride must be >= 1");
  if (cfg->top_k < 0 || cfg->top_k > MH_RELOC_MAX_REFINE) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: top_k must be in 0..8");
  if (cfg->top_k > 0 && !best) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: NULL best with top_k > 0");
  for (size_t p = 0; p < n_poses; ++p) {
    bool fin = true;
    for (int i = 0; i < 9; ++i) fin = fin && std::isfinite(R[9 * p + i]);
    for (int i = 0; i < 3; ++i) fin = fin && std::isfinite(t[3 * p + i]);
    if (!fin) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: pose " + std::to_string(p) + " has an entry that is not finite");
  }
  if (icp->no_order || icp->cap_n > icp->n) return fail(ctx, MH_ERR_UNSUPPORTED, "mh_icp_score_poses: not for the factors of the map-sharded path");
  if (icp->n == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_score_poses: the factor has no points");
  if (icp->map->poisoned) return fail(ctx, MH_ERR_HIP, "mh_icp_score_poses: the map is inconsistent after a failed mutation");
  MH_HIP(ctx, mh_enter(ctx));

  const int n = static_cast<int>(icp->n), np = static_cast<int>(n_poses);
  const int m = mh::reloc_sub_count(n, cfg->stride), n_chunks = mh::reloc_chunks(m);
  // the pinned block
  const size_t h_scores_at = kRelocPosesAt + align256(n_poses * 12 * sizeof(double));
  const size_t h_bytes = h_scores_at + align256(n_poses * sizeof(mh_pose_score));
  MH_HIP(ctx, icp->h_reloc.reserve(h_bytes));  // (no call in flight: nothing reads it)
  // the device block
  const size_t d_sub_at = align256(n_poses * 12 * sizeof(double));
  const size_t d_part_at = d_sub_at + align256(static_cast<size_t>(m) * sizeof(float4));
  const size_t d_scores_at = d_part_at + align256(n_poses * static_cast<size_t>(n_chunks) * sizeof(mh::RelocPartial));
  const size_t d_bytes = d_scores_at + align256(n_poses * sizeof(mh::RelocScore));
  MH_HIP(ctx, icp->d_reloc.reserve(d_bytes, ctx->stream, false));

  char * h = static_cast<char *>(icp->h_reloc.p);
  char * d = static_cast<char *>(icp->d_reloc.p);
  double * hp = reinterpret_cast<double *>(h + kRelocPosesAt);
  for (size_t p = 0; p < n_poses; ++p) {
    std::memcpy(hp + 12 * p, R + 9 * p, 9 * sizeof(double));
    std::memcpy(hp + 12 * p + 9, t + 3 * p, 3 * sizeof(double));
  }
  void * d_h = nullptr;  // the pinned block as the device sees it
  MH_HIP(ctx, hipHostGetDevicePointer(&d_h, icp->h_reloc.p, 0));
  char * dh = static_cast<char *>(d_h);
  MH_HIP(ctx, mh::launch_copy16(dh + kRelocPosesAt, d, n_poses * 12 * sizeof(double), ctx->stream));
  MH_HIP(ctx, mh::launch_reloc_gather(static_cast<const float4 *>(icp->d_src.p), icp->ordered ? static_cast<const uint32_t *>(icp->d_perm.p) : nullptr, n,
                                      cfg->stride, reinterpret_cast<float4 *>(d + d_sub_at), ctx->stream));
  mh::RelocScoreArgs a;
  a.map = map_view(icp->map);
  a.sub = reinterpret_cast<const float4 *>(d + d_sub_at);
  a.m = m;
  a.n_chunks = n_chunks;
  a.n_poses = np;
  a.poses = reinterpret_cast<const double *>(d);
  a.gate2 = cfg->gate * cfg->gate;
  a.partials = reinterpret_cast<mh::RelocPartial *>(d + d_part_at);
  auto * d_scores = reinterpret_cast<mh::RelocScore *>(d + d_scores_at);
  hipError_t e = mh::launch_reloc_score(a, ctx->stream);
  if (e == hipSuccess) e = mh::launch_reloc_fold(a.partials, np, n_chunks, m, d_scores, ctx->stream);
  if (e == hipSuccess && scores) e = hipMemcpyAsync(h + h_scores_at, d_scores, n_poses * sizeof(mh::RelocScore), hipMemcpyDeviceToHost, ctx->stream);
  // the winners: always written (top_k == 0: all -1), so the block never holds an earlier call's
  if (e == hipSuccess) e = mh::launch_reloc_select(d_scores, np, cfg->top_k, reinterpret_cast<mh::RelocBest *>(dh), ctx->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return hip_fail(ctx, e, "mh_icp_score_poses: launch");
  }
  icp->score.n_poses = n_poses;
  icp->score.scores = scores;
  icp->score.best = best;
  hold(icp, Held::score);
  return MH_OK;
}

int mhi::score_wait(mh_icp * icp)
{
  mh_ctx * ctx = icp->ctx;
  const mh_icp::ScoreCall & c = icp->score;
  let_go(icp);
  MH_HIP(ctx, mh_enter(ctx));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const char * h = static_cast<const char *>(icp->h_reloc.p);
  if (c.scores) std::memcpy(c.scores, h + kRelocPosesAt + align256(c.n_poses * 12 * sizeof(double)), c.n_poses * sizeof(mh_pose_score));
  if (c.best) std::memcpy(c.best, reinterpret_cast<const mh::RelocBest *>(h)->index, sizeof(int32_t) * MH_RELOC_MAX_REFINE);
  return MH_OK;
}

static int score_impl(mh_icp * icp, const double * R, const double * t, size_t n_poses, const mh_icp_score_config * cfg, mh_pose_score * scores,
                      int32_t * best, bool blocking)
{
  const int rc = score_begin(icp, R, t, n_poses, cfg, scores, best);
  if (rc != MH_OK || !blocking) return rc;
  return mhi::score_wait(icp);
}

static bool key_before(const mh_pose_score & a, int ia, const mh_pose_score & b, int ib)
{
  mh::RelocScore sa, sb;
  std::memcpy(&sa, &a, sizeof(sa));
  std::memcpy(&sb, &b, sizeof(sb));
  return mh::reloc_before(mh::reloc_key_of(sa, ia), mh::reloc_key_of(sb, ib));
}

// (through the public calls only mh_icp_clone hands an identity on, and it copies the config with it: for such callers the
// identity decides first and this comparison cannot fail on its own; it states the contract's fourth condition)
static bool same_reg_config(const mh_reg_config & a, const mh_reg_config & b)
{
  return a.source_voxel_grid_filter_leaf_size == b.source_voxel_grid_filter_leaf_size &&
         a.source_voxel_grid_min_dist_in_voxel == b.source_voxel_grid_min_dist_in_voxel && a.target_ivox_map_leaf_size == b.target_ivox_map_leaf_size &&
         a.target_ivox_map_min_dist_in_voxel == b.target_ivox_map_min_dist_in_voxel && a.num_corres_points == b.num_corres_points &&
         a.max_corres_distance == b.max_corres_distance && a.plane_validity_distance == b.plane_validity_distance &&
         a.lidar_point_noise_std_dev == b.lidar_point_noise_std_dev && a.use_huber == b.use_huber && a.huber_threshold == b.huber_threshold &&
         a.reg_4_dof == b.reg_4_dof && a.project_on_degneneracy == b.project_on_degneneracy && a.degen_thresh_rot == b.degen_thresh_rot &&
         a.degen_thresh_trans == b.degen_thresh_trans;
}

// batch: mh_icp_relocalise_batch — step 2 is one mh_icp_align_batch over work[], and icp is only read
static int relocalise_impl(mh_icp * icp, const double * R, const double * t, size_t n_poses, const double g_unit[3], const mh_icp_reloc_config * cfg,
                           mh_icp_reloc_result * out, bool batch = false, mh_icp * const * work = nullptr, size_t n_work = 0)
{
  if (!icp || !R || !t || !g_unit || !cfg || !out || (batch && !work))
    return fail(icp ? icp->ctx : nullptr, MH_ERR_INVALID_ARG, batch ? "mh_icp_relocalise_batch: NULL argument" : "mh_icp_relocalise: NULL argument");
  mh_ctx * ctx = icp->ctx;
  if (cfg->score.top_k == 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise: score.top_k must be in 1..8");
  if (!(std::isfinite(cfg->final_gate) && cfg->final_gate > 0.0)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise: final_gate must be finite and > 0");
  // what mh_icp_align would refuse, before anything runs (the factor's own refusals are mh_icp_score_poses's, just below)
  if (const int no = mhi::align_check_config(ctx, cfg->align, "mh_icp_relocalise: align.", "mh_icp_relocalise: align's ")) return no;
  if (batch) {
    // the work factors, before anything runs: enough of them, each a free clone of icp, none twice
    const size_t need = std::min(static_cast<size_t>(std::max(cfg->score.top_k, 0)), n_poses);
    if (n_work < need) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise_batch: fewer work factors than candidates to refine");
    if (ctx->align_batch.n) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise_batch: the context has a batch call in flight");
    for (size_t c = 0; c < n_work; ++c) {
      const mh_icp * w = work[c];
      if (!w) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise_batch: NULL work factor");
      if (w == icp) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise_batch: a work factor is the scored factor itself");
      if (w->cloud_id != icp->cloud_id || w->n != icp->n || w->map != icp->map || w->ctx != ctx || w->binary != icp->binary ||
          !same_reg_config(w->cfg, icp->cfg))
        return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise_batch: a work factor is not a clone of the scored factor");
      if (w->n_pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise_batch: a work factor has calls in flight");
      for (size_t g = 0; g < c; ++g)
        if (work[g] == w) return fail(ctx, MH_ERR_INVALID_ARG, "mh_icp_relocalise_batch: the same work factor twice");
    }
  }
  std::memset(static_cast<void *>(out), 0, sizeof(*out));
  out->best = -1;
  // 1. score and select: one wait
  int32_t best[MH_RELOC_MAX_REFINE];
  int rc = score_impl(icp, R, t, n_poses, &cfg->score, nullptr, best, true);
  if (rc != MH_OK) return rc;
  const mh::RelocBest coarse = *static_cast<const mh::RelocBest *>(icp->h_reloc.p);
  int nc = 0;
  while (nc < MH_RELOC_MAX_REFINE && best[nc] >= 0) ++nc;
  out->n_candidates = nc;
  // 2. the align chain from each, in rank order: one after another on icp, or (batch) side by side, candidate c on work[c]
  std::unique_ptr<mh_icp_align_result[]> ar(new mh_icp_align_result[nc]);
  double Ra[9 * MH_RELOC_MAX_REFINE], ta[3 * MH_RELOC_MAX_REFINE];
  for (int c = 0; c < nc; ++c) {
    mh_icp_reloc_candidate & q = out->cand[c];
    q.index = best[c];
    std::memcpy(&q.coarse, &coarse.score[c], sizeof(q.coarse));
    std::memcpy(Ra + 9 * c, R + 9 * static_cast<size_t>(q.index), 9 * sizeof(double));
    std::memcpy(ta + 3 * c, t + 3 * static_cast<size_t>(q.index), 3 * sizeof(double));
  }
  if (batch) {
    for (int c = 0; c < nc; ++c)
      if ((rc = mh_icp_reset(work[c])) != MH_OK) return rc;
    rc = mhi::align_batch(work, static_cast<size_t>(nc), Ra, ta, g_unit, &cfg->align, ar.get());
    if (rc != MH_OK) return rc;
  } else {
    for (int c = 0; c < nc; ++c) {
      rc = mh_icp_reset(icp);
      if (rc == MH_OK) rc = mh_icp_align(icp, Ra + 9 * c, ta + 3 * c, g_unit, &cfg->align, &ar[c]);
      if (rc != MH_OK) {
        (void)mh_icp_reset(icp);
        return rc;
      }
    }
    rc = mh_icp_reset(icp);
    if (rc != MH_OK) return rc;
  }
  for (int c = 0; c < nc; ++c) {
    mh_icp_reloc_candidate & q = out->cand[c];
    q.iters = ar[c].iters;
    q.converged = ar[c].converged;
    std::memcpy(q.R, ar[c].R, sizeof(q.R));
    std::memcpy(q.t, ar[c].t, sizeof(q.t));
    std::memcpy(Ra + 9 * c, ar[c].R, sizeof(q.R));
    std::memcpy(ta + 3 * c, ar[c].t, sizeof(q.t));
  }
  // 3. the aligned poses once more: every point, the final gate
  mh_icp_score_config fc;
  fc.gate = cfg->final_gate;
  fc.stride = 1;
  fc.top_k = nc;
  mh_pose_score fine[MH_RELOC_MAX_REFINE];
  rc = score_impl(icp, Ra, ta, static_cast<size_t>(nc), &fc, fine, best, true);
  if (rc != MH_OK) return rc;
  for (int c = 0; c < nc; ++c) out->cand[c].fine = fine[c];
  // 4. the first under the key on `fine` (what the device selected; held to the same comparison here)
  int w = 0;
  for (int c = 1; c < nc; ++c)
    if (key_before(fine[c], c, fine[w], w)) w = c;
  if (best[0] != w) return fail(ctx, MH_ERR_HIP, "mh_icp_relocalise: the device ranking of the aligned poses disagrees with the host's");
  out->best = w;
  std::memcpy(out->R, out->cand[w].R, sizeof(out->R));
  std::memcpy(out->t, out->cand[w].t, sizeof(out->t));
  return MH_OK;
}

extern "C" {

int mh_icp_score_poses(mh_icp * icp, const double * R, const double * t, size_t n_poses, const mh_icp_score_config * cfg, mh_pose_score * scores,
                       int32_t * best)
{
  return guarded(icp ? icp->ctx : nullptr, "mh_icp_score_poses", [&]() -> int { return score_impl(icp, R, t, n_poses, cfg, scores, best, true); });
}
int mh_icp_score_poses_async(mh_icp * icp, const double * R, const double * t, size_t n_poses, const mh_icp_score_config * cfg, mh_pose_score * scores,
                             int32_t * best)
{
  return guarded(icp ? icp->ctx : nullptr, "mh_icp_score_poses_async", [&]() -> int { return score_impl(icp, R, t, n_poses, cfg, scores, best, false); });
}
int mh_icp_relocalise(mh_icp * icp, const double * R, const double * t, size_t n_poses, const double g_unit[3], const mh_icp_reloc_config * cfg,
                      mh_icp_reloc_result * out)
{
  return guarded(icp ? icp->ctx : nullptr, "mh_icp_relocalise", [&]() -> int { return relocalise_impl(icp, R, t, n_poses, g_unit, cfg, out); });
}
int mh_icp_relocalise_batch(mh_icp * icp, mh_icp * const * work, size_t n_work, const double * R, const double * t, size_t n_poses, const double g_unit[3],
                            const mh_icp_reloc_config * cfg, mh_icp_reloc_result * out)
{
  return guarded(icp ? icp->ctx : nullptr, "mh_icp_relocalise_batch",
                 [&]() -> int { return relocalise_impl(icp, R, t, n_poses, g_unit, cfg, out, true, work, n_work); });
}

}  // extern "C"
