// C ABI of the target map (include/mimosa_hip.h: mh_map_*): IncrementalVoxelMapPCL / gtsam_points::iVox, resident on
// and maintained by the device.
//
// Reference: include/mimosa/lidar/incremental_voxel_map.hpp:22-54, src/lidar/incremental_voxel_map.cpp:14-62,
// Geometric::updateMap src/lidar/geometric.cpp:483-495 (f32 world transform, copy-then-insert).
// The host side is bookkeeping: capacities, the three small read-backs an insert needs (new voxels, new blocks, totals),
// the LRU cadence (every lru_clear_cycle-th insert).  Kernels: map_kernels.hip.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "carve_device.hpp"
#include "mh_internal.hpp"
#include "rebuild_plan.hpp"

namespace
{

mh::MapArrays arrays_of(const mh_map * m)
{
  mh::MapArrays a;
  a.table = static_cast<int4 *>(m->d_table.p);
  a.table_mask = static_cast<uint32_t>(m->table_cap - 1);
  a.cells = static_cast<uint32_t *>(m->d_cells.p);
  a.buckets = static_cast<float4 *>(m->d_buckets.p);
  a.qbuckets = static_cast<uint32_t *>(m->d_qbuckets.p);
  a.vox = static_cast<int4 *>(m->d_vox.p);
  a.lru = static_cast<unsigned long long *>(m->d_lru.p);
  a.state = m->d_state.as<mh::MapState>();
  return a;
}

int fetch_state(mh_map * m)
{
  mh_ctx * ctx = m->ctx;
  MH_HIP(ctx, hipMemcpyAsync(m->h_state, m->d_state.as<mh::MapState>(), sizeof(mh::MapState), hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MH_OK;
}
int push_state(mh_map * m)
{
  mh_ctx * ctx = m->ctx;
  m->h_state->n_voxels = m->n_voxels;
  m->h_state->n_blocks = m->n_blocks;
  m->h_state->n_points = m->n_points;
  m->h_state->bad_coord = 0;
  MH_HIP(ctx, hipMemcpyAsync(m->d_state.as<mh::MapState>(), m->h_state, sizeof(mh::MapState), hipMemcpyHostToDevice, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // h_state is reused as the read-back target
  return MH_OK;
}

size_t grow(size_t have, size_t need) { return need <= have ? have : need + need / 2 + 64; }

// voxel arrays for at least n voxels (+ one bucket of slack: the k-NN kernels' branch-free loads may touch "slot 31 of
// the last voxel")
int ensure_voxels(mh_map * m, size_t n)
{
  if (n + 2 <= m->vox_cap) return MH_OK;
  mh_ctx * ctx = m->ctx;
  const size_t cap = grow(m->vox_cap, n + 2);
  MH_HIP(ctx, m->d_buckets.reserve(cap * mh::kBucketStride * sizeof(float4), ctx->stream, true));
  MH_HIP(ctx, m->d_qbuckets.reserve(cap * mh::kBucketStride * sizeof(uint32_t), ctx->stream, true));
  MH_HIP(ctx, m->d_vox.reserve(cap * sizeof(int4), ctx->stream, true));
  MH_HIP(ctx, m->d_lru.reserve(cap * sizeof(unsigned long long), ctx->stream, true));
  m->vox_cap = cap;
  return MH_OK;
}
// cell tables for at least n blocks; new tables start empty
int ensure_blocks(mh_map * m, size_t n, size_t n_initialised)
{
  mh_ctx * ctx = m->ctx;
  if (n + 1 > m->block_cap) {
    const size_t cap = grow(m->block_cap, n + 1);
    MH_HIP(ctx, m->d_cells.reserve(cap * mh::kCellsPerBlock * sizeof(uint32_t), ctx->stream, true));
    m->block_cap = cap;
  }
  static_assert(mh::kEmptyCell == 0u, "the byte pattern of the fill below");
  if (n > n_initialised)
    MH_HIP(ctx, hipMemsetAsync(static_cast<uint32_t *>(m->d_cells.p) + n_initialised * mh::kCellsPerBlock, 0x00,
                               (n - n_initialised) * mh::kCellsPerBlock * sizeof(uint32_t), ctx->stream));
  return MH_OK;
}
// hash table with load <= 0.5 for up to n_blocks_bound blocks
int ensure_table(mh_map * m, size_t n_blocks_bound)
{
  if (n_blocks_bound * 2 <= m->table_cap) return MH_OK;
  mh_ctx * ctx = m->ctx;
  size_t cap = m->table_cap ? m->table_cap : 1024;
  while (cap < n_blocks_bound * 2) cap *= 2;
  DevBuf nt;
  MH_HIP(ctx, nt.reserve(cap * sizeof(int4), ctx->stream, false));
  MH_HIP(ctx, hipMemsetAsync(nt.p, 0xFF, cap * sizeof(int4), ctx->stream));
  if (m->table_cap)
    MH_HIP(ctx, mh::launch_map_rehash(static_cast<const int4 *>(m->d_table.p), static_cast<uint32_t>(m->table_cap), static_cast<int4 *>(nt.p),
                                      static_cast<uint32_t>(cap), ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  m->d_table = std::move(nt);
  m->table_cap = cap;
  return MH_OK;
}

int ensure_scratch(mh_map * m, size_t n)
{
  mh_ctx * ctx = m->ctx;
  const size_t k = n ? n : 1;
  MH_HIP(ctx, m->s_pts.reserve(k * sizeof(float4), ctx->stream, false));
  MH_HIP(ctx, m->s_group.reserve(mh::map_group_bytes(k), ctx->stream, false));
  MH_HIP(ctx, m->s_seg_vid.reserve(k * sizeof(uint32_t), ctx->stream, false));
  MH_HIP(ctx, m->s_seg_added.reserve(k * sizeof(uint32_t), ctx->stream, false));
  MH_HIP(ctx, m->s_blk_new.reserve(((k + 255) / 256 + 1) * sizeof(uint32_t), ctx->stream, false));
  return MH_OK;
}
mh::InsertScratch scratch_of(const mh_map * m)
{
  mh::InsertScratch s;
  s.pts = static_cast<float4 *>(m->s_pts.p);
  s.group = m->s_group.p;
  s.seg_vid = static_cast<uint32_t *>(m->s_seg_vid.p);
  s.seg_added = static_cast<uint32_t *>(m->s_seg_added.p);
  s.blk_new = static_cast<uint32_t *>(m->s_blk_new.p);
  return s;
}

// The compaction both erasures share (the LRU purge, and a carve that empties voxels): of the map's nv voxels those with
// s_flags[v] != 0 survive, voxel v at id s_pos[v] (keep of them), in their order and with their LRU stamps; buckets, coarse
// copies, coordinates and stamps move into fresh arrays, and the block table and every cell word are rebuilt from the
// survivors' coordinates.
int compact_voxels(mh_map * m, uint32_t nv, uint32_t keep, const char * what, const char * what_words)
{
  mh_ctx * ctx = m->ctx;
  int rc = MH_OK;
  mh::MapArrays a = arrays_of(m);
  // fresh voxel arrays; the old ones are the compaction source
  DevBuf ob = std::move(m->d_buckets), oq = std::move(m->d_qbuckets), ov = std::move(m->d_vox), ol = std::move(m->d_lru);
  const size_t old_cap = m->vox_cap;
  m->vox_cap = 0;
  auto restore = [&]() {  // (whatever of the fresh arrays exists is released by the assignments)
    m->d_buckets = std::move(ob);
    m->d_qbuckets = std::move(oq);
    m->d_vox = std::move(ov);
    m->d_lru = std::move(ol);
    m->vox_cap = old_cap;
  };
  rc = ensure_voxels(m, keep);
  if (rc != MH_OK) {
    restore();
    return rc;
  }
  mh::MapArrays src = a, dst = arrays_of(m);
  src.buckets = static_cast<float4 *>(ob.p);
  src.qbuckets = static_cast<uint32_t *>(oq.p);
  src.vox = static_cast<int4 *>(ov.p);
  src.lru = static_cast<unsigned long long *>(ol.p);
  m->n_voxels = keep;
  m->n_blocks = 0;
  m->n_points = 0;
  rc = push_state(m);
  hipError_t e = hipSuccess;
  if (rc == MH_OK) e = mh::launch_map_purge_compact(src, dst, nv, static_cast<const uint32_t *>(m->s_flags.p), static_cast<const uint32_t *>(m->s_pos.p), ctx->stream);
  if (rc == MH_OK && e == hipSuccess) e = hipMemsetAsync(m->d_table.p, 0xFF, m->table_cap * sizeof(int4), ctx->stream);
  if (rc == MH_OK && e == hipSuccess) e = mh::launch_map_claim_blocks(dst, 0, keep, ctx->stream);
  if (rc == MH_OK && e == hipSuccess) rc = fetch_state(m);
  if (rc != MH_OK || e != hipSuccess) {
    // the fresh arrays and the table are half written and the counters already name the compacted map: there is no way back
    // to the old state from here.  The map is marked unusable instead of being left to answer from garbage ids.
    (void)hipStreamSynchronize(ctx->stream);
    m->poisoned = true;
    return rc != MH_OK ? rc : hip_fail(ctx, e, what);  // (the old arrays go back on the way out)
  }
  m->n_blocks = m->h_state->n_blocks;
  m->n_points = m->h_state->n_points;
  ob.release();
  oq.release();
  ov.release();
  ol.release();
  rc = ensure_blocks(m, m->n_blocks, 0);
  if (rc != MH_OK) {
    m->poisoned = true;  // voxels without their cell words
    return rc;
  }
  dst = arrays_of(m);
  {
    hipError_t e2 = mh::launch_map_write_words(dst, 0, keep, ctx->stream);
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(ctx->stream);
    if (e2 != hipSuccess) {
      m->poisoned = true;
      return hip_fail(ctx, e2, what_words);
    }
  }
  return MH_OK;
}

// iVox's LRU purge: voxels with lru + horizon < counter are erased, the survivors keep their
// order; tables are rebuilt.  Everything stays on the device: the survivors are compacted into fresh arrays.
int purge_lru(mh_map * m)
{
  mh_ctx * ctx = m->ctx;
  if (m->n_voxels == 0) return MH_OK;
  const uint32_t nv = m->n_voxels;
  MH_HIP(ctx, m->s_flags.reserve(nv * sizeof(uint32_t), ctx->stream, false));
  MH_HIP(ctx, m->s_pos.reserve(nv * sizeof(uint32_t), ctx->stream, false));
  MH_HIP(ctx, m->s_temp.reserve(mh::map_temp_bytes(nv), ctx->stream, false));
  mh::MapArrays a = arrays_of(m);
  MH_HIP(ctx, mh::launch_map_purge_flags(a, nv, static_cast<unsigned long long>(m->cfg.lru_horizon), m->lru_counter,
                                         static_cast<uint32_t *>(m->s_flags.p), static_cast<uint32_t *>(m->s_pos.p), m->s_temp.p, m->s_temp.cap,
                                         ctx->stream));
  int rc = fetch_state(m);
  if (rc != MH_OK) return rc;
  const uint32_t keep = m->h_state->n_keep;
  if (keep == nv) return MH_OK;
  rc = compact_voxels(m, nv, keep, "mh_map_insert: LRU purge", "mh_map_insert: LRU purge (cell words)");
  if (rc != MH_OK) return rc;
  m->purges++;
  return MH_OK;
}

// A chunk of keyframes inserted as one batch (mh_map_rebuild_from_keyframes): after phase C every touched voxel's stamp becomes
// lru_counter + (the chunk's last keyframe with a point in it).  rel: the kc + 1 prefix offsets of the chunk, on the device.
struct ChunkStamps
{
  const uint32_t * d_rel;
  uint32_t kc;
};

// Phases A.2 to C of an insert of n > 0 points whose phase A.1 is enqueued (the points in s_pts, their keys in the batch hash):
// grouping, new voxels, blocks, FlatContainer::add per touched voxel.  The insert and the rebuild share it; `stamps` is the rebuild's.
// `who` names the entry point in error texts.
int insert_grouped(mh_map * m, const char * who, size_t n, const ChunkStamps * stamps)
{
  mh_ctx * ctx = m->ctx;
  const mh::InsertScratch s = scratch_of(m);
  mh::MapArrays a = arrays_of(m);
  MH_HIP(ctx, mh::launch_map_insert_group(a, static_cast<uint32_t>(n), s, ctx->stream));
  int rc = fetch_state(m);
  if (rc != MH_OK) return rc;
  if (m->h_state->bad_coord) {
    (void)push_state(m);  // clears the flag; nothing was modified yet
    return fail(ctx, MH_ERR_UNSUPPORTED, std::string(who) + ": a point is NaN or its voxel coordinate exceeds +-2^20");
  }
  const uint32_t n_new = m->h_state->n_new_voxels, before = m->n_voxels;
  if (static_cast<uint64_t>(before) + n_new >= (1u << 27)) return fail(ctx, MH_ERR_UNSUPPORTED, std::string(who) + ": more than 2^27 voxels");
  rc = ensure_voxels(m, static_cast<size_t>(before) + n_new);
  if (rc == MH_OK && n_new) rc = ensure_table(m, static_cast<size_t>(m->n_blocks) + 8 * static_cast<size_t>(n_new));
  if (rc != MH_OK) return rc;
  a = arrays_of(m);
  if (n_new) {
    MH_HIP(ctx, mh::launch_map_create_voxels(a, static_cast<uint32_t>(n), before, m->lru_counter, s, ctx->stream));
    rc = fetch_state(m);
    if (rc != MH_OK) return rc;
    const uint32_t nb = m->h_state->n_blocks;
    rc = ensure_blocks(m, nb, m->n_blocks);
    if (rc != MH_OK) return rc;
    m->n_blocks = nb;
    a = arrays_of(m);
  }
  MH_HIP(ctx, mh::launch_map_insert_points(a, static_cast<uint32_t>(n), before + n_new, static_cast<uint32_t>(m->cfg.max_points_in_cell), m->min_sq,
                                           m->inv_leaf, m->lru_counter, s, ctx->stream));
  if (stamps) MH_HIP(ctx, mh::launch_map_rebuild_stamp(a, stamps->d_rel, stamps->kc, static_cast<uint32_t>(n), m->lru_counter, s, ctx->stream));
  rc = fetch_state(m);
  if (rc != MH_OK) return rc;
  m->n_voxels = m->h_state->n_voxels;
  m->n_points = m->h_state->n_points;
  return MH_OK;
}

// iVox::insert on a batch already on the device, optional f32 transform (12 floats on the device).  Synchronous: the map is
// current when this returns.  (It speaks as mh_map_insert whoever calls it.)
int insert_device(mh_map * m, const DeviceCloud & src, const float * d_Rt12)
{
  mh_ctx * ctx = m->ctx;
  const size_t n = src.n;
  if (const int rc = check_cloud_size(ctx, "mh_map_insert", n); rc != MH_OK) return rc;
  if (m->poisoned) return fail(ctx, MH_ERR_HIP, "mh_map_insert: the map is inconsistent after a failed mutation");
  // Factors of other contexts (HIP streams) may be reading this map: the arrays are modified in place and may be
  // reallocated, so the streams of the contexts that hold factors on it are waited for first (none in the usual
  // copy-then-insert: the fresh copy has no factor yet).
  MH_HIP(ctx, map_wait_readers(m));
  if (n) {
    int rc = ensure_scratch(m, n);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh::launch_map_insert_assign(arrays_of(m), src.d, static_cast<uint32_t>(n), static_cast<uint32_t>(src.stride), d_Rt12, m->inv_leaf, scratch_of(m),
                                             ctx->stream));
    rc = insert_grouped(m, "mh_map_insert", n, nullptr);
    if (rc != MH_OK) return rc;
  }
  m->inserts++;
  // ++lru_counter; every lru_clear_cycle inserts the stale voxels go
  if ((++m->lru_counter) % static_cast<uint64_t>(m->cfg.lru_clear_cycle) == 0) return purge_lru(m);
  return MH_OK;
}

// mh_map_rebuild_from_keyframes on a fresh map: the listed keyframes chunk by chunk (rebuild_plan.hpp).  sizes / src: points and
// arena offset per listed keyframe; poses: 12 floats each (R row-major, t).
int rebuild_fill(mh_map * m, const mh_keyframes * kf, const std::vector<uint64_t> & sizes, const std::vector<uint64_t> & src, const float * R, const float * t,
                 uint64_t budget, mh_map_rebuild_result * res)
{
  mh_ctx * ctx = m->ctx;
  const char * who = "mh_map_rebuild_from_keyframes";
  const size_t K = sizes.size();
  const std::vector<mh::RebuildChunk> plan = mh::rebuild_plan(sizes.data(), K, m->lru_counter, static_cast<uint64_t>(m->cfg.lru_clear_cycle), budget);
  for (const mh::RebuildChunk & c : plan)
    if (const int rc = check_cloud_size(ctx, who, c.points); rc != MH_OK) return rc;
  // the whole plan goes to the device once: [RebuildKeyframe x K | prefix offsets: (k1 - k0 + 1) words per chunk]
  const size_t kf_bytes = K * sizeof(mh::RebuildKeyframe), rel_words = K + plan.size();
  DevTemp<char> d_plan;
  const size_t plan_bytes = kf_bytes + rel_words * sizeof(uint32_t);
  if (K) {
    MH_HIP(ctx, d_plan.alloc(plan_bytes));
    size_t pinned_bytes = 4096;  // (the pinned cache keeps blocks by their exact size)
    while (pinned_bytes < plan_bytes) pinned_bytes <<= 1;
    PinnedBuf h_plan;
    MH_HIP(ctx, h_plan.reserve(plan_bytes, pinned_bytes));
    mh::RebuildKeyframe * hk = h_plan.as<mh::RebuildKeyframe>();
    uint32_t * hr = reinterpret_cast<uint32_t *>(h_plan.as<char>() + kf_bytes);
    for (size_t j = 0; j < K; ++j) {
      hk[j].src = src[j];
      std::memcpy(hk[j].Rt12, R + 9 * j, 9 * sizeof(float));
      std::memcpy(hk[j].Rt12 + 9, t + 3 * j, 3 * sizeof(float));
    }
    size_t w = 0;
    for (const mh::RebuildChunk & c : plan) {
      uint32_t at = 0;
      for (size_t j = c.k0; j < c.k1; ++j) {
        hr[w++] = at;
        at += static_cast<uint32_t>(sizes[j]);
      }
      hr[w++] = at;
    }
    hipError_t e = hipMemcpyAsync(d_plan.p, h_plan.p, plan_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, who);
  }
  const mh::RebuildKeyframe * d_kf = reinterpret_cast<const mh::RebuildKeyframe *>(d_plan.p);
  const uint32_t * d_rel = reinterpret_cast<const uint32_t *>(d_plan.p + kf_bytes);
  size_t w = 0;
  for (const mh::RebuildChunk & c : plan) {
    const uint32_t kc = static_cast<uint32_t>(c.k1 - c.k0);
    if (c.points) {
      const size_t n = static_cast<size_t>(c.points);
      int rc = ensure_scratch(m, n);
      if (rc != MH_OK) return rc;
      MH_HIP(ctx, mh::launch_map_rebuild_assign(arrays_of(m), kf->arena(), d_kf + c.k0, d_rel + w, kc, static_cast<uint32_t>(n), m->inv_leaf, scratch_of(m),
                                                ctx->stream));
      const ChunkStamps stamps{d_rel + w, kc};
      rc = insert_grouped(m, who, n, &stamps);
      if (rc != MH_OK) return rc;
    }
    w += kc + 1;
    m->inserts += kc;
    m->lru_counter += kc;
    res->keyframes += kc;
    res->points_offered += static_cast<int64_t>(c.points);
    res->chunks++;
    if (c.purge_after) {
      const int rc = purge_lru(m);
      if (rc != MH_OK) return rc;
      res->purges++;
    }
  }
  res->n_points = static_cast<int64_t>(m->n_points);
  res->n_voxels = m->n_voxels;
  return MH_OK;
}

// What insert_device would do to this batch, without doing it: phase A as the insert runs it, then phase C's rule on buckets held
// in registers (map_preview_points_kernel).  Nothing a reader of the map sees is written — only the insert scratch and the
// per-insert words of the state block — so the streams of other contexts' factors are not waited for.  One wait for the device.
int preview_device(mh_map * m, const char * who, const DeviceCloud & src, const float * d_Rt12, mh_map_insert_preview * out, uint8_t * outcome)
{
  mh_ctx * ctx = m->ctx;
  const size_t n = src.n;
  std::memset(out, 0, sizeof(*out));
  if (const int rc = check_cloud_size(ctx, who, n); rc != MH_OK) return rc;
  if (m->poisoned) return fail(ctx, MH_ERR_HIP, std::string(who) + ": the map is inconsistent after a failed mutation");
  if (n == 0) return MH_OK;
  int rc = ensure_scratch(m, n);
  if (rc != MH_OK) return rc;
  const size_t words = 2 * n * sizeof(uint32_t);
  MH_HIP(ctx, m->s_preview.reserve(words + n, ctx->stream, false));
  uint32_t * seg_close = static_cast<uint32_t *>(m->s_preview.p);
  uint8_t * d_outcome = outcome ? reinterpret_cast<uint8_t *>(m->s_preview.p) + words : nullptr;
  const mh::InsertScratch s = scratch_of(m);
  const mh::MapArrays a = arrays_of(m);
  MH_HIP(ctx, mh::launch_map_insert_prepare(a, src.d, static_cast<uint32_t>(n), static_cast<uint32_t>(src.stride), d_Rt12, m->inv_leaf, s, ctx->stream));
  // a rejected batch (bad_coord) is grouped well-formed under voxel (0,0,0) and the kernel below only reads: it can run before the
  // flag has been looked at, which spares a second wait
  MH_HIP(ctx, mh::launch_map_preview_points(a, static_cast<uint32_t>(n), m->n_voxels, static_cast<uint32_t>(m->cfg.max_points_in_cell), m->min_sq, s,
                                            seg_close, seg_close + n, d_outcome, ctx->stream));
  rc = fetch_state(m);
  if (rc != MH_OK) return rc;
  if (m->h_state->bad_coord) {
    (void)push_state(m);  // clears the flag, as the insert does
    return fail(ctx, MH_ERR_UNSUPPORTED, std::string(who) + ": a point is NaN or its voxel coordinate exceeds +-2^20");
  }
  if (static_cast<uint64_t>(m->n_voxels) + m->h_state->n_new_voxels >= (1u << 27)) return fail(ctx, MH_ERR_UNSUPPORTED, std::string(who) + ": more than 2^27 voxels");
  if (outcome) {
    MH_HIP(ctx, hipMemcpyAsync(outcome, d_outcome, n, hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  out->n_points = static_cast<int64_t>(n);
  out->n_added = m->h_state->preview[0];
  out->n_too_close = m->h_state->preview[1];
  out->n_voxel_full = m->h_state->preview[2];
  out->n_touched_voxels = m->h_state->n_segments;
  out->n_new_voxels = m->h_state->n_new_voxels;
  return MH_OK;
}

// mh_map_carve* on a batch already on the device.  The image and the per-voxel words are scratch; with cfg.apply == 0 nothing else
// is written (the counters travel in MapState::carve), so — like the insert preview — the streams of other contexts' factors
// are not waited for.  With apply the buckets are compacted in place, and voxels left without a point are erased by the LRU
// purge's compaction.
int carve_check(const mh_ctx * ctx, const char * who, size_t stride, const double * origin, const double * R, const double * t,
                const mh_map_carve_config & c)
{
  const std::string w(who);
  if (const int rc = check_stride(ctx, who, stride); rc != MH_OK) return rc;
  if (c.grid < mh::kCarveGridMin || c.grid > mh::kCarveGridMax) return fail(ctx, MH_ERR_INVALID_ARG, w + ": grid must be in 4..512");
  if (c.ring < 0 || c.ring > mh::kCarveRingMax) return fail(ctx, MH_ERR_INVALID_ARG, w + ": ring must be in 0..2");
  if (c.apply != 0 && c.apply != 1) return fail(ctx, MH_ERR_INVALID_ARG, w + ": apply must be 0 or 1");
  for (double v : {c.range_min, c.range_max, c.margin_abs, c.margin_rel})
    if (!std::isfinite(v)) return fail(ctx, MH_ERR_INVALID_ARG, w + ": a config value is not finite");
  if (!(c.range_min > 0) || !(c.range_min < c.range_max)) return fail(ctx, MH_ERR_INVALID_ARG, w + ": 0 < range_min < range_max is required");
  if (c.margin_abs < 0 || c.margin_rel < 0) return fail(ctx, MH_ERR_INVALID_ARG, w + ": margins must be >= 0");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(R[i])) return fail(ctx, MH_ERR_INVALID_ARG, w + ": the pose is not finite");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(t[i]) || !std::isfinite(origin[i])) return fail(ctx, MH_ERR_INVALID_ARG, w + ": the pose or the origin is not finite");
  return MH_OK;
}

int carve_device(mh_map * m, const char * who, const DeviceCloud & src, const double * origin, const double * R, const double * t,
                 const mh_map_carve_config & c, mh_map_carve_result * out)
{
  mh_ctx * ctx = m->ctx;
  const size_t n = src.n;
  std::memset(out, 0, sizeof(*out));
  if (const int rc = check_cloud_size(ctx, who, n); rc != MH_OK) return rc;
  if (m->poisoned) return fail(ctx, MH_ERR_HIP, std::string(who) + ": the map is inconsistent after a failed mutation");
  if (n == 0) return MH_OK;
  if (c.apply) MH_HIP(ctx, map_wait_readers(m));
  mh::CarveParams P;
  std::memcpy(P.R, R, sizeof(P.R));
  std::memcpy(P.t, t, sizeof(P.t));
  std::memcpy(P.origin, origin, sizeof(P.origin));
  P.range_min2 = c.range_min * c.range_min;
  P.range_max2 = c.range_max * c.range_max;
  P.margin_abs = c.margin_abs;
  P.margin_rel = c.margin_rel;
  P.N = c.grid;
  P.ring = c.ring;
  double sensor_W[3];  // for the per-voxel early-out only
  for (int a = 0; a < 3; ++a) sensor_W[a] = R[3 * a] * origin[0] + R[3 * a + 1] * origin[1] + R[3 * a + 2] * origin[2] + t[a];
  const uint32_t nv = m->n_voxels;
  const size_t nvs = nv ? nv : 1;
  MH_HIP(ctx, m->s_carve_img.reserve(mh::carve_image_bytes(c.grid), ctx->stream, false));
  MH_HIP(ctx, m->s_carve_vox.reserve(nvs * sizeof(uint32_t), ctx->stream, false));
  MH_HIP(ctx, m->s_flags.reserve(nvs * sizeof(uint32_t), ctx->stream, false));
  if (c.apply) {  // what erasing emptied voxels needs, while a failure still leaves the map untouched
    MH_HIP(ctx, m->s_pos.reserve(nvs * sizeof(uint32_t), ctx->stream, false));
    MH_HIP(ctx, m->s_temp.reserve(mh::map_temp_bytes(nv), ctx->stream, false));
  }
  MH_HIP(ctx, mh::launch_carve_image(src.d, static_cast<uint32_t>(n), static_cast<uint32_t>(src.stride), P, m->s_carve_img.p, ctx->stream));
  MH_HIP(ctx, mh::launch_carve_test(arrays_of(m), nv, P, m->s_carve_img.p, m->cfg.leaf_size, sensor_W, c.range_max, c.apply != 0,
                                    static_cast<uint32_t *>(m->s_carve_vox.p), static_cast<uint32_t *>(m->s_flags.p), ctx->stream));
  int rc = fetch_state(m);
  if (rc != MH_OK) return rc;
  const unsigned long long * c6 = m->h_state->carve;
  out->n_obs_used = static_cast<int64_t>(c6[0]);
  out->n_cells_hit = static_cast<int64_t>(c6[1]);
  out->n_tested = static_cast<int64_t>(c6[2]);
  out->n_removed = static_cast<int64_t>(c6[3]);
  out->n_voxels_touched = static_cast<int64_t>(c6[4]);
  out->n_voxels_emptied = static_cast<int64_t>(c6[5]);
  if (!c.apply) return MH_OK;
  m->n_points = m->h_state->n_points;
  if (out->n_voxels_emptied == 0) return MH_OK;
  // emptied voxels go the way the LRU purge's go: positions of the survivors, then the shared compaction.  Until it is through
  // the map holds voxels without a point, which nothing else tolerates: a failure on the way leaves it marked unusable.
  const hipError_t e = mh::launch_map_keep_positions(arrays_of(m), nv, static_cast<const uint32_t *>(m->s_flags.p), static_cast<uint32_t *>(m->s_pos.p),
                                                     m->s_temp.p, m->s_temp.cap, ctx->stream);
  rc = e == hipSuccess ? fetch_state(m) : hip_fail(ctx, e, who);
  if (rc != MH_OK) {
    m->poisoned = true;
    return rc;
  }
  const uint32_t keep = m->h_state->n_keep;
  const std::string what = std::string(who) + ": compaction", what_words = std::string(who) + ": compaction (cell words)";
  rc = compact_voxels(m, nv, keep, what.c_str(), what_words.c_str());
  if (rc != MH_OK) {
    m->poisoned = true;  // also where the purge could go back to its old arrays: here they hold the emptied voxels
    return rc;
  }
  if (m->n_blocks == 0) {  // nothing is left: block 0's table as mh_map_create leaves it
    MH_HIP(ctx, hipMemsetAsync(m->d_cells.p, 0x00, mh::kCellsPerBlock * sizeof(uint32_t), ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MH_OK;
}

void map_free(mh_map * m)
{
  if (m->h_state) (void)hipHostFree(m->h_state);
  delete m;
}

int map_alloc(mh_ctx * ctx, const mh_map_config & cfg, mh_map ** out)
{
  mh_map * m = new mh_map;
  m->ctx = ctx;
  m->cfg = cfg;
  m->inv_leaf = 1.0 / cfg.leaf_size;
  m->min_sq = cfg.min_dist_in_cell * cfg.min_dist_in_cell;
  m->n_off = mh::neighbor_offsets(cfg.neighbor_voxel_mode, m->off);
  hipError_t e = m->d_state.alloc(sizeof(mh::MapState));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&m->h_state), sizeof(mh::MapState), hipHostMallocDefault);
  if (e != hipSuccess) {
    map_free(m);
    return hip_fail(ctx, e, "mh_map_create");
  }
  std::memset(m->h_state, 0, sizeof(mh::MapState));
  *out = m;
  return MH_OK;
}

// mh_map_create, also the first half of mh_map_rebuild_from_keyframes (`who` in the texts; cap_code: what a max_points_in_cell
// outside 1..20 answers)
int map_create(mh_ctx * ctx, const char * who, const mh_map_config * cfg, int cap_code, mh_map ** out)
{
  const std::string w(who);
  if (!(cfg->leaf_size > 0)) return fail(ctx, MH_ERR_INVALID_ARG, w + ": leaf_size must be > 0");
  if (cfg->max_points_in_cell < 1 || cfg->max_points_in_cell > mh::kBucketStride) return fail(ctx, cap_code, w + ": max_points_in_cell must be in 1..20");
  const int md = cfg->neighbor_voxel_mode;
  if (md != 1 && md != 7 && md != 19 && md != 27) return fail(ctx, MH_ERR_INVALID_ARG, w + ": neighbor_voxel_mode must be 1, 7, 19 or 27");
  if (cfg->lru_clear_cycle < 1) return fail(ctx, MH_ERR_INVALID_ARG, w + ": lru_clear_cycle must be >= 1");
  if (cfg->lru_horizon < 0) return fail(ctx, MH_ERR_INVALID_ARG, w + ": lru_horizon must be >= 0");
  MH_HIP(ctx, mh_enter(ctx));
  mh_map * m = nullptr;
  int rc = map_alloc(ctx, *cfg, &m);
  if (rc != MH_OK) return rc;
  rc = ensure_table(m, 256);
  if (rc == MH_OK) rc = ensure_voxels(m, 64);
  if (rc == MH_OK) rc = ensure_blocks(m, 1, 0);  // block 0's table must exist: absent-block lookups read it
  if (rc == MH_OK) rc = push_state(m);
  if (rc != MH_OK) {
    map_free(m);
    return rc;
  }
  MH_HIP(ctx, hipMemsetAsync(m->d_buckets.p, 0, m->d_buckets.cap, ctx->stream));
  MH_HIP(ctx, hipMemsetAsync(m->d_qbuckets.p, 0, m->d_qbuckets.cap, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out = m;
  return MH_OK;
}

// R (9) and t (3) as the 12 floats the kernels read, on the device in `buf`
int upload_rt12(const mh_ctx * ctx, DevBuf & buf, const float * R, const float * t, const float ** d_rt)
{
  float rt[12];
  std::memcpy(rt, R, 9 * sizeof(float));
  std::memcpy(rt + 9, t, 3 * sizeof(float));
  MH_HIP(ctx, buf.reserve(sizeof(rt), ctx->stream, false));
  MH_HIP(ctx, hipMemcpyAsync(buf.p, rt, sizeof(rt), hipMemcpyHostToDevice, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // rt is a stack buffer
  *d_rt = buf.as<const float>();
  return MH_OK;
}

// the body cloud of a scan, for the entry points that take no `which`: they name the call that is missing
int body_cloud(const mh_ctx * ctx, const char * who, const mh_scan * scan, DeviceCloud * out)
{
  if (!scan->preprocessed) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": no mh_scan_preprocess_geometric before");
  return scan_cloud(ctx, who, scan, 1, Residence::same_device, out);
}

int check_shard(const mh_ctx * ctx, const char * who, int world, int rank, int block_log2)
{
  if (world < 1 || world > 64 || rank < 0 || rank >= world || block_log2 < 0 || block_log2 > 10)
    return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": world in 1..64, 0 <= rank < world, block_log2 in 0..10");
  return MH_OK;
}

// This rank's share of a batch (mh_map_insert_shard*): the points whose voxel lies in one of the rank's blocks or in their halo,
// in their order, packed into s_shard.  One wait for the device (the count).
int shard_keep(mh_map * map, const DeviceCloud & src, int world, int rank, int block_log2, DeviceCloud * kept)
{
  mh_ctx * ctx = map->ctx;
  const size_t n = src.n;
  *kept = DeviceCloud{map->s_shard.as<const float>(), 0, 3};
  if (!n) return MH_OK;
  MH_HIP(ctx, map->s_flags.reserve(n * sizeof(uint32_t), ctx->stream, false));
  MH_HIP(ctx, map->s_pos.reserve(n * sizeof(uint32_t), ctx->stream, false));
  MH_HIP(ctx, map->s_temp.reserve(std::max(mh::shard_temp_bytes(n), mh::map_temp_bytes(n)), ctx->stream, false));
  MH_HIP(ctx, map->s_shard.reserve(n * 3 * sizeof(float), ctx->stream, false));
  MH_HIP(ctx, mh::launch_shard_filter(src.d, static_cast<uint32_t>(n), static_cast<uint32_t>(src.stride), map->inv_leaf, static_cast<uint32_t>(world),
                                      static_cast<uint32_t>(rank), block_log2, static_cast<uint32_t *>(map->s_flags.p), static_cast<uint32_t *>(map->s_pos.p),
                                      static_cast<float *>(map->s_shard.p), &map->d_state.as<mh::MapState>()->n_keep, map->s_temp.p, map->s_temp.cap, ctx->stream));
  const int rc = fetch_state(map);
  if (rc == MH_OK) *kept = DeviceCloud{map->s_shard.as<const float>(), map->h_state->n_keep, 3};
  return rc;
}
}  // namespace

extern "C" {

int mh_map_create(mh_ctx * ctx, const mh_map_config * cfg, mh_map ** out)
{
  if (!ctx || !cfg || !out) return fail(ctx, MH_ERR_INVALID_ARG, "mh_map_create: NULL argument");
  *out = nullptr;
  return guarded(ctx, "mh_map_create", [&]() -> int { return map_create(ctx, "mh_map_create", cfg, MH_ERR_UNSUPPORTED, out); });
}

int mh_map_rebuild_from_keyframes(mh_keyframes * kf, const mh_map_config * cfg, const int32_t * order, size_t n_order, const float * R_W_K,
                                  const float * t_W_K, const mh_map_rebuild_config * rc_cfg, mh_map ** out, mh_map_rebuild_result * res)
{
  const char * who = "mh_map_rebuild_from_keyframes";
  if (out) *out = nullptr;
  if (!kf || !cfg || !out || !res) return fail(kf ? kf->ctx : nullptr, MH_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
  mh_ctx * ctx = kf->ctx;
  return guarded(ctx, who, [&]() -> int {
    std::memset(res, 0, sizeof(*res));
    if (!ctx) return fail(nullptr, MH_ERR_INVALID_ARG, std::string(who) + ": the store's context was shut down; the handle can only be destroyed");
    if (n_order && !order) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": n_order > 0 with a NULL order");
    if (rc_cfg && (rc_cfg->chunk_points < 0 || rc_cfg->reserved != 0)) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": chunk_points must be >= 0, reserved 0");
    // the list: every entry in stored order, or `order` (each entry at most once)
    const size_t size = kf->tags.size();
    const size_t K = order ? n_order : size;
    std::vector<uint64_t> sizes(K), src(K);
    std::vector<char> seen(order ? size : 0, 0);
    for (size_t j = 0; j < K; ++j) {
      size_t i = j;
      if (order) {
        if (order[j] < 0 || static_cast<size_t>(order[j]) >= size) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": order holds an index out of range");
        i = static_cast<size_t>(order[j]);
        if (seen[i]) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": order lists an entry twice");
        seen[i] = 1;
      }
      src[j] = kf->offsets[i];
      sizes[j] = kf->offsets[i + 1] - kf->offsets[i];
    }
    if (K && (!R_W_K || !t_W_K)) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": NULL poses with a non-empty list");
    for (size_t j = 0; j < 9 * K; ++j)
      if (!std::isfinite(R_W_K[j])) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": a pose entry is not finite");
    for (size_t j = 0; j < 3 * K; ++j)
      if (!std::isfinite(t_W_K[j])) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": a pose entry is not finite");
    const uint64_t budget = rc_cfg && rc_cfg->chunk_points > 0 ? static_cast<uint64_t>(rc_cfg->chunk_points) : (uint64_t(4) << 20);
    mh_map * m = nullptr;
    int rc = map_create(ctx, who, cfg, MH_ERR_INVALID_ARG, &m);
    if (rc != MH_OK) return rc;
    rc = rebuild_fill(m, kf, sizes, src, R_W_K, t_W_K, budget, res);
    if (rc != MH_OK) {  // the half-built map is released; the text of the failure stays
      (void)hipStreamSynchronize(ctx->stream);
      map_free(m);
      std::memset(res, 0, sizeof(*res));
      return rc;
    }
    *out = m;
    return MH_OK;
  });
}

int mh_map_insert(mh_map * map, const float * xyz, size_t n, size_t stride_floats)
{
  if (!map || (!xyz && n)) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_insert: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_insert", [&]() -> int {
    int rc = check_stride(ctx, "mh_map_insert", stride_floats);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    if (n > (size_t(1) << 40) / 12) return fail(ctx, MH_ERR_OOM, "mh_map_insert: batch too large");
    DeviceCloud cloud;
    if ((rc = map->in.upload(ctx, xyz, n, stride_floats, &cloud)) != MH_OK) return rc;  // (the insert waits for the stream: fetch_state)
    map->upload_bytes += static_cast<int64_t>(n * 3 * sizeof(float));
    return insert_device(map, cloud, nullptr);
  });
}

/* One rank's share of an insert into a map that is sharded by spatial hash: of the batch every rank
 * receives, this rank keeps the points whose voxel lies in one of its shard blocks or in their one-voxel halo, in
 * the original order (iVox's insertion rule is per voxel), and inserts those. */
int mh_map_insert_shard(mh_map * map, const float * xyz, size_t n, size_t stride_floats, int world, int rank, int block_log2)
{
  if (!map || (!xyz && n)) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_insert_shard: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_insert_shard", [&]() -> int {
    int rc = check_stride(ctx, "mh_map_insert_shard", stride_floats);
    if (rc == MH_OK) rc = check_shard(ctx, "mh_map_insert_shard", world, rank, block_log2);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    DeviceCloud cloud, kept;
    if (n) {
      if ((rc = check_cloud_size(ctx, "mh_map_insert_shard", n)) != MH_OK) return rc;
      if ((rc = map->in.upload(ctx, xyz, n, stride_floats, &cloud)) != MH_OK) return rc;  // (shard_keep waits for the stream)
      map->upload_bytes += static_cast<int64_t>(n * 3 * sizeof(float));
    }
    if ((rc = shard_keep(map, cloud, world, rank, block_log2, &kept)) != MH_OK) return rc;
    return insert_device(map, kept, nullptr);
  });
}

// This rank's share of Geometric::updateMap's insert of a device-resident scan: the f32 world transform of the body cloud
// (mh_transform_f32's kernel, the arithmetic of geometric.cpp:483-490), the shard filter and the greedy insert, all on the
// device — what mh_scan_get_points + mh_transform_f32 + mh_map_insert_shard do through the host, without the three copies.
int mh_map_insert_shard_from_scan(mh_map * map, const mh_scan * scan, const float R_W_Be[9], const float t_W_Be[3], int world, int rank, int block_log2)
{
  const char * who = "mh_map_insert_shard_from_scan";
  if (!map || !scan || !R_W_Be || !t_W_Be) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, who, [&]() -> int {
    DeviceCloud body, kept;
    int rc = body_cloud(ctx, who, scan, &body);
    if (rc == MH_OK) rc = check_shard(ctx, who, world, rank, block_log2);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    if (body.n) {
      const float * d_rt = nullptr;
      if ((rc = upload_rt12(ctx, map->s_rt, R_W_Be, t_W_Be, &d_rt)) != MH_OK) return rc;
      // a copy of the body cloud (the scan keeps its own), transformed in place; the filter reads xyz at the records' stride
      MH_HIP(ctx, map->in.d.reserve(body.n * sizeof(mh_point32), ctx->stream, false));
      MH_HIP(ctx, hipMemcpyAsync(map->in.d.p, body.d, body.n * sizeof(mh_point32), hipMemcpyDeviceToDevice, ctx->stream));
      MH_HIP(ctx, mh::launch_transform(static_cast<mh_point32 *>(map->in.d.p), static_cast<int>(body.n), d_rt, ctx->stream));
      body.d = map->in.d.as<const float>();
    }
    if ((rc = shard_keep(map, body, world, rank, block_log2, &kept)) != MH_OK) return rc;
    return insert_device(map, kept, nullptr);
  });
}

int mh_map_insert_device(mh_map * map, const void * d_points, size_t n, size_t stride_floats, const float * R, const float * t)
{
  if (!map || (!d_points && n)) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_insert_device: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_insert_device", [&]() -> int {
    int rc = check_stride(ctx, "mh_map_insert_device", stride_floats);
    if (rc == MH_OK) rc = check_rt_pair(ctx, "mh_map_insert_device", R, t);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    const float * d_rt = nullptr;
    if (R && (rc = upload_rt12(ctx, map->s_rt, R, t, &d_rt)) != MH_OK) return rc;
    return insert_device(map, DeviceCloud{static_cast<const float *>(d_points), n, stride_floats}, d_rt);
  });
}

int mh_map_insert_from_scan(mh_map * map, const mh_scan * scan, const float R_W_Be[9], const float t_W_Be[3])
{
  if (!map || !scan) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_insert_from_scan: NULL argument");
  DeviceCloud body;
  const int rc = body_cloud(map->ctx, "mh_map_insert_from_scan", scan, &body);
  return rc != MH_OK ? rc : mh_map_insert_device(map, body.d, body.n, body.stride, R_W_Be, t_W_Be);
}

int mh_map_preview_insert(mh_map * map, const float * xyz, size_t n, size_t stride_floats, mh_map_insert_preview * out, uint8_t * outcome)
{
  if (!map || !out || (!xyz && n)) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_preview_insert: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_preview_insert", [&]() -> int {
    int rc = check_stride(ctx, "mh_map_preview_insert", stride_floats);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    DeviceCloud cloud{nullptr, n, 3};  // (a batch that will be refused is not staged)
    // a preview is no upload of the map's: upload_bytes does not move.  (The preview waits for the stream: fetch_state.)
    if (n <= kCloudMax && !map->poisoned && (rc = map->in.upload(ctx, xyz, n, stride_floats, &cloud)) != MH_OK) return rc;
    return preview_device(map, "mh_map_preview_insert", cloud, nullptr, out, outcome);
  });
}

int mh_map_preview_insert_device(mh_map * map, const void * d_points, size_t n, size_t stride_floats, const float * R, const float * t,
                                 mh_map_insert_preview * out, uint8_t * outcome)
{
  if (!map || !out || (!d_points && n)) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_preview_insert_device: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_preview_insert_device", [&]() -> int {
    int rc = check_stride(ctx, "mh_map_preview_insert_device", stride_floats);
    if (rc == MH_OK) rc = check_rt_pair(ctx, "mh_map_preview_insert_device", R, t);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    const float * d_rt = nullptr;
    if (R && (rc = upload_rt12(ctx, map->s_rt, R, t, &d_rt)) != MH_OK) return rc;
    return preview_device(map, "mh_map_preview_insert_device", DeviceCloud{static_cast<const float *>(d_points), n, stride_floats}, d_rt, out, outcome);
  });
}

int mh_map_preview_insert_from_scan(mh_map * map, const mh_scan * scan, const float R_W_Be[9], const float t_W_Be[3], mh_map_insert_preview * out,
                                    uint8_t * outcome)
{
  if (!map || !scan || !out) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_preview_insert_from_scan: NULL argument");
  DeviceCloud body;
  const int rc = body_cloud(map->ctx, "mh_map_preview_insert_from_scan", scan, &body);
  return rc != MH_OK ? rc : mh_map_preview_insert_device(map, body.d, body.n, body.stride, R_W_Be, t_W_Be, out, outcome);
}

int mh_map_carve(mh_map * map, const float * xyz, size_t n, size_t stride_floats, const double origin_F[3], const double R_W_F[9], const double t_W_F[3],
                 const mh_map_carve_config * cfg, mh_map_carve_result * out)
{
  if (!map || !out || !cfg || !origin_F || !R_W_F || !t_W_F || (!xyz && n))
    return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_carve: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_carve", [&]() -> int {
    int rc = carve_check(ctx, "mh_map_carve", stride_floats, origin_F, R_W_F, t_W_F, *cfg);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    DeviceCloud cloud{nullptr, n, 3};  // (a batch that will be refused is not staged)
    // no upload of the map's: upload_bytes does not move.  (The carve waits for the stream: fetch_state.)
    if (n <= kCloudMax && !map->poisoned && (rc = map->in.upload(ctx, xyz, n, stride_floats, &cloud)) != MH_OK) return rc;
    return carve_device(map, "mh_map_carve", cloud, origin_F, R_W_F, t_W_F, *cfg, out);
  });
}

int mh_map_carve_device(mh_map * map, const void * d_points, size_t n, size_t stride_floats, const double origin_F[3], const double R_W_F[9],
                        const double t_W_F[3], const mh_map_carve_config * cfg, mh_map_carve_result * out)
{
  if (!map || !out || !cfg || !origin_F || !R_W_F || !t_W_F || (!d_points && n))
    return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_carve_device: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_carve_device", [&]() -> int {
    const int rc = carve_check(ctx, "mh_map_carve_device", stride_floats, origin_F, R_W_F, t_W_F, *cfg);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    return carve_device(map, "mh_map_carve_device", DeviceCloud{static_cast<const float *>(d_points), n, stride_floats}, origin_F, R_W_F, t_W_F, *cfg, out);
  });
}

int mh_map_carve_from_scan(mh_map * map, const mh_scan * scan, int which, const double origin_F[3], const double R_W_F[9], const double t_W_F[3],
                           const mh_map_carve_config * cfg, mh_map_carve_result * out)
{
  if (!map || !scan || !out || !cfg || !origin_F || !R_W_F || !t_W_F)
    return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_carve_from_scan: NULL argument");
  DeviceCloud cloud;
  const int rc = scan_cloud(map->ctx, "mh_map_carve_from_scan", scan, which, Residence::same_device, &cloud);
  return rc != MH_OK ? rc : mh_map_carve_device(map, cloud.d, cloud.n, cloud.stride, origin_F, R_W_F, t_W_F, cfg, out);
}

int mh_map_copy(const mh_map * src, mh_map ** out)
{
  if (!src || !out) return fail(src ? src->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_copy: NULL argument");
  *out = nullptr;
  mh_ctx * ctx = src->ctx;
  return guarded(ctx, "mh_map_copy", [&]() -> int {
    if (src->poisoned) return fail(ctx, MH_ERR_HIP, "mh_map_copy: the map is inconsistent after a failed mutation");
    MH_HIP(ctx, mh_enter(ctx));
    mh_map * m = nullptr;
    int rc = map_alloc(ctx, src->cfg, &m);
    if (rc != MH_OK) return rc;
    // deep copy, device to device, with growth headroom (Geometric::updateMap inserts right after copying)
    m->table_cap = src->table_cap;
    hipError_t e = m->d_table.reserve(src->table_cap * sizeof(int4), ctx->stream, false);
    if (e == hipSuccess) e = hipMemcpyAsync(m->d_table.p, src->d_table.p, src->table_cap * sizeof(int4), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) {
      rc = ensure_voxels(m, static_cast<size_t>(src->n_voxels) + src->n_voxels / 16 + 1024);
      if (rc == MH_OK) rc = ensure_blocks(m, static_cast<size_t>(src->n_blocks) + src->n_blocks / 16 + 256, static_cast<size_t>(src->n_blocks) + src->n_blocks / 16 + 256);
    }
    const size_t nv = static_cast<size_t>(src->n_voxels) + 1;  // + the slack bucket
    auto cp = [&](const DevBuf & a, DevBuf & b, size_t bytes) {
      return bytes && e == hipSuccess && rc == MH_OK ? hipMemcpyAsync(b.p, a.p, bytes < a.cap ? bytes : a.cap, hipMemcpyDeviceToDevice, ctx->stream) : e;
    };
    e = cp(src->d_buckets, m->d_buckets, nv * mh::kBucketStride * sizeof(float4));
    e = cp(src->d_qbuckets, m->d_qbuckets, nv * mh::kBucketStride * sizeof(uint32_t));
    e = cp(src->d_vox, m->d_vox, static_cast<size_t>(src->n_voxels) * sizeof(int4));
    e = cp(src->d_lru, m->d_lru, static_cast<size_t>(src->n_voxels) * sizeof(unsigned long long));
    e = cp(src->d_cells, m->d_cells, (static_cast<size_t>(src->n_blocks) + 1) * mh::kCellsPerBlock * sizeof(uint32_t));
    m->n_voxels = src->n_voxels;
    m->n_blocks = src->n_blocks;
    m->n_points = src->n_points;
    m->lru_counter = src->lru_counter;
    if (e == hipSuccess && rc == MH_OK) rc = push_state(m);
    if (e != hipSuccess || rc != MH_OK) {
      (void)hipStreamSynchronize(ctx->stream);
      map_free(m);
      return rc != MH_OK ? rc : hip_fail(ctx, e, "mh_map_copy");
    }
    *out = m;
    return MH_OK;
  });
}

int mh_map_retain(mh_map * map)
{
  if (!map) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_map_retain: map is NULL");
  map->refs.fetch_add(1);
  return MH_OK;
}

void mh_map_release(mh_map * map)
{
  if (!map) return;
  if (map->refs.fetch_sub(1) == 1) {
    (void)mh_enter(map->ctx);
    (void)hipStreamSynchronize(map->ctx->stream);  // the last factor is gone (each waited for its own stream): only the map's own work can be in flight
    map_free(map);
  }
}

int mh_map_get_stats(const mh_map * map, mh_map_stats * out)
{
  if (!map || !out) return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_get_stats: NULL argument");
  out->n_voxels = map->n_voxels;
  out->n_points = static_cast<int64_t>(map->n_points);
  out->n_blocks = map->n_blocks;
  out->device_bytes = static_cast<int64_t>(map->d_table.cap + map->d_cells.cap + map->d_buckets.cap + map->d_qbuckets.cap + map->d_vox.cap + map->d_lru.cap);
  out->uploads = map->inserts;
  out->upload_bytes = map->upload_bytes;
  out->delta_uploads = map->inserts;
  out->full_uploads = 0;
  return MH_OK;
}

int mh_map_get_cloud(const mh_map * cmap, float * xyz, size_t capacity_points, size_t * n_out)
{
  if (!cmap || !n_out) return fail(cmap ? cmap->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_get_cloud: NULL argument");
  mh_map * map = const_cast<mh_map *>(cmap);  // scratch buffers only
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_get_cloud", [&]() -> int {
    if (map->poisoned) return fail(ctx, MH_ERR_HIP, "mh_map_get_cloud: the map is inconsistent after a failed mutation");
    *n_out = static_cast<size_t>(map->n_points);
    if (!xyz || map->n_points == 0) return MH_OK;
    MH_HIP(ctx, mh_enter(ctx));
    const uint32_t nv = map->n_voxels;
    const size_t np = static_cast<size_t>(map->n_points);
    MH_HIP(ctx, map->s_flags.reserve(nv * sizeof(uint32_t), ctx->stream, false));
    MH_HIP(ctx, map->s_pos.reserve(nv * sizeof(uint32_t), ctx->stream, false));
    MH_HIP(ctx, map->s_temp.reserve(mh::map_temp_bytes(nv), ctx->stream, false));
    MH_HIP(ctx, map->in.d.reserve(np * 3 * sizeof(float), ctx->stream, false));
    MH_HIP(ctx, mh::launch_map_cloud(arrays_of(map), nv, static_cast<uint32_t *>(map->s_flags.p), static_cast<uint32_t *>(map->s_pos.p),
                                     static_cast<float *>(map->in.d.p), np, map->s_temp.p, map->s_temp.cap, ctx->stream));
    const size_t take = np < capacity_points ? np : capacity_points;
    MH_HIP(ctx, hipMemcpyAsync(xyz, map->in.d.p, take * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MH_OK;
  });
}

int mh_map_knn(mh_map * map, const double * queries, size_t n, int k, double * point_xyz, double * sq_dists, int32_t * found)
{
  if (!map || !queries || !point_xyz || !sq_dists || !found)
    return fail(map ? map->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_map_knn: NULL argument");
  mh_ctx * ctx = map->ctx;
  return guarded(ctx, "mh_map_knn", [&]() -> int {
    if (k < 1 || k > 8) return fail(ctx, MH_ERR_UNSUPPORTED, "mh_map_knn: k must be in 1..8");
    if (map->poisoned) return fail(ctx, MH_ERR_HIP, "mh_map_knn: the map is inconsistent after a failed mutation");
    MH_HIP(ctx, mh_enter(ctx));
    if (n == 0) return MH_OK;
    DevTemp<double> d_q, d_p, d_s;
    DevTemp<int32_t> d_f;
    MH_HIP(ctx, d_q.alloc(n * 3 * sizeof(double)));
    MH_HIP(ctx, d_p.alloc(n * k * 3 * sizeof(double)));
    MH_HIP(ctx, d_s.alloc(n * k * sizeof(double)));
    MH_HIP(ctx, d_f.alloc(n * sizeof(int32_t)));
    MH_HIP(ctx, hipMemcpyAsync(d_q, queries, n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(ctx, mh::launch_map_knn(map_view(map), d_q, static_cast<int>(n), k, d_p, d_s, d_f, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(point_xyz, d_p, n * k * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(sq_dists, d_s, n * k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(found, d_f, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MH_OK;
  });
}

}  // extern "C"
