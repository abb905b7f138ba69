// Place-recognition entry points of the C ABI (include/mimosa_hip.h): mh_place_db_*, mh_place_describe*.  The kernels are
// place_kernels.hip, the arithmetic place_device.hpp.  Everything runs on the context's stream; a call that hands a result to
// the host ends in one wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "mh_internal.hpp"
#include "place_device.hpp"

static_assert(sizeof(mh_place_score) == sizeof(mh::PlaceScore) && sizeof(mh_place_config) == 40 && sizeof(mh_place_hit) == 24, "mh_place_* layout");
static_assert(MH_PLACE_RINGS == mh::kPlaceRings && MH_PLACE_SECTORS == mh::kPlaceSectors && MH_PLACE_MAX_HITS == mh::kPlaceMaxHits, "mh_place_* constants");

// the database's pinned block: [hits, 256 B | a descriptor, 4 800 B -> 4 864 | scores, 16 B per entry]
constexpr size_t kPlaceDescBytes = mh::kPlaceCells * sizeof(float);
constexpr size_t kPlaceHostDescAt = sizeof(mh::PlaceBest);
constexpr size_t kPlaceHostScoresAt = kPlaceHostDescAt + 4864;

struct mh_place_db final : CtxOwned
{
  mh_place_config cfg{};
  mh::PlaceParams P{};     // everything of the descriptor rule but R
  size_t size = 0;
  std::vector<int64_t> tags;
  // what goes back when the context does
  struct Memory
  {
    DevBuf desc;     // float: capacity x 1 200
    DevBuf norms;    // double: capacity x 60
    DevBuf scores;   // PlaceScore: capacity
    DevBuf query;    // [a descriptor, 4 864 B | its norms, 512 B | hits, 256 B]
    PinnedBuf h;     // the pinned block
    HostStage in;    // a host batch on its way in
  } mem;
  float * d_desc() const { return mem.desc.as<float>(); }
  double * d_norms() const { return mem.norms.as<double>(); }
  mh::PlaceScore * d_scores() const { return mem.scores.as<mh::PlaceScore>(); }
  char * d_query() const { return mem.query.as<char>(); }
  char * h() const { return mem.h.as<char>(); }
  void ctx_gone() override
  {
    mem = Memory{};
    size = 0;
    tags.clear();
  }
};
constexpr size_t kPlaceQueryNormsAt = 4864, kPlaceQueryBestAt = kPlaceQueryNormsAt + 512, kPlaceQueryBytes = kPlaceQueryBestAt + sizeof(mh::PlaceBest);

namespace
{
// every entry point but destroy: a database whose context was shut down
int place_alive(const mh_place_db * db, const char * who) { return ctx_alive(db, who, "database"); }

int place_check_R(const mh_ctx * ctx, const char * who, const double * R)
{
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(R[i])) return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": R_G_F has an entry that is not finite");
  return MH_OK;
}

int place_check_desc(const mh_ctx * ctx, const char * who, const float * desc)
{
  for (int i = 0; i < mh::kPlaceCells; ++i)
    if (!(std::isfinite(desc[i]) && desc[i] >= 0.0f))
      return fail(ctx, MH_ERR_INVALID_ARG, std::string(who) + ": descriptor entry " + std::to_string(i) + " is negative or not finite");
  return MH_OK;
}

// enqueue: d_desc (device, 1 200 floats) = the descriptor of the batch
int place_describe_to(mh_place_db * db, const char * who, const DeviceCloud & src, const double * R, float * d_desc)
{
  mh::PlaceParams P = db->P;
  std::memcpy(P.R, R, sizeof(P.R));
  const hipError_t e = mh::launch_place_describe(src.d, static_cast<uint32_t>(src.n), static_cast<uint32_t>(src.stride), P, d_desc, db->ctx->stream);
  return e == hipSuccess ? MH_OK : hip_fail(db->ctx, e, who);
}

// describe into the query block, bring the descriptor to the caller: one wait
int place_describe_out(mh_place_db * db, const char * who, const DeviceCloud & src, const double * R, float * desc)
{
  mh_ctx * ctx = db->ctx;
  const int rc = place_describe_to(db, who, src, R, reinterpret_cast<float *>(db->d_query()));
  if (rc != MH_OK) return rc;
  MH_HIP(ctx, hipMemcpyAsync(db->h() + kPlaceHostDescAt, db->d_query(), kPlaceDescBytes, hipMemcpyDeviceToHost, ctx->stream));
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(desc, db->h() + kPlaceHostDescAt, kPlaceDescBytes);
  return MH_OK;
}

int place_check_query(const mh_place_db * db, const char * who, size_t n_search, int32_t top_k)
{
  const std::string w(who);
  if (top_k < 1 || top_k > MH_PLACE_MAX_HITS) return fail(db->ctx, MH_ERR_INVALID_ARG, w + ": top_k must be in 1..16");
  if (db->size == 0) return fail(db->ctx, MH_ERR_INVALID_ARG, w + ": the database is empty");
  if (n_search > db->size) return fail(db->ctx, MH_ERR_INVALID_ARG, w + ": n_search is greater than the size");
  return MH_OK;
}

// the query's descriptor is in the query block: norms, distances, selection, the copies; one wait
int place_query_chain(mh_place_db * db, const char * who, size_t n_search, int32_t top_k, mh_place_hit * hits, mh_place_score * all)
{
  mh_ctx * ctx = db->ctx;
  const int m = static_cast<int>(n_search ? n_search : db->size);
  const float * q = reinterpret_cast<const float *>(db->d_query());
  double * qn = reinterpret_cast<double *>(db->d_query() + kPlaceQueryNormsAt);
  mh::PlaceBest * d_best = reinterpret_cast<mh::PlaceBest *>(db->d_query() + kPlaceQueryBestAt);
  hipError_t e = mh::launch_place_norms(q, qn, ctx->stream);
  if (e == hipSuccess) e = mh::launch_place_query(q, qn, db->d_desc(), db->d_norms(), m, db->cfg.min_overlap, db->d_scores(), ctx->stream);
  if (e == hipSuccess) e = mh::launch_place_select(db->d_scores(), m, top_k, d_best, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(db->h(), d_best, sizeof(mh::PlaceBest), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && all)
    e = hipMemcpyAsync(db->h() + kPlaceHostScoresAt, db->d_scores(), static_cast<size_t>(m) * sizeof(mh::PlaceScore), hipMemcpyDeviceToHost, ctx->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return hip_fail(ctx, e, who);
  }
  MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const mh::PlaceBest * b = reinterpret_cast<const mh::PlaceBest *>(db->h());
  for (int k = 0; k < top_k; ++k) {
    mh_place_hit & hk = hits[k];
    hk.index = b->index[k];
    hk.shift = b->shift[k];
    hk.dist = b->dist[k];
    hk.tag = 0;
    if (hk.index >= 0) {
      if (hk.index >= m) return fail(ctx, MH_ERR_HIP, std::string(who) + ": the device selected an entry outside the search");
      hk.tag = db->tags[static_cast<size_t>(hk.index)];
    }
  }
  if (all) std::memcpy(all, db->h() + kPlaceHostScoresAt, static_cast<size_t>(m) * sizeof(mh::PlaceScore));
  return MH_OK;
}

// (before the context is looked at: a config is refused the same way with and without one)
int place_check_config(const mh_ctx * ctx, const mh_place_config * cfg)
{
  for (double v : {cfg->r_min, cfg->r_max, cfg->z_min, cfg->z_max})
    if (!std::isfinite(v)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_create: a config value is not finite");
  if (!(cfg->r_min > 0.0) || !(cfg->r_max > cfg->r_min)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_create: 0 < r_min < r_max is required");
  if (!(cfg->z_min < cfg->z_max)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_create: z_min < z_max is required");
  if (cfg->min_overlap < 1 || cfg->min_overlap > MH_PLACE_SECTORS) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_create: min_overlap must be in 1..60");
  if (cfg->capacity < 1 || cfg->capacity > mh::kPlaceMaxEntries) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_create: capacity must be in 1..65536");
  return MH_OK;
}

int place_create(mh_ctx * ctx, const mh_place_config * cfg, mh_place_db ** out)
{
  MH_HIP(ctx, mh_enter(ctx));
  mh_place_db * db = new mh_place_db;
  db->cfg = *cfg;
  db->P.r_min2 = cfg->r_min * cfg->r_min;
  db->P.z_min = cfg->z_min;
  db->P.z_max = cfg->z_max;
  mh::place_ring_table(cfg->r_max, db->P.b2);
  const size_t cap = static_cast<size_t>(cfg->capacity);
  db->tags.reserve(cap);
  const size_t h_bytes = kPlaceHostScoresAt + cap * sizeof(mh::PlaceScore);
  hipError_t e = db->mem.desc.alloc(cap * kPlaceDescBytes);
  if (e == hipSuccess) e = db->mem.norms.alloc(cap * mh::kPlaceSectors * sizeof(double));
  if (e == hipSuccess) e = db->mem.scores.alloc(cap * sizeof(mh::PlaceScore));
  if (e == hipSuccess) e = db->mem.query.alloc(kPlaceQueryBytes);
  if (e == hipSuccess) e = db->mem.h.reserve(h_bytes, h_bytes);
  if (e != hipSuccess) {
    delete db;
    return hip_fail(ctx, e, "mh_place_db_create");
  }
  ctx_register(db, ctx);
  *out = db;
  return MH_OK;
}

// the entry the next add fills, after the checks every add shares
int place_add_check(const mh_place_db * db, const char * who)
{
  if (db->size >= static_cast<size_t>(db->cfg.capacity)) return fail(db->ctx, MH_ERR_INVALID_ARG, std::string(who) + ": the database is full");
  return MH_OK;
}
}  // namespace

extern "C" {

int mh_place_db_create(mh_ctx * ctx, const mh_place_config * cfg, mh_place_db ** out)
{
  if (out) *out = nullptr;
  if (!cfg || !out) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_create: NULL argument");
  return guarded(ctx, "mh_place_db_create", [&]() -> int {
    const int rc = place_check_config(ctx, cfg);
    if (rc != MH_OK) return rc;
    if (!ctx) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_create: NULL argument");
    return place_create(ctx, cfg, out);
  });
}

void mh_place_db_destroy(mh_place_db * db)
{
  if (!db) return;
  if (mh_ctx * ctx = db->ctx) {
    (void)mh_enter(ctx);
    (void)hipStreamSynchronize(ctx->stream);  // the pinned blocks go back: nothing may still be copying into them
    ctx_unregister(db);
  }
  delete db;
}

size_t mh_place_db_size(const mh_place_db * db) { return db && db->ctx ? db->size : 0; }

int mh_place_describe(mh_place_db * db, const float * xyz, size_t n, size_t stride_floats, const double R_G_F[9], float * desc)
{
  if (!db || !R_G_F || !desc || (!xyz && n)) return fail(db ? db->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_place_describe: NULL argument");
  return guarded(db->ctx, "mh_place_describe", [&]() -> int {
    int rc = place_alive(db, "mh_place_describe");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    if ((rc = check_stride(ctx, "mh_place_describe", stride_floats)) != MH_OK) return rc;
    if ((rc = place_check_R(ctx, "mh_place_describe", R_G_F)) != MH_OK) return rc;
    if ((rc = check_cloud_size(ctx, "mh_place_describe", n)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    DeviceCloud cloud;
    if ((rc = db->mem.in.upload(ctx, xyz, n, stride_floats, &cloud)) != MH_OK) return rc;  // (place_describe_out waits for the stream)
    return place_describe_out(db, "mh_place_describe", cloud, R_G_F, desc);
  });
}

int mh_place_describe_device(mh_place_db * db, const void * d_points, size_t n, size_t stride_floats, const double R_G_F[9], float * desc)
{
  if (!db || !R_G_F || !desc || (!d_points && n)) return fail(db ? db->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_place_describe_device: NULL argument");
  return guarded(db->ctx, "mh_place_describe_device", [&]() -> int {
    int rc = place_alive(db, "mh_place_describe_device");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    if ((rc = check_stride(ctx, "mh_place_describe_device", stride_floats)) != MH_OK) return rc;
    if ((rc = place_check_R(ctx, "mh_place_describe_device", R_G_F)) != MH_OK) return rc;
    if ((rc = check_cloud_size(ctx, "mh_place_describe_device", n)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    return place_describe_out(db, "mh_place_describe_device", DeviceCloud{static_cast<const float *>(d_points), n, stride_floats}, R_G_F, desc);
  });
}

int mh_place_describe_from_scan(mh_place_db * db, const mh_scan * scan, int which, const double R_G_F[9], float * desc)
{
  if (!db || !scan || !R_G_F || !desc) return fail(db ? db->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_place_describe_from_scan: NULL argument");
  return guarded(db->ctx, "mh_place_describe_from_scan", [&]() -> int {
    int rc = place_alive(db, "mh_place_describe_from_scan");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    DeviceCloud cloud;
    if ((rc = scan_cloud(ctx, "mh_place_describe_from_scan", scan, which, Residence::same_device, &cloud)) != MH_OK) return rc;
    if ((rc = place_check_R(ctx, "mh_place_describe_from_scan", R_G_F)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    return place_describe_out(db, "mh_place_describe_from_scan", cloud, R_G_F, desc);
  });
}

int mh_place_db_add(mh_place_db * db, const float * desc, int64_t tag, int32_t * index)
{
  if (!db || !desc) return fail(db ? db->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_place_db_add: NULL argument");
  return guarded(db->ctx, "mh_place_db_add", [&]() -> int {
    int rc = place_alive(db, "mh_place_db_add");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    if ((rc = place_add_check(db, "mh_place_db_add")) != MH_OK) return rc;
    if ((rc = place_check_desc(ctx, "mh_place_db_add", desc)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    float * slot = db->d_desc() + db->size * mh::kPlaceCells;
    std::memcpy(db->h() + kPlaceHostDescAt, desc, kPlaceDescBytes);
    MH_HIP(ctx, hipMemcpyAsync(slot, db->h() + kPlaceHostDescAt, kPlaceDescBytes, hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(ctx, mh::launch_place_norms(slot, db->d_norms() + db->size * mh::kPlaceSectors, ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the pinned block is the next call's too)
    if (index) *index = static_cast<int32_t>(db->size);
    db->tags.push_back(tag);
    ++db->size;
    return MH_OK;
  });
}

int mh_place_db_add_from_scan(mh_place_db * db, const mh_scan * scan, int which, const double R_G_F[9], int64_t tag, int32_t * index)
{
  if (!db || !scan || !R_G_F) return fail(db ? db->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_place_db_add_from_scan: NULL argument");
  return guarded(db->ctx, "mh_place_db_add_from_scan", [&]() -> int {
    int rc = place_alive(db, "mh_place_db_add_from_scan");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    if ((rc = place_add_check(db, "mh_place_db_add_from_scan")) != MH_OK) return rc;
    DeviceCloud cloud;
    if ((rc = scan_cloud(ctx, "mh_place_db_add_from_scan", scan, which, Residence::same_device, &cloud)) != MH_OK) return rc;
    if ((rc = place_check_R(ctx, "mh_place_db_add_from_scan", R_G_F)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    // on the device from end to end, and nothing waits: the entry is behind this call on the context's stream, where every
    // reader of it is enqueued.  (A launch that fails leaves the size where it was: the slot is simply written again.)
    float * slot = db->d_desc() + db->size * mh::kPlaceCells;
    rc = place_describe_to(db, "mh_place_db_add_from_scan", cloud, R_G_F, slot);
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh::launch_place_norms(slot, db->d_norms() + db->size * mh::kPlaceSectors, ctx->stream));
    if (index) *index = static_cast<int32_t>(db->size);
    db->tags.push_back(tag);
    ++db->size;
    return MH_OK;
  });
}

int mh_place_db_get(mh_place_db * db, int32_t index, float * desc, int64_t * tag)
{
  if (!db) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_place_db_get: NULL argument");
  return guarded(db->ctx, "mh_place_db_get", [&]() -> int {
    const int rc = place_alive(db, "mh_place_db_get");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    if (index < 0 || static_cast<size_t>(index) >= db->size) return fail(ctx, MH_ERR_INVALID_ARG, "mh_place_db_get: index out of range");
    if (desc) {
      MH_HIP(ctx, mh_enter(ctx));
      MH_HIP(ctx, hipMemcpyAsync(db->h() + kPlaceHostDescAt, db->d_desc() + static_cast<size_t>(index) * mh::kPlaceCells, kPlaceDescBytes,
                                 hipMemcpyDeviceToHost, ctx->stream));
      MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
      std::memcpy(desc, db->h() + kPlaceHostDescAt, kPlaceDescBytes);
    }
    if (tag) *tag = db->tags[static_cast<size_t>(index)];
    return MH_OK;
  });
}

int mh_place_db_query(mh_place_db * db, const float * desc, size_t n_search, int32_t top_k, mh_place_hit * hits, mh_place_score * all)
{
  if (!db || !desc || !hits) return fail(db ? db->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_place_db_query: NULL argument");
  return guarded(db->ctx, "mh_place_db_query", [&]() -> int {
    int rc = place_alive(db, "mh_place_db_query");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    if ((rc = place_check_query(db, "mh_place_db_query", n_search, top_k)) != MH_OK) return rc;
    if ((rc = place_check_desc(ctx, "mh_place_db_query", desc)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    std::memcpy(db->h() + kPlaceHostDescAt, desc, kPlaceDescBytes);
    MH_HIP(ctx, hipMemcpyAsync(db->d_query(), db->h() + kPlaceHostDescAt, kPlaceDescBytes, hipMemcpyHostToDevice, ctx->stream));
    return place_query_chain(db, "mh_place_db_query", n_search, top_k, hits, all);
  });
}

int mh_place_db_query_from_scan(mh_place_db * db, const mh_scan * scan, int which, const double R_G_F[9], size_t n_search, int32_t top_k,
                                mh_place_hit * hits, mh_place_score * all)
{
  if (!db || !scan || !R_G_F || !hits) return fail(db ? db->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_place_db_query_from_scan: NULL argument");
  return guarded(db->ctx, "mh_place_db_query_from_scan", [&]() -> int {
    int rc = place_alive(db, "mh_place_db_query_from_scan");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = db->ctx;
    if ((rc = place_check_query(db, "mh_place_db_query_from_scan", n_search, top_k)) != MH_OK) return rc;
    DeviceCloud cloud;
    if ((rc = scan_cloud(ctx, "mh_place_db_query_from_scan", scan, which, Residence::same_device, &cloud)) != MH_OK) return rc;
    if ((rc = place_check_R(ctx, "mh_place_db_query_from_scan", R_G_F)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    rc = place_describe_to(db, "mh_place_db_query_from_scan", cloud, R_G_F, reinterpret_cast<float *>(db->d_query()));
    if (rc != MH_OK) return rc;
    return place_query_chain(db, "mh_place_db_query_from_scan", n_search, top_k, hits, all);
  });
}

}  // extern "C"
