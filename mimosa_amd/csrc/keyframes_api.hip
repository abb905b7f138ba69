// Keyframe cloud store of the C ABI (include/mimosa_hip.h): mh_keyframes_*.  One device arena of packed float4 (x, y, z, 1), an
// offset table on the host and on the device, a tag per entry; no pose.  The pack kernel is in rebuild_kernels.hip; the reader
// of the store, mh_map_rebuild_from_keyframes, in map_api.hip.  Everything runs on the context's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mh_internal.hpp"

static_assert(sizeof(mh_keyframes_config) == 16 && sizeof(mh_keyframes_info) == 40, "mh_keyframes_* layout");

namespace
{
constexpr int32_t kKeyframesMax = 65536;

// every entry point but destroy: a store whose context was shut down
int keyframes_alive(const mh_keyframes * kf, const char * who) { return ctx_alive(kf, who, "store"); }

// the checks every add shares: room for one more entry of n points
int keyframes_add_check(const mh_keyframes * kf, const char * who, size_t n)
{
  if (kf->tags.size() >= static_cast<size_t>(kf->cfg.capacity_keyframes)) return fail(kf->ctx, MH_ERR_INVALID_ARG, std::string(who) + ": the store is full (keyframes)");
  if (n > static_cast<uint64_t>(kf->cfg.capacity_points) - kf->offsets.back()) return fail(kf->ctx, MH_ERR_INVALID_ARG, std::string(who) + ": the store is full (points)");
  return MH_OK;
}

// enqueue the new entry behind everything on the stream, and book it
int keyframes_append(mh_keyframes * kf, const char * who, const DeviceCloud & src, int64_t tag, int32_t * index)
{
  mh_ctx * ctx = kf->ctx;
  const size_t i = kf->tags.size(), n = src.n;
  const uint64_t at = kf->offsets.back();
  // (a launch that fails leaves the books where they were: the slot is simply written again)
  const hipError_t e = mh::launch_keyframes_pack(src.d, static_cast<uint32_t>(n), static_cast<uint32_t>(src.stride), kf->arena() + at, kf->mem.d_offsets.as<unsigned long long>() + i, at + n,
                                                 ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, who);
  if (index) *index = static_cast<int32_t>(i);
  kf->tags.push_back(tag);
  kf->offsets.push_back(at + n);
  return MH_OK;
}

int keyframes_create(mh_ctx * ctx, const mh_keyframes_config * cfg, mh_keyframes ** out)
{
  MH_HIP(ctx, mh_enter(ctx));
  mh_keyframes * kf = new mh_keyframes;
  kf->cfg = *cfg;
  kf->tags.reserve(static_cast<size_t>(cfg->capacity_keyframes));
  kf->offsets.reserve(static_cast<size_t>(cfg->capacity_keyframes) + 1);
  const size_t off_bytes = (static_cast<size_t>(cfg->capacity_keyframes) + 1) * sizeof(unsigned long long);
  hipError_t e = kf->mem.d_arena.alloc(static_cast<size_t>(cfg->capacity_points) * sizeof(float4));
  if (e == hipSuccess) e = kf->mem.d_offsets.alloc(off_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(kf->mem.d_offsets.p, 0, off_bytes, ctx->stream);
  if (e != hipSuccess) {
    delete kf;
    return hip_fail(ctx, e, "mh_keyframes_create");
  }
  ctx_register(kf, ctx);
  *out = kf;
  return MH_OK;
}
}  // namespace

extern "C" {

int mh_keyframes_create(mh_ctx * ctx, const mh_keyframes_config * cfg, mh_keyframes ** out)
{
  if (out) *out = nullptr;
  if (!cfg || !out) return fail(ctx, MH_ERR_INVALID_ARG, "mh_keyframes_create: NULL argument");
  return guarded(ctx, "mh_keyframes_create", [&]() -> int {
    if (cfg->capacity_keyframes < 1 || cfg->capacity_keyframes > kKeyframesMax)
      return fail(ctx, MH_ERR_INVALID_ARG, "mh_keyframes_create: capacity_keyframes must be in 1..65536");
    if (cfg->capacity_points < 1 || cfg->capacity_points > (int64_t(1) << 40)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_keyframes_create: capacity_points must be in 1..2^40");
    if (cfg->reserved != 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_keyframes_create: reserved must be 0");
    if (!ctx) return fail(ctx, MH_ERR_INVALID_ARG, "mh_keyframes_create: NULL argument");
    return keyframes_create(ctx, cfg, out);
  });
}

void mh_keyframes_destroy(mh_keyframes * kf)
{
  if (!kf) return;
  if (mh_ctx * ctx = kf->ctx) {
    (void)mh_enter(ctx);
    (void)hipStreamSynchronize(ctx->stream);  // the arena goes back: nothing may still be reading it
    ctx_unregister(kf);
  }
  delete kf;
}

size_t mh_keyframes_size(const mh_keyframes * kf) { return kf && kf->ctx ? kf->tags.size() : 0; }

int mh_keyframes_get_info(const mh_keyframes * kf, mh_keyframes_info * out)
{
  if (!kf || !out) return fail(kf ? kf->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_keyframes_get_info: NULL argument");
  return guarded(kf->ctx, "mh_keyframes_get_info", [&]() -> int {
    const int rc = keyframes_alive(kf, "mh_keyframes_get_info");
    if (rc != MH_OK) return rc;
    out->keyframes = static_cast<int64_t>(kf->tags.size());
    out->points = static_cast<int64_t>(kf->offsets.back());
    out->capacity_keyframes = kf->cfg.capacity_keyframes;
    out->capacity_points = kf->cfg.capacity_points;
    out->device_bytes = kf->cfg.capacity_points * static_cast<int64_t>(sizeof(float4)) +
                        (static_cast<int64_t>(kf->cfg.capacity_keyframes) + 1) * static_cast<int64_t>(sizeof(unsigned long long));
    return MH_OK;
  });
}

int mh_keyframes_add(mh_keyframes * kf, const float * xyz, size_t n, size_t stride_floats, int64_t tag, int32_t * index)
{
  if (!kf || (!xyz && n)) return fail(kf ? kf->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_keyframes_add: NULL argument");
  return guarded(kf->ctx, "mh_keyframes_add", [&]() -> int {
    int rc = keyframes_alive(kf, "mh_keyframes_add");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = kf->ctx;
    if ((rc = check_stride(ctx, "mh_keyframes_add", stride_floats)) != MH_OK) return rc;
    if ((rc = keyframes_add_check(kf, "mh_keyframes_add", n)) != MH_OK) return rc;
    if ((rc = check_cloud_size(ctx, "mh_keyframes_add", n)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    DeviceCloud cloud;  // packed xyz through the pinned block, then the pack kernel every add shares
    if ((rc = kf->mem.in.upload(ctx, xyz, n, stride_floats, &cloud)) != MH_OK) return rc;
    rc = keyframes_append(kf, "mh_keyframes_add", cloud, tag, index);
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the pinned block is the next call's too, and mh_keyframes_get's)
    return rc;
  });
}

int mh_keyframes_add_device(mh_keyframes * kf, const void * d_points, size_t n, size_t stride_floats, int64_t tag, int32_t * index)
{
  if (!kf || (!d_points && n)) return fail(kf ? kf->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_keyframes_add_device: NULL argument");
  return guarded(kf->ctx, "mh_keyframes_add_device", [&]() -> int {
    int rc = keyframes_alive(kf, "mh_keyframes_add_device");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = kf->ctx;
    if ((rc = check_stride(ctx, "mh_keyframes_add_device", stride_floats)) != MH_OK) return rc;
    if ((rc = keyframes_add_check(kf, "mh_keyframes_add_device", n)) != MH_OK) return rc;
    if (n > kCloudMax || stride_floats > 0xffffffffu) return fail(ctx, MH_ERR_UNSUPPORTED, "mh_keyframes_add_device: batch too large");
    MH_HIP(ctx, mh_enter(ctx));
    return keyframes_append(kf, "mh_keyframes_add_device", DeviceCloud{static_cast<const float *>(d_points), n, stride_floats}, tag, index);
  });
}

int mh_keyframes_add_from_scan(mh_keyframes * kf, const mh_scan * scan, int which, int64_t tag, int32_t * index)
{
  if (!kf || !scan) return fail(kf ? kf->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_keyframes_add_from_scan: NULL argument");
  return guarded(kf->ctx, "mh_keyframes_add_from_scan", [&]() -> int {
    int rc = keyframes_alive(kf, "mh_keyframes_add_from_scan");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = kf->ctx;
    // the entry is ordered behind the scan's stages by the stream they share: a scan of another context is refused
    DeviceCloud cloud;
    if ((rc = scan_cloud(ctx, "mh_keyframes_add_from_scan", scan, which, Residence::same_context, &cloud)) != MH_OK) return rc;
    if ((rc = keyframes_add_check(kf, "mh_keyframes_add_from_scan", cloud.n)) != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    return keyframes_append(kf, "mh_keyframes_add_from_scan", cloud, tag, index);
  });
}

int mh_keyframes_get(mh_keyframes * kf, int32_t index, float * xyz, size_t capacity_points, size_t * n_out, int64_t * tag)
{
  if (!kf) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_keyframes_get: NULL argument");
  return guarded(kf->ctx, "mh_keyframes_get", [&]() -> int {
    int rc = keyframes_alive(kf, "mh_keyframes_get");
    if (rc != MH_OK) return rc;
    mh_ctx * ctx = kf->ctx;
    if (index < 0 || static_cast<size_t>(index) >= kf->tags.size()) return fail(ctx, MH_ERR_INVALID_ARG, "mh_keyframes_get: index out of range");
    const uint64_t at = kf->offsets[static_cast<size_t>(index)], n = kf->offsets[static_cast<size_t>(index) + 1] - at;
    const size_t take = xyz ? static_cast<size_t>(std::min<uint64_t>(n, capacity_points)) : 0;
    if (take) {
      MH_HIP(ctx, mh_enter(ctx));
      MH_HIP(ctx, kf->mem.in.h.reserve(take * sizeof(float4)));  // (mh_keyframes_add, the other user of the block, has waited)
      MH_HIP(ctx, hipMemcpyAsync(kf->mem.in.h.p, kf->arena() + at, take * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
      MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const float * h = kf->mem.in.h.as<const float>();
      for (size_t i = 0; i < take; ++i) std::memcpy(xyz + 3 * i, h + 4 * i, 3 * sizeof(float));
    }
    if (n_out) *n_out = static_cast<size_t>(n);
    if (tag) *tag = kf->tags[static_cast<size_t>(index)];
    return MH_OK;
  });
}

int mh_keyframes_device_points(mh_keyframes * kf, int32_t index, const float ** d_xyz1, size_t * n)
{
  if (!kf || !d_xyz1 || !n) return fail(kf ? kf->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_keyframes_device_points: NULL argument");
  return guarded(kf->ctx, "mh_keyframes_device_points", [&]() -> int {
    const int rc = keyframes_alive(kf, "mh_keyframes_device_points");
    if (rc != MH_OK) return rc;
    if (index < 0 || static_cast<size_t>(index) >= kf->tags.size()) return fail(kf->ctx, MH_ERR_INVALID_ARG, "mh_keyframes_device_points: index out of range");
    const uint64_t at = kf->offsets[static_cast<size_t>(index)];
    *d_xyz1 = reinterpret_cast<const float *>(kf->arena() + at);
    *n = static_cast<size_t>(kf->offsets[static_cast<size_t>(index) + 1] - at);
    return MH_OK;
  });
}

}  // extern "C"
