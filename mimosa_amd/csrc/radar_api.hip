// C ABI of the radar Doppler path (include/mimosa_hip.h: mh_radar_*): radar::Manager's front end and DopplerHessianFactor.
//
// Reference: src/radar/manager.cpp:111-181 (Manager::preprocess), include/mimosa/radar/factor.hpp:54-188
// (DopplerHessianFactor), include/mimosa/radar/utils.hpp (TargetData), include/mimosa/radar/manager.hpp:20-33 (config).
// Device work is in radar_kernels.hip.  What stays on the host is per factor and per call: the 3 x 3 products of the state
// that every target of the factor shares (factor.hpp:100-118), and the expansion of the 55 sums into the six dense blocks.
// There is no CPU fallback: every entry point needs the context's HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "mh_internal.hpp"
#include "radar_device.hpp"

static_assert(sizeof(mh_radar_target) == 64, "mh_radar_target is TargetData: 8 doubles");

struct mh_radar_scan
{
  mh_ctx * ctx = nullptr;
  DevBuf d_raw, d_targets, d_bd, d_count;
  PinnedBuf h_count;  // pinned landing word of the kept count (a uint32_t)
  size_t n_in = 0, n_valid = 0;
  bool prepared = false;
};

struct mh_radar_factor
{
  mh_ctx * ctx = nullptr;
  size_t n = 0;
  DevBuf d_bd;    // per target: bearing, radial_speed (radar_device.hpp)
  DevBuf d_args;  // the RadarLinArgs of the call in flight / the last call
  double R_B_S[9], t_B_S[3], omega[3], sigma = 0;
  // pinned, mapped: the argument block the kernel's argument copy reads, then the kernel's 55 sums (written by the kernel)
  PinnedBuf h_io;
  void * d_io = nullptr;
  mh::RadarLinArgs last{};  // state of the last linearize (mh_radar_factor_get_residuals)
  bool linearized = false, pending = false, pending_timed = false;
  hipEvent_t done = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

namespace
{
constexpr size_t kIoBytes = 4096;
constexpr size_t kIoOut = 512;  // byte offset of the sums in h_io (behind the argument block)
static_assert(sizeof(mh::RadarLinArgs) <= kIoOut && kIoOut + mh::kRadarOutStride * sizeof(double) <= kIoBytes, "h_io layout");
constexpr size_t kBatchArgBytes = MH_RADAR_MAX_BATCH * sizeof(mh::RadarLinArgs);
constexpr size_t kBatchBytes = kBatchArgBytes + MH_RADAR_MAX_BATCH * mh::kRadarOutStride * sizeof(double);

// deg2rad<float> (include/mimosa/utils.hpp): (deg * float(M_PI)) / 180.f in float
float deg2rad_f(float deg) { return (deg * static_cast<float>(M_PI)) / 180.f; }

void mat3_mul(const double * A, const double * B, double * C)  // row-major C = A B
{
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
void mat3_tr(const double * A, double * T)
{
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) T[3 * r + c] = A[3 * c + r];
}
void skew(const double * v, double * S)  // gtsam::skewSymmetric
{
  S[0] = 0;
  S[1] = -v[2];
  S[2] = v[1];
  S[3] = v[2];
  S[4] = 0;
  S[5] = -v[0];
  S[6] = -v[1];
  S[7] = v[0];
  S[8] = 0;
}

// factor.hpp:100-118 and the per-target Jacobian factors (:141-152) that do not depend on the target
mh::RadarLinArgs make_args(const mh_radar_factor * f, const double * R_W_B, const double * v_W, const double * bias_gyro)
{
  mh::RadarLinArgs a{};
  double RrbT[9], RbwT[9], S[9], T1[9], T2[9];
  mat3_tr(f->R_B_S, RrbT);
  mat3_tr(R_W_B, RbwT);
  // linear_velocity_from_angular_B = (angular_velocity_B - gyro bias) x l_R_B
  const double w[3] = {f->omega[0] - bias_gyro[0], f->omega[1] - bias_gyro[1], f->omega[2] - bias_gyro[2]};
  const double * l = f->t_B_S;
  const double vfa[3] = {w[1] * l[2] - w[2] * l[1], w[2] * l[0] - w[0] * l[2], w[0] * l[1] - w[1] * l[0]};
  double vB[3];
  for (int r = 0; r < 3; ++r) vB[r] = RbwT[3 * r] * v_W[0] + RbwT[3 * r + 1] * v_W[1] + RbwT[3 * r + 2] * v_W[2] + vfa[r];
  for (int r = 0; r < 3; ++r) a.vR[r] = RrbT[3 * r] * vB[0] + RrbT[3 * r + 1] * vB[1] + RrbT[3 * r + 2] * vB[2];
  // J1 rotation = -b^T R_R_B^T (R_B_W^T [v_W]x R_B_W)
  skew(v_W, S);
  mat3_mul(RbwT, S, T1);
  mat3_mul(T1, R_W_B, T2);
  mat3_mul(RrbT, T2, a.A1);
  // J2 = -b^T R_R_B^T R_B_W^T
  mat3_mul(RrbT, RbwT, a.A2);
  // J3 gyroscope = -b^T R_R_B^T [l_R_B]x
  skew(l, S);
  mat3_mul(RrbT, S, a.A3);
  a.inv_sigma = 1.0 / f->sigma;
  a.targets = static_cast<const double4 *>(f->d_bd.p);
  a.n = static_cast<uint32_t>(f->n);
  return a;
}

// the 55 sums -> HessianFactor(X, V, B, G11, G12, G13, g1, G22, G23, g2, G33, g3, f) (factor.hpp:185-186); every entry
// the reference leaves at its structural zero is +0.0, the symmetric blocks are filled from one value per pair
void expand(const double * s, size_t n_targets, mh_radar_result * out)
{
  std::memset(out, 0, sizeof(*out));
  auto H = [s](int r, int c) {
    if (r > c) std::swap(r, c);
    return s[r * 9 - r * (r - 1) / 2 + (c - r)];
  };
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      out->G11[6 * r + c] = H(r, c);
      out->G12[3 * r + c] = H(r, 3 + c);
      out->G13[6 * r + 3 + c] = H(r, 6 + c);
      out->G22[3 * r + c] = H(3 + r, 3 + c);
      out->G23[6 * r + 3 + c] = H(3 + r, 6 + c);
      out->G33[6 * (3 + r) + 3 + c] = H(6 + r, 6 + c);
    }
  for (int r = 0; r < 3; ++r) {
    out->g1[r] = s[45 + r];
    out->g2[r] = s[48 + r];
    out->g3[3 + r] = s[51 + r];
  }
  out->f = s[54];
  out->n_targets = n_targets;
  out->gpu_ms = -1.f;
}

bool have_state(const double * R, const double * v, const double * b) { return R && v && b; }

int factor_new(mh_ctx * ctx, size_t n, const double R_B_S[9], const double t_B_S[3], const double omega[3], double sigma,
               mh_radar_factor ** out)
{
  mh_radar_factor * f = new mh_radar_factor;
  f->ctx = ctx;
  f->n = n;
  std::memcpy(f->R_B_S, R_B_S, sizeof(f->R_B_S));
  std::memcpy(f->t_B_S, t_B_S, sizeof(f->t_B_S));
  std::memcpy(f->omega, omega, sizeof(f->omega));
  f->sigma = sigma;
  hipError_t e = f->h_io.reserve(kIoBytes, kIoBytes);
  if (e == hipSuccess) e = hipHostGetDevicePointer(&f->d_io, f->h_io.p, 0);
  if (e == hipSuccess) e = f->d_bd.reserve(n * sizeof(double4), ctx->stream, false);
  if (e == hipSuccess) e = f->d_args.reserve(sizeof(mh::RadarLinArgs), ctx->stream, false);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&f->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    mh_radar_factor_destroy(f);
    return hip_fail(ctx, e, "mh_radar_factor_create");
  }
  *out = f;
  return MH_OK;
}

int check_factor_args(mh_ctx * ctx, size_t n, const double * R_B_S, const double * t_B_S, const double * omega, double sigma,
                      const char * what)
{
  if (!R_B_S || !t_B_S || !omega) return fail(ctx, MH_ERR_INVALID_ARG, std::string(what) + ": NULL argument");
  if (n > 0x7FFFFFFFu) return fail(ctx, MH_ERR_INVALID_ARG, std::string(what) + ": more than 2^31 - 1 targets");
  if (!(sigma > 0)) return fail(ctx, MH_ERR_INVALID_ARG, std::string(what) + ": noise_sigma must be > 0");
  return MH_OK;
}

int radar_enqueue(mh_radar_factor * f, const double * R_W_B, const double * v_W, const double * bias_gyro)
{
  mh_ctx * ctx = f->ctx;
  MH_HIP(ctx, mh_enter(ctx));
  const bool timed = ctx->profiling > 0;
  const mh::RadarLinArgs a = make_args(f, R_W_B, v_W, bias_gyro);
  std::memcpy(f->h_io.p, &a, sizeof(a));
  double * d_out = reinterpret_cast<double *>(static_cast<char *>(f->d_io) + kIoOut);
  if (timed && !f->ev[0]) {
    MH_HIP(ctx, hipEventCreate(&f->ev[0]));
    MH_HIP(ctx, hipEventCreate(&f->ev[1]));
  }
  if (f->n > 0) {  // (no kernel for a factor without targets: the sums are zero)
    MH_HIP(ctx, hipMemcpyAsync(f->d_args.p, f->h_io.p, sizeof(a), hipMemcpyHostToDevice, ctx->stream));
    if (timed) MH_HIP(ctx, hipEventRecord(f->ev[0], ctx->stream));
    MH_HIP(ctx, mh::launch_radar_linearize(static_cast<const mh::RadarLinArgs *>(f->d_args.p), 1, d_out, ctx->stream));
    if (timed) MH_HIP(ctx, hipEventRecord(f->ev[1], ctx->stream));
  }
  MH_HIP(ctx, hipEventRecord(f->done, ctx->stream));
  f->last = a;
  f->linearized = true;
  f->pending_timed = timed && f->n > 0;
  f->pending = true;
  return MH_OK;
}

int radar_finish(mh_radar_factor * f, mh_radar_result * out)
{
  mh_ctx * ctx = f->ctx;
  f->pending = false;
  MH_HIP(ctx, mh_enter(ctx));
  MH_HIP(ctx, hipEventSynchronize(f->done));  // the end of the kernel makes its host writes visible
  static const double zeros[mh::kRadarOutStride] = {};
  const double * s = f->n > 0 ? reinterpret_cast<const double *>(f->h_io.as<const char>() + kIoOut) : zeros;
  expand(s, f->n, out);
  if (f->pending_timed) (void)hipEventElapsedTime(&out->gpu_ms, f->ev[0], f->ev[1]);
  return MH_OK;
}
}  // namespace

extern "C" {

int mh_radar_scan_create(mh_ctx * ctx, mh_radar_scan ** out)
{
  if (!ctx || !out) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_scan_create: NULL argument");
  *out = nullptr;
  return guarded(ctx, "mh_radar_scan_create", [&]() -> int {
    MH_HIP(ctx, mh_enter(ctx));
    mh_radar_scan * s = new mh_radar_scan;
    s->ctx = ctx;
    hipError_t e = s->h_count.reserve(4096, 4096);
    if (e == hipSuccess) e = s->d_count.reserve(64, ctx->stream, false);
    if (e != hipSuccess) {
      mh_radar_scan_destroy(s);
      return hip_fail(ctx, e, "mh_radar_scan_create");
    }
    *out = s;
    return MH_OK;
  });
}

void mh_radar_scan_destroy(mh_radar_scan * s)
{
  if (!s) return;
  (void)mh_enter(s->ctx);
  (void)hipStreamSynchronize(s->ctx->stream);
  const DrainedScope drained;
  delete s;
}

int mh_radar_prepare_input(mh_radar_scan * s, const void * raw, size_t n, const mh_radar_layout * layout, const mh_radar_config * cfg,
                           mh_radar_info * info)
{
  if (!s || !layout || !cfg || (n && !raw)) return fail(s ? s->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_radar_prepare_input: NULL argument");
  mh_ctx * ctx = s->ctx;
  return guarded(ctx, "mh_radar_prepare_input", [&]() -> int {
    if (layout->kind == MH_RADAR_MMWAVE_DOPPLER_RESIDUAL)  // manager.cpp:43-54: decoded, then "Unsupported point type"
      return fail(ctx, MH_ERR_UNSUPPORTED, "mh_radar_prepare_input: Unsupported point type (mmWaveDopplerResidualPoint)");
    if (layout->kind != MH_RADAR_RIO && layout->kind != MH_RADAR_MMWAVE)
      return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_prepare_input: unknown layout kind");
    const uint32_t step = layout->point_step;
    for (uint32_t off : {layout->off_x, layout->off_y, layout->off_z, layout->off_intensity, layout->off_velocity})
      if (off % 4 != 0 || static_cast<uint64_t>(off) + 4 > step)
        return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_prepare_input: a field offset is not a multiple of 4 inside point_step");
    if (step == 0 || step % 4 != 0) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_prepare_input: point_step must be a multiple of 4");
    if (n > 0x7FFFFFFFu) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_prepare_input: more than 2^31 - 1 points");
    MH_HIP(ctx, mh_enter(ctx));
    s->prepared = false;
    MH_HIP(ctx, s->d_raw.reserve(n * step, ctx->stream, false));
    MH_HIP(ctx, s->d_targets.reserve(n * sizeof(mh_radar_target), ctx->stream, false));
    MH_HIP(ctx, s->d_bd.reserve(n * sizeof(double4), ctx->stream, false));
    if (n) MH_HIP(ctx, hipMemcpyAsync(s->d_raw.p, raw, n * step, hipMemcpyHostToDevice, ctx->stream));
    mh::RadarFilter fl;
    fl.rio = layout->kind == MH_RADAR_RIO ? 1u : 0u;
    fl.point_step = step;
    fl.off_x = layout->off_x;
    fl.off_y = layout->off_y;
    fl.off_z = layout->off_z;
    fl.off_intensity = layout->off_intensity;
    fl.off_velocity = layout->off_velocity;
    fl.range_min = cfg->range_min;
    fl.range_max = cfg->range_max;
    fl.thr_azimuth = deg2rad_f(cfg->threshold_azimuth_deg);
    fl.thr_elevation = deg2rad_f(cfg->threshold_elevation_deg);
    fl.filter_min_db = cfg->filter_min_db;
    MH_HIP(ctx, mh::launch_radar_prepare(s->d_raw.p, static_cast<uint32_t>(n), fl, static_cast<mh_radar_target *>(s->d_targets.p),
                                         static_cast<double4 *>(s->d_bd.p), static_cast<uint32_t *>(s->d_count.p), ctx->stream));
    MH_HIP(ctx, hipMemcpyAsync(s->h_count.p, s->d_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->n_in = n;
    s->n_valid = *s->h_count.as<uint32_t>();
    s->prepared = true;
    if (info) {
      info->n_points_in = n;
      info->n_points_valid = s->n_valid;
    }
    return MH_OK;
  });
}

int mh_radar_get_targets(const mh_radar_scan * s, mh_radar_target * out, size_t capacity, size_t * n_out)
{
  if (!s) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_radar_get_targets: scan is NULL");
  mh_ctx * ctx = s->ctx;
  return guarded(ctx, "mh_radar_get_targets", [&]() -> int {
    if (!s->prepared) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_get_targets: call mh_radar_prepare_input first");
    if (n_out) *n_out = s->n_valid;
    if (!out) return MH_OK;
    if (capacity < s->n_valid) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_get_targets: capacity too small");
    MH_HIP(ctx, mh_enter(ctx));
    if (s->n_valid) {
      MH_HIP(ctx, hipMemcpyAsync(out, s->d_targets.p, s->n_valid * sizeof(mh_radar_target), hipMemcpyDeviceToHost, ctx->stream));
      MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MH_OK;
  });
}

int mh_radar_factor_create(mh_ctx * ctx, const mh_radar_target * targets, size_t n, const double R_B_S[9], const double t_B_S[3],
                           const double angular_velocity_B[3], double noise_sigma, mh_radar_factor ** out)
{
  if (!ctx || !out || (n && !targets)) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_create: NULL argument");
  *out = nullptr;
  return guarded(ctx, "mh_radar_factor_create", [&]() -> int {
    int rc = check_factor_args(ctx, n, R_B_S, t_B_S, angular_velocity_B, noise_sigma, "mh_radar_factor_create");
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    mh_radar_factor * f = nullptr;
    rc = factor_new(ctx, n, R_B_S, t_B_S, angular_velocity_B, noise_sigma, &f);
    if (rc != MH_OK) return rc;
    if (n) {
      DevTemp<mh_radar_target> d_t;
      hipError_t e = d_t.alloc(n * sizeof(mh_radar_target));
      if (e == hipSuccess) e = hipMemcpyAsync(d_t.p, targets, n * sizeof(mh_radar_target), hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = mh::launch_radar_bearing(d_t.p, static_cast<uint32_t>(n), static_cast<double4 *>(f->d_bd.p), ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's buffer may go away when the call returns
      if (e != hipSuccess) {
        mh_radar_factor_destroy(f);
        return hip_fail(ctx, e, "mh_radar_factor_create");
      }
    }
    *out = f;
    return MH_OK;
  });
}

int mh_radar_factor_create_from_scan(const mh_radar_scan * s, const double R_B_S[9], const double t_B_S[3], const double angular_velocity_B[3],
                                     double noise_sigma, mh_radar_factor ** out)
{
  if (!s || !out) return fail(s ? s->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_radar_factor_create_from_scan: NULL argument");
  *out = nullptr;
  mh_ctx * ctx = s->ctx;
  return guarded(ctx, "mh_radar_factor_create_from_scan", [&]() -> int {
    if (!s->prepared) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_create_from_scan: call mh_radar_prepare_input first");
    int rc = check_factor_args(ctx, s->n_valid, R_B_S, t_B_S, angular_velocity_B, noise_sigma, "mh_radar_factor_create_from_scan");
    if (rc != MH_OK) return rc;
    MH_HIP(ctx, mh_enter(ctx));
    mh_radar_factor * f = nullptr;
    rc = factor_new(ctx, s->n_valid, R_B_S, t_B_S, angular_velocity_B, noise_sigma, &f);
    if (rc != MH_OK) return rc;
    if (s->n_valid) {  // stream-ordered behind the scan's kernel; no host round trip
      const hipError_t e = hipMemcpyAsync(f->d_bd.p, s->d_bd.p, s->n_valid * sizeof(double4), hipMemcpyDeviceToDevice, ctx->stream);
      if (e != hipSuccess) {
        mh_radar_factor_destroy(f);
        return hip_fail(ctx, e, "mh_radar_factor_create_from_scan");
      }
    }
    *out = f;
    return MH_OK;
  });
}

int mh_radar_factor_clone(const mh_radar_factor * src, mh_radar_factor ** out)
{
  if (!src || !out) return fail(src ? src->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_radar_factor_clone: NULL argument");
  *out = nullptr;
  mh_ctx * ctx = src->ctx;
  return guarded(ctx, "mh_radar_factor_clone", [&]() -> int {
    MH_HIP(ctx, mh_enter(ctx));
    mh_radar_factor * f = nullptr;
    const int rc = factor_new(ctx, src->n, src->R_B_S, src->t_B_S, src->omega, src->sigma, &f);
    if (rc != MH_OK) return rc;
    if (src->n) {
      const hipError_t e = hipMemcpyAsync(f->d_bd.p, src->d_bd.p, src->n * sizeof(double4), hipMemcpyDeviceToDevice, ctx->stream);
      if (e != hipSuccess) {
        mh_radar_factor_destroy(f);
        return hip_fail(ctx, e, "mh_radar_factor_clone");
      }
    }
    *out = f;
    return MH_OK;
  });
}

void mh_radar_factor_destroy(mh_radar_factor * f)
{
  if (!f) return;
  (void)mh_enter(f->ctx);
  (void)hipStreamSynchronize(f->ctx->stream);  // a call in flight still reads the targets and writes h_io
  for (hipEvent_t e : {f->done, f->ev[0], f->ev[1]})
    if (e) (void)hipEventDestroy(e);
  const DrainedScope drained;
  delete f;
}

size_t mh_radar_factor_size(const mh_radar_factor * f) { return f ? f->n : 0; }

int mh_radar_factor_linearize(mh_radar_factor * f, const double R_W_B[9], const double v_W[3], const double bias_gyro[3], mh_radar_result * out)
{
  if (!f || !out || !have_state(R_W_B, v_W, bias_gyro))
    return fail(f ? f->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize: NULL argument");
  mh_ctx * ctx = f->ctx;
  return guarded(ctx, "mh_radar_factor_linearize", [&]() -> int {
    if (f->pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize: a call is in flight (mh_radar_factor_wait first)");
    const int rc = radar_enqueue(f, R_W_B, v_W, bias_gyro);
    return rc != MH_OK ? rc : radar_finish(f, out);
  });
}

int mh_radar_factor_linearize_async(mh_radar_factor * f, const double R_W_B[9], const double v_W[3], const double bias_gyro[3])
{
  if (!f || !have_state(R_W_B, v_W, bias_gyro))
    return fail(f ? f->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize_async: NULL argument");
  mh_ctx * ctx = f->ctx;
  return guarded(ctx, "mh_radar_factor_linearize_async", [&]() -> int {
    if (f->pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize_async: a call is already in flight");
    return radar_enqueue(f, R_W_B, v_W, bias_gyro);
  });
}

int mh_radar_factor_wait(mh_radar_factor * f, mh_radar_result * out)
{
  if (!f || !out) return fail(f ? f->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_radar_factor_wait: NULL argument");
  mh_ctx * ctx = f->ctx;
  return guarded(ctx, "mh_radar_factor_wait", [&]() -> int {
    if (!f->pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_wait: no call in flight");
    return radar_finish(f, out);
  });
}

int mh_radar_factor_linearize_batch(mh_radar_factor * const * factors, size_t n_factors, const double * R_W_B, const double * v_W,
                                    const double * bias_gyro, mh_radar_result * out)
{
  if (!factors || n_factors == 0 || !factors[0] || !have_state(R_W_B, v_W, bias_gyro) || !out)
    return fail(factors && n_factors && factors[0] ? factors[0]->ctx : nullptr, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize_batch: NULL argument or no factors");
  mh_ctx * ctx = factors[0]->ctx;
  return guarded(ctx, "mh_radar_factor_linearize_batch", [&]() -> int {
    if (n_factors > MH_RADAR_MAX_BATCH)
      return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize_batch: more than MH_RADAR_MAX_BATCH factors");
    for (size_t i = 0; i < n_factors; ++i) {
      if (!factors[i]) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize_batch: NULL factor");
      if (factors[i]->ctx != ctx) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize_batch: factors of different contexts");
      if (factors[i]->pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_linearize_batch: a factor has a call in flight");
    }
    MH_HIP(ctx, mh_enter(ctx));
    const bool timed = ctx->profiling > 0;
    PinnedBuf h;  // the staging block goes back to the pool on every exit path (the call waits for its kernel)
    MH_HIP(ctx, h.reserve(kBatchBytes, kBatchBytes));
    void * d_h = nullptr;
    MH_HIP(ctx, hipHostGetDevicePointer(&d_h, h.p, 0));
    mh::RadarLinArgs * args = h.as<mh::RadarLinArgs>();
    for (size_t i = 0; i < n_factors; ++i) args[i] = make_args(factors[i], R_W_B + 9 * i, v_W + 3 * i, bias_gyro + 3 * i);
    DevTemp<mh::RadarLinArgs> d_args;
    MH_HIP(ctx, d_args.alloc(n_factors * sizeof(mh::RadarLinArgs)));
    MH_HIP(ctx, hipMemcpyAsync(d_args.p, args, n_factors * sizeof(mh::RadarLinArgs), hipMemcpyHostToDevice, ctx->stream));
    double * d_out = reinterpret_cast<double *>(static_cast<char *>(d_h) + kBatchArgBytes);
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timed) {
      MH_HIP(ctx, hipEventCreate(&ev[0]));
      MH_HIP(ctx, hipEventCreate(&ev[1]));
      MH_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    }
    // ONE launch for the window; a factor without targets gets a workgroup that writes zeros
    MH_HIP(ctx, mh::launch_radar_linearize(d_args.p, static_cast<uint32_t>(n_factors), d_out, ctx->stream));
    if (timed) MH_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = -1.f;
    if (timed) {
      (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
      (void)hipEventDestroy(ev[0]);
      (void)hipEventDestroy(ev[1]);
    }
    const double * s = reinterpret_cast<const double *>(h.as<const char>() + kBatchArgBytes);
    for (size_t i = 0; i < n_factors; ++i) {
      expand(s + i * mh::kRadarOutStride, factors[i]->n, &out[i]);
      out[i].gpu_ms = ms;
      factors[i]->last = args[i];
      factors[i]->linearized = true;
    }
    return MH_OK;
  });
}

int mh_radar_factor_get_residuals(const mh_radar_factor * f, double * e_whitened, double * weight)
{
  if (!f) return fail(nullptr, MH_ERR_INVALID_ARG, "mh_radar_factor_get_residuals: factor is NULL");
  mh_ctx * ctx = f->ctx;
  return guarded(ctx, "mh_radar_factor_get_residuals", [&]() -> int {
    if (!f->linearized) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_get_residuals: no linearize yet");
    if (f->pending) return fail(ctx, MH_ERR_INVALID_ARG, "mh_radar_factor_get_residuals: a call is in flight (mh_radar_factor_wait first)");
    if (f->n == 0 || (!e_whitened && !weight)) return MH_OK;
    MH_HIP(ctx, mh_enter(ctx));
    DevTemp<mh::RadarLinArgs> d_args;
    DevTemp<double> d_e, d_w;
    MH_HIP(ctx, d_args.alloc(sizeof(mh::RadarLinArgs)));
    MH_HIP(ctx, d_e.alloc(f->n * sizeof(double)));
    MH_HIP(ctx, d_w.alloc(f->n * sizeof(double)));
    MH_HIP(ctx, hipMemcpyAsync(d_args.p, &f->last, sizeof(f->last), hipMemcpyHostToDevice, ctx->stream));
    MH_HIP(ctx, mh::launch_radar_residuals(d_args.p, static_cast<uint32_t>(f->n), d_e.p, d_w.p, ctx->stream));
    if (e_whitened) MH_HIP(ctx, hipMemcpyAsync(e_whitened, d_e.p, f->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (weight) MH_HIP(ctx, hipMemcpyAsync(weight, d_w.p, f->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MH_OK;
  });
}

}  // extern "C"
