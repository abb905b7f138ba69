// Radar Doppler path (radar_kernels.hip / radar_api.hip): what the C ABI and the kernels share.  Not installed, not part of
// the boundary.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mimosa_hip.h"

namespace mh
{
// Manager::preprocess (src/radar/manager.cpp:111-181): the decoded layout and the gates, all in float as the reference's
// ManagerConfig holds them (include/mimosa/radar/manager.hpp:20-33).  The thresholds are deg2rad<float> of the config values,
// computed on the host.
struct RadarFilter
{
  uint32_t rio;  // 1: rioPoint (x' = y, y' = -x, intensity = snr_db, velocity = v_doppler_mps), 0: mmWavePoint
  uint32_t point_step, off_x, off_y, off_z, off_intensity, off_velocity;
  float range_min, range_max, thr_azimuth, thr_elevation, filter_min_db;
};

// One factor of one linearize call (DopplerHessianFactor::linearize, include/mimosa/radar/factor.hpp:98-188), reduced on the
// host to three 3 x 3 matrices and a vector (row-major).  Per target with bearing b = p / range:
//   e  = -b . vR - doppler
//   J1 = -b^T A1 (rotation columns of X), J2 = -b^T A2 (V), J3 = -b^T A3 (gyroscope columns of B)
struct RadarLinArgs
{
  double A1[9], A2[9], A3[9];
  double vR[3];
  double inv_sigma;
  const double4 * targets;  // per target: bearing (x, y, z) / range, radial_speed
  uint32_t n;
  uint32_t pad;
};

// What one factor's workgroup writes: the upper triangle of sum w^2 j j^T over j = (J1 rot, J2, J3 gyro) / sigma (45, row by
// row), the gradient -sum w^2 j e / sigma^2 (9), f (1), one spare.
constexpr int kRadarSums = 55;
constexpr int kRadarOutStride = 56;
constexpr int kRadarThreads = 256;  // one workgroup per factor

// decode + gates + stable compaction, one workgroup; *count = number of targets kept
hipError_t launch_radar_prepare(const void * raw, uint32_t n, const RadarFilter & f, mh_radar_target * targets, double4 * bd,
                                uint32_t * count, hipStream_t stream);
// the bearing / Doppler records of host-supplied targets (mh_radar_factor_create)
hipError_t launch_radar_bearing(const mh_radar_target * targets, uint32_t n, double4 * bd, hipStream_t stream);
// one workgroup per factor: out[f * kRadarOutStride + k], k < kRadarSums
hipError_t launch_radar_linearize(const RadarLinArgs * args, uint32_t n_factors, double * out, hipStream_t stream);
// per target of one factor: the whitened residual e / sigma before the robust weight, and the weight (the same arithmetic as
// the linearize kernel)
hipError_t launch_radar_residuals(const RadarLinArgs * args, uint32_t n, double * e_whitened, double * weight, hipStream_t stream);
}  // namespace mh
