// C++ host mirror of the reference's radar classes over the C ABI (include/mimosa_hip.h, mh_radar_*):
//
//   ManagerConfig          include/mimosa/radar/manager.hpp:20-33
//   TargetData / PType     include/mimosa/radar/utils.hpp:17-52
//   Manager::callback      src/radar/manager.cpp:26-109 (timestamp correction, point-type dispatch, factor construction)
//   Manager::preprocess    src/radar/manager.cpp:111-181
//   DopplerHessianFactor   include/mimosa/radar/factor.hpp:22-188
//
// Same names, constructor arguments and keys (X(0), V(0), B(0), manager.cpp:84-86).  The mean gyro rate over the exposure
// (manager.cpp:56-75) comes from the IMU manager and is the caller's argument, as in the reference's constructor.  ROS
// publishers, loggers and config_utilities are dropped; the static / dynamic split is not computed (the reference never
// fills it).  Header-only; link with libmimosa_hip.so.  The arithmetic runs behind the C ABI on the GPU, there is no CPU
// fallback.
#pragma once

#include <gtsam/navigation/ImuBias.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "lidar.hpp"

namespace mimosa_hip
{
namespace radar
{
using gtsam::symbol_shorthand::B;
using gtsam::symbol_shorthand::V;
using lidar::Context;

// manager.hpp:20-33 (base.T_B_S is the one field of SensorManagerBaseConfig the radar path reads)
struct ManagerConfig
{
  Pose3 T_B_S = Pose3();
  bool is_exposure_compensated = true;
  float range_min = 0.1f;
  float range_max = 20.0f;
  float threshold_azimuth_deg = 60.0f;
  float threshold_elevation_deg = 60.0f;
  float filter_min_db = 5;
  float frame_ms = 18.5f;
  float noise_sigma = 0.1f;
};

// utils.hpp:17-41
struct TargetData
{
  double x, y, z, range, azimuth, elevation, radial_speed, intensity;
  TargetData(double x, double y, double z, double range, double azimuth, double elevation, double radial_speed, double intensity)
  : x(x), y(y), z(z), range(range), azimuth(azimuth), elevation(elevation), radial_speed(radial_speed), intensity(intensity)
  {
  }
};
typedef std::vector<TargetData> TargetVector;
static_assert(sizeof(TargetData) == sizeof(mh_radar_target), "TargetData is mh_radar_target");

// utils.hpp:45-51; decodePointType's field match is the caller's: it describes the record with an mh_radar_layout
enum class PType { Unknown, Rio, mmWave, mmWaveDopplerResidual };

// manager.cpp:34: the timestamp is moved to the centre of the exposure unless the driver already did
inline double correctedTimestamp(const ManagerConfig & config, double header_ts)
{
  return header_ts + (config.is_exposure_compensated ? 0 : config.frame_ms * 1e-3 / 2);
}

class DopplerHessianFactor : public NonlinearFactor
{
public:
  using Ptr = std::shared_ptr<DopplerHessianFactor>;

  // factor.hpp:54-65
  DopplerHessianFactor(const std::shared_ptr<Context> & ctx, const TargetVector & targets, const Pose3 & pose_R_B,
                       const gtsam::Vector3 & angular_velocity_B, const Key key0, const Key key1, const Key key2, const double noise_sigma)
  : NonlinearFactor(KeyVector{key0, key1, key2}), ctx_(ctx)
  {
    const PoseRM T = rowMajor(pose_R_B);
    const A3 w = toArray(angular_velocity_B);
    ctx_->check(mh_radar_factor_create(ctx_->get(), reinterpret_cast<const mh_radar_target *>(targets.data()), targets.size(), T.R.data(),
                                       T.t.data(), w.data(), noise_sigma, &f_),
                "mh_radar_factor_create");
  }
  // the same from a prepared device-resident scan (Manager::preprocess's valid_targets_), device to device
  DopplerHessianFactor(const std::shared_ptr<Context> & ctx, const mh_radar_scan * scan, const Pose3 & pose_R_B,
                       const gtsam::Vector3 & angular_velocity_B, const Key key0, const Key key1, const Key key2, const double noise_sigma)
  : NonlinearFactor(KeyVector{key0, key1, key2}), ctx_(ctx)
  {
    const PoseRM T = rowMajor(pose_R_B);
    const A3 w = toArray(angular_velocity_B);
    ctx_->check(mh_radar_factor_create_from_scan(scan, T.R.data(), T.t.data(), w.data(), noise_sigma, &f_), "mh_radar_factor_create_from_scan");
  }
  ~DopplerHessianFactor() override { mh_radar_factor_destroy(f_); }
  DopplerHessianFactor(const DopplerHessianFactor &) = delete;
  DopplerHessianFactor & operator=(const DopplerHessianFactor &) = delete;

  NonlinearFactor::shared_ptr clone() const override  // :67-73
  {
    std::shared_ptr<DopplerHessianFactor> c(new DopplerHessianFactor(ctx_, keys()));
    ctx_->check(mh_radar_factor_clone(f_, &c->f_), "mh_radar_factor_clone");
    return c;
  }
  size_t dim() const override { return 15; }                   // :75-78
  double error(const Values &) const override { return 0.0; }  // :91-96 (the reference prints and returns 0)
  size_t numTargets() const { return mh_radar_factor_size(f_); }

  std::shared_ptr<GaussianFactor> linearize(const Values & c) const override  // :98-188
  {
    mh_radar_result r;
    State s = state(c);
    ctx_->check(mh_radar_factor_linearize(f_, s.R.data(), s.v.data(), s.bg.data(), &r), "mh_radar_factor_linearize");
    return toHessian(r);
  }
  // linearize() split in two so that the smoother can queue it next to the LiDAR factors on the same stream
  void linearizeAsync(const Values & c) const
  {
    State s = state(c);
    ctx_->check(mh_radar_factor_linearize_async(f_, s.R.data(), s.v.data(), s.bg.data()), "mh_radar_factor_linearize_async");
  }
  std::shared_ptr<GaussianFactor> collect() const
  {
    mh_radar_result r;
    ctx_->check(mh_radar_factor_wait(f_, &r), "mh_radar_factor_wait");
    return toHessian(r);
  }
  // every factor of the window in one launch; all on one context
  static std::vector<std::shared_ptr<GaussianFactor>> linearizeBatch(const std::vector<const DopplerHessianFactor *> & factors, const Values & c)
  {
    std::vector<std::shared_ptr<GaussianFactor>> out;
    if (factors.empty()) return out;
    std::vector<mh_radar_factor *> hs;
    std::vector<double> R, v, bg;
    for (const DopplerHessianFactor * f : factors) {
      const State s = f->state(c);
      hs.push_back(f->f_);
      R.insert(R.end(), s.R.begin(), s.R.end());
      v.insert(v.end(), s.v.begin(), s.v.end());
      bg.insert(bg.end(), s.bg.begin(), s.bg.end());
    }
    std::vector<mh_radar_result> r(factors.size());
    factors[0]->ctx_->check(mh_radar_factor_linearize_batch(hs.data(), hs.size(), R.data(), v.data(), bg.data(), r.data()),
                            "mh_radar_factor_linearize_batch");
    for (size_t i = 0; i < factors.size(); ++i) out.push_back(factors[i]->toHessian(r[i]));
    return out;
  }

private:
  DopplerHessianFactor(const std::shared_ptr<Context> & ctx, const KeyVector & keys) : NonlinearFactor(keys), ctx_(ctx) {}

  struct State
  {
    A9 R;
    A3 v, bg;
  };
  State state(const Values & c) const
  {
    // :100-111: the rotation of X (its translation is not read), V, and the gyroscope part of B
    const Pose3 pose_B_W = c.at<Pose3>(keys()[0]);
    const gtsam::Vector3 linear_velocity_W = c.at<gtsam::Vector3>(keys()[1]);
    const gtsam::imuBias::ConstantBias imu_bias_B = c.at<gtsam::imuBias::ConstantBias>(keys()[2]);
    return State{rowMajor(pose_B_W.rotation().matrix()), toArray(linear_velocity_W), toArray(imu_bias_B.gyroscope())};
  }
  static gtsam::Matrix block(const double * rm, int rows, int cols)
  {
    gtsam::Matrix M(rows, cols);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) M(r, c) = rm[cols * r + c];
    return M;
  }
  static gtsam::Vector vec(const double * v, int n)
  {
    gtsam::Vector o(n);
    for (int i = 0; i < n; ++i) o(i) = v[i];
    return o;
  }
  std::shared_ptr<GaussianFactor> toHessian(const mh_radar_result & r) const  // :185-186
  {
    return std::make_shared<HessianFactor>(keys()[0], keys()[1], keys()[2], block(r.G11, 6, 6), block(r.G12, 6, 3), block(r.G13, 6, 6),
                                           vec(r.g1, 6), block(r.G22, 3, 3), block(r.G23, 3, 6), vec(r.g2, 3), block(r.G33, 6, 6),
                                           vec(r.g3, 6), r.f);
  }

  std::shared_ptr<Context> ctx_;
  mh_radar_factor * f_ = nullptr;
};

// radar::Manager's per-message work (manager.cpp:26-109, :111-181) without ROS: preprocess a PointCloud2's bytes on the device,
// then build the factor from the device-resident targets.
class Manager
{
public:
  Manager(const std::shared_ptr<Context> & ctx, const ManagerConfig & config) : ctx_(ctx), config_(config)
  {
    ctx_->check(mh_radar_scan_create(ctx_->get(), &scan_), "mh_radar_scan_create");
  }
  ~Manager() { mh_radar_scan_destroy(scan_); }
  Manager(const Manager &) = delete;
  Manager & operator=(const Manager &) = delete;

  // manager.cpp:43-54 + :111-181.  mmWaveDopplerResidual and Unknown throw "Unsupported point type", as the reference does.
  void preprocess(PType type, const void * data, size_t n_points, const mh_radar_layout & fields)
  {
    if (type != PType::Rio && type != PType::mmWave) throw std::runtime_error("Unsupported point type");
    mh_radar_layout layout = fields;
    layout.kind = type == PType::Rio ? MH_RADAR_RIO : MH_RADAR_MMWAVE;
    const mh_radar_config cfg{config_.range_min, config_.range_max, config_.threshold_azimuth_deg, config_.threshold_elevation_deg,
                              config_.filter_min_db, config_.noise_sigma};
    mh_radar_info info;
    ctx_->check(mh_radar_prepare_input(scan_, data, n_points, &layout, &cfg, &info), "mh_radar_prepare_input");
    n_points_in_ = info.n_points_in;
    n_points_valid_ = info.n_points_valid;
  }
  // manager.cpp:84-86: the factor of this message over the device-resident valid_targets_
  DopplerHessianFactor::Ptr makeFactor(const gtsam::Vector3 & angular_velocity_mean) const
  {
    return std::make_shared<DopplerHessianFactor>(ctx_, scan_, config_.T_B_S, angular_velocity_mean, X(0), V(0), B(0), config_.noise_sigma);
  }
  TargetVector validTargets() const  // valid_targets_ copied to the host
  {
    size_t n = 0;
    ctx_->check(mh_radar_get_targets(scan_, nullptr, 0, &n), "mh_radar_get_targets");
    std::vector<mh_radar_target> t(n);
    if (n) ctx_->check(mh_radar_get_targets(scan_, t.data(), n, &n), "mh_radar_get_targets");
    TargetVector out;
    out.reserve(n);
    for (const mh_radar_target & p : t) out.emplace_back(p.x, p.y, p.z, p.range, p.azimuth, p.elevation, p.radial_speed, p.intensity);
    return out;
  }
  size_t numPointsIn() const { return n_points_in_; }        // debug_msg_.n_points_in
  size_t numPointsValid() const { return n_points_valid_; }  // debug_msg_.n_points_valid
  const ManagerConfig & config() const { return config_; }

private:
  std::shared_ptr<Context> ctx_;
  ManagerConfig config_;
  mh_radar_scan * scan_ = nullptr;
  size_t n_points_in_ = 0, n_points_valid_ = 0;
};
}  // namespace radar
}  // namespace mimosa_hip
