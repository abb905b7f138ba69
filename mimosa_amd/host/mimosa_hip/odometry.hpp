// odometry::Manager counterpart (src/odometry/manager.cpp:22-67, include/mimosa/odometry/utils.hpp:19-32) without ROS: gate an
// external odometry message by the D-optimality of its pose covariance, turn consecutive accepted poses into the relative
// motion of the body and emit it as a gtsam::BetweenFactor<gtsam::Pose3> with diagonal sigmas — and, as the same data, an
// ICPFactor::WindowEdge for the fixed-lag chain on the device (mh_icp_window_optimise_edges).  Host-only: no kernel.
#pragma once

#include <cmath>
#include <memory>

#include <gtsam/linear/NoiseModel.h>
#include <gtsam/slam/BetweenFactor.h>

#include "lidar.hpp"

namespace mimosa_hip
{
namespace odometry
{
// the determinant of a 6 x 6 matrix (row-major) by Gaussian elimination with partial pivoting
inline double determinant6(const double cov[36])
{
  double a[36];
  for (int i = 0; i < 36; ++i) a[i] = cov[i];
  double det = 1.0;
  for (int k = 0; k < 6; ++k) {
    int piv = k;
    for (int r = k + 1; r < 6; ++r)
      if (std::fabs(a[6 * r + k]) > std::fabs(a[6 * piv + k])) piv = r;
    if (a[6 * piv + k] == 0.0) return 0.0;
    if (piv != k) {
      for (int c = 0; c < 6; ++c) std::swap(a[6 * k + c], a[6 * piv + c]);
      det = -det;
    }
    det *= a[7 * k];
    for (int r = k + 1; r < 6; ++r) {
      const double m = a[6 * r + k] / a[7 * k];
      for (int c = k; c < 6; ++c) a[6 * r + c] -= m * a[6 * k + c];
    }
  }
  return det;
}

// utils.hpp:21, as written there: exp(log(pow(det, 1 / rows))).  A negative determinant gives NaN (pow of a negative base with
// a fractional exponent), and NaN > thresh is false: such a message passes the gate, as in the reference.
inline double calcDoptimality(const double cov[36]) { return std::exp(std::log(std::pow(determinant6(cov), 1.0 / 6.0))); }

struct ManagerConfig
{
  Pose3 T_B_S;  // SensorManagerBaseConfig::T_B_S
  float d_opt_thresh = 1;
  float sigma_rot_deg = 1.0;
  float sigma_trans_m = 0.5;
};

class Manager
{
public:
  // what an accepted message behind the first one produces
  struct Measurement
  {
    std::shared_ptr<gtsam::BetweenFactor<Pose3>> factor;  // BetweenFactor(X(prev_key), X(0), T_Bkm1_Bk, Diagonal::Sigmas), manager.cpp:53
    Pose3 T_Bkm1_Bk;
    V6D sigmas;          // (deg2rad(sigma_rot_deg) x 3, sigma_trans_m x 3)
    uint64_t prev_key;   // the key the previous accepted message was declared under
  };
  enum class Outcome
  {
    Rejected,     // the gate: d_opt > d_opt_thresh; the previous pose does not advance (manager.cpp:38-41)
    Initialised,  // the first accepted message: no factor (manager.cpp:45)
    Factor,
  };

  explicit Manager(const ManagerConfig & config) : config_(config) {}

  // manager.cpp:22-67 for one message: the pose T_Ow_Sk with its covariance (row-major 6 x 6, as nav_msgs::Odometry carries it),
  // declared under new_key (graph::Manager::declare's key, which the caller owns).  `out` is written for Outcome::Factor.
  Outcome callback(const Pose3 & T_Ow_Sk, const double pose_covariance[36], uint64_t new_key, Measurement & out)
  {
    last_d_opt_ = calcDoptimality(pose_covariance);
    if (last_d_opt_ > config_.d_opt_thresh) return Outcome::Rejected;
    Outcome what = Outcome::Initialised;
    if (initialized_) {
      out.T_Bkm1_Bk = config_.T_B_S * T_Ow_Skm1_.inverse() * T_Ow_Sk * config_.T_B_S.inverse();
      const double sr = static_cast<double>(config_.sigma_rot_deg) * M_PI / 180.0, st = config_.sigma_trans_m;
      gtsam::Vector s(6);
      for (int i = 0; i < 3; ++i) {
        s(i) = sr;
        s(3 + i) = st;
      }
      for (int i = 0; i < 6; ++i) out.sigmas(i) = s(i);
      // the 0 key is the one graph::Manager::declare maps to the new key (manager.cpp:52)
      out.factor = std::make_shared<gtsam::BetweenFactor<Pose3>>(X(prev_key_), X(0), out.T_Bkm1_Bk, gtsam::noiseModel::Diagonal::Sigmas(s));
      out.prev_key = prev_key_;
      what = Outcome::Factor;
    }
    T_Ow_Skm1_ = T_Ow_Sk;
    prev_key_ = new_key;
    initialized_ = true;
    return what;
  }
  // the same measurement for the device chain: poses a < b of the window are the states of prev_key and of the new key
  static lidar::ICPFactor::WindowEdge windowEdge(const Measurement & m, size_t a, size_t b)
  {
    return lidar::ICPFactor::windowEdgeFromSigmas(a, b, m.T_Bkm1_Bk, m.sigmas);
  }
  double lastDoptimality() const { return last_d_opt_; }
  bool initialized() const { return initialized_; }

private:
  ManagerConfig config_;
  bool initialized_ = false;
  uint64_t prev_key_ = 0;
  Pose3 T_Ow_Skm1_;
  double last_d_opt_ = 0.0;
};

}  // namespace odometry
}  // namespace mimosa_hip
