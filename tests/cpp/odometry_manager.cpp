// Drives odometry::Manager of the C++ host mirror (mimosa_amd/host/mimosa_hip/odometry.hpp) for tests/test_odometry_cpu.py.
// stdin: d_opt_thresh, sigma_rot_deg, sigma_trans_m, T_B_S (R[9] row-major, t[3]), the number of messages, per message the key,
// T_Ow_S (R[9], t[3]) and the covariance (36, row-major).  stdout: JSON, per message the D-optimality, the outcome and, for a
// factor, its keys, measurement, sigmas and the window edge made from it.
#include <cstdio>
#include <cstdlib>

#include "../../mimosa_amd/host/mimosa_hip/odometry.hpp"

using namespace mimosa_hip;

static double rd()
{
  double v = 0;
  if (std::scanf("%lf", &v) != 1) std::exit(2);
  return v;
}
static Pose3 rd_pose()
{
  double R[9], t[3];
  for (double & v : R) v = rd();
  for (double & v : t) v = rd();
  return pose3(R, t);
}
static void num(double v)
{
  if (std::isnan(v))
    std::printf("NaN");
  else if (std::isinf(v))
    std::printf(v > 0 ? "Infinity" : "-Infinity");
  else
    std::printf("%.17g", v);
}
static void arr(const char * name, const double * v, int n)
{
  std::printf("\"%s\": [", name);
  for (int i = 0; i < n; ++i) {
    std::printf("%s", i ? ", " : "");
    num(v[i]);
  }
  std::printf("]");
}

int main()
{
  odometry::ManagerConfig cfg;
  cfg.d_opt_thresh = static_cast<float>(rd());
  cfg.sigma_rot_deg = static_cast<float>(rd());
  cfg.sigma_trans_m = static_cast<float>(rd());
  cfg.T_B_S = rd_pose();
  odometry::Manager mgr(cfg);
  const int n = static_cast<int>(rd());
  std::printf("[");
  for (int k = 0; k < n; ++k) {
    const uint64_t key = static_cast<uint64_t>(rd());
    const Pose3 T = rd_pose();
    double cov[36];
    for (double & v : cov) v = rd();
    odometry::Manager::Measurement m;
    const odometry::Manager::Outcome o = mgr.callback(T, cov, key, m);
    std::printf("%s{\"d_opt\": ", k ? ", " : "");
    num(mgr.lastDoptimality());
    std::printf(", \"det\": ");
    num(odometry::determinant6(cov));
    std::printf(", \"outcome\": \"%s\"", o == odometry::Manager::Outcome::Rejected ? "rejected" : o == odometry::Manager::Outcome::Initialised ? "initialised" : "factor");
    if (o == odometry::Manager::Outcome::Factor) {
      const PoseRM Z = rowMajor(m.factor->measured());
      const auto model = std::dynamic_pointer_cast<gtsam::noiseModel::Diagonal>(m.factor->noiseModel());
      double s[6], info[36];
      for (int i = 0; i < 6; ++i) s[i] = model ? model->sigmas()(i) : -1.0;
      const lidar::ICPFactor::WindowEdge e = odometry::Manager::windowEdge(m, 1, 3);
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) info[6 * r + c] = e.info(r, c);
      const PoseRM EZ = rowMajor(e.Z);
      std::printf(", \"key1\": %llu, \"key2\": %llu, \"prev_key\": %llu, \"dim\": %zu, ", static_cast<unsigned long long>(m.factor->key1()),
                  static_cast<unsigned long long>(m.factor->key2()), static_cast<unsigned long long>(m.prev_key), m.factor->dim());
      arr("R", Z.R.data(), 9);
      std::printf(", ");
      arr("t", Z.t.data(), 3);
      std::printf(", ");
      arr("sigmas", s, 6);
      std::printf(", \"edge\": {\"a\": %zu, \"b\": %zu, ", e.a, e.b);
      arr("R", EZ.R.data(), 9);
      std::printf(", ");
      arr("t", EZ.t.data(), 3);
      std::printf(", ");
      arr("info", info, 36);
      std::printf("}");
    }
    std::printf("}");
  }
  std::printf("]\n");
  return 0;
}
