// Drives the C++ host mirror of the radar classes (mimosa_amd/host/mimosa_hip/radar.hpp) through the reference's call order
//   Manager::callback: preprocess(PointCloud2) -> DopplerHessianFactor(valid_targets_, T_B_S, omega, X(0), V(0), B(0), sigma)
//   -> linearize(Values) -> clone -> linearize
// on inputs written by tests/test_gpu_radar.py, and prints the results as JSON.
//
// Input (binio vectors): raw record bytes (uint8), layout {kind, point_step, off_x, off_y, off_z, off_intensity, off_velocity}
// (int32), config {range_min, range_max, thr_az, thr_el, filter_min_db, noise_sigma} (float), T_B_S {R row-major, t} (double),
// omega (double), state {R_W_B row-major, t_W_B, v_W, bias_gyro} (double).
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../mimosa_amd/host/mimosa_hip/binio.hpp"
#include "../../mimosa_amd/host/mimosa_hip/radar.hpp"

using namespace mimosa_hip;
using mimosa_hip::binio::read_vec;
using mimosa_hip::lidar::Context;

static void dump_factor(const char * name, const std::shared_ptr<GaussianFactor> & g, bool last)
{
  const auto h = std::dynamic_pointer_cast<HessianFactor>(g);
  if (!h) throw std::runtime_error("linearize did not return a HessianFactor");
  const gtsam::Matrix G = h->information();
  const gtsam::Vector v = h->linearTerm();
  std::printf("\"%s\": {\"keys\": [", name);
  for (size_t i = 0; i < h->keys().size(); ++i) std::printf("%llu%s", static_cast<unsigned long long>(h->keys()[i]), i + 1 < h->keys().size() ? ", " : "");
  std::printf("], \"information\": [");
  for (int r = 0; r < G.rows(); ++r)
    for (int c = 0; c < G.cols(); ++c) std::printf("%.17g%s", G(r, c), (r + 1 < G.rows() || c + 1 < G.cols()) ? ", " : "");
  std::printf("], \"linear\": [");
  for (int i = 0; i < v.size(); ++i) std::printf("%.17g%s", v(i), i + 1 < v.size() ? ", " : "");
  std::printf("], \"f\": %.17g}%s\n", h->constantTerm(), last ? "" : ",");
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto raw = read_vec<uint8_t>(f);
  const auto lay = read_vec<int32_t>(f);
  const auto cf = read_vec<float>(f);
  const auto tbs = read_vec<double>(f);
  const auto om = read_vec<double>(f);
  const auto st = read_vec<double>(f);
  if (lay.size() != 7 || cf.size() != 6 || tbs.size() != 12 || om.size() != 3 || st.size() != 18) {
    std::cerr << "radar_pipeline: malformed input\n";
    return 2;
  }
  try {
    auto ctx = std::make_shared<Context>(0);
    radar::ManagerConfig config;
    config.T_B_S = pose3(tbs.data(), tbs.data() + 9);
    config.range_min = cf[0];
    config.range_max = cf[1];
    config.threshold_azimuth_deg = cf[2];
    config.threshold_elevation_deg = cf[3];
    config.filter_min_db = cf[4];
    config.noise_sigma = cf[5];
    radar::Manager manager(ctx, config);
    mh_radar_layout fields{lay[0], static_cast<uint32_t>(lay[1]), static_cast<uint32_t>(lay[2]), static_cast<uint32_t>(lay[3]),
                           static_cast<uint32_t>(lay[4]), static_cast<uint32_t>(lay[5]), static_cast<uint32_t>(lay[6])};
    const radar::PType type = lay[0] == MH_RADAR_RIO ? radar::PType::Rio : radar::PType::mmWave;
    const size_t n_points = raw.size() / fields.point_step;
    manager.preprocess(type, raw.data(), n_points, fields);

    const gtsam::Vector3 omega(om[0], om[1], om[2]);
    Values values;
    values.insert(X(0), pose3(st.data(), st.data() + 9));
    values.insert(radar::V(0), gtsam::Vector3(st[12], st[13], st[14]));
    values.insert(radar::B(0), gtsam::imuBias::ConstantBias(gtsam::Vector3(0.5, -0.5, 0.25), gtsam::Vector3(st[15], st[16], st[17])));

    auto factor = manager.makeFactor(omega);                     // device-resident targets (manager.cpp:84-86)
    const radar::TargetVector targets = manager.validTargets();  // the same targets through the host
    radar::DopplerHessianFactor host_factor(ctx, targets, config.T_B_S, omega, X(0), radar::V(0), radar::B(0), config.noise_sigma);
    auto cloned = factor->clone();

    std::printf("{\n\"n_points_in\": %zu, \"n_points_valid\": %zu, \"dim\": %zu, \"n_targets\": %zu,\n", manager.numPointsIn(),
                manager.numPointsValid(), factor->dim(), factor->numTargets());
    std::printf("\"corrected_ts\": %.17g,\n", radar::correctedTimestamp(config, 100.0));
    std::printf("\"X0\": %llu, \"V0\": %llu, \"B0\": %llu,\n", static_cast<unsigned long long>(X(0)), static_cast<unsigned long long>(radar::V(0)),
                static_cast<unsigned long long>(radar::B(0)));
    dump_factor("from_scan", factor->linearize(values), false);
    dump_factor("from_targets", host_factor.linearize(values), false);
    dump_factor("clone", cloned->linearize(values), false);
    std::vector<const radar::DopplerHessianFactor *> window{factor.get(), &host_factor};
    const auto batch = radar::DopplerHessianFactor::linearizeBatch(window, values);
    dump_factor("batch0", batch[0], true);
    std::printf("}\n");
  } catch (const std::exception & e) {
    std::cerr << "radar_pipeline: " << e.what() << "\n";
    return 1;
  }
  return 0;
}
