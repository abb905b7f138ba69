// Drives a WIDE pose graph (mh_pose_graph_create_wide) through the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp: PoseGraph
// with a max_far, poseGraphEdge) and through the C ABI on the same graph, for tests/test_gpu_pose_graph_wide_host.py.
// Input file (little-endian, length-prefixed vectors of doubles): poses (12 per pose: R row-major, t), fixed flags (one per
// pose), edges (50 per edge: a, b, Z_R, Z_t, info), config (iters, check_every, damping, eps_rot, eps_trans, max_far).
// Prints one JSON object.
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../mimosa_amd/host/mimosa_hip/lidar.hpp"

using namespace mimosa_hip;
using namespace mimosa_hip::lidar;

static std::vector<double> read_vec(std::ifstream & f)
{
  uint64_t n = 0;
  f.read(reinterpret_cast<char *>(&n), 8);
  std::vector<double> v(n);
  f.read(reinterpret_cast<char *>(v.data()), static_cast<std::streamsize>(n * sizeof(double)));
  return v;
}
template <typename T>
static bool same(const std::vector<T> & a, const std::vector<T> & b)
{
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto P = read_vec(f), FX = read_vec(f), ED = read_vec(f), CF = read_vec(f);
  const size_t n = P.size() / 12, E = ED.size() / 50;
  if (P.size() != 12 * n || FX.size() != n || ED.size() != 50 * E || CF.size() != 6) return 2;
  try {
    auto ctx = std::make_shared<Context>(0);
    std::vector<PoseRM> poses(n);
    std::vector<double> R(9 * n), t(3 * n);
    std::vector<uint8_t> fixed(n);
    for (size_t i = 0; i < n; ++i) {
      std::copy(&P[12 * i], &P[12 * i + 9], poses[i].R.begin());
      std::copy(&P[12 * i + 9], &P[12 * i + 12], poses[i].t.begin());
      std::copy(&P[12 * i], &P[12 * i + 9], &R[9 * i]);
      std::copy(&P[12 * i + 9], &P[12 * i + 12], &t[3 * i]);
      fixed[i] = FX[i] != 0.0 ? 1 : 0;
    }
    std::vector<mh_window_edge> edges;
    for (size_t e = 0; e < E; ++e) {
      const double * q = &ED[50 * e];
      PoseRM Z;
      std::array<double, 36> info;
      std::copy(q + 2, q + 11, Z.R.begin());
      std::copy(q + 11, q + 14, Z.t.begin());
      std::copy(q + 14, q + 50, info.begin());
      edges.push_back(poseGraphEdge(static_cast<int32_t>(q[0]), static_cast<int32_t>(q[1]), Z, info));
    }
    mh_pose_graph_config cfg{};
    cfg.iters = static_cast<int32_t>(CF[0]);
    cfg.check_every = static_cast<int32_t>(CF[1]);
    cfg.damping = CF[2];
    cfg.eps_rot = CF[3];
    cfg.eps_trans = CF[4];
    const size_t max_far = static_cast<size_t>(CF[5]);

    PoseGraph mirror(ctx, n, E, max_far);
    mirror.setPoses(poses);
    mirror.setFixed(fixed);
    mirror.setEdges(edges);
    mh_pose_graph * plain = nullptr;
    ctx->check(mh_pose_graph_create_wide(ctx->get(), n, E, max_far, &plain), "mh_pose_graph_create_wide");
    ctx->check(mh_pose_graph_set_poses(plain, R.data(), t.data(), n), "mh_pose_graph_set_poses");
    ctx->check(mh_pose_graph_set_fixed(plain, fixed.data()), "mh_pose_graph_set_fixed");
    ctx->check(mh_pose_graph_set_edges(plain, edges.data(), E), "mh_pose_graph_set_edges");

    std::vector<double> chi2_m, r_m, chi2_p(E), r_p(6 * E);
    double f_p = 0.0;
    const double f_m = mirror.residuals(&chi2_m, &r_m);
    ctx->check(mh_pose_graph_residuals(plain, r_p.data(), chi2_p.data(), &f_p), "mh_pose_graph_residuals");
    std::printf("{\n\"residuals_equal\": %d,\n\"f\": %.17g,\n", same(chi2_m, chi2_p) && same(r_m, r_p) && !std::memcmp(&f_m, &f_p, sizeof(double)) ? 1 : 0, f_m);

    std::vector<double> tp_m, tp_p(static_cast<size_t>(cfg.iters) * n * 12, 0.0);
    const mh_pose_graph_result res_m = mirror.optimise(cfg, &tp_m);
    mh_pose_graph_result res_p{};
    ctx->check(mh_pose_graph_optimise(plain, &cfg, &res_p, tp_p.data()), "mh_pose_graph_optimise");
    std::printf("\"optimise_equal\": %d,\n", !std::memcmp(&res_m, &res_p, sizeof(res_m)) && same(tp_m, tp_p) ? 1 : 0);
    std::vector<double> R_p(9 * n), t_p(3 * n);
    size_t n_p = 0;
    ctx->check(mh_pose_graph_get_poses(plain, R_p.data(), t_p.data(), n, &n_p), "mh_pose_graph_get_poses");
    const std::vector<PoseRM> got = mirror.poses();
    bool eq = got.size() == n && n_p == n && mirror.size() == n;
    for (size_t i = 0; eq && i < n; ++i) eq = !std::memcmp(got[i].R.data(), &R_p[9 * i], 72) && !std::memcmp(got[i].t.data(), &t_p[3 * i], 24);
    std::printf("\"poses_equal\": %d,\n\"iters\": %d,\n\"converged\": %d,\n\"n_far\": %d,\n\"f_first\": %.17g,\n\"f_last\": %.17g,\n", eq ? 1 : 0, res_m.iters,
                res_m.converged, res_m.n_far, res_m.f_first, res_m.f_last);
    std::printf("\"poses\": [");
    for (size_t i = 0; i < got.size(); ++i) {
      for (size_t q = 0; q < 9; ++q) std::printf("%s%.17g", (i || q) ? ", " : "", got[i].R[q]);
      for (size_t q = 0; q < 3; ++q) std::printf(", %.17g", got[i].t[q]);
    }
    std::printf("]\n}\n");
    mh_pose_graph_destroy(plain);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "pose_graph_wide_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
