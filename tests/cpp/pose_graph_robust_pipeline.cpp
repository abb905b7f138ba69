// Drives the pose graph's priors and losses through the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp: PoseGraph
// setPriors / setLoss / priorResiduals / weights, posePrior, poseGraphLoss) and through the C ABI on the same graph, for
// tests/test_gpu_pose_graph_robust_host.py.
// Input file (little-endian, length-prefixed vectors of doubles): poses (12 per pose: R row-major, t), fixed flags (one per
// pose), edges (50 per edge: a, b, Z_R, Z_t, info), priors (49 per prior: pose, Z_R, Z_t, info), edge losses (2 per edge: kind,
// param), prior losses (2 per prior), config (iters, check_every, damping, eps_rot, eps_trans).
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
static void put(const char * name, const std::vector<double> & v)
{
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("],\n");
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto P = read_vec(f), FX = read_vec(f), ED = read_vec(f), PR = read_vec(f), EL = read_vec(f), PL = read_vec(f), CF = read_vec(f);
  const size_t n = P.size() / 12, E = ED.size() / 50, NP = PR.size() / 49;
  if (P.size() != 12 * n || FX.size() != n || ED.size() != 50 * E || PR.size() != 49 * NP || EL.size() != 2 * E || PL.size() != 2 * NP || CF.size() != 5) return 2;
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
    std::vector<mh_pose_graph_loss> edge_loss, prior_loss;
    for (size_t e = 0; e < E; ++e) {
      const double * q = &ED[50 * e];
      PoseRM Z;
      std::array<double, 36> info;
      std::copy(q + 2, q + 11, Z.R.begin());
      std::copy(q + 11, q + 14, Z.t.begin());
      std::copy(q + 14, q + 50, info.begin());
      edges.push_back(poseGraphEdge(static_cast<int32_t>(q[0]), static_cast<int32_t>(q[1]), Z, info));
      edge_loss.push_back(poseGraphLoss(static_cast<int32_t>(EL[2 * e]), EL[2 * e + 1]));
    }
    // the mirror's priors go through Pose3 and Matrix6 (posePrior); the C ABI's are filled from the file as it is
    std::vector<mh_pose_prior> priors_m, priors_p(NP);
    for (size_t k = 0; k < NP; ++k) {
      const double * q = &PR[49 * k];
      priors_m.push_back(posePrior(static_cast<int32_t>(q[0]), pose3(q + 1, q + 10), matrix6(q + 13)));
      priors_p[k].pose = static_cast<int32_t>(q[0]);
      std::copy(q + 1, q + 10, priors_p[k].Z_R);
      std::copy(q + 10, q + 13, priors_p[k].Z_t);
      std::copy(q + 13, q + 49, priors_p[k].info);
      prior_loss.push_back(poseGraphLoss(static_cast<int32_t>(PL[2 * k]), PL[2 * k + 1]));
    }
    bool priors_equal = true;
    for (size_t k = 0; k < NP; ++k) priors_equal = priors_equal && !std::memcmp(&priors_m[k], &priors_p[k], sizeof(mh_pose_prior));
    mh_pose_graph_config cfg{};
    cfg.iters = static_cast<int32_t>(CF[0]);
    cfg.check_every = static_cast<int32_t>(CF[1]);
    cfg.damping = CF[2];
    cfg.eps_rot = CF[3];
    cfg.eps_trans = CF[4];

    PoseGraph mirror(ctx, n, E);
    mirror.setPoses(poses);
    mirror.setFixed(fixed);
    mirror.setEdges(edges);
    mirror.setPriors(priors_m);
    mirror.setLoss(edge_loss, prior_loss);
    mh_pose_graph * plain = nullptr;
    ctx->check(mh_pose_graph_create(ctx->get(), n, E, &plain), "mh_pose_graph_create");
    ctx->check(mh_pose_graph_set_poses(plain, R.data(), t.data(), n), "mh_pose_graph_set_poses");
    ctx->check(mh_pose_graph_set_fixed(plain, fixed.data()), "mh_pose_graph_set_fixed");
    ctx->check(mh_pose_graph_set_edges(plain, edges.data(), E), "mh_pose_graph_set_edges");
    ctx->check(mh_pose_graph_set_priors(plain, priors_p.data(), NP), "mh_pose_graph_set_priors");
    ctx->check(mh_pose_graph_set_loss(plain, E ? edge_loss.data() : nullptr, NP ? prior_loss.data() : nullptr), "mh_pose_graph_set_loss");

    std::vector<double> we_m, wp_m, d_m, c_m, we_p(E), wp_p(NP), d_p(6 * NP), c_p(NP);
    double f_p = 0.0;
    const double f_m = mirror.weights(&we_m, &wp_m);
    mirror.priorResiduals(&d_m, &c_m);
    ctx->check(mh_pose_graph_weights(plain, we_p.data(), wp_p.data(), &f_p), "mh_pose_graph_weights");
    ctx->check(mh_pose_graph_prior_residuals(plain, d_p.data(), c_p.data()), "mh_pose_graph_prior_residuals");
    const bool ev = same(we_m, we_p) && same(wp_m, wp_p) && same(d_m, d_p) && same(c_m, c_p) && !std::memcmp(&f_m, &f_p, sizeof(double));
    std::printf("{\n\"priors_equal\": %d,\n\"evaluations_equal\": %d,\n\"f\": %.17g,\n", priors_equal ? 1 : 0, ev ? 1 : 0, f_m);
    put("w_edges", we_m);
    put("w_priors", wp_m);
    put("prior_chi2", c_m);

    std::vector<double> tp_m, tp_p(static_cast<size_t>(cfg.iters) * n * 12, 0.0);
    const mh_pose_graph_result res_m = mirror.optimise(cfg, &tp_m);
    mh_pose_graph_result res_p{};
    ctx->check(mh_pose_graph_optimise(plain, &cfg, &res_p, tp_p.data()), "mh_pose_graph_optimise");
    std::printf("\"optimise_equal\": %d,\n", !std::memcmp(&res_m, &res_p, sizeof(res_m)) && same(tp_m, tp_p) ? 1 : 0);
    // setEdges drops the edges' losses, setPriors the priors': every weight is 1 again
    mirror.setEdges(edges);
    mirror.setPriors(priors_m);
    std::vector<double> we_1, wp_1;
    mirror.weights(&we_1, &wp_1);
    bool ones = we_1.size() == E && wp_1.size() == NP;
    for (double w : we_1) ones = ones && w == 1.0;
    for (double w : wp_1) ones = ones && w == 1.0;
    const std::vector<PoseRM> got = mirror.poses();
    std::printf("\"dropped\": %d,\n\"iters\": %d,\n\"converged\": %d,\n\"n_far\": %d,\n\"f_first\": %.17g,\n\"f_last\": %.17g,\n", ones ? 1 : 0, res_m.iters,
                res_m.converged, res_m.n_far, res_m.f_first, res_m.f_last);
    std::printf("\"poses\": [");
    for (size_t i = 0; i < got.size(); ++i) {
      for (size_t q = 0; q < 9; ++q) std::printf("%s%.17g", (i || q) ? ", " : "", got[i].R[q]);
      for (size_t q = 0; q < 3; ++q) std::printf(", %.17g", got[i].t[q]);
    }
    std::printf("]\n}\n");
    mh_pose_graph_destroy(plain);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "pose_graph_robust_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
