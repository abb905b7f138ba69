// Drives the pose graph's marginal covariances through the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp: PoseGraph
// covariances / jointCovariances / gate) and through the C ABI on the same graph, for tests/test_gpu_pose_graph_cov_host.py.
// Input file (little-endian, length-prefixed vectors of doubles): poses (12 per pose: R row-major, t), fixed flags (one per
// pose), edges (50 per edge: a, b, Z_R, Z_t, info), candidates (50 each, as edges; NOT set into the graph), damping (1).
// The pairs asked for are the candidates' poses.  Prints one JSON object.
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
static bool same(const std::vector<double> & a, const std::vector<double> & b)
{
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}
static void put(const char * name, const std::vector<double> & v, const char * tail)
{
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s\n", tail);
}
static std::vector<mh_window_edge> edges_of(const std::vector<double> & ED)
{
  std::vector<mh_window_edge> out;
  for (size_t e = 0; e < ED.size() / 50; ++e) {
    const double * q = &ED[50 * e];
    PoseRM Z;
    std::array<double, 36> info;
    std::copy(q + 2, q + 11, Z.R.begin());
    std::copy(q + 11, q + 14, Z.t.begin());
    std::copy(q + 14, q + 50, info.begin());
    out.push_back(poseGraphEdge(static_cast<int32_t>(q[0]), static_cast<int32_t>(q[1]), Z, info));
  }
  return out;
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto P = read_vec(f), FX = read_vec(f), ED = read_vec(f), CA = read_vec(f), DA = read_vec(f);
  const size_t n = P.size() / 12, E = ED.size() / 50, NC = CA.size() / 50;
  if (P.size() != 12 * n || FX.size() != n || ED.size() != 50 * E || CA.size() != 50 * NC || DA.size() != 1 || NC > MH_PGO_COV_PAIRS_MAX) return 2;
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
    const std::vector<mh_window_edge> edges = edges_of(ED), cand = edges_of(CA);
    std::vector<std::pair<int32_t, int32_t>> pairs;
    std::vector<int32_t> ij;
    for (const auto & e : cand) {
      pairs.emplace_back(e.pose_a, e.pose_b);
      ij.push_back(e.pose_a);
      ij.push_back(e.pose_b);
    }

    PoseGraph mirror(ctx, n, E);
    mirror.setPoses(poses);
    mirror.setFixed(fixed);
    mirror.setEdges(edges);
    mh_pose_graph * plain = nullptr;
    ctx->check(mh_pose_graph_create(ctx->get(), n, E, &plain), "mh_pose_graph_create");
    ctx->check(mh_pose_graph_set_poses(plain, R.data(), t.data(), n), "mh_pose_graph_set_poses");
    ctx->check(mh_pose_graph_set_fixed(plain, fixed.data()), "mh_pose_graph_set_fixed");
    ctx->check(mh_pose_graph_set_edges(plain, edges.data(), E), "mh_pose_graph_set_edges");

    std::vector<double> cov_m, cov_j, joint_m, cov_p(36 * n), joint_p(144 * NC);
    const mh_pose_graph_cov_info i1 = mirror.covariances(DA[0], &cov_m);
    const mh_pose_graph_cov_info i2 = mirror.jointCovariances(DA[0], pairs, &joint_m, &cov_j);
    mh_pose_graph_cov_info i3{};
    ctx->check(mh_pose_graph_covariances(plain, DA[0], cov_p.data(), NC ? ij.data() : nullptr, NC, NC ? joint_p.data() : nullptr, &i3), "mh_pose_graph_covariances");
    const bool equal = same(cov_m, cov_p) && same(cov_j, cov_p) && same(joint_m, joint_p) && i1.flags == i3.flags && i2.flags == i3.flags && i2.n_pairs == i3.n_pairs &&
                       i1.n_pairs == 0 && i1.n_far == i3.n_far && i1.n_poses == i3.n_poses;
    const std::vector<PoseGraph::Gate> g = mirror.gate(cand, DA[0]);
    std::vector<double> r, chi2, d2;
    bool valid = true;
    for (const auto & q : g) {
      r.insert(r.end(), q.r.begin(), q.r.end());
      chi2.push_back(q.chi2);
      d2.push_back(q.d2);
      valid = valid && q.valid;
    }
    std::printf("{\n\"calls_equal\": %d,\n\"flags\": %d,\n\"n_far\": %d,\n\"valid\": %d,\n", equal ? 1 : 0, i3.flags, i3.n_far, valid ? 1 : 0);
    put("cov", cov_m, ",");
    put("joint", joint_m, ",");
    put("r", r, ",");
    put("chi2", chi2, ",");
    put("d2", d2, "");
    std::printf("}\n");
    mh_pose_graph_destroy(plain);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "pose_graph_cov_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
