// Drives ICPFactor::optimiseWindowEdges / optimiseWindowEdgesAsync of the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp) on
// inputs written by tests/test_gpu_window_edges_host.py: map, scan (cloned W times), registration config, W start poses, the
// window settings, the two thresholds, the linear factors, the edges with a dense information matrix and the edges given by
// diagonal sigmas (through ICPFactor::windowEdgeFromSigmas) in; out as JSON, each on fresh factors: optimiseWindowLin,
// optimiseWindowEdges without an edge, optimiseWindowEdges, optimiseWindowEdgesAsync, optimiseWindowEdges under the thresholds —
// the optimised poses, the trace, the evaluated masks and what the factors report afterwards.  Input file: little-endian
// length-prefixed vectors.
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../mimosa_amd/host/mimosa_hip/lidar.hpp"

using namespace mimosa_hip;
using namespace mimosa_hip::lidar;

template <typename T>
static std::vector<T> read_vec(std::ifstream & f)
{
  uint64_t n = 0;
  f.read(reinterpret_cast<char *>(&n), 8);
  std::vector<T> v(n);
  f.read(reinterpret_cast<char *>(v.data()), static_cast<std::streamsize>(n * sizeof(T)));
  return v;
}
static void dump(const char * name, const double * v, int n, bool last = false)
{
  std::printf("\"%s\": [", name);
  for (int i = 0; i < n; ++i) std::printf("%.17g%s", v[i], i + 1 < n ? ", " : "");
  std::printf("]%s\n", last ? "" : ",");
}

static void report(const ICPFactor::WindowResult & r, const std::vector<ICPFactor::Ptr> & factors)
{
  std::printf("{\"iters\": %d, \"converged\": %d,\n\"poses\": [", r.iters, r.converged ? 1 : 0);
  for (size_t i = 0; i < r.poses.size(); ++i) {
    const PoseRM T = rowMajor(r.poses[i]);
    std::printf("%s{", i ? ", " : "");
    dump("R", T.R.data(), 9);
    dump("t", T.t.data(), 3, true);
    std::printf("}");
  }
  std::printf("],\n\"trace\": [");
  for (size_t i = 0; i < r.trace.size(); ++i)
    std::printf("%s[%.17g, %.17g, %.17g, %d, %u]", i ? ", " : "", r.trace[i].f, r.trace[i].step_rot, r.trace[i].step_trans, r.trace[i].flags, r.trace[i].degenerate);
  std::printf("],\n\"evaluated\": [");
  for (size_t i = 0; i < r.evaluated.size(); ++i) std::printf("%s%u", i ? ", " : "", r.evaluated[i]);
  std::printf("],\n\"counts\": [");
  for (size_t i = 0; i < factors.size(); ++i) std::printf("%s%d", i ? ", " : "", factors[i]->getLinearizeCount());
  std::printf("],\n\"last_f\": [");
  for (size_t i = 0; i < factors.size(); ++i) std::printf("%s%.17g", i ? ", " : "", factors[i]->lastResult().f);
  std::printf("]}");
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto map_xyz = read_vec<float>(f);   // 3 per point
  const auto scan = read_vec<Point>(f);      // sensor frame
  const auto regb = read_vec<uint8_t>(f);    // mh_reg_config
  const auto pose = read_vec<double>(f);     // (R (9), t (3)) x W
  const auto zs = read_vec<double>(f);       // (present, R (9), t (3)) x W
  const auto set = read_vec<double>(f);      // iters, between_info[6], prior_info[6], damping, eps_rot, eps_trans, check_every
  const auto thr = read_vec<double>(f);      // relin_rot, relin_trans
  const auto lin = read_vec<double>(f);      // (pose, R (9), t (3), H (36, row-major), b (6), f) x n_lin
  const auto edg = read_vec<double>(f);      // (a, b, R (9), t (3), info (36, row-major)) x n
  const auto sig = read_vec<double>(f);      // (a, b, R (9), t (3), sigmas (6)) x n
  if (!f || edg.size() % 50 || sig.size() % 20 || regb.size() != sizeof(RegistrationConfig) || pose.empty() || pose.size() % 12 || zs.size() != pose.size() / 12 * 13 || set.size() != 17 || thr.size() != 2 ||
      lin.size() % 56)
    return 3;
  try {
    const size_t W = pose.size() / 12;
    RegistrationConfig reg;
    std::memcpy(&reg, regb.data(), sizeof(reg));
    auto ctx = std::make_shared<Context>(0);
    auto map = std::make_shared<IncrementalVoxelMapPCL>(ctx, reg.target_ivox_map_leaf_size);
    map->set_lru_horizon(1000);
    map->set_neighbor_voxel_mode(19);
    map->set_min_dist_in_cell(reg.target_ivox_map_min_dist_in_voxel);
    map->insert(map_xyz.data(), map_xyz.size() / 3);
    ICPFactor::WindowConfig wc;
    wc.iters = static_cast<int>(set[0]);
    for (int i = 0; i < 6; ++i) {
      wc.between_info[i] = set[1 + i];
      wc.prior_info[i] = set[7 + i];
    }
    wc.damping = set[13];
    wc.eps_rot = set[14];
    wc.eps_trans = set[15];
    wc.check_every = static_cast<int>(set[16]);
    std::vector<Pose3> poses(W);
    std::vector<ICPFactor::WindowBetween> between(W);
    for (size_t i = 0; i < W; ++i) {
      poses[i] = pose3(&pose[12 * i], &pose[12 * i + 9]);
      between[i].present = zs[13 * i] != 0.0;
      between[i].Z = pose3(&zs[13 * i + 1], &zs[13 * i + 10]);
    }
    std::vector<ICPFactor::WindowLinear> linear;
    for (size_t j = 0; j < lin.size() / 56; ++j) {
      const double * q = &lin[56 * j];
      const size_t at = static_cast<size_t>(q[0]);
      gtsam::Vector g(6);
      for (int i = 0; i < 6; ++i) g(i) = -q[49 + i];  // a HessianFactor carries -b
      const HessianFactor h(X(at), matrix6(q + 13), g, q[55]);
      linear.push_back(ICPFactor::windowLinearFrom(h, at, pose3(q + 1, q + 10)));
    }
    std::vector<ICPFactor::WindowEdge> edges;
    for (size_t j = 0; j < edg.size() / 50; ++j) {
      const double * q = &edg[50 * j];
      ICPFactor::WindowEdge e;
      e.a = static_cast<size_t>(q[0]);
      e.b = static_cast<size_t>(q[1]);
      e.Z = pose3(q + 2, q + 11);
      e.info = matrix6(q + 14);
      edges.push_back(e);
    }
    for (size_t j = 0; j < sig.size() / 20; ++j) {
      const double * q = &sig[20 * j];
      V6D s;
      for (int i = 0; i < 6; ++i) s(i) = q[14 + i];
      edges.push_back(ICPFactor::windowEdgeFromSigmas(static_cast<size_t>(q[0]), static_cast<size_t>(q[1]), pose3(q + 2, q + 11), s));
    }
    ICPFactor::WindowRelin given;
    given.rot = thr[0];
    given.trans = thr[1];
    const Unit3 down(0.0, 0.0, -1.0);
    std::printf("{\"runs\": [");
    for (int pass = 0; pass < 5; ++pass) {
      std::vector<ICPFactor::Ptr> factors;
      for (size_t i = 0; i < W; ++i) {
        factors.push_back(std::make_shared<ICPFactor>(X(i), map, scan, reg));
        factors.back()->computeComponents(false);
      }
      ICPFactor::WindowResult r;
      if (pass == 0) {
        r = ICPFactor::optimiseWindowLin(factors, poses, between, down, wc, linear);
      } else if (pass == 1) {
        r = ICPFactor::optimiseWindowEdges(factors, poses, between, down, wc, linear, {});
      } else if (pass == 3) {
        auto call = ICPFactor::optimiseWindowEdgesAsync(factors, poses, between, down, wc, linear, edges);
        r = call->wait();
      } else {
        r = ICPFactor::optimiseWindowEdges(factors, poses, between, down, wc, linear, edges, pass == 4 ? &given : nullptr);
      }
      std::printf("%s", pass ? ",\n" : "");
      report(r, factors);
    }
    std::printf("]}\n");
  } catch (const std::exception & e) {
    std::fprintf(stderr, "window_edge_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
