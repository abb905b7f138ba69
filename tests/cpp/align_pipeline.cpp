// Drives ICPFactor::align of the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp) on inputs written by
// tests/test_gpu_icp_align_host.py: map, scan, registration config, start pose and align settings in; the aligned Pose3, the
// trace and what the factor reports afterwards (getLinearizeCount, lastResult) out as JSON.  The factor is then linearized once
// more at the aligned pose, the way a smoother would take it over.  Input file: little-endian length-prefixed vectors.
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

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto map_xyz = read_vec<float>(f);   // 3 per point
  const auto scan = read_vec<Point>(f);      // sensor frame
  const auto regb = read_vec<uint8_t>(f);    // mh_reg_config
  const auto pose = read_vec<double>(f);     // R (9), t (3)
  const auto set = read_vec<double>(f);      // max_iters, eps_rot, eps_trans, damping, prior sigmas (rot, trans), check_every
  if (!f || regb.size() != sizeof(RegistrationConfig) || pose.size() != 12 || set.size() != 7) return 3;
  try {
    RegistrationConfig reg;
    std::memcpy(&reg, regb.data(), sizeof(reg));
    auto ctx = std::make_shared<Context>(0);
    auto map = std::make_shared<IncrementalVoxelMapPCL>(ctx, reg.target_ivox_map_leaf_size);
    map->set_lru_horizon(1000);
    map->set_neighbor_voxel_mode(19);
    map->set_min_dist_in_cell(reg.target_ivox_map_min_dist_in_voxel);
    map->insert(map_xyz.data(), map_xyz.size() / 3);
    ICPFactor factor(X(0), map, scan, reg);
    factor.computeComponents(false);
    ICPFactor::AlignConfig ac;
    ac.max_iters = static_cast<int>(set[0]);
    ac.eps_rot = set[1];
    ac.eps_trans = set[2];
    ac.damping = set[3];
    ac.prior_sigma_rot = set[4];
    ac.prior_sigma_trans = set[5];
    ac.check_every = static_cast<int>(set[6]);
    const ICPFactor::AlignResult r = factor.align(pose3(pose.data(), pose.data() + 9), Unit3(0.0, 0.0, -1.0), ac);
    const PoseRM T = rowMajor(r.pose);
    std::printf("{\n");
    dump("R", T.R.data(), 9);
    dump("t", T.t.data(), 3);
    std::printf("\"iters\": %d, \"converged\": %d, \"trace_rows\": %zu,\n", r.iters, r.converged ? 1 : 0, r.trace.size());
    std::printf("\"trace\": [");
    for (size_t i = 0; i < r.trace.size(); ++i) {
      std::printf("%s{", i ? ", " : "");
      dump("R", r.trace[i].R, 9);
      dump("t", r.trace[i].t, 3);
      std::printf("\"f\": %.17g, \"step_rot\": %.17g, \"step_trans\": %.17g, \"n_knn\": %lld, \"degenerate\": %d}", r.trace[i].f, r.trace[i].step_rot,
                  r.trace[i].step_trans, static_cast<long long>(r.trace[i].n_knn), r.trace[i].degenerate);
    }
    std::printf("],\n");
    // the factor reports the last evaluated iteration, as after a linearize at that pose
    std::printf("\"count_after_align\": %d,\n", factor.getLinearizeCount());
    dump("last_H", factor.lastResult().H_ss, 36);
    dump("last_b", factor.lastResult().b_s, 6);
    std::printf("\"last_f\": %.17g,\n", factor.lastResult().f);
    Values v;
    v.insert(G(0), Unit3(0.0, 0.0, -1.0));
    v.insert(X(0), r.pose);
    const auto h = std::static_pointer_cast<HessianFactor>(factor.linearize(v));
    std::printf("\"count_after_linearize\": %d, \"f_at_aligned_pose\": %.17g\n}\n", factor.getLinearizeCount(), h->constantTerm());
  } catch (const std::exception & e) {
    std::fprintf(stderr, "align_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
