// Drives ICPFactor::alignBatch[Async] / relocaliseBatch of the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp) on inputs
// written by tests/test_gpu_align_batch_host.py: map, scan, registration config, the start poses of the batch, the centre pose of
// the relocalisation grid, the grid, the score / relocalise settings and the align settings in; every member's result, whether
// the call that did not wait gave the same, the grid, the relocalise result and what the factors report afterwards out as JSON.  Input
// file: little-endian length-prefixed vectors.
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
static void dump_score(const char * name, const mh_pose_score & s)
{
  std::printf("\"%s\": [%d, %d, %d, %.17g], ", name, s.n_points, s.n_occupied, s.n_inliers, s.sum_sq);
}
static void dump_pose(const Pose3 & P)
{
  const PoseRM T = rowMajor(P);
  dump("R", T.R.data(), 9);
  dump("t", T.t.data(), 3, true);
}
static bool same(const std::vector<ICPFactor::AlignResult> & a, const std::vector<ICPFactor::AlignResult> & b)
{
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    const PoseRM Ta = rowMajor(a[i].pose), Tb = rowMajor(b[i].pose);
    if (a[i].iters != b[i].iters || a[i].converged != b[i].converged || a[i].trace.size() != b[i].trace.size()) return false;
    if (std::memcmp(Ta.R.data(), Tb.R.data(), 72) != 0 || std::memcmp(Ta.t.data(), Tb.t.data(), 24) != 0) return false;
    for (size_t k = 0; k < a[i].trace.size(); ++k)
      if (a[i].trace[k].f != b[i].trace[k].f || a[i].trace[k].n_knn != b[i].trace[k].n_knn ||
          std::memcmp(a[i].trace[k].R, b[i].trace[k].R, 72) != 0 || std::memcmp(a[i].trace[k].t, b[i].trace[k].t, 24) != 0)
        return false;
  }
  return true;
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto map_xyz = read_vec<float>(f);  // 3 per point
  const auto scan = read_vec<Point>(f);     // sensor frame
  const auto regb = read_vec<uint8_t>(f);   // mh_reg_config
  const auto starts = read_vec<double>(f);  // per member R (9), t (3)
  const auto pose = read_vec<double>(f);    // R (9), t (3): the centre of the grid
  const auto grid = read_vec<double>(f);    // half_xy, step_xy, half_yaw, step_yaw
  const auto sc = read_vec<double>(f);      // gate, stride, top_k, final_gate
  const auto set = read_vec<double>(f);     // max_iters, eps_rot, eps_trans, damping, prior sigmas (rot, trans), check_every
  if (!f || regb.size() != sizeof(RegistrationConfig) || starts.empty() || starts.size() % 12 || pose.size() != 12 || grid.size() != 4 || sc.size() != 4 ||
      set.size() != 7)
    return 3;
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
    ICPFactor::RelocConfig rc;
    rc.score.gate = sc[0];
    rc.score.stride = static_cast<int>(sc[1]);
    rc.score.top_k = static_cast<int>(sc[2]);
    rc.final_gate = sc[3];
    rc.align.max_iters = static_cast<int>(set[0]);
    rc.align.eps_rot = set[1];
    rc.align.eps_trans = set[2];
    rc.align.damping = set[3];
    rc.align.prior_sigma_rot = set[4];
    rc.align.prior_sigma_trans = set[5];
    rc.align.check_every = static_cast<int>(set[6]);
    const Unit3 g(0.0, 0.0, -1.0);

    // the batch on clones of the factor, twice: waited for in the call, and collected later
    const size_t B = starts.size() / 12;
    std::vector<Pose3> T0;
    for (size_t i = 0; i < B; ++i) T0.push_back(pose3(starts.data() + 12 * i, starts.data() + 12 * i + 9));
    std::vector<ICPFactor::AlignResult> res[2];
    std::vector<int> counts;
    for (int round = 0; round < 2; ++round) {
      std::vector<std::shared_ptr<ICPFactor>> own;
      std::vector<ICPFactor *> members;
      for (size_t i = 0; i < B; ++i) {
        own.push_back(std::static_pointer_cast<ICPFactor>(factor.clone()));
        members.push_back(own.back().get());
      }
      if (round == 0) {
        res[0] = ICPFactor::alignBatch(members, T0, g, rc.align);
      } else {
        ICPFactor::AlignBatchCall call = ICPFactor::alignBatchAsync(members, T0, g, rc.align);
        res[1] = call.wait();
      }
      if (round == 0)
        for (const ICPFactor * m : members) counts.push_back(m->getLinearizeCount());
    }
    std::printf("{\n\"async_equal\": %d,\n\"members\": [", same(res[0], res[1]) ? 1 : 0);
    for (size_t i = 0; i < B; ++i) {
      const ICPFactor::AlignResult & r = res[0][i];
      std::printf("%s{\"iters\": %d, \"converged\": %d, \"count\": %d, \"n_trace\": %zu, \"f_last\": %.17g, ", i ? ", " : "", r.iters, r.converged ? 1 : 0,
                  counts[i], r.trace.size(), r.trace.back().f);
      dump_pose(r.pose);
      std::printf("}");
    }
    std::printf("],\n");

    const std::vector<Pose3> poses = ICPFactor::poseGrid(pose3(pose.data(), pose.data() + 9), grid[0], grid[1], grid[2], grid[3]);
    std::printf("\"grid\": [");
    for (size_t i = 0; i < poses.size(); ++i) {
      std::printf("%s{", i ? ", " : "");
      dump_pose(poses[i]);
      std::printf("}");
    }
    std::printf("],\n");
    const ICPFactor::RelocResult r = factor.relocaliseBatch(poses, g, rc);
    const ICPFactor::RelocResult again = factor.relocaliseBatch(poses, g, rc);  // on the clones it kept
    const PoseRM Ta = rowMajor(r.pose), Tb = rowMajor(again.pose);
    const bool repeat_equal = again.best == r.best && std::memcmp(Ta.R.data(), Tb.R.data(), 72) == 0 && std::memcmp(Ta.t.data(), Tb.t.data(), 24) == 0;
    std::printf("\"reloc\": {\"best\": %d, \"repeat_equal\": %d, \"pose\": {", r.best, repeat_equal ? 1 : 0);
    dump_pose(r.pose);
    std::printf("}, \"candidates\": [");
    for (size_t i = 0; i < r.candidates.size(); ++i) {
      const ICPFactor::RelocCandidate & c = r.candidates[i];
      std::printf("%s{\"index\": %d, \"iters\": %d, \"converged\": %d, ", i ? ", " : "", c.index, c.iters, c.converged ? 1 : 0);
      dump_score("coarse", c.coarse);
      dump_score("fine", c.fine);
      dump_pose(c.pose);
      std::printf("}");
    }
    std::printf("]},\n\"count_after\": %d\n}\n", factor.getLinearizeCount());
  } catch (const std::exception & e) {
    std::fprintf(stderr, "align_batch_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
