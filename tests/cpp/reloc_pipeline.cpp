// Drives ICPFactor::poseGrid / scorePoses[Async] / relocalise of the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp) on
// inputs written by tests/test_gpu_reloc_host.py: map, scan, registration config, the centre pose of the grid, the grid, the
// score / relocalise settings and the align settings in; the grid, every pose's score, the winners, the relocalise result and
// what the factor reports afterwards out as JSON.  Input file: little-endian length-prefixed vectors.
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
static void dump_score(const char * name, const mh_pose_score & s, bool last = false)
{
  std::printf("\"%s\": [%d, %d, %d, %.17g]%s", name, s.n_points, s.n_occupied, s.n_inliers, s.sum_sq, last ? "" : ", ");
}
static void dump_pose(const Pose3 & P)
{
  const PoseRM T = rowMajor(P);
  dump("R", T.R.data(), 9);
  dump("t", T.t.data(), 3, true);
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto map_xyz = read_vec<float>(f);  // 3 per point
  const auto scan = read_vec<Point>(f);     // sensor frame
  const auto regb = read_vec<uint8_t>(f);   // mh_reg_config
  const auto pose = read_vec<double>(f);    // R (9), t (3): the centre of the grid
  const auto grid = read_vec<double>(f);    // half_xy, step_xy, half_yaw, step_yaw
  const auto sc = read_vec<double>(f);      // gate, stride, top_k, final_gate
  const auto set = read_vec<double>(f);     // max_iters, eps_rot, eps_trans, damping, prior sigmas (rot, trans), check_every
  if (!f || regb.size() != sizeof(RegistrationConfig) || pose.size() != 12 || grid.size() != 4 || sc.size() != 4 || set.size() != 7) return 3;
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
    const std::vector<Pose3> poses = ICPFactor::poseGrid(pose3(pose.data(), pose.data() + 9), grid[0], grid[1], grid[2], grid[3]);
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

    const ICPFactor::ScoreResult s = factor.scorePoses(poses, rc.score);
    ICPFactor::ScoreCall call = factor.scorePosesAsync(poses, rc.score);
    const ICPFactor::ScoreResult a = call.wait();
    const ICPFactor::ScoreResult w = factor.scorePoses(poses, rc.score, false);  // the winners alone
    const bool async_equal = a.best == s.best && a.scores.size() == s.scores.size() &&
                             std::memcmp(a.scores.data(), s.scores.data(), s.scores.size() * sizeof(mh_pose_score)) == 0;
    std::printf("{\n\"n_poses\": %zu, \"async_equal\": %d, \"winners_alone_equal\": %d, \"count_before\": %d,\n", poses.size(), async_equal ? 1 : 0,
                (w.best == s.best && w.scores.empty()) ? 1 : 0, factor.getLinearizeCount());
    std::printf("\"grid\": [");
    for (size_t i = 0; i < poses.size(); ++i) {
      std::printf("%s{", i ? ", " : "");
      dump_pose(poses[i]);
      std::printf("}");
    }
    std::printf("],\n\"scores\": [");
    for (size_t i = 0; i < s.scores.size(); ++i)
      std::printf("%s[%d, %d, %d, %.17g]", i ? ", " : "", s.scores[i].n_points, s.scores[i].n_occupied, s.scores[i].n_inliers, s.scores[i].sum_sq);
    std::printf("],\n\"best\": [");
    for (size_t i = 0; i < s.best.size(); ++i) std::printf("%s%d", i ? ", " : "", s.best[i]);
    std::printf("],\n");

    const ICPFactor::RelocResult r = factor.relocalise(poses, Unit3(0.0, 0.0, -1.0), rc);
    std::printf("\"reloc\": {\"best\": %d, \"pose\": {", r.best);
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
    std::fprintf(stderr, "reloc_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
