// Drives ICPFactor::marginaliseWindowJoint[Async] and optimiseWindowJoint[Async] of the C++ host mirror
// (mimosa_amd/host/mimosa_hip/lidar.hpp) on inputs written by tests/test_gpu_icp_window_joint.py: map, scan (cloned W times),
// registration config, W poses, the window settings, the linear factors, the edges and the carried joint factor (may be absent)
// in; out as JSON, each on fresh factors: the joint marginal from the blocking call, from the asynchronous call, and the poses
// optimiseWindowJoint (blocking, then asynchronous) reaches on the window without its oldest pose with the rebased marginal as its
// joint factor, the edges that do not touch pose 0 and no prior.  Input file: little-endian length-prefixed vectors.
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

static void report(const ICPFactor::WindowJointMarginal & m, const std::vector<ICPFactor::Ptr> & factors)
{
  const size_t n = m.here.poses.size();
  std::printf("{\"valid\": %d, \"n_ties\": %d, \"f\": %.17g, \"poses\": [", m.valid ? 1 : 0, m.n_ties, m.here.f);
  for (size_t k = 0; k < n; ++k) std::printf("%s%zu", k ? ", " : "", m.here.poses[k]);
  std::printf("], \"rebased\": [");
  for (size_t k = 0; k < n; ++k) std::printf("%s%zu", k ? ", " : "", m.prior.poses[k]);
  std::printf("],\n");
  dump("H", m.here.H.data(), static_cast<int>(m.here.H.size()));
  dump("b", m.here.b.data(), static_cast<int>(m.here.b.size()));
  std::vector<double> at;
  for (const Pose3 & T : m.here.at) {
    const PoseRM L = rowMajor(T);
    at.insert(at.end(), L.R.begin(), L.R.end());
    at.insert(at.end(), L.t.begin(), L.t.end());
  }
  dump("at", at.data(), static_cast<int>(at.size()));
  std::printf("\"counts\": [");
  for (size_t i = 0; i < factors.size(); ++i) std::printf("%s%d", i ? ", " : "", factors[i]->getLinearizeCount());
  std::printf("], \"oldest_f\": %.17g}", factors[0]->lastResult().f);
}
static void report(const ICPFactor::WindowResult & r)
{
  std::printf("{\"iters\": %d, \"poses\": [", r.iters);
  for (size_t i = 0; i < r.poses.size(); ++i) {
    const PoseRM T = rowMajor(r.poses[i]);
    std::printf("%s{", i ? ", " : "");
    dump("R", T.R.data(), 9);
    dump("t", T.t.data(), 3, true);
    std::printf("}");
  }
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
  const auto lin = read_vec<double>(f);      // (pose, R (9), t (3), H (36, row-major), b (6), f) x n_lin
  const auto edg = read_vec<double>(f);      // (a, b, R (9), t (3), info (36, row-major)) x n
  const auto jnt = read_vec<double>(f);      // empty, or n, (pose, R (9), t (3)) x n, H (6n x 6n, row-major), b (6n), f
  if (!f || edg.size() % 50 || regb.size() != sizeof(RegistrationConfig) || pose.size() < 24 || pose.size() % 12 || zs.size() != pose.size() / 12 * 13 ||
      set.size() != 17 || lin.size() % 56)
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
      ICPFactor::WindowLinear l;
      l.pose = static_cast<size_t>(q[0]);
      l.at = pose3(q + 1, q + 10);
      l.H = matrix6(q + 13);
      for (int i = 0; i < 6; ++i) l.b(i) = q[49 + i];
      l.f = q[55];
      linear.push_back(l);
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
    ICPFactor::WindowJoint carried;
    if (!jnt.empty()) {
      const size_t nj = static_cast<size_t>(jnt[0]);
      if (jnt.size() != 1 + 13 * nj + 36 * nj * nj + 6 * nj + 1) return 3;
      for (size_t m = 0; m < nj; ++m) {
        const double * q = &jnt[1 + 13 * m];
        carried.poses.push_back(static_cast<size_t>(q[0]));
        carried.at.push_back(pose3(q + 1, q + 10));
      }
      const double * q = &jnt[1 + 13 * nj];
      carried.H.assign(q, q + 36 * nj * nj);
      carried.b.assign(q + 36 * nj * nj, q + 36 * nj * nj + 6 * nj);
      carried.f = q[36 * nj * nj + 6 * nj];
    }
    const ICPFactor::WindowJoint * joint = jnt.empty() ? nullptr : &carried;
    const Unit3 down(0.0, 0.0, -1.0);
    auto fresh = [&] {
      std::vector<ICPFactor::Ptr> factors;
      for (size_t i = 0; i < W; ++i) {
        factors.push_back(std::make_shared<ICPFactor>(X(i), map, scan, reg));
        factors.back()->computeComponents(false);
      }
      return factors;
    };
    std::printf("{\"runs\": [");
    auto a = fresh();
    const ICPFactor::WindowJointMarginal m = ICPFactor::marginaliseWindowJoint(a, poses, between, down, wc, linear, edges, joint);
    report(m, a);
    std::printf(",\n");
    auto b = fresh();
    auto call = ICPFactor::marginaliseWindowJointAsync(b, poses, between, down, wc, linear, edges, joint);
    report(call->waitJointMarginal(), b);
    // the window without its oldest pose: the rebased marginal is its joint factor, the edges that stay are rebased too
    const std::vector<Pose3> rest_poses(poses.begin() + 1, poses.end());
    std::vector<ICPFactor::WindowBetween> rest_between(between.begin() + 1, between.end());
    rest_between[0].present = false;
    std::vector<ICPFactor::WindowEdge> rest_edges;
    for (ICPFactor::WindowEdge e : edges)
      if (e.a > 0) {
        e.a -= 1;
        e.b -= 1;
        rest_edges.push_back(e);
      }
    ICPFactor::WindowConfig wr = wc;
    for (double & v : wr.prior_info) v = 0.0;
    std::printf("],\n\"slid\": [");
    auto c = fresh();
    report(ICPFactor::optimiseWindowJoint(std::vector<ICPFactor::Ptr>(c.begin() + 1, c.end()), rest_poses, rest_between, down, wr, {}, rest_edges, &m.prior));
    std::printf(",\n");
    auto d = fresh();
    auto opt = ICPFactor::optimiseWindowJointAsync(std::vector<ICPFactor::Ptr>(d.begin() + 1, d.end()), rest_poses, rest_between, down, wr, {}, rest_edges, &m.prior);
    report(opt->wait());
    std::printf("]}\n");
  } catch (const std::exception & e) {
    std::fprintf(stderr, "window_joint_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
