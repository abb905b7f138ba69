// Drives Geometric::updateMap of the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp) twice per run, with
// GeometricConfig::map_keyframe_min_new_fraction at each value the test passes, on inputs written by
// tests/test_gpu_map_preview_host.py (the inputs of host_pipeline.cpp, then the fractions).  Each fraction runs through the
// device-resident front end (previewInsertBodyCloud) and through the host cloud (mh_transform_f32 + previewInsert).  Before the
// second updateMap the driver makes a preview of its own on the map as it stands; out as JSON: per run the decisions, the debug
// block's fraction and counts, the driver's own preview and the map's stats after either call.
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
static Pose3 pose_from(const double * p) { return pose3(p, p + 9); }
static void dump_preview(const char * name, const mh_map_insert_preview & p)
{
  std::printf("\"%s\": [%lld, %lld, %lld, %lld, %lld, %lld], ", name, static_cast<long long>(p.n_points), static_cast<long long>(p.n_added),
              static_cast<long long>(p.n_too_close), static_cast<long long>(p.n_voxel_full), static_cast<long long>(p.n_touched_voxels),
              static_cast<long long>(p.n_new_voxels));
}
static void dump_step(const char * name, Geometric & geo, bool last = false)
{
  mh_map_stats s{};
  if (mh_map_get_stats(geo.map()->underlying(), &s) != MH_OK) throw std::runtime_error("mh_map_get_stats");
  std::printf("\"%s\": {\"map_updated\": %d, \"map_new_fraction\": %.17g, ", name, geo.debug().map_updated ? 1 : 0, geo.debug().map_new_fraction);
  dump_preview("map_preview", geo.debug().map_preview);
  std::printf("\"n_points\": %lld, \"n_voxels\": %lld, \"uploads\": %lld}%s", static_cast<long long>(s.n_points), static_cast<long long>(s.n_voxels),
              static_cast<long long>(s.uploads), last ? "" : ", ");
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  auto map_xyz = read_vec<float>(f);        // 3 per point
  auto scan = read_vec<Point>(f);           // skewed scan, sensor frame
  auto unique_ns = read_vec<uint32_t>(f);
  auto poses12 = read_vec<double>(f);       // T_Le_Lt per unique ns: R(9) t(3)
  auto misc = read_vec<double>(f);          // T_B_L (12), T_W_B of the first updateMap (12), of the second (12)
  auto raw = read_vec<PointOuster>(f);      // the raw cloud the scan came from, for the device-resident front end
  auto fractions = read_vec<double>(f);
  if (!f || misc.size() != 36 || raw.empty() || fractions.empty()) return 3;
  try {
    auto ctx = std::make_shared<Context>(0);
    std::vector<Pose3> T_Le_Lt(unique_ns.size());
    for (size_t g = 0; g < unique_ns.size(); ++g) T_Le_Lt[g] = pose_from(&poses12[12 * g]);
    deskewPoints(*ctx, scan, unique_ns, T_Le_Lt);
    std::printf("{\"default_fraction\": %.17g, \"runs\": [\n", GeometricConfig().map_keyframe_min_new_fraction);
    bool first_run = true;
    for (const double fraction : fractions)
      for (int device = 1; device >= 0; --device) {
        GeometricConfig cfg;
        cfg.T_B_L = pose_from(&misc[0]);
        cfg.point_skip_divisor = 4;
        cfg.map_keyframe_trans_thresh = 2;
        cfg.map_keyframe_rot_thresh_deg = 30;
        cfg.initial_clouds_to_force_map_update = 1;
        cfg.lru_horizon = 1000;
        cfg.neighbor_voxel_mode = 19;
        cfg.scan_to_map.source_voxel_grid_min_dist_in_voxel = 0.15f;
        cfg.scan_to_map.target_ivox_map_min_dist_in_voxel = 0.15f;
        cfg.map_keyframe_min_new_fraction = fraction;
        Geometric geo(ctx, cfg);
        geo.map()->insert(map_xyz.data(), map_xyz.size() / 3);  // pre-built local map
        ScanFrontEnd fe(ctx);
        ManagerInputConfig icfg = defaultManagerInputConfig();
        icfg.create_full_res_pointcloud = 1;
        icfg.point_skip_divisor = cfg.point_skip_divisor;
        fe.prepareInput(raw.data(), raw.size(), icfg, 100.0);
        fe.deskewPoints(T_Le_Lt);
        Geometric probe(ctx, cfg);
        if (device) {
          geo.preprocess(fe, 0.0);
        } else {
          probe.preprocess(fe, 0.0);  // the device scan's body cloud, for the driver's own preview
          std::vector<size_t> idxs;  // point_skip_divisor filter, manager.cpp:318
          for (size_t i = 0; i < scan.size(); ++i)
            if (scan[i].idx % static_cast<uint32_t>(cfg.point_skip_divisor) == 0) idxs.push_back(i);
          geo.preprocess(scan, idxs, 0.0);
        }
        const Key X0 = X(1);
        Values values;
        values.insert(X0, pose_from(&misc[12]));
        std::printf("%s{\"fraction\": %.17g, \"device\": %d, ", first_run ? "" : ",\n", fraction, device);
        first_run = false;
        geo.updateMap(X0, values);  // forced: initial_clouds_to_force_map_update
        dump_step("first", geo);
        values.update(X0, pose_from(&misc[24]));
        const mh_map_insert_preview own = geo.map()->previewInsertBodyCloud(fe.underlying(), pose_from(&misc[24]));
        dump_preview("own_preview", own);
        geo.updateMap(X0, values);
        dump_step("second", geo, true);
        std::printf("}");
      }
    std::printf("\n]}\n");
  } catch (const std::exception & e) {
    std::fprintf(stderr, "map_preview_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
