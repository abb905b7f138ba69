// Drives map carving through the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp) and through the C ABI on the same data,
// for tests/test_gpu_map_carve_host.py:
//   IncrementalVoxelMapPCL::carve                      against mh_map_carve on a copy of the map (preview and apply)
//   Geometric::updateMap with map_carve_grid = 0       against copy + f32 transform + insert through the C ABI: what it did before
//   Geometric::updateMap with map_carve_grid = 16      against copy + mh_map_carve + f32 transform + insert through the C ABI
//   the same from a device-resident scan (ScanFrontEnd) against the host-cloud path of the same scan
// Input file (little-endian, length-prefixed vectors): map xyz, clutter xyz, the scan (Point, lidar frame, deskewed), the raw
// Ouster cloud it came from, doubles T_B_L (12) T_W_B (12).  Prints one JSON object.
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
static bool same(const mh_map_carve_result & a, const mh_map_carve_result & b) { return !std::memcmp(&a, &b, sizeof(a)); }
static bool same_cloud(IncrementalVoxelMapPCL & a, IncrementalVoxelMapPCL & b)
{
  const PointCloud ca = a.getCloud(), cb = b.getCloud();
  if (ca.size() != cb.size()) return false;
  for (size_t i = 0; i < ca.size(); ++i)
    if (std::memcmp(&ca[i].x, &cb[i].x, 3 * sizeof(float))) return false;
  return true;
}
static void print(const char * name, const mh_map_carve_result & r)
{
  std::printf("\"%s\": [%lld, %lld, %lld, %lld, %lld, %lld],\n", name, static_cast<long long>(r.n_obs_used), static_cast<long long>(r.n_cells_hit),
              static_cast<long long>(r.n_tested), static_cast<long long>(r.n_removed), static_cast<long long>(r.n_voxels_touched),
              static_cast<long long>(r.n_voxels_emptied));
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  auto map_xyz = read_vec<float>(f);
  auto clutter = read_vec<float>(f);
  auto scan = read_vec<Point>(f);
  auto raw = read_vec<PointOuster>(f);
  auto misc = read_vec<double>(f);
  try {
    auto ctx = std::make_shared<Context>(0);
    const Pose3 T_B_L = pose3(&misc[0], &misc[9]), T_W_B = pose3(&misc[12], &misc[21]);
    GeometricConfig cfg;
    cfg.T_B_L = T_B_L;
    cfg.initial_clouds_to_force_map_update = 1;
    cfg.lru_horizon = 1000;
    cfg.neighbor_voxel_mode = 19;
    cfg.scan_to_map.source_voxel_grid_min_dist_in_voxel = 0.15f;
    cfg.scan_to_map.target_ivox_map_min_dist_in_voxel = 0.15f;
    mh_map_carve_config cc{};
    cc.grid = 16;
    cc.ring = 1;
    cc.range_min = 0.5;
    cc.range_max = 6.0;
    cc.margin_abs = 0.2;
    cc.margin_rel = 0.01;
    const V3D origin_B = T_B_L.translation();
    const PoseRM T = rowMajor(T_W_B);
    const A3 o = toArray(origin_B);

    // the body cloud as Geometric::preprocess makes it: every point, f32 transform by T_B_L on the device
    PointCloud Be = scan;
    float Rt[12];
    toFloat12(T_B_L, Rt);
    ctx->check(mh_transform_f32(ctx->get(), Be.data(), Be.size(), Rt, Rt + 9), "mh_transform_f32");
    std::vector<size_t> idxs(scan.size());
    for (size_t i = 0; i < idxs.size(); ++i) idxs[i] = i;
    const Key X0 = X(1);
    Values values;
    values.insert(X0, T_W_B);

    auto seeded = [&](const GeometricConfig & c) {
      auto g = std::make_unique<Geometric>(ctx, c);
      g->map()->insert(map_xyz.data(), map_xyz.size() / 3);
      g->map()->insert(clutter.data(), clutter.size() / 3);
      return g;
    };
    std::printf("{\n");

    // ---- the map's own calls ----
    auto base = seeded(cfg);
    auto m1 = base->map()->fork(), m2 = base->map()->fork();
    cc.apply = 0;
    const mh_map_carve_result pv = m1->carve(Be, origin_B, T_W_B, cc);
    mh_map_carve_result r{};
    ctx->check(mh_map_carve(m2->underlying(), &Be[0].x, Be.size(), sizeof(Point) / sizeof(float), o.data(), T.R.data(), T.t.data(), &cc, &r), "mh_map_carve");
    print("preview", pv);
    std::printf("\"preview_equal\": %d,\n\"preview_moves_nothing\": %d,\n", same(pv, r) ? 1 : 0, same_cloud(*m1, *base->map()) ? 1 : 0);
    cc.apply = 1;
    const mh_map_carve_result ap = m1->carve(Be, origin_B, T_W_B, cc);
    ctx->check(mh_map_carve(m2->underlying(), &Be[0].x, Be.size(), sizeof(Point) / sizeof(float), o.data(), T.R.data(), T.t.data(), &cc, &r), "mh_map_carve");
    std::printf("\"apply_equal\": %d,\n\"apply_clouds_equal\": %d,\n\"points_before\": %zu,\n\"points_after\": %zu,\n", same(ap, r) && same(ap, pv) ? 1 : 0,
                same_cloud(*m1, *m2) ? 1 : 0, base->map()->getCloud().size(), m1->getCloud().size());

    // ---- updateMap, switch off: copy + transform + insert, as before ----
    PointCloud W = Be;
    toFloat12(T_W_B, Rt);
    ctx->check(mh_transform_f32(ctx->get(), W.data(), W.size(), Rt, Rt + 9), "mh_transform_f32");
    {
      auto g = seeded(cfg);
      g->preprocess(scan, idxs, 0.0);
      auto by_hand = g->map()->fork();
      g->updateMap(X0, values);
      by_hand->insert(W);
      std::printf("\"off_equal\": %d,\n\"off_carved\": %d,\n", same_cloud(*g->map(), *by_hand) ? 1 : 0, g->debug().map_carved ? 1 : 0);
    }
    // ---- updateMap, switch on ----
    GeometricConfig on = cfg;
    on.map_carve_grid = cc.grid;
    on.map_carve_ring = cc.ring;
    on.map_carve_range_min = cc.range_min;
    on.map_carve_range_max = cc.range_max;
    on.map_carve_margin_abs = cc.margin_abs;
    on.map_carve_margin_rel = cc.margin_rel;
    mh_map_carve_result host_counters{};
    {
      auto g = seeded(on);
      g->preprocess(scan, idxs, 0.0);
      auto by_hand = g->map()->fork();
      g->updateMap(X0, values);
      ctx->check(mh_map_carve(by_hand->underlying(), &Be[0].x, Be.size(), sizeof(Point) / sizeof(float), o.data(), T.R.data(), T.t.data(), &cc, &r), "mh_map_carve");
      by_hand->insert(W);
      host_counters = g->debug().map_carve;
      print("update_map", host_counters);
      std::printf("\"on_equal\": %d,\n\"on_counters_equal\": %d,\n\"on_carved\": %d,\n", same_cloud(*g->map(), *by_hand) ? 1 : 0, same(host_counters, r) ? 1 : 0,
                  g->debug().map_carved ? 1 : 0);
    }
    // ---- the same from a device-resident scan: Be_cloud_ is carved by and inserted from where it lies ----
    {
      auto g = seeded(on);
      ScanFrontEnd fe(ctx);
      ManagerInputConfig icfg = defaultManagerInputConfig();
      icfg.create_full_res_pointcloud = 1;
      icfg.point_skip_divisor = 1;
      fe.prepareInput(raw.data(), raw.size(), icfg, 100.0);
      std::vector<Pose3> still(fe.uniqueNs().size());
      fe.deskewPoints(still);
      g->preprocess(fe, 0.0);
      auto by_hand = g->map()->fork();
      g->updateMap(X0, values);
      const mh_map_carve_result viaScan = by_hand->carveFromScan(fe.underlying(), 1, origin_B, T_W_B, cc);
      by_hand->insertBodyCloud(fe.underlying(), T_W_B);
      print("update_map_device", g->debug().map_carve);
      std::printf("\"device_equal\": %d,\n\"device_counters_equal\": %d\n", same_cloud(*g->map(), *by_hand) ? 1 : 0, same(g->debug().map_carve, viaScan) ? 1 : 0);
    }
    std::printf("}\n");
  } catch (const std::exception & e) {
    std::fprintf(stderr, "map_carve_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
