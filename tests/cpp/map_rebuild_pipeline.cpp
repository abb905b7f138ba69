// Drives the keyframe cloud store and the map rebuild through the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp), for
// tests/test_gpu_map_rebuild_host.py:
//   KeyframeStore::add / get / size / info                        a cloud goes in and comes back bit for bit
//   Geometric with map_keyframe_store_capacity > 0, K keyframes   rebuildMap(map_poses_) gives a map equal to ivox_map_ — from
//                                                                 device-resident scans and from host clouds
//   rebuildMap at shifted poses                                   against a twin made by hand: one mh_map_insert_device per stored cloud
//   the refusals of rebuildMap; with the switch off no store exists and updateMap builds the map it built before
// Input file (little-endian, length-prefixed vectors): doubles T_B_L (12) then T_W_B (12) per scan; then per scan the deskewed
// cloud (Point, lidar frame) and the raw Ouster cloud it came from.  Prints one JSON object.
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
static bool same_cloud(const PointCloud & ca, const PointCloud & cb)
{
  if (ca.size() != cb.size()) return false;
  for (size_t i = 0; i < ca.size(); ++i)
    if (std::memcmp(&ca[i].x, &cb[i].x, 3 * sizeof(float))) return false;
  return true;
}
// the cloud and every field of the stats but device_bytes.  grown: b is the map updateMap grew by copy-then-insert — a copy counts
// its uploads from zero, so the insert counters (and the bytes host clouds moved) are its own and are left out
static bool same_map(IncrementalVoxelMapPCL & a, IncrementalVoxelMapPCL & b, bool grown = false)
{
  mh_map_stats sa{}, sb{};
  if (mh_map_get_stats(a.underlying(), &sa) != MH_OK || mh_map_get_stats(b.underlying(), &sb) != MH_OK) return false;
  sa.device_bytes = sb.device_bytes = 0;
  if (grown) {
    sa.uploads = sb.uploads = sa.delta_uploads = sb.delta_uploads = 0;
    sa.upload_bytes = sb.upload_bytes = 0;
  }
  return !std::memcmp(&sa, &sb, sizeof(sa)) && same_cloud(a.getCloud(), b.getCloud());
}
template <typename F>
static int throws(F && f)
{
  try {
    f();
  } catch (const std::runtime_error &) {
    return 1;
  }
  return 0;
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  auto misc = read_vec<double>(f);
  const size_t K = misc.size() / 12 - 1;
  std::vector<PointCloud> scans(K);
  std::vector<std::vector<PointOuster>> raws(K);
  for (size_t k = 0; k < K; ++k) {
    scans[k] = read_vec<Point>(f);
    raws[k] = read_vec<PointOuster>(f);
  }
  try {
    auto ctx = std::make_shared<Context>(0);
    const Pose3 T_B_L = pose3(&misc[0], &misc[9]);
    std::vector<Pose3> T_W_B;
    for (size_t k = 0; k < K; ++k) T_W_B.push_back(pose3(&misc[12 * (k + 1)], &misc[12 * (k + 1) + 9]));
    GeometricConfig off;
    off.T_B_L = T_B_L;
    off.initial_clouds_to_force_map_update = K;  // every scan is a keyframe
    off.lru_horizon = 2;                          // short: with more than 10 scans iVox's purge (every 10 inserts) falls inside the run
    off.neighbor_voxel_mode = 19;
    off.scan_to_map.source_voxel_grid_min_dist_in_voxel = 0.15f;
    off.scan_to_map.target_ivox_map_min_dist_in_voxel = 0.15f;
    GeometricConfig on = off;
    on.map_keyframe_store_capacity = static_cast<int>(K);
    on.map_keyframe_store_points = 0;
    for (size_t k = 0; k < K; ++k) on.map_keyframe_store_points += static_cast<int64_t>(scans[k].size());

    auto run_device = [&](Geometric & g) {
      for (size_t k = 0; k < K; ++k) {
        ScanFrontEnd fe(ctx);
        ManagerInputConfig icfg = defaultManagerInputConfig();
        icfg.create_full_res_pointcloud = 1;
        icfg.point_skip_divisor = 1;
        fe.prepareInput(raws[k].data(), raws[k].size(), icfg, 100.0);
        std::vector<Pose3> still(fe.uniqueNs().size());
        fe.deskewPoints(still);
        g.preprocess(fe, 0.0);
        Values values;
        values.insert(X(k + 1), T_W_B[k]);
        g.updateMap(X(k + 1), values);
      }
    };
    auto run_host = [&](Geometric & g) {
      for (size_t k = 0; k < K; ++k) {
        std::vector<size_t> idxs(scans[k].size());
        for (size_t i = 0; i < idxs.size(); ++i) idxs[i] = i;
        g.preprocess(scans[k], idxs, 0.0);
        Values values;
        values.insert(X(k + 1), T_W_B[k]);
        g.updateMap(X(k + 1), values);
      }
    };
    std::printf("{\n");

    // ---- the store through the mirror ----
    {
      KeyframeStore st(ctx, 2, static_cast<int64_t>(scans[0].size()));
      const int32_t i0 = st.add(scans[0], 41), i1 = st.add(PointCloud(), -2);
      int64_t tag0 = 0, tag1 = 0;
      const PointCloud back = st.get(0, &tag0), none = st.get(1, &tag1);
      const mh_keyframes_info info = st.info();
      std::printf("\"store_roundtrip\": %d,\n\"store_full_throws\": %d,\n",
                  i0 == 0 && i1 == 1 && st.size() == 2 && tag0 == 41 && tag1 == -2 && none.empty() && same_cloud(back, scans[0]) && info.keyframes == 2 &&
                      info.points == static_cast<int64_t>(scans[0].size()) ? 1 : 0,
                  throws([&] { st.add(PointCloud(), 0); }));
    }
    // ---- Geometric with the store on, device-resident scans ----
    {
      Geometric g(ctx, on);
      run_device(g);
      auto grown = g.map();
      const mh_map_rebuild_result res = g.rebuildMap(g.mapPoses());
      std::printf("\"device_keyframes\": %lld,\n\"device_points\": %lld,\n\"device_same_poses_equal\": %d,\n\"device_is_a_new_map\": %d,\n",
                  static_cast<long long>(res.keyframes), static_cast<long long>(res.n_points), same_map(*g.map(), *grown, true) ? 1 : 0, g.map() != grown ? 1 : 0);
      // shifted poses against a twin made by hand from the store's own device clouds
      std::vector<Pose3> corrected;
      for (size_t k = 0; k < K; ++k) {
        PoseRM T = rowMajor(T_W_B[k]);
        T.t[0] += 0.13 * static_cast<double>(k);
        T.t[1] -= 0.07 * static_cast<double>(k);
        corrected.push_back(pose3(T.R.data(), T.t.data()));
      }
      g.rebuildMap(corrected);
      IncrementalVoxelMapPCL twin(ctx, off.scan_to_map.target_ivox_map_leaf_size);
      twin.set_lru_horizon(off.lru_horizon);
      twin.set_neighbor_voxel_mode(off.neighbor_voxel_mode);
      twin.set_min_dist_in_cell(off.scan_to_map.target_ivox_map_min_dist_in_voxel);
      for (size_t k = 0; k < K; ++k) {
        const float * d = nullptr;
        size_t n = 0;
        ctx->check(mh_keyframes_device_points(g.keyframeStore()->underlying(), static_cast<int32_t>(k), &d, &n), "mh_keyframes_device_points");
        float Rt[12];
        toFloat12(corrected[k], Rt);
        ctx->check(mh_map_insert_device(twin.underlying(), d, n, 4, Rt, Rt + 9), "mh_map_insert_device");
      }
      std::printf("\"shifted_equal\": %d,\n\"shifted_differs_from_grown\": %d,\n\"map_poses_replaced\": %d,\n", same_map(*g.map(), twin) ? 1 : 0,
                  same_cloud(g.map()->getCloud(), grown->getCloud()) ? 0 : 1,
                  g.mapPoses().size() == K && rowMajor(g.mapPoses()[K - 1]).t[0] == rowMajor(corrected[K - 1]).t[0] ? 1 : 0);
      std::vector<Pose3> short_list(corrected.begin(), corrected.end() - 1);
      std::printf("\"wrong_length_throws\": %d,\n", throws([&] { g.rebuildMap(short_list); }));
    }
    // ---- the same from host clouds ----
    {
      Geometric g(ctx, on);
      run_host(g);
      auto grown = g.map();
      g.rebuildMap(g.mapPoses());
      std::printf("\"host_same_poses_equal\": %d,\n", same_map(*g.map(), *grown, true) ? 1 : 0);
    }
    // ---- the switch off: no store, the map updateMap built before; a carved map is refused ----
    {
      Geometric a(ctx, off), b(ctx, on);
      run_device(a);
      run_device(b);
      std::printf("\"off_no_store\": %d,\n\"off_map_unchanged\": %d,\n\"off_rebuild_throws\": %d,\n", a.keyframeStore() ? 0 : 1, same_map(*a.map(), *b.map()) ? 1 : 0,
                  throws([&] { a.rebuildMap(a.mapPoses()); }));
      GeometricConfig carved = on;
      carved.map_carve_grid = 16;
      Geometric c(ctx, carved);
      std::printf("\"carved_rebuild_throws\": %d\n", throws([&] { c.rebuildMap({}); }));
    }
    std::printf("}\n");
  } catch (const std::exception & e) {
    std::fprintf(stderr, "map_rebuild_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
