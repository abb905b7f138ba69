// Drives place recognition through the C++ host mirror (mimosa_amd/host/mimosa_hip/lidar.hpp: PlaceDatabase, levelRotation,
// placeCandidatePose) and through the C ABI on the same data, for tests/test_gpu_place_host.py.
// Input file (little-endian, length-prefixed vectors): the raw Ouster clouds of two keyframes and of a query, then doubles:
// g_unit_F (3), the keyframe pose T_W_Fk (12), shift (1).  Prints one JSON object.
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
static bool same(const PlaceDescriptor & a, const PlaceDescriptor & b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(float)); }
static bool same(const std::vector<mh_place_hit> & a, const std::vector<mh_place_hit> & b)
{
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].index != b[i].index || a[i].shift != b[i].shift || std::memcmp(&a[i].dist, &b[i].dist, sizeof(double)) || a[i].tag != b[i].tag) return false;
  return true;
}
static void print9(const char * name, const A9 & a)
{
  std::printf("\"%s\": [", name);
  for (int i = 0; i < 9; ++i) std::printf("%s%.17g", i ? ", " : "", a[static_cast<size_t>(i)]);
  std::printf("],\n");
}

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<std::vector<PointOuster>> raw;
  for (int i = 0; i < 3; ++i) raw.push_back(read_vec<PointOuster>(f));
  auto misc = read_vec<double>(f);
  if (misc.size() != 16) return 2;
  try {
    auto ctx = std::make_shared<Context>(0);
    mh_place_config cfg{};
    cfg.r_min = 0.5;
    cfg.r_max = 40.0;
    cfg.z_min = -2.0;
    cfg.z_max = 30.0;
    cfg.min_overlap = 30;
    cfg.capacity = 8;
    const A9 R_G_F = levelRotation(A3{misc[0], misc[1], misc[2]});
    const A9 I = detail::identity33();
    std::printf("{\n");
    print9("level", R_G_F);
    print9("level_down", levelRotation(A3{0.0, 0.0, -1.0}));
    print9("level_up", levelRotation(A3{0.0, 0.0, 2.0}));
    print9("candidate_R", rowMajor(placeCandidatePose(pose3(&misc[3], &misc[12]), R_G_F, I, static_cast<int>(misc[15]))).R);

    ManagerInputConfig icfg = defaultManagerInputConfig();
    icfg.create_full_res_pointcloud = 1;
    std::vector<std::unique_ptr<ScanFrontEnd>> fe;
    for (const auto & r : raw) {
      fe.push_back(std::make_unique<ScanFrontEnd>(ctx));
      fe.back()->prepareInput(r.data(), r.size(), icfg, 100.0);
    }
    PlaceDatabase mirror(ctx, cfg);
    mh_place_db * plain = nullptr;
    ctx->check(mh_place_db_create(ctx->get(), &cfg, &plain), "mh_place_db_create");

    // describe: a host cloud through the mirror, the scan it came from through the C ABI
    const PointCloud full = fe[2]->download(0);
    const PlaceDescriptor d_host = mirror.describe(full, R_G_F), d_scan = mirror.describeFromScan(fe[2]->underlying(), 0, R_G_F);
    PlaceDescriptor d_abi(d_host.size());
    ctx->check(mh_place_describe_from_scan(plain, fe[2]->underlying(), 0, R_G_F.data(), d_abi.data()), "mh_place_describe_from_scan");
    int occupied = 0;
    for (float v : d_abi) occupied += v > 0.0f ? 1 : 0;
    std::printf("\"describe_equal\": %d,\n\"occupied\": %d,\n", same(d_host, d_abi) && same(d_scan, d_abi) ? 1 : 0, occupied);

    // add: from a scan and from a host descriptor, both ways
    int32_t idx = -1;
    const int32_t i0 = mirror.addFromScan(fe[0]->underlying(), 0, 70);
    const int32_t i1 = mirror.add(mirror.describeFromScan(fe[1]->underlying(), 0), 71);
    ctx->check(mh_place_db_add_from_scan(plain, fe[0]->underlying(), 0, I.data(), 70, &idx), "mh_place_db_add_from_scan");
    PlaceDescriptor k1(d_host.size());
    ctx->check(mh_place_describe_from_scan(plain, fe[1]->underlying(), 0, I.data(), k1.data()), "mh_place_describe_from_scan");
    ctx->check(mh_place_db_add(plain, k1.data(), 71, &idx), "mh_place_db_add");
    int64_t tag = 0;
    PlaceDescriptor g0(d_host.size());
    ctx->check(mh_place_db_get(plain, 0, g0.data(), nullptr), "mh_place_db_get");
    std::printf("\"add_indices\": [%d, %d, %d],\n\"sizes\": [%zu, %zu],\n", i0, i1, idx, mirror.size(), mh_place_db_size(plain));
    const PlaceDescriptor m1 = mirror.get(1, &tag);
    std::printf("\"get_equal\": %d,\n", same(mirror.get(0), g0) && same(m1, k1) && tag == 71 ? 1 : 0);

    // query: a host descriptor and a scan, both ways
    std::vector<mh_place_score> all_m, all_p(2);
    const auto h_m = mirror.query(mirror.describeFromScan(fe[2]->underlying(), 0), 4, 0, &all_m);
    const auto h_s = mirror.queryFromScan(fe[2]->underlying(), 0, 4);
    std::vector<mh_place_hit> h_p(4);
    ctx->check(mh_place_db_query_from_scan(plain, fe[2]->underlying(), 0, I.data(), 0, 4, h_p.data(), all_p.data()), "mh_place_db_query_from_scan");
    std::printf("\"query_equal\": %d,\n", same(h_m, h_p) && same(h_s, h_p) && all_m.size() == 2 && !std::memcmp(all_m.data(), all_p.data(), 2 * sizeof(mh_place_score)) ? 1 : 0);
    std::printf("\"hits\": [");
    for (size_t i = 0; i < h_m.size(); ++i)
      std::printf("%s[%d, %d, %.17g, %lld]", i ? ", " : "", h_m[i].index, h_m[i].shift, h_m[i].dist, static_cast<long long>(h_m[i].tag));
    std::printf("]\n}\n");
    mh_place_db_destroy(plain);
  } catch (const std::exception & e) {
    std::fprintf(stderr, "place_pipeline: %s\n", e.what());
    return 1;
  }
  return 0;
}
