// CPU-only driver for mimosa_hip::lidar::imuSegments (the IMU intervals mh_scan_deskew_imu takes, src/lidar/manager.cpp:459-492):
// reads the inputs written by tests/test_deskew_imu_cpu.py (the layout of tests/cpp/deskew_poses.cpp), prints per interval
// t0, t1, R (9), p (3), v (3), acc (3), omega (3).
#include <cstdio>
#include <fstream>

#include "../../mimosa_amd/host/mimosa_hip/lidar.hpp"
#include "../../mimosa_amd/host/mimosa_hip/photometric.hpp"

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

int main(int argc, char ** argv)
{
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const auto imu_t = read_vec<double>(f);
  const auto meas = read_vec<double>(f);   // per sample: acc(3) gyro(3)
  const auto navd = read_vec<double>(f);   // per sample: R(9) p(3) v(3)
  const auto misc = read_vec<double>(f);   // bias_acc(3) bias_gyro(3) ...
  std::vector<V3D> acc(imu_t.size()), gyro(imu_t.size());
  std::vector<NavState> nav(imu_t.size());
  for (size_t j = 0; j < imu_t.size(); ++j) {
    acc[j] = vector3(&meas[6 * j]);
    gyro[j] = vector3(&meas[6 * j + 3]);
    nav[j] = NavState(pose3(&navd[15 * j], &navd[15 * j + 9]), vector3(&navd[15 * j + 12]));
  }
  try {
    const std::vector<mh_imu_segment> seg = imuSegments(imu_t, acc, gyro, nav, vector3(&misc[0]), vector3(&misc[3]));
    static_assert(sizeof(mh_imu_segment) == 23 * sizeof(double), "mh_imu_segment is 23 doubles");
    std::printf("[");
    for (size_t c = 0; c < seg.size(); ++c) {
      const double * d = reinterpret_cast<const double *>(&seg[c]);
      std::printf("%s[", c ? ",\n" : "");
      for (int i = 0; i < 23; ++i) std::printf("%.17g%s", d[i], i < 22 ? ", " : "");
      std::printf("]");
    }
    std::printf("]\n");
  } catch (const std::exception & e) {
    std::fprintf(stderr, "imu_segments: %s\n", e.what());
    return 1;
  }
  return 0;
}
