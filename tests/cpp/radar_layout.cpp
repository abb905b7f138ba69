// Prints sizeof / offsetof of the radar structs of include/mimosa_hip.h as JSON, for tests/test_radar_cpu.py to compare with
// the ctypes mirrors in mimosa_amd/capi.py.
#include <cstddef>
#include <cstdio>

#include "../../include/mimosa_hip.h"

#define FIELD(T, f) std::printf("\"%s.%s\": %zu, ", #T, #f, offsetof(T, f))
#define SIZE(T) std::printf("\"%s\": %zu, ", #T, sizeof(T))

int main()
{
  std::printf("{");
  SIZE(mh_radar_config);
  FIELD(mh_radar_config, range_min);
  FIELD(mh_radar_config, range_max);
  FIELD(mh_radar_config, threshold_azimuth_deg);
  FIELD(mh_radar_config, threshold_elevation_deg);
  FIELD(mh_radar_config, filter_min_db);
  FIELD(mh_radar_config, noise_sigma);
  SIZE(mh_radar_layout);
  FIELD(mh_radar_layout, kind);
  FIELD(mh_radar_layout, point_step);
  FIELD(mh_radar_layout, off_x);
  FIELD(mh_radar_layout, off_y);
  FIELD(mh_radar_layout, off_z);
  FIELD(mh_radar_layout, off_intensity);
  FIELD(mh_radar_layout, off_velocity);
  SIZE(mh_radar_target);
  FIELD(mh_radar_target, x);
  FIELD(mh_radar_target, y);
  FIELD(mh_radar_target, z);
  FIELD(mh_radar_target, range);
  FIELD(mh_radar_target, azimuth);
  FIELD(mh_radar_target, elevation);
  FIELD(mh_radar_target, radial_speed);
  FIELD(mh_radar_target, intensity);
  SIZE(mh_radar_info);
  FIELD(mh_radar_info, n_points_in);
  FIELD(mh_radar_info, n_points_valid);
  SIZE(mh_radar_result);
  FIELD(mh_radar_result, G11);
  FIELD(mh_radar_result, G12);
  FIELD(mh_radar_result, G13);
  FIELD(mh_radar_result, G22);
  FIELD(mh_radar_result, G23);
  FIELD(mh_radar_result, G33);
  FIELD(mh_radar_result, g1);
  FIELD(mh_radar_result, g2);
  FIELD(mh_radar_result, g3);
  FIELD(mh_radar_result, f);
  FIELD(mh_radar_result, n_targets);
  FIELD(mh_radar_result, gpu_ms);
  std::printf("\"MH_RADAR_MAX_BATCH\": %d, \"MH_RADAR_RIO\": %d, \"MH_RADAR_MMWAVE\": %d, \"MH_RADAR_MMWAVE_DOPPLER_RESIDUAL\": %d}\n",
              MH_RADAR_MAX_BATCH, MH_RADAR_RIO, MH_RADAR_MMWAVE, MH_RADAR_MMWAVE_DOPPLER_RESIDUAL);
  return 0;
}
