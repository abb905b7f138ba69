// C++ host mirror of the reference's LiDAR geometric classes over the C ABI (include/mimosa_hip.h):
//
//   IncrementalVoxelMapPCL   include/mimosa/lidar/incremental_voxel_map.hpp:22-54
//   ICPFactor                include/mimosa/lidar/geometric_factor.hpp:25-563
//   Geometric                include/mimosa/lidar/geometric.hpp:36-89, src/lidar/geometric.cpp
//   Manager::deskewPoints    src/lidar/manager.cpp:385-512 (the per-point part, :496-509)
//
// Same constructor / method / getter names and argument meaning, same call order, same error
// behaviour (std::runtime_error for fatal conditions, per-point failures are statuses).  ROS
// publishers, loggers and config_utilities are replaced by plain structs.  Header-only; link with
// libmimosa_hip.so.  All arithmetic happens behind the C ABI on the GPU — nothing here computes a
// residual, and there is no CPU fallback.
#pragma once

#include <algorithm>
#include <cstring>
#include <limits>
#include <memory>
#include <unordered_map>

#include "../../../include/mimosa_hip.h"
#include "types.hpp"

namespace mimosa_hip
{
namespace lidar
{
using Point = mh_point32;                 // include/mimosa/lidar/point.hpp:18-39
using PointCloud = std::vector<Point>;    // pcl::PointCloud<Point>
using RegistrationConfig = mh_reg_config; // include/mimosa/lidar/geometric_config.hpp:17-33

inline RegistrationConfig defaultRegistrationConfig()
{
  // struct defaults of geometric_config.hpp:17-33
  RegistrationConfig c{};
  c.source_voxel_grid_filter_leaf_size = 0.5f;
  c.source_voxel_grid_min_dist_in_voxel = 0.1f;
  c.target_ivox_map_leaf_size = 0.5f;
  c.target_ivox_map_min_dist_in_voxel = 0.1f;
  c.num_corres_points = 5;
  c.max_corres_distance = 2.24f;
  c.plane_validity_distance = 0.04f;
  c.lidar_point_noise_std_dev = 0.02f;
  c.use_huber = 1;
  c.huber_threshold = 1.345f;
  c.reg_4_dof = 0;
  c.project_on_degneneracy = 1;
  c.degen_thresh_rot = 10;
  c.degen_thresh_trans = 15;
  return c;
}

// GeometricConfig, geometric_config.hpp:37-55 (ROS frame names / log settings dropped)
struct GeometricConfig
{
  bool enabled = true;
  Pose3 T_B_L = Pose3();
  int point_skip_divisor = 1;
  int ring_skip_divisor = 1;
  float map_keyframe_trans_thresh = 0.1f;
  float map_keyframe_rot_thresh_deg = 10;
  // Not in the reference: > 0 replaces the pose test of updateMap by what the test stands in for (geometric.cpp:460-464) — the
  // scan becomes a keyframe when an insert preview says the map would keep at least this fraction of its points.  0 = the pose test.
  double map_keyframe_min_new_fraction = 0;
  // Not in the reference: > 0 carves the forked map by the keyframe's own scan before the insert (mh_map_carve*): map points the
  // scan sees through, on a cube-map direction grid of this many cells per face edge, are removed.  0 = off, the reference's
  // behaviour bit for bit.  The fields after it are mh_map_carve_config's.
  int map_carve_grid = 0;
  int map_carve_ring = 1;
  double map_carve_range_min = 0.5, map_carve_range_max = 60.0;
  double map_carve_margin_abs = 0.3, map_carve_margin_rel = 0.0;
  // Not in the reference: > 0 keeps every keyframe's Be_cloud_ in a device-resident KeyframeStore of this many keyframes and
  // map_keyframe_store_points points in all (both > 0), so that Geometric::rebuildMap can rebuild the map at corrected poses after
  // a loop closure.  0 = off: no store exists and the reference's behaviour holds bit for bit.  The caller sizes the store: a
  // keyframe that does not fit makes updateMap throw.
  int map_keyframe_store_capacity = 0;
  int64_t map_keyframe_store_points = 0;
  size_t initial_clouds_to_force_map_update = 10;
  size_t lru_horizon = 100;
  size_t neighbor_voxel_mode = 7;
  RegistrationConfig scan_to_map = defaultRegistrationConfig();
};

// One context per process/device; thrown errors carry mh_last_error().
class Context
{
public:
  explicit Context(int device = 0) : device_(device)
  {
    if (mh_init(device, &ctx_) != MH_OK) throw std::runtime_error(std::string("mh_init: ") + mh_last_error(nullptr));
  }
  int device() const { return device_; }
  ~Context() { mh_shutdown(ctx_); }
  Context(const Context &) = delete;
  Context & operator=(const Context &) = delete;
  mh_ctx * get() const { return ctx_; }
  void check(int rc, const char * what) const
  {
    if (rc != MH_OK) throw std::runtime_error(std::string(what) + ": " + mh_last_error(ctx_));
  }

private:
  int device_ = 0;
  mh_ctx * ctx_ = nullptr;
};

// ---------------------------------------------------------------------------------------------
class IncrementalVoxelMapPCL
{
public:
  using Ptr = std::shared_ptr<IncrementalVoxelMapPCL>;

  IncrementalVoxelMapPCL(const std::shared_ptr<Context> & ctx, const float leaf_size) : ctx_(ctx)
  {
    cfg_.leaf_size = leaf_size;  // iVox defaults, overridden by Geometric's ctor (geometric.cpp:23-28)
    cfg_.min_dist_in_cell = 0.1;
    cfg_.max_points_in_cell = 20;
    cfg_.neighbor_voxel_mode = 7;
    cfg_.lru_horizon = 100;
    cfg_.lru_clear_cycle = 10;
  }
  // Deep copy constructor (incremental_voxel_map.hpp:33-42)
  IncrementalVoxelMapPCL(const IncrementalVoxelMapPCL & other) : ctx_(other.ctx_), cfg_(other.cfg_)
  {
    if (other.map_) ctx_->check(mh_map_copy(other.map_, &map_), "mh_map_copy");
  }
  IncrementalVoxelMapPCL & operator=(const IncrementalVoxelMapPCL &) = delete;
  ~IncrementalVoxelMapPCL() { mh_map_release(map_); }

  // Successor for copy-then-insert (geometric.cpp:494-495): a deep copy, device to device (the map lives on the GPU;
  // 0.2 ms for a 5 M-point map).  THIS object stays valid and unchanged for the factors that hold it.
  std::shared_ptr<IncrementalVoxelMapPCL> fork()
  {
    ensure();
    std::shared_ptr<IncrementalVoxelMapPCL> next(new IncrementalVoxelMapPCL(ctx_, cfg_, nullptr));
    ctx_->check(mh_map_copy(map_, &next->map_), "mh_map_copy");
    return next;
  }

  // iVox setters used at geometric.cpp:25-28 — must precede the first insert
  void set_lru_horizon(size_t h) { require_empty(); cfg_.lru_horizon = static_cast<int64_t>(h); }
  void set_neighbor_voxel_mode(size_t m) { require_empty(); cfg_.neighbor_voxel_mode = static_cast<int32_t>(m); }
  void set_min_dist_in_cell(double d) { require_empty(); cfg_.min_dist_in_cell = d; }

  void insert(const PointCloud & cloud)  // incremental_voxel_map.cpp:19-24
  {
    ensure();
    if (!cloud.empty())
      ctx_->check(mh_map_insert(map_, &cloud[0].x, cloud.size(), sizeof(Point) / sizeof(float)), "mh_map_insert");
  }
  void insert(const float * xyz, size_t n)
  {
    ensure();
    ctx_->check(mh_map_insert(map_, xyz, n, 3), "mh_map_insert");
  }
  // Geometric::updateMap's insert (geometric.cpp:483-495) of a device-resident scan's Be_cloud_: f32 world transform
  // + greedy insert on the GPU, nothing crosses PCIe.  (ScanFrontEnd is declared below.)
  void insertBodyCloud(mh_scan * scan, const Pose3 & T_W_Be)
  {
    ensure();
    float Rt[12];
    toFloat12(T_W_Be, Rt);
    ctx_->check(mh_map_insert_from_scan(map_, scan, Rt, Rt + 9), "mh_map_insert_from_scan");
  }
  // What insert() / insertBodyCloud() would do to the map, read-only (mh_map_preview_insert*): counts of the points it would keep,
  // refuse as too close, refuse because their voxel is full; outcome (optional) receives one byte per point.
  mh_map_insert_preview previewInsert(const PointCloud & cloud, uint8_t * outcome = nullptr)
  {
    ensure();
    mh_map_insert_preview pv{};
    ctx_->check(mh_map_preview_insert(map_, cloud.empty() ? nullptr : &cloud[0].x, cloud.size(), sizeof(Point) / sizeof(float), &pv, outcome),
                "mh_map_preview_insert");
    return pv;
  }
  mh_map_insert_preview previewInsert(const float * xyz, size_t n, uint8_t * outcome = nullptr)
  {
    ensure();
    mh_map_insert_preview pv{};
    ctx_->check(mh_map_preview_insert(map_, xyz, n, 3, &pv, outcome), "mh_map_preview_insert");
    return pv;
  }
  mh_map_insert_preview previewInsertBodyCloud(mh_scan * scan, const Pose3 & T_W_Be, uint8_t * outcome = nullptr)
  {
    ensure();
    float Rt[12];
    toFloat12(T_W_Be, Rt);
    mh_map_insert_preview pv{};
    ctx_->check(mh_map_preview_insert_from_scan(map_, scan, Rt, Rt + 9, &pv, outcome), "mh_map_preview_insert_from_scan");
    return pv;
  }
  // Map carving (mh_map_carve*): remove (cfg.apply) or count the map points that observations in a frame F — its pose in the map
  // frame T_W_F, the sensor at origin_F in F — see through.  Not in the reference.
  mh_map_carve_result carve(const PointCloud & cloud_F, const V3D & origin_F, const Pose3 & T_W_F, const mh_map_carve_config & cfg)
  {
    return carve(cloud_F.empty() ? nullptr : &cloud_F[0].x, cloud_F.size(), sizeof(Point) / sizeof(float), origin_F, T_W_F, cfg);
  }
  mh_map_carve_result carve(const float * xyz, size_t n, size_t stride_floats, const V3D & origin_F, const Pose3 & T_W_F,
                            const mh_map_carve_config & cfg)
  {
    ensure();
    const PoseRM T = rowMajor(T_W_F);
    const A3 o = toArray(origin_F);
    mh_map_carve_result r{};
    ctx_->check(mh_map_carve(map_, xyz, n, stride_floats, o.data(), T.R.data(), T.t.data(), &cfg, &r), "mh_map_carve");
    return r;
  }
  // ... by a device-resident scan: which = 0 points_full_ (the lidar frame), 1 Be_cloud_ (the body frame)
  mh_map_carve_result carveFromScan(mh_scan * scan, int which, const V3D & origin_F, const Pose3 & T_W_F, const mh_map_carve_config & cfg)
  {
    ensure();
    const PoseRM T = rowMajor(T_W_F);
    const A3 o = toArray(origin_F);
    mh_map_carve_result r{};
    ctx_->check(mh_map_carve_from_scan(map_, scan, which, o.data(), T.R.data(), T.t.data(), &cfg, &r), "mh_map_carve_from_scan");
    return r;
  }
  // incremental_voxel_map.cpp:26-32: true iff k neighbours were found; coordinates instead of ids
  bool knn_search(const V3D & point, const size_t k, std::vector<V3D> & neighbours, std::vector<double> & sq_dists)
  {
    ensure();
    neighbours.assign(k, V3D());
    sq_dists.assign(k, 0.0);
    int32_t found = 0;
    const A3 q = toArray(point);
    std::vector<double> nb(3 * k);
    ctx_->check(mh_map_knn(map_, q.data(), 1, static_cast<int>(k), nb.data(), sq_dists.data(), &found), "mh_map_knn");
    for (size_t i = 0; i < k; ++i) neighbours[i] = vector3(&nb[3 * i]);
    return static_cast<size_t>(found) == k;
  }
  PointCloud getCloud()  // incremental_voxel_map.cpp:34-38
  {
    ensure();
    size_t n = 0;
    ctx_->check(mh_map_get_cloud(map_, nullptr, 0, &n), "mh_map_get_cloud");
    std::vector<float> xyz(3 * n);
    ctx_->check(mh_map_get_cloud(map_, xyz.data(), n, &n), "mh_map_get_cloud");
    PointCloud out(n, Point{});
    for (size_t i = 0; i < n; ++i) {
      out[i].x = xyz[3 * i];
      out[i].y = xyz[3 * i + 1];
      out[i].z = xyz[3 * i + 2];
    }
    return out;
  }
  mh_map * underlying()
  {
    ensure();
    return map_;
  }
  const std::shared_ptr<Context> & context() const { return ctx_; }
  const mh_map_config & config() const { return cfg_; }

private:
  friend class KeyframeStore;  // rebuild() hands a finished mh_map over
  IncrementalVoxelMapPCL(const std::shared_ptr<Context> & ctx, const mh_map_config & cfg, std::nullptr_t) : ctx_(ctx), cfg_(cfg) {}
  void ensure()
  {
    if (!map_) ctx_->check(mh_map_create(ctx_->get(), &cfg_, &map_), "mh_map_create");
  }
  void require_empty() const
  {
    if (map_) throw std::runtime_error("IncrementalVoxelMapPCL: settings must be applied before the first insert");
  }
  std::shared_ptr<Context> ctx_;
  mh_map_config cfg_{};
  mh_map * map_ = nullptr;
};

// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Device-resident scan front end: the part of lidar::Manager between the PointCloud2 callback and the
// geometric factor (prepareInput lidar/manager.cpp:149-383, deskewPoints' per-point loop :496-509),
// with the cloud uploaded once and kept on the GPU.  Geometric::preprocess / getFactors below consume it.
using PointOuster = mh_ouster_point;  // include/mimosa/lidar/point.hpp:42-50
using ManagerInputConfig = mh_input_config;

// The reference's other sensor point types (include/mimosa/lidar/point.hpp:52-131): the records a driver publishes, with
// the members where PCL's EIGEN_ALIGN16 structs put them, and the layout that selects each type's branches of
// Manager::prepareInput<PointT> (tag filter, reflectivity-as-intensity, time decoding, whether the ring filter applies).
struct alignas(16) PointOusterOdyssey { float x, y, z, data_c; uint32_t t; uint16_t reflectivity, near_ir; };
struct alignas(16) PointOusterR8 { float x, y, z, data_c; float intensity; uint32_t t; uint16_t reflectivity; uint8_t ring; };
struct alignas(16) PointHesai { float x, y, z, data_c; float intensity; double timestamp; uint16_t ring; };
struct alignas(16) PointLivox { float x, y, z, data_c; float intensity; uint8_t tag, line; double timestamp; };
struct alignas(16) PointLivoxFromCustom2 { float x, y, z; uint32_t t; float intensity; uint8_t tag, line; };
struct alignas(16) PointVelodyne { float x, y, z, data_c; float intensity; uint16_t ring; float time; };
struct alignas(16) PointVelodyneAnybotics { float x, y, z, data_c; float intensity; float ring; float time; };
struct alignas(16) PointRslidar { float x, y, z, data_c; float intensity; uint16_t ring; double timestamp; };

namespace detail
{
inline mh_point_layout xyz(uint32_t stride, uint32_t off_intensity, uint32_t off_time, mh_time_kind tk)
{
  mh_point_layout L{};
  L.stride = stride;
  L.off_x = 0;
  L.off_y = 4;
  L.off_z = 8;
  L.off_intensity = off_intensity;
  L.off_time = off_time;
  L.time_kind = tk;
  return L;
}
inline mh_point_layout with_ring(mh_point_layout L, uint32_t off, mh_ring_kind kind, bool filter)
{
  L.off_ring = off;
  L.ring_kind = kind;
  L.ring_filter = filter ? 1 : 0;
  return L;
}
inline mh_point_layout with_tag(mh_point_layout L, uint32_t off)
{
  L.off_tag = off;
  L.has_tag = 1;
  return L;
}
}  // namespace detail

template <typename PointT> mh_point_layout layoutOf();
template <> inline mh_point_layout layoutOf<PointOuster>()
{
  return detail::with_ring(detail::xyz(sizeof(PointOuster), offsetof(PointOuster, intensity), offsetof(PointOuster, t), MH_TIME_U32_NS),
                           offsetof(PointOuster, ring), MH_RING_U16, true);
}
template <> inline mh_point_layout layoutOf<PointOusterOdyssey>()
{
  mh_point_layout L = detail::xyz(sizeof(PointOusterOdyssey), offsetof(PointOusterOdyssey, reflectivity), offsetof(PointOusterOdyssey, t), MH_TIME_U32_NS);
  L.intensity_is_u16 = 1;
  return L;
}
template <> inline mh_point_layout layoutOf<PointOusterR8>()
{
  return detail::with_ring(detail::xyz(sizeof(PointOusterR8), offsetof(PointOusterR8, intensity), offsetof(PointOusterR8, t), MH_TIME_U32_NS),
                           offsetof(PointOusterR8, ring), MH_RING_U8, true);
}
template <> inline mh_point_layout layoutOf<PointHesai>()
{
  return detail::with_ring(detail::xyz(sizeof(PointHesai), offsetof(PointHesai, intensity), offsetof(PointHesai, timestamp), MH_TIME_F64_S_ABS),
                           offsetof(PointHesai, ring), MH_RING_U16, true);
}
template <> inline mh_point_layout layoutOf<PointLivox>()
{
  return detail::with_tag(detail::xyz(sizeof(PointLivox), offsetof(PointLivox, intensity), offsetof(PointLivox, timestamp), MH_TIME_F64_NS_ABS),
                          offsetof(PointLivox, tag));
}
template <> inline mh_point_layout layoutOf<PointLivoxFromCustom2>()
{
  return detail::with_tag(detail::xyz(sizeof(PointLivoxFromCustom2), offsetof(PointLivoxFromCustom2, intensity), offsetof(PointLivoxFromCustom2, t),
                                      MH_TIME_U32_NS),
                          offsetof(PointLivoxFromCustom2, tag));
}
template <> inline mh_point_layout layoutOf<PointVelodyne>()
{
  return detail::with_ring(detail::xyz(sizeof(PointVelodyne), offsetof(PointVelodyne, intensity), offsetof(PointVelodyne, time), MH_TIME_F32_S),
                           offsetof(PointVelodyne, ring), MH_RING_U16, true);
}
template <> inline mh_point_layout layoutOf<PointVelodyneAnybotics>()
{
  return detail::with_ring(detail::xyz(sizeof(PointVelodyneAnybotics), offsetof(PointVelodyneAnybotics, intensity),
                                       offsetof(PointVelodyneAnybotics, time), MH_TIME_F32_S),
                           offsetof(PointVelodyneAnybotics, ring), MH_RING_F32, false);
}
template <> inline mh_point_layout layoutOf<PointRslidar>()
{
  return detail::with_ring(detail::xyz(sizeof(PointRslidar), offsetof(PointRslidar, intensity), offsetof(PointRslidar, timestamp), MH_TIME_F64_S_ABS),
                           offsetof(PointRslidar, ring), MH_RING_U16, true);
}

// the cloud's shape and the two Manager flags that re-order it first (lidar/manager.hpp:28-29)
struct CloudOrder
{
  uint32_t width = 0, height = 1;  // width 0: n x 1
  bool transpose_pointcloud = false, organize_pointcloud_by_ring = false;
};

inline ManagerInputConfig defaultManagerInputConfig()
{
  // struct defaults of lidar/manager.hpp:24-41 (+ GeometricConfig skip divisors)
  ManagerInputConfig c{};
  c.range_min = 0.0f;
  c.range_max = 100.0f;
  c.intensity_min = 0.0f;
  c.intensity_max = 1e10f;
  c.ns_max = 1e9f;
  c.z_offset = 0.0f;
  c.create_full_res_pointcloud = 0;
  c.point_skip_divisor = 1;
  c.ring_skip_divisor = 1;
  return c;
}

class ScanFrontEnd
{
public:
  explicit ScanFrontEnd(const std::shared_ptr<Context> & ctx) : ctx_(ctx)
  {
    ctx_->check(mh_scan_create(ctx_->get(), &scan_), "mh_scan_create");
  }
  ~ScanFrontEnd() { mh_scan_destroy(scan_); }
  ScanFrontEnd(const ScanFrontEnd &) = delete;
  ScanFrontEnd & operator=(const ScanFrontEnd &) = delete;

  // Manager::prepareInput<PointOuster>: filters, points_full_, geometric subset, unique_ns_.
  // corrected_ts_ = header_ts + last_point_ns * 1e-9 (manager.cpp:336).
  void prepareInput(const PointOuster * raw, size_t n, const ManagerInputConfig & cfg, const double header_ts)
  {
    ctx_->check(mh_scan_prepare_input(scan_, raw, n, &cfg, &info_), "mh_scan_prepare_input");
    corrected_ts_ = header_ts + info_.last_point_ns * 1.0e-9;
    fetchUniqueNs();
  }
  // Pipelined input: prefetch() stages the NEXT cloud (pinned copy + host-to-device copy on this front end's own copy stream)
  // while another ScanFrontEnd is being processed — it may run on another host thread; prepareInputPrefetched() is
  // prepareInput on the staged cloud (the device waits for the copy, the host does not).
  void prefetch(const PointOuster * raw, size_t n) { ctx_->check(mh_scan_prefetch(scan_, raw, n), "mh_scan_prefetch"); }
  void prepareInputPrefetched(const ManagerInputConfig & cfg, const double header_ts)
  {
    ctx_->check(mh_scan_prepare_input_prefetched(scan_, &cfg, &info_), "mh_scan_prepare_input_prefetched");
    corrected_ts_ = header_ts + info_.last_point_ns * 1.0e-9;
    fetchUniqueNs();
  }
  // Manager::prepareInput<PointT> for any of the reference's point types (the sensor's own records go to the device).
  // transpose_pointcloud is honoured for PointRslidar / PointVelodyneAnybotics only, as in the reference (:177-203).
  template <typename PointT>
  void prepareInput(const PointT * raw, size_t n, const ManagerInputConfig & cfg, const double header_ts, const CloudOrder & order)
  {
    const mh_point_layout L = layoutOf<PointT>();
    const bool may_transpose = std::is_same<PointT, PointRslidar>::value || std::is_same<PointT, PointVelodyneAnybotics>::value;
    const uint32_t width = order.width ? order.width : static_cast<uint32_t>(n);
    ctx_->check(mh_scan_prepare_input_layout(scan_, raw, n, &L, width, order.height, may_transpose && order.transpose_pointcloud ? 1 : 0,
                                             order.organize_pointcloud_by_ring ? 1 : 0, header_ts, &cfg, &info_),
                "mh_scan_prepare_input_layout");
    corrected_ts_ = header_ts + info_.last_point_ns * 1.0e-9;
    fetchUniqueNs();
  }
  // points_raw_ (manager.cpp:376-380): keep a copy of points_full_ as it was before deskewPoints — Photometric::preprocess
  // reads it (call before deskewPoints)
  void keepRaw(bool keep) { ctx_->check(mh_scan_keep_raw(scan_, keep ? 1 : 0), "mh_scan_keep_raw"); }
  const std::vector<uint32_t> & uniqueNs() const { return unique_ns_; }  // the IMU propagation runs over these
  // A caller that deskews with deskewPointsFromImu needs no timestamp on the host: with `keep` false prepareInput* leaves
  // uniqueNs() empty and skips mh_scan_get_unique_ns (a stream wait and a copy for a cloud with per-point times)
  void keepUniqueNsOnHost(bool keep) { unique_ns_on_host_ = keep; }
  double correctedTs() const { return corrected_ts_; }
  const mh_scan_info & info() const { return info_; }

  // Manager::deskewPoints, per-point part: T_Le_Lt[g] belongs to uniqueNs()[g] (manager.cpp:496-509)
  void deskewPoints(const std::vector<Pose3> & T_Le_Lt)
  {
    if (T_Le_Lt.size() != unique_ns_.size()) throw std::runtime_error("deskewPoints: one pose per unique timestamp");
    std::vector<float> Rt12(12 * T_Le_Lt.size());
    for (size_t g = 0; g < T_Le_Lt.size(); ++g) toFloat12(T_Le_Lt[g], &Rt12[12 * g]);
    ctx_->check(mh_scan_deskew(scan_, Rt12.data(), T_Le_Lt.size()), "mh_scan_deskew");
  }
  // the same from n poses laid out as the C ABI takes them, in double: R row-major (9), then t (3) — a caller that forms the
  // poses as plain arrays anyway (replay.hpp) skips the round trip through Pose3
  void deskewPoints(const double * Rt12, const size_t n)
  {
    if (n != unique_ns_.size()) throw std::runtime_error("deskewPoints: one pose per unique timestamp");
    std::vector<float> f(12 * n);
    for (size_t i = 0; i < 12 * n; ++i) f[i] = static_cast<float>(Rt12[i]);
    ctx_->check(mh_scan_deskew(scan_, f.data(), n), "mh_scan_deskew");
  }
  // Manager::deskewPoints with the pose part (manager.cpp:455-499) on the device too: `segments` from imuSegments() below,
  // gravity = unit vector * |g|, T_W_Be = propagated_state_.pose() (:492-493).  No segment: the first, uninitialised cloud
  // (:399-408).  An IMU buffer that ends before the last point is reported by the next call that waits for the device.
  void deskewPointsFromImu(const std::vector<mh_imu_segment> & segments, const double header_ts, const V3D & gravity, const Pose3 & T_W_Be,
                           const Pose3 & T_B_S)
  {
    const PoseRM le_w = rowMajor(T_B_S.inverse() * T_W_Be.inverse()), b_s = rowMajor(T_B_S);  // T_Le_W (:496)
    const double g[3] = {gravity(0), gravity(1), gravity(2)};
    ctx_->check(mh_scan_deskew_imu(scan_, segments.data(), segments.size(), header_ts, g, le_w.R.data(), le_w.t.data(), b_s.R.data(), b_s.t.data()),
                "mh_scan_deskew_imu");
  }
  // interpolated_map_T_Le_Lt_'s poses as deskewPointsFromImu left them on the device, for a caller that still wants them
  std::vector<Pose3> deskewPoses() const
  {
    size_t n = 0;
    ctx_->check(mh_scan_get_deskew_poses(scan_, nullptr, 0, &n), "mh_scan_get_deskew_poses");
    std::vector<double> T(12 * n);
    ctx_->check(mh_scan_get_deskew_poses(scan_, T.data(), n, &n), "mh_scan_get_deskew_poses");
    std::vector<Pose3> out(n);
    for (size_t g = 0; g < n; ++g) out[g] = pose3(&T[12 * g], &T[12 * g + 9]);
    return out;
  }
  // which: 0 points_full_, 1 Be_cloud_, 2 sm_Be_cloud_ds_
  PointCloud download(int which) const
  {
    size_t n = 0;
    ctx_->check(mh_scan_get_points(scan_, which, nullptr, 0, &n), "mh_scan_get_points");
    PointCloud out(n);
    ctx_->check(mh_scan_get_points(scan_, which, out.data(), out.size(), &n), "mh_scan_get_points");
    return out;
  }
  mh_scan * underlying() { return scan_; }
  const std::shared_ptr<Context> & context() const { return ctx_; }
  mh_scan_info & mutableInfo() { return info_; }

private:
  void fetchUniqueNs()
  {
    unique_ns_.resize(unique_ns_on_host_ ? info_.n_unique_ns : 0);
    if (!unique_ns_on_host_) return;
    size_t m = 0;
    ctx_->check(mh_scan_get_unique_ns(scan_, unique_ns_.data(), unique_ns_.size(), &m), "mh_scan_get_unique_ns");
  }
  std::shared_ptr<Context> ctx_;
  mh_scan * scan_ = nullptr;
  mh_scan_info info_{};
  std::vector<uint32_t> unique_ns_;
  bool unique_ns_on_host_ = true;
  double corrected_ts_ = 0;
};

// ---------------------------------------------------------------------------------------------
// Place recognition (mh_place_*; not in the reference): a keyframe database of ring x sector scan descriptors, searched on the
// device.  It stores a tag per entry and no pose: poses stay with the caller, because a smoother moves them.
using PlaceDescriptor = std::vector<float>;  // MH_PLACE_RINGS * MH_PLACE_SECTORS floats, ring-major

namespace detail
{
inline A9 mul33(const A9 & a, const A9 & b)
{
  A9 c{};
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j) c[3 * r + j] += a[3 * r + k] * b[3 * k + j];
  return c;
}
inline A9 transposed33(const A9 & a) { return A9{a[0], a[3], a[6], a[1], a[4], a[7], a[2], a[5], a[8]}; }
inline A9 identity33() { return A9{1, 0, 0, 0, 1, 0, 0, 0, 1}; }
}  // namespace detail

// R_G_F for a gravity direction measured in F: the smallest rotation that takes -g to +z (row-major).  The antipodal case is a
// turn by pi about x.
inline A9 levelRotation(const A3 & g_unit_F)
{
  const double n = std::sqrt(g_unit_F[0] * g_unit_F[0] + g_unit_F[1] * g_unit_F[1] + g_unit_F[2] * g_unit_F[2]);
  const double a0 = -g_unit_F[0] / n, a1 = -g_unit_F[1] / n, c = -g_unit_F[2] / n;
  if (c <= -1.0 + 1e-12) return A9{1, 0, 0, 0, -1, 0, 0, 0, -1};
  const double v0 = a1, v1 = -a0;  // a x z = (v0, v1, 0)
  const A9 K{0, 0, v1, 0, 0, -v0, -v1, v0, 0};
  const A9 KK = detail::mul33(K, K);
  A9 R = detail::identity33();
  for (int i = 0; i < 9; ++i) R[i] += K[i] + KK[i] / (1.0 + c);
  return R;
}

// The pose a hit proposes for the query's frame: T_W_Fq = T_W_Fk * (R_G_Fk^T Rz(+shift * 6 deg) R_G_Fq, 0)
inline Pose3 placeCandidatePose(const Pose3 & T_W_Fk, const A9 & R_G_Fk, const A9 & R_G_Fq, int shift)
{
  const double a = static_cast<double>(shift) * (2.0 * 3.14159265358979323846 / MH_PLACE_SECTORS);
  const A9 Rz{std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a), 0, 0, 0, 1};
  const PoseRM k = rowMajor(T_W_Fk);
  const A9 R = detail::mul33(k.R, detail::mul33(detail::transposed33(R_G_Fk), detail::mul33(Rz, R_G_Fq)));
  return pose3(R.data(), k.t.data());
}

class PlaceDatabase
{
public:
  PlaceDatabase(const std::shared_ptr<Context> & ctx, const mh_place_config & cfg) : ctx_(ctx), cfg_(cfg)
  {
    ctx_->check(mh_place_db_create(ctx_->get(), &cfg_, &db_), "mh_place_db_create");
  }
  ~PlaceDatabase() { mh_place_db_destroy(db_); }
  PlaceDatabase(const PlaceDatabase &) = delete;
  PlaceDatabase & operator=(const PlaceDatabase &) = delete;

  size_t size() const { return mh_place_db_size(db_); }
  const mh_place_config & config() const { return cfg_; }

  // the descriptor of a cloud in a frame F that R_G_F levels
  PlaceDescriptor describe(const PointCloud & cloud_F, const A9 & R_G_F = detail::identity33())
  {
    PlaceDescriptor d(kCells);
    ctx_->check(mh_place_describe(db_, cloud_F.empty() ? nullptr : &cloud_F[0].x, cloud_F.size(), sizeof(Point) / sizeof(float), R_G_F.data(), d.data()),
                "mh_place_describe");
    return d;
  }
  // which: 0 points_full_, 1 Be_cloud_
  PlaceDescriptor describeFromScan(mh_scan * scan, int which, const A9 & R_G_F = detail::identity33())
  {
    PlaceDescriptor d(kCells);
    ctx_->check(mh_place_describe_from_scan(db_, scan, which, R_G_F.data(), d.data()), "mh_place_describe_from_scan");
    return d;
  }
  int32_t add(const PlaceDescriptor & desc, int64_t tag)
  {
    if (desc.size() != kCells) throw std::runtime_error("PlaceDatabase::add: a descriptor has 1200 floats");
    int32_t index = -1;
    ctx_->check(mh_place_db_add(db_, desc.data(), tag, &index), "mh_place_db_add");
    return index;
  }
  int32_t addFromScan(mh_scan * scan, int which, int64_t tag, const A9 & R_G_F = detail::identity33())
  {
    int32_t index = -1;
    ctx_->check(mh_place_db_add_from_scan(db_, scan, which, R_G_F.data(), tag, &index), "mh_place_db_add_from_scan");
    return index;
  }
  PlaceDescriptor get(int32_t index, int64_t * tag = nullptr)
  {
    PlaceDescriptor d(kCells);
    ctx_->check(mh_place_db_get(db_, index, d.data(), tag), "mh_place_db_get");
    return d;
  }
  // the top_k hits in rank order (index -1 behind the last real one); n_search = 0 searches every entry; all (optional) receives
  // {D, shift} of every searched entry
  std::vector<mh_place_hit> query(const PlaceDescriptor & desc, int32_t top_k, size_t n_search = 0, std::vector<mh_place_score> * all = nullptr)
  {
    if (desc.size() != kCells) throw std::runtime_error("PlaceDatabase::query: a descriptor has 1200 floats");
    std::vector<mh_place_hit> hits(top_k > 0 ? static_cast<size_t>(top_k) : 0);
    if (all) all->resize(n_search ? n_search : size());
    ctx_->check(mh_place_db_query(db_, desc.data(), n_search, top_k, hits.data(), all ? all->data() : nullptr), "mh_place_db_query");
    return hits;
  }
  std::vector<mh_place_hit> queryFromScan(mh_scan * scan, int which, int32_t top_k, const A9 & R_G_F = detail::identity33(), size_t n_search = 0,
                                          std::vector<mh_place_score> * all = nullptr)
  {
    std::vector<mh_place_hit> hits(top_k > 0 ? static_cast<size_t>(top_k) : 0);
    if (all) all->resize(n_search ? n_search : size());
    ctx_->check(mh_place_db_query_from_scan(db_, scan, which, R_G_F.data(), n_search, top_k, hits.data(), all ? all->data() : nullptr),
                "mh_place_db_query_from_scan");
    return hits;
  }
  mh_place_db * underlying() { return db_; }

private:
  static constexpr size_t kCells = static_cast<size_t>(MH_PLACE_RINGS) * MH_PLACE_SECTORS;
  std::shared_ptr<Context> ctx_;  // (declared first: the database goes before its context)
  mh_place_config cfg_;
  mh_place_db * db_ = nullptr;
};

// The clouds of the keyframes on the device, each in its own frame, with a tag and no pose (mh_keyframes_*): what a map needs to
// be rebuilt at the poses a pose graph corrected.  Capacities are fixed at creation; an add that does not fit throws.
class KeyframeStore
{
public:
  KeyframeStore(const std::shared_ptr<Context> & ctx, int32_t capacity_keyframes, int64_t capacity_points) : ctx_(ctx)
  {
    mh_keyframes_config cfg{};
    cfg.capacity_keyframes = capacity_keyframes;
    cfg.capacity_points = capacity_points;
    ctx_->check(mh_keyframes_create(ctx_->get(), &cfg, &kf_), "mh_keyframes_create");
  }
  ~KeyframeStore() { mh_keyframes_destroy(kf_); }
  KeyframeStore(const KeyframeStore &) = delete;
  KeyframeStore & operator=(const KeyframeStore &) = delete;

  size_t size() const { return mh_keyframes_size(kf_); }
  mh_keyframes_info info() const
  {
    mh_keyframes_info i{};
    ctx_->check(mh_keyframes_get_info(kf_, &i), "mh_keyframes_get_info");
    return i;
  }
  int32_t add(const PointCloud & cloud, int64_t tag)
  {
    int32_t index = -1;
    ctx_->check(mh_keyframes_add(kf_, cloud.empty() ? nullptr : &cloud[0].x, cloud.size(), sizeof(Point) / sizeof(float), tag, &index), "mh_keyframes_add");
    return index;
  }
  // Be_cloud_ of a device-resident scan, device to device, nothing waits
  int32_t addBodyCloud(mh_scan * scan, int64_t tag)
  {
    int32_t index = -1;
    ctx_->check(mh_keyframes_add_from_scan(kf_, scan, 1, tag, &index), "mh_keyframes_add_from_scan");
    return index;
  }
  PointCloud get(int32_t index, int64_t * tag = nullptr)
  {
    size_t n = 0;
    ctx_->check(mh_keyframes_get(kf_, index, nullptr, 0, &n, tag), "mh_keyframes_get");
    std::vector<float> xyz(3 * n);
    ctx_->check(mh_keyframes_get(kf_, index, xyz.data(), n, &n, tag), "mh_keyframes_get");
    PointCloud out(n, Point{});
    for (size_t i = 0; i < n; ++i) {
      out[i].x = xyz[3 * i];
      out[i].y = xyz[3 * i + 1];
      out[i].z = xyz[3 * i + 2];
    }
    return out;
  }
  // mh_map_rebuild_from_keyframes: the map that map_cfg and one insert per listed keyframe at poses[j] give (poses rounded by
  // toFloat12, as updateMap's are), bit for bit.  order empty: every entry in stored order.
  IncrementalVoxelMapPCL::Ptr rebuild(const std::vector<Pose3> & poses, const mh_map_config & map_cfg, const std::vector<int32_t> & order = {},
                                      int64_t chunk_points = 0, mh_map_rebuild_result * result = nullptr)
  {
    const size_t K = order.empty() ? size() : order.size();
    if (poses.size() != K) throw std::runtime_error("KeyframeStore::rebuild: one pose per listed keyframe");
    std::vector<float> R(9 * K), t(3 * K);
    for (size_t j = 0; j < K; ++j) {
      float Rt[12];
      toFloat12(poses[j], Rt);
      std::copy(Rt, Rt + 9, R.begin() + 9 * j);
      std::copy(Rt + 9, Rt + 12, t.begin() + 3 * j);
    }
    mh_map_rebuild_config rc{};
    rc.chunk_points = chunk_points;
    mh_map_rebuild_result res{};
    IncrementalVoxelMapPCL::Ptr out(new IncrementalVoxelMapPCL(ctx_, map_cfg, nullptr));
    ctx_->check(mh_map_rebuild_from_keyframes(kf_, &map_cfg, order.empty() ? nullptr : order.data(), order.size(), R.data(), t.data(), &rc, &out->map_, &res),
                "mh_map_rebuild_from_keyframes");
    if (result) *result = res;
    return out;
  }
  mh_keyframes * underlying() { return kf_; }

private:
  std::shared_ptr<Context> ctx_;  // (declared first: the store goes before its context)
  mh_keyframes * kf_ = nullptr;
};

// A pose graph over all keyframes, optimised on the device (mh_pose_graph_*): where a loop closure found by PlaceDatabase and
// measured by mh_icp_relocalise goes when its ends are further apart than the fixed-lag window is long.  Poses are world from
// keyframe, row-major as the C ABI takes them (PoseRM: no conversion touches a bit); an edge is the window's mh_window_edge.
inline mh_window_edge poseGraphEdge(int32_t pose_a, int32_t pose_b, const PoseRM & Z_ab, const std::array<double, 36> & info)
{
  mh_window_edge e{};
  e.pose_a = pose_a;
  e.pose_b = pose_b;
  std::copy(Z_ab.R.begin(), Z_ab.R.end(), e.Z_R);
  std::copy(Z_ab.t.begin(), Z_ab.t.end(), e.Z_t);
  std::copy(info.begin(), info.end(), e.info);
  return e;
}

// a prior on keyframe `pose`: the measured pose Z (world from keyframe) and its information in (rotation, translation) order
inline mh_pose_prior posePrior(int32_t pose, const Pose3 & Z, const gtsam::Matrix6 & info)
{
  mh_pose_prior p{};
  const PoseRM z = rowMajor(Z);
  p.pose = pose;
  std::copy(z.R.begin(), z.R.end(), p.Z_R);
  std::copy(z.t.begin(), z.t.end(), p.Z_t);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) p.info[6 * r + c] = info(r, c);
  return p;
}
inline mh_pose_graph_loss poseGraphLoss(int32_t kind, double param)
{
  mh_pose_graph_loss l{};
  l.kind = kind;
  l.param = param;
  return l;
}

class PoseGraph
{
public:
  // max_far 0: a plain graph (at most MH_PGO_FAR_MAX far edges); 1 .. MH_PGO_FAR_LIMIT: a wide one
  PoseGraph(const std::shared_ptr<Context> & ctx, size_t max_poses, size_t max_edges, size_t max_far = 0) : ctx_(ctx)
  {
    if (max_far == 0)
      ctx_->check(mh_pose_graph_create(ctx_->get(), max_poses, max_edges, &pg_), "mh_pose_graph_create");
    else
      ctx_->check(mh_pose_graph_create_wide(ctx_->get(), max_poses, max_edges, max_far, &pg_), "mh_pose_graph_create_wide");
  }
  ~PoseGraph() { mh_pose_graph_destroy(pg_); }
  PoseGraph(const PoseGraph &) = delete;
  PoseGraph & operator=(const PoseGraph &) = delete;

  // another count than before drops the edges, the fixed flags, the priors and the losses
  void setPoses(const std::vector<PoseRM> & poses)
  {
    std::vector<double> R(9 * poses.size()), t(3 * poses.size());
    for (size_t i = 0; i < poses.size(); ++i) {
      std::copy(poses[i].R.begin(), poses[i].R.end(), R.begin() + static_cast<std::ptrdiff_t>(9 * i));
      std::copy(poses[i].t.begin(), poses[i].t.end(), t.begin() + static_cast<std::ptrdiff_t>(3 * i));
    }
    ctx_->check(mh_pose_graph_set_poses(pg_, R.data(), t.data(), poses.size()), "mh_pose_graph_set_poses");
    if (poses.size() != n_) n_edges_ = n_priors_ = 0;
    n_ = poses.size();
  }
  // one flag per pose; empty: no pose is fixed
  void setFixed(const std::vector<uint8_t> & fixed)
  {
    if (!fixed.empty() && fixed.size() != n_) throw std::runtime_error("PoseGraph::setFixed: one flag per pose");
    ctx_->check(mh_pose_graph_set_fixed(pg_, fixed.empty() ? nullptr : fixed.data()), "mh_pose_graph_set_fixed");
  }
  void setEdges(const std::vector<mh_window_edge> & edges)
  {
    ctx_->check(mh_pose_graph_set_edges(pg_, edges.empty() ? nullptr : edges.data(), edges.size()), "mh_pose_graph_set_edges");
    n_edges_ = edges.size();
  }
  // replaces the prior list (and drops the priors' losses)
  void setPriors(const std::vector<mh_pose_prior> & priors)
  {
    ctx_->check(mh_pose_graph_set_priors(pg_, priors.empty() ? nullptr : priors.data(), priors.size()), "mh_pose_graph_set_priors");
    n_priors_ = priors.size();
  }
  // one loss per edge and one per prior, each in list order; an empty vector: no loss on any of them
  void setLoss(const std::vector<mh_pose_graph_loss> & edges, const std::vector<mh_pose_graph_loss> & priors = {})
  {
    if (!edges.empty() && edges.size() != n_edges_) throw std::runtime_error("PoseGraph::setLoss: one loss per edge");
    if (!priors.empty() && priors.size() != n_priors_) throw std::runtime_error("PoseGraph::setLoss: one loss per prior");
    ctx_->check(mh_pose_graph_set_loss(pg_, edges.empty() ? nullptr : edges.data(), priors.empty() ? nullptr : priors.data()), "mh_pose_graph_set_loss");
  }
  // every prior at the stored poses: d (6 per prior) and chi2 = d^T Om d, each optional.  Nothing moves.
  void priorResiduals(std::vector<double> * d, std::vector<double> * chi2 = nullptr)
  {
    if (d) d->resize(6 * n_priors_);
    if (chi2) chi2->resize(n_priors_);
    ctx_->check(mh_pose_graph_prior_residuals(pg_, d && n_priors_ ? d->data() : nullptr, chi2 && n_priors_ ? chi2->data() : nullptr),
                "mh_pose_graph_prior_residuals");
  }
  // the sum of rho at the stored poses; the weight of every edge and of every prior (each optional).  Nothing moves.
  double weights(std::vector<double> * w_edges = nullptr, std::vector<double> * w_priors = nullptr)
  {
    double f = 0.0;
    if (w_edges) w_edges->resize(n_edges_);
    if (w_priors) w_priors->resize(n_priors_);
    ctx_->check(mh_pose_graph_weights(pg_, w_edges && n_edges_ ? w_edges->data() : nullptr, w_priors && n_priors_ ? w_priors->data() : nullptr, &f),
                "mh_pose_graph_weights");
    return f;
  }
  std::vector<PoseRM> poses()
  {
    std::vector<double> R(9 * n_), t(3 * n_);
    size_t n = 0;
    ctx_->check(mh_pose_graph_get_poses(pg_, R.data(), t.data(), n_, &n), "mh_pose_graph_get_poses");
    std::vector<PoseRM> out(n);
    for (size_t i = 0; i < n; ++i) {
      std::copy(R.begin() + static_cast<std::ptrdiff_t>(9 * i), R.begin() + static_cast<std::ptrdiff_t>(9 * i + 9), out[i].R.begin());
      std::copy(t.begin() + static_cast<std::ptrdiff_t>(3 * i), t.begin() + static_cast<std::ptrdiff_t>(3 * i + 3), out[i].t.begin());
    }
    return out;
  }
  // the cost at the stored poses; chi2 (optional): r^T Om r per edge — what rejects a false loop before it is accepted; r
  // (optional): the residuals, 6 per edge.  Nothing moves.
  double residuals(std::vector<double> * chi2 = nullptr, std::vector<double> * r = nullptr)
  {
    double f = 0.0;
    if (chi2) chi2->resize(n_edges_);
    if (r) r->resize(6 * n_edges_);
    ctx_->check(mh_pose_graph_residuals(pg_, r && n_edges_ ? r->data() : nullptr, chi2 && n_edges_ ? chi2->data() : nullptr, &f), "mh_pose_graph_residuals");
    return f;
  }
  // trace_poses (optional): cfg.iters x n x 12 doubles, the rows of executed iterations filled
  mh_pose_graph_result optimise(const mh_pose_graph_config & cfg, std::vector<double> * trace_poses = nullptr)
  {
    mh_pose_graph_result out{};
    if (trace_poses) trace_poses->assign(static_cast<size_t>(cfg.iters > 0 ? cfg.iters : 0) * n_ * 12, 0.0);
    ctx_->check(mh_pose_graph_optimise(pg_, &cfg, &out, trace_poses ? trace_poses->data() : nullptr), "mh_pose_graph_optimise");
    return out;
  }
  // Sigma = A^-1 at the stored poses (rule 10 of the header): cov takes 36 doubles per pose, block (i, i) row-major in
  // (rotation, translation) order.  flags == 4 in the result: a pivot was not positive and the library wrote nothing into cov (it
  // has been resized to 36 n; what it holds is not a result).  Nothing moves.
  mh_pose_graph_cov_info covariances(double damping, std::vector<double> * cov)
  {
    mh_pose_graph_cov_info info{};
    cov->resize(36 * n_);
    ctx_->check(mh_pose_graph_covariances(pg_, damping, cov->data(), nullptr, 0, nullptr, &info), "mh_pose_graph_covariances");
    return info;
  }
  // the 12 x 12 joint [[S_ii, S_ij], [S_ij^T, S_jj]] of up to MH_PGO_COV_PAIRS_MAX pairs i < j, 144 doubles each; cov optional
  mh_pose_graph_cov_info jointCovariances(double damping, const std::vector<std::pair<int32_t, int32_t>> & pairs, std::vector<double> * joint,
                                          std::vector<double> * cov = nullptr)
  {
    mh_pose_graph_cov_info info{};
    std::vector<int32_t> ij;
    for (const auto & p : pairs) {
      ij.push_back(p.first);
      ij.push_back(p.second);
    }
    joint->resize(144 * pairs.size());
    if (cov) cov->resize(36 * n_);
    if (pairs.empty()) return cov ? covariances(damping, cov) : info;
    ctx_->check(mh_pose_graph_covariances(pg_, damping, cov ? cov->data() : nullptr, ij.data(), pairs.size(), joint->data(), &info), "mh_pose_graph_covariances");
    return info;
  }
  // One candidate loop against the joint marginal of its two poses: the residual r of rule 1 at the stored poses, the plain
  // chi2 = r^T Om r, and d2 = r^T (J S J^T + Om^-1)^-1 r with J = [J_a | I] — chi^2 with 6 degrees of freedom for a true loop,
  // whatever the drift between the two poses.  valid == false: a pivot was not positive (d2 is not computed).
  struct Gate
  {
    std::array<double, 6> r{};
    double chi2 = 0.0, d2 = 0.0;
    bool valid = false;
  };
  // up to MH_PGO_COV_PAIRS_MAX candidates that are NOT in the graph.  Small host arithmetic on jointCovariances.
  std::vector<Gate> gate(const std::vector<mh_window_edge> & candidates, double damping = 0.0)
  {
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (const auto & e : candidates) pairs.emplace_back(e.pose_a, e.pose_b);
    std::vector<double> joint;
    const mh_pose_graph_cov_info info = jointCovariances(damping, pairs, &joint);
    const std::vector<PoseRM> T = poses();
    std::vector<Gate> out(candidates.size());
    for (size_t k = 0; k < candidates.size(); ++k) {
      const mh_window_edge & e = candidates[k];
      const PoseRM &A = T[static_cast<size_t>(e.pose_a)], &B = T[static_cast<size_t>(e.pose_b)];
      double abR[9], abt[3], J[6][12] = {}, M[6][6], x[6];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) abR[3 * r + c] = A.R[r] * B.R[c] + A.R[3 + r] * B.R[3 + c] + A.R[6 + r] * B.R[6 + c];
        abt[r] = A.R[r] * (B.t[0] - A.t[0]) + A.R[3 + r] * (B.t[1] - A.t[1]) + A.R[6 + r] * (B.t[2] - A.t[2]);
      }
      // r = [Log(Z.R^T R_ab), Z.R^T (t_ab - Z.t)]
      double Re[9];
      Gate & g = out[k];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Re[3 * r + c] = e.Z_R[r] * abR[c] + e.Z_R[3 + r] * abR[3 + c] + e.Z_R[6 + r] * abR[6 + c];
        g.r[static_cast<size_t>(3 + r)] = e.Z_R[r] * (abt[0] - e.Z_t[0]) + e.Z_R[3 + r] * (abt[1] - e.Z_t[1]) + e.Z_R[6 + r] * (abt[2] - e.Z_t[2]);
      }
      const double cs = std::min(1.0, std::max(-1.0, (Re[0] + Re[4] + Re[8] - 1.0) / 2.0)), th = std::acos(cs), s = th < 1e-9 ? 0.5 : th / (2.0 * std::sin(th));
      g.r[0] = (Re[7] - Re[5]) * s;
      g.r[1] = (Re[2] - Re[6]) * s;
      g.r[2] = (Re[3] - Re[1]) * s;
      // J_a = -Ad(T_ab^-1): R_i = R_ab^T, t_i = -R_ab^T t_ab; Ad = [[R_i, 0], [hat(t_i) R_i, R_i]];  J_b = I
      double Ri[9], ti[3];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Ri[3 * r + c] = abR[3 * c + r];
        ti[r] = -(abR[r] * abt[0] + abR[3 + r] * abt[1] + abR[6 + r] * abt[2]);
      }
      const double hat[9] = {0.0, -ti[2], ti[1], ti[2], 0.0, -ti[0], -ti[1], ti[0], 0.0};
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          J[r][c] = J[3 + r][3 + c] = -Ri[3 * r + c];
          J[3 + r][c] = -(hat[3 * r] * Ri[c] + hat[3 * r + 1] * Ri[3 + c] + hat[3 * r + 2] * Ri[6 + c]);
        }
      for (int r = 0; r < 6; ++r) J[r][6 + r] = 1.0;
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) g.chi2 += g.r[static_cast<size_t>(r)] * e.info[6 * r + c] * g.r[static_cast<size_t>(c)];
      if (info.flags != 0) continue;
      // M = J S J^T + Om^-1, then M x = r: both by Gauss-Jordan with partial pivoting on 6 x 6
      const double * S = &joint[144 * k];
      double JS[6][12] = {}, W[6][12];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 12; ++c)
          for (int m = 0; m < 12; ++m) JS[r][c] += J[r][m] * S[12 * m + c];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
          W[r][c] = e.info[6 * r + c];
          W[r][6 + c] = r == c ? 1.0 : 0.0;
        }
      if (!eliminate6(W, 12)) continue;
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
          M[r][c] = W[r][6 + c];
          for (int m = 0; m < 12; ++m) M[r][c] += JS[r][m] * J[c][m];
        }
      for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) W[r][c] = M[r][c];
        W[r][6] = g.r[static_cast<size_t>(r)];
      }
      if (!eliminate6(W, 7)) continue;
      for (int r = 0; r < 6; ++r) x[r] = W[r][6];
      for (int r = 0; r < 6; ++r) g.d2 += g.r[static_cast<size_t>(r)] * x[r];
      g.valid = true;
    }
    return out;
  }
  size_t size() const { return n_; }
  mh_pose_graph * underlying() { return pg_; }

private:
  // [A | B] (6 rows, `cols` columns) -> [I | A^-1 B] by Gauss-Jordan with partial pivoting; false: A is singular
  static bool eliminate6(double W[6][12], int cols)
  {
    for (int j = 0; j < 6; ++j) {
      int piv = j;
      for (int r = j + 1; r < 6; ++r)
        if (std::fabs(W[r][j]) > std::fabs(W[piv][j])) piv = r;
      if (!(std::fabs(W[piv][j]) > 0.0)) return false;
      for (int c = 0; c < cols; ++c) std::swap(W[j][c], W[piv][c]);
      const double d = W[j][j];
      for (int c = 0; c < cols; ++c) W[j][c] /= d;
      for (int r = 0; r < 6; ++r) {
        if (r == j) continue;
        const double f = W[r][j];
        for (int c = 0; c < cols; ++c) W[r][c] -= f * W[j][c];
      }
    }
    return true;
  }
  std::shared_ptr<Context> ctx_;  // (declared first: the graph goes before its context)
  mh_pose_graph * pg_ = nullptr;
  size_t n_ = 0, n_edges_ = 0, n_priors_ = 0;
};

// The GaussianFactor ICPFactor::linearize returns: gtsam::HessianFactor(keys()[0], H, -b, f) (geometric_factor.hpp:559-560),
// binary HessianFactor(k0, k1, H_ss, H_st, -b_s, H_tt, -b_t, f) (:459-462), from the C ABI's row-major result.
inline std::shared_ptr<HessianFactor> hessianFrom(const KeyVector & keys, bool binary, const mh_icp_result & r)
{
  gtsam::Vector g1(6);
  for (int i = 0; i < 6; ++i) g1(i) = -r.b_s[i];
  if (!binary) return std::make_shared<HessianFactor>(keys[0], matrix6(r.H_ss), g1, r.f);
  gtsam::Vector g2(6);
  for (int i = 0; i < 6; ++i) g2(i) = -r.b_t[i];
  return std::make_shared<HessianFactor>(keys[0], keys[1], matrix6(r.H_ss), matrix6(r.H_st), g1, matrix6(r.H_tt), g2, r.f);
}

class ICPFactor : public NonlinearFactor
{
public:
  using Ptr = std::shared_ptr<ICPFactor>;
  enum class RejectStatus {  // geometric_factor.hpp:35-46
    Unprocessed = 0,
    InsufficientCorresPoints,
    CorresMaxDist,
    EigenSolverFail,
    MinEigenValueLow,
    Line,
    CorresPlaneInvalid,
    MaxError,
    Valid
  };

  // unary: key_source is T_W_B, the cloud is registered to the map frame (:119-129)
  ICPFactor(const Key key_source, IncrementalVoxelMapPCL::Ptr ivox_target, const PointCloud & cloud_source,
            const RegistrationConfig & config)
  : NonlinearFactor(KeyVector{key_source}), is_binary_(false), ivox_target_(std::move(ivox_target)), n_(cloud_source.size())
  {
    create(cloud_source, config);
  }
  // binary (:131-142)
  ICPFactor(const Key key_source, const Key key_target, IncrementalVoxelMapPCL::Ptr ivox_target,
            const PointCloud & cloud_source, const RegistrationConfig & config)
  : NonlinearFactor(KeyVector{key_source, key_target}), is_binary_(true), ivox_target_(std::move(ivox_target)), n_(cloud_source.size())
  {
    create(cloud_source, config);
  }
  // unary, source cloud = the scan front end's sm_Be_cloud_ds_, taken from device memory
  ICPFactor(const Key key_source, IncrementalVoxelMapPCL::Ptr ivox_target, ScanFrontEnd & scan, const RegistrationConfig & config)
  : NonlinearFactor(KeyVector{key_source}), is_binary_(false), ivox_target_(std::move(ivox_target)), n_(scan.info().n_downsampled)
  {
    std::memset(&last_, 0, sizeof(last_));
    ctx().check(mh_icp_create_from_scan(ctx().get(), ivox_target_->underlying(), scan.underlying(), &config, 0, &icp_),
                "mh_icp_create_from_scan");
  }
  ~ICPFactor() override { mh_icp_destroy(icp_); }

  NonlinearFactor::shared_ptr clone() const override  // :160-164 deep-copies the per-point state
  {
    std::shared_ptr<ICPFactor> c(new ICPFactor(*this, CloneTag{}));
    return c;
  }
  // Whether linearize() also runs the component-localizability / status-histogram pass (getLocalizabilities' *_comp
  // outputs, lastResult().status_hist).  Geometric::getFactors reads them right after its own linearize and switches the
  // pass off before the factor goes to the smoother, whose re-linearizations never have them read.
  void computeComponents(bool on) { ctx().check(mh_icp_set_components(icp_, on ? 1 : 0), "mh_icp_set_components"); }
  size_t dim() const override { return 6; }                  // :166
  double error(const Values &) const override { return 0.0; }  // :168-174 (the reference prints and returns 0)

  std::shared_ptr<GaussianFactor> linearize(const Values & c) const override  // :231-562
  {
    // :247-257 — T_W_S = c.at<Pose3>(keys()[0]), T_W_T for the binary factor, global_z from c.at<Unit3>(G(0)) (read unconditionally)
    const PoseRM Ts = rowMajor(c.at<Pose3>(keys()[0]));
    PoseRM Tt{};
    if (is_binary_) Tt = rowMajor(c.at<Pose3>(keys()[1]));
    const A3 g = toArray(c.at<Unit3>(G(0)).unitVector());
    mh_icp_result r;
    ctx().check(mh_icp_linearize(icp_, Ts.R.data(), Ts.t.data(), is_binary_ ? Tt.R.data() : nullptr, is_binary_ ? Tt.t.data() : nullptr, g.data(), &r),
                "mh_icp_linearize");
    last_ = r;
    return toHessian(r);
  }

  // Every live factor of the smoother window re-linearized in ONE device pass (what ISAM2's update + additional
  // iterations, src/graph/manager.cpp:585-588, do one factor at a time): same results as factors[i]->linearize(c), bit
  // for bit.  All factors unary or all binary, one context.
  static std::vector<std::shared_ptr<GaussianFactor>> linearizeBatch(const std::vector<Ptr> & factors, const Values & c)
  {
    std::vector<std::shared_ptr<GaussianFactor>> out;
    if (factors.empty()) return out;
    const size_t n = factors.size();
    const bool binary = factors[0]->is_binary_;
    std::vector<mh_icp *> h(n);
    std::vector<double> Rs(9 * n), ts(3 * n), Rt(binary ? 9 * n : 0), tt(binary ? 3 * n : 0), g(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const ICPFactor & f = *factors[i];
      if (f.is_binary_ != binary) throw std::runtime_error("ICPFactor::linearizeBatch: unary and binary factors mixed");
      h[i] = f.icp_;
      const PoseRM Ts = rowMajor(c.at<Pose3>(f.keys()[0]));
      std::memcpy(&Rs[9 * i], Ts.R.data(), 72);
      std::memcpy(&ts[3 * i], Ts.t.data(), 24);
      if (binary) {
        const PoseRM Tt = rowMajor(c.at<Pose3>(f.keys()[1]));
        std::memcpy(&Rt[9 * i], Tt.R.data(), 72);
        std::memcpy(&tt[3 * i], Tt.t.data(), 24);
      }
      const A3 gu = toArray(c.at<Unit3>(G(0)).unitVector());
      std::memcpy(&g[3 * i], gu.data(), 24);
    }
    std::vector<mh_icp_result> r(n);
    factors[0]->ctx().check(mh_icp_linearize_batch(h.data(), n, Rs.data(), ts.data(), binary ? Rt.data() : nullptr,
                                                   binary ? tt.data() : nullptr, g.data(), r.data()),
                            "mh_icp_linearize_batch");
    for (size_t i = 0; i < n; ++i) {
      factors[i]->last_ = r[i];
      out.push_back(factors[i]->toHessian(r[i]));
    }
    return out;
  }

  // Scan-to-map alignment from a rough pose (no counterpart in the reference, which leaves the loop to GTSAM): the whole
  // Gauss-Newton loop — linearize, 6 x 6 solve, retract — as one chain of launches on the device, one wait (mh_icp_align).
  struct AlignConfig
  {
    int max_iters = 10;
    double eps_rot = 1e-6, eps_trans = 1e-6, damping = 0.0, prior_sigma_rot = 0.0, prior_sigma_trans = 0.0;
    int check_every = 0;
  };
  struct AlignResult
  {
    Pose3 pose;
    int iters = 0;
    bool converged = false;
    std::vector<mh_icp_align_trace> trace;  // one row per executed iteration
  };
  AlignResult align(const Pose3 & T0, const Unit3 & g, const AlignConfig & config)
  {
    const PoseRM T = rowMajor(T0);
    const A3 gu = toArray(g.unitVector());
    mh_icp_align_config c;
    c.max_iters = config.max_iters;
    c.eps_rot = config.eps_rot;
    c.eps_trans = config.eps_trans;
    c.damping = config.damping;
    c.prior_sigma_rot = config.prior_sigma_rot;
    c.prior_sigma_trans = config.prior_sigma_trans;
    c.check_every = config.check_every;
    std::unique_ptr<mh_icp_align_result> r(new mh_icp_align_result);
    ctx().check(mh_icp_align(icp_, T.R.data(), T.t.data(), gu.data(), &c, r.get()), "mh_icp_align");
    last_ = r->last;
    AlignResult out;
    out.pose = pose3(r->R, r->t);
    out.iters = r->iters;
    out.converged = r->converged != 0;
    out.trace.assign(r->trace, r->trace + r->iters);
    return out;
  }

  // Several alignments side by side (mh_icp_align_batch): factors[i] from T0[i], all in one chain of launches — per iteration the
  // batch's K3 launches and one step launch — with one wait.  Every member is aligned exactly as align() aligns it and stops on
  // its own; one config serves all.  1 .. MH_ALIGN_BATCH_MAX unary factors of one context, each at most once.
  static std::vector<AlignResult> alignBatch(const std::vector<ICPFactor *> & factors, const std::vector<Pose3> & T0, const Unit3 & g,
                                             const AlignConfig & config)
  {
    AlignBatchCall call = alignBatchBegin(factors, T0, g, config, false);
    return call.take();
  }
  // The same without waiting: wait() collects it (mh_icp_align_batch_wait).  No other call on a member until then; the call
  // object must outlive the wait, and the factors the call object.
  class AlignBatchCall
  {
  public:
    std::vector<AlignResult> wait()
    {
      if (pending_) {
        pending_ = false;
        factors_[0]->ctx().check(mh_icp_align_batch_wait(factors_[0]->ctx().get()), "mh_icp_align_batch_wait");
      }
      return take();
    }

  private:
    friend class ICPFactor;
    std::vector<AlignResult> take()
    {
      std::vector<AlignResult> out(factors_.size());
      for (size_t i = 0; i < factors_.size(); ++i) {
        const mh_icp_align_result & r = results_[i];
        factors_[i]->last_ = r.last;
        out[i].pose = pose3(r.R, r.t);
        out[i].iters = r.iters;
        out[i].converged = r.converged != 0;
        out[i].trace.assign(r.trace, r.trace + r.iters);
      }
      return out;
    }
    std::vector<ICPFactor *> factors_;
    bool pending_ = false;
    std::unique_ptr<mh_icp_align_result[]> results_;  // on the heap: the library writes into them when the call is collected
  };
  static AlignBatchCall alignBatchAsync(const std::vector<ICPFactor *> & factors, const std::vector<Pose3> & T0, const Unit3 & g,
                                        const AlignConfig & config)
  {
    return alignBatchBegin(factors, T0, g, config, true);
  }

  // Relocalisation (no counterpart in the reference): candidate poses of this factor's cloud scored against its map in one chain
  // of launches and ranked on the device (mh_icp_score_poses), and the few best refined with align() (mh_icp_relocalise).  For
  // the caller who has no pose inside the association gate yet.
  struct ScoreConfig
  {
    double gate = 1.0;  // m
    int stride = 1;     // every stride-th point, counted in the order the cloud was given
    int top_k = 0;      // winners selected on the device (0 .. MH_RELOC_MAX_REFINE)
  };
  struct ScoreResult
  {
    std::vector<mh_pose_score> scores;  // one per pose; empty when they were not asked for
    std::vector<int> best;              // top_k pose indices in rank order (fewer when there are fewer poses)
  };
  ScoreResult scorePoses(const std::vector<Pose3> & poses, const ScoreConfig & config, bool want_scores = true)
  {
    ScoreCall call = scorePosesBegin(poses, config, want_scores, false);
    return call.take();
  }
  // The same without waiting: wait() collects it (mh_icp_wait).  No other call on the factor until then; the call object must
  // outlive the wait.
  class ScoreCall
  {
  public:
    ScoreResult wait()
    {
      if (pending_) {
        pending_ = false;
        owner_->ctx().check(mh_icp_wait(owner_->icp_), "mh_icp_wait");
      }
      return take();
    }

  private:
    friend class ICPFactor;
    ScoreResult take()
    {
      ScoreResult r;
      r.scores = *scores_;
      for (int i = 0; i < top_k_ && (*best_)[static_cast<size_t>(i)] >= 0; ++i) r.best.push_back((*best_)[static_cast<size_t>(i)]);
      return r;
    }
    ICPFactor * owner_ = nullptr;
    bool pending_ = false;
    int top_k_ = 0;
    // on the heap: the library writes into them when the call is collected, wherever the call object has moved to
    std::unique_ptr<std::vector<mh_pose_score>> scores_;
    std::unique_ptr<std::array<int32_t, MH_RELOC_MAX_REFINE>> best_;
  };
  ScoreCall scorePosesAsync(const std::vector<Pose3> & poses, const ScoreConfig & config, bool want_scores = true)
  {
    return scorePosesBegin(poses, config, want_scores, true);
  }

  struct RelocConfig
  {
    ScoreConfig score{1.0, 4, 4};
    AlignConfig align;
    double final_gate = 0.1;  // m: the gate of the re-score of the aligned poses (every point)
  };
  struct RelocCandidate
  {
    int index = -1, iters = 0;
    bool converged = false;
    mh_pose_score coarse{}, fine{};
    Pose3 pose;  // aligned
  };
  struct RelocResult
  {
    Pose3 pose;    // the winner's aligned pose
    int best = -1; // into candidates
    std::vector<RelocCandidate> candidates;  // in the rank order of the coarse pass
  };
  // The factor is left reset (its association state is a freshly constructed factor's); getLinearizeCount() has advanced by the
  // iterations the alignments ran.
  RelocResult relocalise(const std::vector<Pose3> & poses, const Unit3 & g, const RelocConfig & config)
  {
    std::vector<double> R, t;
    flattenPoses(poses, R, t);
    const A3 gu = toArray(g.unitVector());
    mh_icp_reloc_config c;
    c.score = scoreConfig(config.score);
    c.align = alignConfig(config.align);
    c.final_gate = config.final_gate;
    std::unique_ptr<mh_icp_reloc_result> r(new mh_icp_reloc_result);
    ctx().check(mh_icp_relocalise(icp_, R.data(), t.data(), poses.size(), gu.data(), &c, r.get()), "mh_icp_relocalise");
    RelocResult out;
    out.pose = pose3(r->R, r->t);
    out.best = r->best;
    for (int i = 0; i < r->n_candidates; ++i) {
      const mh_icp_reloc_candidate & q = r->cand[i];
      RelocCandidate k;
      k.index = q.index;
      k.iters = q.iters;
      k.converged = q.converged != 0;
      k.coarse = q.coarse;
      k.fine = q.fine;
      k.pose = pose3(q.R, q.t);
      last_.linearize_count += q.iters;  // what getLinearizeCount() reports: the library's count moved with the alignments
      out.candidates.push_back(k);
    }
    return out;
  }
  // relocalise() with the candidates aligned side by side (mh_icp_relocalise_batch) on clones of this factor, which it makes on
  // first use and keeps.  The one difference: this factor is only read — it is NOT reset, and neither its association state nor
  // getLinearizeCount() move.
  RelocResult relocaliseBatch(const std::vector<Pose3> & poses, const Unit3 & g, const RelocConfig & config)
  {
    std::vector<double> R, t;
    flattenPoses(poses, R, t);
    const A3 gu = toArray(g.unitVector());
    mh_icp_reloc_config c;
    c.score = scoreConfig(config.score);
    c.align = alignConfig(config.align);
    c.final_gate = config.final_gate;
    const size_t need = std::min(static_cast<size_t>(std::max(config.score.top_k, 0)), poses.size());
    while (reloc_work_.size() < need) reloc_work_.push_back(Ptr(new ICPFactor(*this, CloneTag{})));
    std::vector<mh_icp *> work;
    for (const Ptr & w : reloc_work_) work.push_back(w->icp_);
    std::unique_ptr<mh_icp_reloc_result> r(new mh_icp_reloc_result);
    ctx().check(mh_icp_relocalise_batch(icp_, work.data(), work.size(), R.data(), t.data(), poses.size(), gu.data(), &c, r.get()),
                "mh_icp_relocalise_batch");
    RelocResult out;
    out.pose = pose3(r->R, r->t);
    out.best = r->best;
    for (int i = 0; i < r->n_candidates; ++i) {
      const mh_icp_reloc_candidate & q = r->cand[i];
      RelocCandidate k;
      k.index = q.index;
      k.iters = q.iters;
      k.converged = q.converged != 0;
      k.coarse = q.coarse;
      k.fine = q.fine;
      k.pose = pose3(q.R, q.t);
      reloc_work_[static_cast<size_t>(i)]->last_.linearize_count += q.iters;
      out.candidates.push_back(k);
    }
    return out;
  }
  // Candidate poses around T0: translations T0.t + (ix step_xy, iy step_xy, 0), ix, iy in -nx .. nx with nx = floor(half_xy /
  // step_xy + 1e-9), and rotations Rz(iw step_yaw) T0.R (a yaw about the WORLD z axis, radians), iw in -nw .. nw with nw =
  // floor(half_yaw / step_yaw + 1e-9); a step <= 0 gives that axis its centre node alone.  Order (the pose index is part of the
  // ranking): yaw slowest, then x, then y fastest, each ascending from its negative end — the enumeration of capi.pose_grid.
  static std::vector<Pose3> poseGrid(const Pose3 & T0, double half_xy, double step_xy, double half_yaw, double step_yaw)
  {
    const PoseRM T = rowMajor(T0);
    const int nx = step_xy > 0.0 ? static_cast<int>(std::floor(half_xy / step_xy + 1e-9)) : 0;
    const int nw = step_yaw > 0.0 ? static_cast<int>(std::floor(half_yaw / step_yaw + 1e-9)) : 0;
    std::vector<Pose3> out;
    out.reserve(static_cast<size_t>(2 * nw + 1) * static_cast<size_t>(2 * nx + 1) * static_cast<size_t>(2 * nx + 1));
    for (int iw = -nw; iw <= nw; ++iw) {
      const double a = iw * step_yaw, c = std::cos(a), s = std::sin(a);
      const double Rz[9] = {c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0};
      double Rw[9];
      for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) Rw[3 * r + k] = (Rz[3 * r] * T.R[k] + Rz[3 * r + 1] * T.R[3 + k]) + Rz[3 * r + 2] * T.R[6 + k];
      for (int ix = -nx; ix <= nx; ++ix)
        for (int iy = -nx; iy <= nx; ++iy) {
          const double tt[3] = {T.t[0] + ix * step_xy, T.t[1] + iy * step_xy, T.t[2]};
          out.push_back(pose3(Rw, tt));
        }
    }
    return out;
  }

  // The smoother's loop over a window of unary factors (no counterpart in the reference, which leaves it to ISAM2): linearize
  // every factor, assemble the block-tridiagonal system of the factors, the between factors and the prior on the oldest pose,
  // solve, retract every pose — as one chain of launches on the device, one wait (mh_icp_window_optimise).
  struct WindowConfig
  {
    int iters = 6;
    double between_info[6] = {0, 0, 0, 0, 0, 0}, prior_info[6] = {0, 0, 0, 0, 0, 0};
    double damping = 1e-9, eps_rot = 0.0, eps_trans = 0.0;
    int check_every = 0;
  };
  struct WindowBetween
  {
    bool present = false;
    Pose3 Z;  // the measured T_{i-1}^-1 T_i
  };
  struct WindowResult
  {
    std::vector<Pose3> poses;
    int iters = 0;
    bool converged = false;
    std::vector<mh_icp_window_trace> trace;  // one row per executed iteration
    std::vector<uint32_t> evaluated;         // optimiseWindowRelin: per executed iteration, bit i: factor i ran K3
  };
  // ISAM2's per-variable relinearization thresholds (graph/manager.cpp:51-73): a factor is evaluated again only once its pose
  // has moved past them from the pose of its last evaluation (mh_icp_window_optimise_relin)
  struct WindowRelin
  {
    double rot = 1.75e-2, trans = 5.0e-3;  // rad, m: config/enwide/params.yaml:32-33
  };
  // A Hessian factor the host linearized once, on one pose of the window (mh_icp_window_optimise_lin): the model
  // f + 2 b^T x + x^T H x in the tangent of `at`, the convention of mh_icp_result.H_ss / b_s / f — what
  // HessianFactor(key, H, -b, f) receives.  The chain carries it to the current pose of its variable in every iteration.
  struct WindowLinear
  {
    size_t pose = 0;  // index into the window
    Pose3 at;         // where H, b, f were evaluated
    M66 H;
    V6D b;
    double f = 0.0;
  };
  // from the unary HessianFactor a linearize() returned (which carries -b) and the pose it was linearized at
  static WindowLinear windowLinearFrom(const HessianFactor & h, size_t pose, const Pose3 & at)
  {
    WindowLinear l;
    l.pose = pose;
    l.at = at;
    const gtsam::Matrix G = h.information();
    const gtsam::Vector g = h.linearTerm();
    if (G.rows() != 6 || G.cols() != 6 || g.size() != 6) throw std::runtime_error("ICPFactor::windowLinearFrom: a factor over one pose only");
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) l.H(r, c) = G(r, c);
      l.b(r) = -g(r);
    }
    l.f = h.constantTerm();
    return l;
  }
  // A between factor on any pair of poses a < b of the window, with its own measurement and a dense information matrix in
  // (rotation, translation) order (mh_icp_window_optimise_edges): what BetweenFactor<Pose3>(X(a), X(b), Z, model) is to ISAM2.
  struct WindowEdge
  {
    size_t a = 0, b = 0;  // indices into the window
    Pose3 Z;              // the measured T_a^-1 T_b
    M66 info;
  };
  // from diagonal sigmas (rotation rad x 3, translation m x 3), the order of noiseModel::Diagonal::Sigmas on a Pose3
  static WindowEdge windowEdgeFromSigmas(size_t a, size_t b, const Pose3 & Z, const V6D & sigmas)
  {
    WindowEdge e;
    e.a = a;
    e.b = b;
    e.Z = Z;
    e.info = M66::Zero();
    for (int r = 0; r < 6; ++r) e.info(r, r) = 1.0 / (sigmas(r) * sigmas(r));
    return e;
  }
  // What eliminating the oldest pose of the window leaves on the pose behind it (mh_icp_window_marginalise): `prior` is a linear
  // factor on pose 0 of the window WITHOUT its oldest pose, linearized at that pose as given — what optimiseWindowLin /
  // optimiseWindowEdges take.  valid == false: the oldest pose's block had no positive pivot; prior.H, b, f are zero.
  struct WindowMarginal
  {
    bool valid = false;
    int n_ties = 0;  // the between entry of pose 1 plus the edges on (0, 1)
    WindowLinear prior;
  };
  // ONE dense factor on up to four poses of the window (mh_window_joint_factor): the model f + 2 b^T x + x^T H x, x the stacked
  // tangents of the member poses at their `at`; what eliminating the oldest pose leaves once an odometry edge reaches from it
  // past pose 1.  H: 6 n x 6 n row-major, b: 6 n, n = poses.size().
  struct WindowJoint
  {
    std::vector<size_t> poses;  // strictly ascending indices into the window
    std::vector<Pose3> at;      // the linearization pose of each member
    std::vector<double> H, b;
    double f = 0.0;
  };
  // mh_icp_window_marginalise_joint: `here` carries the separator's indices in the window the call was made on, `prior` the same
  // factor rebased to the window WITHOUT its oldest pose (every index minus one) — what optimiseWindowJoint takes there.
  struct WindowJointMarginal
  {
    bool valid = false;
    int n_ties = 0;  // the between entry of pose 1 plus every edge from pose 0
    WindowJoint here, prior;
  };
  // a call in flight (optimiseWindowAsync, marginaliseWindowAsync, ...): wait() / waitMarginal() / waitJointMarginal() collects it
  class WindowCall
  {
  public:
    WindowJointMarginal waitJointMarginal()
    {
      factors_[0]->ctx().check(mh_icp_window_wait(factors_[0]->ctx().get()), "mh_icp_window_wait");
      return finishJointMarginal();
    }
    WindowResult wait()
    {
      factors_[0]->ctx().check(mh_icp_window_wait(factors_[0]->ctx().get()), "mh_icp_window_wait");
      return finish();
    }
    WindowMarginal waitMarginal()
    {
      factors_[0]->ctx().check(mh_icp_window_wait(factors_[0]->ctx().get()), "mh_icp_window_wait");
      return finishMarginal();
    }

  private:
    friend class ICPFactor;
    WindowMarginal finishMarginal()
    {
      WindowMarginal out;
      out.valid = m_->valid != 0;
      out.n_ties = m_->n_ties;
      out.prior.pose = static_cast<size_t>(m_->prior.pose - 1);
      out.prior.at = pose3(m_->prior.L_R, m_->prior.L_t);
      out.prior.H = matrix6(m_->prior.H);
      for (int r = 0; r < 6; ++r) out.prior.b(r) = m_->prior.b[r];
      out.prior.f = m_->prior.f;
      factors_[0]->last_ = m_->oldest;
      return out;
    }
    std::unique_ptr<mh_window_marginal> m_;  // set: the call is mh_icp_window_marginalise
    WindowJointMarginal finishJointMarginal()
    {
      WindowJointMarginal out;
      out.valid = jm_->valid != 0;
      out.n_ties = jm_->n_ties;
      const mh_window_joint_factor & q = jm_->prior;
      const size_t n = static_cast<size_t>(q.n_poses);
      for (size_t m = 0; m < n; ++m) {
        out.here.poses.push_back(static_cast<size_t>(q.pose[m]));
        out.here.at.push_back(pose3(q.L_R + 9 * m, q.L_t + 3 * m));
      }
      out.here.H.resize(36 * n * n);
      out.here.b.assign(q.b, q.b + 6 * n);
      for (size_t r = 0; r < 6 * n; ++r)
        for (size_t c = 0; c < 6 * n; ++c) out.here.H[6 * n * r + c] = q.H[24 * r + c];
      out.here.f = q.f;
      out.prior = out.here;
      for (size_t & i : out.prior.poses) i -= 1;
      factors_[0]->last_ = jm_->oldest;
      return out;
    }
    std::unique_ptr<mh_window_joint_marginal> jm_;  // set: the call is mh_icp_window_marginalise_joint
    std::unique_ptr<mh_window_joint_factor> joint_;
    WindowResult finish()
    {
      WindowResult out;
      out.iters = r_->iters;
      out.converged = r_->converged != 0;
      out.trace.assign(r_->trace, r_->trace + r_->iters);
      if (relin_on_) out.evaluated.assign(masks_.begin(), masks_.begin() + r_->iters);
      for (size_t i = 0; i < factors_.size(); ++i) {
        out.poses.push_back(pose3(r_->R + 9 * i, r_->t + 3 * i));
        factors_[i]->last_ = r_->last[i];
      }
      return out;
    }
    std::vector<Ptr> factors_;
    std::vector<mh_icp *> h_;
    std::vector<double> R_, t_, ZR_, Zt_;
    std::vector<int32_t> has_Z_;
    A3 g_{};
    mh_icp_window_config c_{};
    std::unique_ptr<mh_icp_window_result> r_;
    bool relin_on_ = false;
    mh_icp_window_relin relin_{};
    std::vector<uint32_t> masks_;
    std::vector<mh_window_linear_factor> lin_;
    std::vector<mh_window_edge> edges_;
  };
  static WindowResult optimiseWindow(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses, const std::vector<WindowBetween> & between,
                                     const Unit3 & g, const WindowConfig & config)
  {
    return startWindow(factors, poses, between, g, config, true)->finish();
  }
  static std::unique_ptr<WindowCall> optimiseWindowAsync(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                         const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config)
  {
    return startWindow(factors, poses, between, g, config, false);
  }
  static WindowResult optimiseWindowRelin(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses, const std::vector<WindowBetween> & between,
                                          const Unit3 & g, const WindowConfig & config, const WindowRelin & relin)
  {
    return startWindow(factors, poses, between, g, config, true, &relin)->finish();
  }
  static std::unique_ptr<WindowCall> optimiseWindowRelinAsync(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                              const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config,
                                                              const WindowRelin & relin)
  {
    return startWindow(factors, poses, between, g, config, false, &relin);
  }
  // either of the above (relin == nullptr: every factor is evaluated in every iteration) with linear factors on the poses
  static WindowResult optimiseWindowLin(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses, const std::vector<WindowBetween> & between,
                                        const Unit3 & g, const WindowConfig & config, const std::vector<WindowLinear> & linear, const WindowRelin * relin = nullptr)
  {
    return startWindow(factors, poses, between, g, config, true, relin, &linear)->finish();
  }
  static std::unique_ptr<WindowCall> optimiseWindowLinAsync(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                            const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config,
                                                            const std::vector<WindowLinear> & linear, const WindowRelin * relin = nullptr)
  {
    return startWindow(factors, poses, between, g, config, false, relin, &linear);
  }

  // ... and with edges on any pair of poses; an empty `edges` takes the same entry point with no edge
  static WindowResult optimiseWindowEdges(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses, const std::vector<WindowBetween> & between,
                                          const Unit3 & g, const WindowConfig & config, const std::vector<WindowLinear> & linear,
                                          const std::vector<WindowEdge> & edges, const WindowRelin * relin = nullptr)
  {
    return startWindow(factors, poses, between, g, config, true, relin, &linear, &edges)->finish();
  }
  static std::unique_ptr<WindowCall> optimiseWindowEdgesAsync(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                              const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config,
                                                              const std::vector<WindowLinear> & linear, const std::vector<WindowEdge> & edges,
                                                              const WindowRelin * relin = nullptr)
  {
    return startWindow(factors, poses, between, g, config, false, relin, &linear, &edges);
  }

  // The marginal prior of the oldest pose at `poses` (nothing is iterated): of `config` between_info, prior_info and damping are
  // used; linear factors and edges as optimiseWindowEdges takes them.  Only factors[0] is linearized (once).
  static WindowMarginal marginaliseWindow(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses, const std::vector<WindowBetween> & between,
                                          const Unit3 & g, const WindowConfig & config, const std::vector<WindowLinear> & linear,
                                          const std::vector<WindowEdge> & edges)
  {
    return startWindow(factors, poses, between, g, config, true, nullptr, &linear, &edges, true)->finishMarginal();
  }
  static std::unique_ptr<WindowCall> marginaliseWindowAsync(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                            const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config,
                                                            const std::vector<WindowLinear> & linear, const std::vector<WindowEdge> & edges)
  {
    return startWindow(factors, poses, between, g, config, false, nullptr, &linear, &edges, true);
  }

  // optimiseWindowEdges with one joint factor (mh_icp_window_optimise_joint); joint == nullptr: optimiseWindowEdges itself
  static WindowResult optimiseWindowJoint(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses, const std::vector<WindowBetween> & between,
                                          const Unit3 & g, const WindowConfig & config, const std::vector<WindowLinear> & linear,
                                          const std::vector<WindowEdge> & edges, const WindowJoint * joint, const WindowRelin * relin = nullptr)
  {
    return startWindow(factors, poses, between, g, config, true, relin, &linear, &edges, false, joint, true)->finish();
  }
  static std::unique_ptr<WindowCall> optimiseWindowJointAsync(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                              const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config,
                                                              const std::vector<WindowLinear> & linear, const std::vector<WindowEdge> & edges,
                                                              const WindowJoint * joint, const WindowRelin * relin = nullptr)
  {
    return startWindow(factors, poses, between, g, config, false, relin, &linear, &edges, false, joint, true);
  }
  // marginaliseWindow for an oldest pose tied beyond pose 1, by edges (0, b) or by the carried joint factor (which must contain
  // pose 0; nullptr: none): the marginal on the separator, up to four poses (mh_icp_window_marginalise_joint)
  static WindowJointMarginal marginaliseWindowJoint(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                    const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config,
                                                    const std::vector<WindowLinear> & linear, const std::vector<WindowEdge> & edges, const WindowJoint * joint)
  {
    return startWindow(factors, poses, between, g, config, true, nullptr, &linear, &edges, true, joint, true)->finishJointMarginal();
  }
  static std::unique_ptr<WindowCall> marginaliseWindowJointAsync(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses,
                                                                 const std::vector<WindowBetween> & between, const Unit3 & g, const WindowConfig & config,
                                                                 const std::vector<WindowLinear> & linear, const std::vector<WindowEdge> & edges,
                                                                 const WindowJoint * joint)
  {
    return startWindow(factors, poses, between, g, config, false, nullptr, &linear, &edges, true, joint, true);
  }

  // getters, :48-72
  std::vector<RejectStatus> getStatuses() const
  {
    std::vector<int32_t> s(n_);
    if (n_) ctx().check(mh_icp_get_state(icp_, s.data(), nullptr, nullptr), "mh_icp_get_state");
    std::vector<RejectStatus> out(n_);
    for (size_t i = 0; i < n_; ++i) out[i] = static_cast<RejectStatus>(s[i]);
    return out;
  }
  std::vector<V3D> getCorresMeansTarget() const
  {
    std::vector<double> v(3 * n_);
    if (n_) ctx().check(mh_icp_get_state(icp_, nullptr, v.data(), nullptr), "mh_icp_get_state");
    std::vector<V3D> m(n_);
    for (size_t i = 0; i < n_; ++i) m[i] = vector3(&v[3 * i]);
    return m;
  }
  std::vector<V3D> getCorresNormalsTarget() const
  {
    std::vector<double> v(3 * n_);
    if (n_) ctx().check(mh_icp_get_state(icp_, nullptr, nullptr, v.data()), "mh_icp_get_state");
    std::vector<V3D> m(n_);
    for (size_t i = 0; i < n_; ++i) m[i] = vector3(&v[3 * i]);
    return m;
  }
  void getLocalizabilities(V3D & trans_comp, V3D & rot_comp, V3D & trans_final, V3D & rot_final, M33 & eigenvectors_trans,
                           M33 & eigenvectors_rot)
  {
    trans_comp = vector3(last_.loc_trans_comp);
    rot_comp = vector3(last_.loc_rot_comp);
    trans_final = vector3(last_.loc_trans_final);
    rot_final = vector3(last_.loc_rot_final);
    eigenvectors_trans = matrix3(last_.eigvec_trans);
    eigenvectors_rot = matrix3(last_.eigvec_rot);
  }
  void getDegenInfo(V3D & rot, M33 & eigenvectors_rot, V3D & trans, M33 & eigenvectors_trans)
  {
    rot = vector3(last_.degen_rot);
    eigenvectors_rot = matrix3(last_.degen_eigvec_rot);
    trans = vector3(last_.degen_trans);
    eigenvectors_trans = matrix3(last_.degen_eigvec_trans);
  }
  int getLinearizeCount() const { return last_.linearize_count; }
  const mh_icp_result & lastResult() const { return last_; }  // incl. the status histogram of geometric.cpp:280-323

private:
  std::shared_ptr<HessianFactor> toHessian(const mh_icp_result & r) const
  {
    return hessianFrom(keys(), is_binary_, r);
  }
  struct CloneTag
  {
  };
  ICPFactor(const ICPFactor & o, CloneTag)
  : NonlinearFactor(KeyVector(o.keys())), is_binary_(o.is_binary_), ivox_target_(o.ivox_target_), n_(o.n_), last_(o.last_)
  {
    ctx().check(mh_icp_clone(o.icp_, &icp_), "mh_icp_clone");
  }
  void create(const PointCloud & cloud, const RegistrationConfig & config)
  {
    std::memset(&last_, 0, sizeof(last_));
    ctx().check(mh_icp_create(ctx().get(), ivox_target_->underlying(), cloud.data(), cloud.size(), &config, is_binary_ ? 1 : 0,
                              &icp_),
                "mh_icp_create");
  }
  const Context & ctx() const { return *ivox_target_->context(); }
  static void flattenPoses(const std::vector<Pose3> & poses, std::vector<double> & R, std::vector<double> & t)
  {
    R.resize(9 * poses.size());
    t.resize(3 * poses.size());
    for (size_t i = 0; i < poses.size(); ++i) {
      const PoseRM T = rowMajor(poses[i]);
      std::memcpy(&R[9 * i], T.R.data(), 72);
      std::memcpy(&t[3 * i], T.t.data(), 24);
    }
  }
  static mh_icp_score_config scoreConfig(const ScoreConfig & config)
  {
    mh_icp_score_config c;
    c.gate = config.gate;
    c.stride = config.stride;
    c.top_k = config.top_k;
    return c;
  }
  static mh_icp_align_config alignConfig(const AlignConfig & config)
  {
    mh_icp_align_config c;
    c.max_iters = config.max_iters;
    c.eps_rot = config.eps_rot;
    c.eps_trans = config.eps_trans;
    c.damping = config.damping;
    c.prior_sigma_rot = config.prior_sigma_rot;
    c.prior_sigma_trans = config.prior_sigma_trans;
    c.check_every = config.check_every;
    return c;
  }
  static AlignBatchCall alignBatchBegin(const std::vector<ICPFactor *> & factors, const std::vector<Pose3> & T0, const Unit3 & g,
                                        const AlignConfig & config, bool async)
  {
    const size_t n = factors.size();
    if (!n || T0.size() != n) throw std::runtime_error("ICPFactor::alignBatch: one start pose per factor, at least one factor");
    for (const ICPFactor * f : factors)
      if (!f) throw std::runtime_error("ICPFactor::alignBatch: null factor");
    std::vector<double> R, t;
    flattenPoses(T0, R, t);  // (the library has copied the poses when the call returns)
    const A3 gu = toArray(g.unitVector());
    const mh_icp_align_config c = alignConfig(config);
    std::vector<mh_icp *> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = factors[i]->icp_;
    AlignBatchCall call;
    call.factors_ = factors;
    call.results_.reset(new mh_icp_align_result[n]);
    const Context & cx = factors[0]->ctx();
    if (async) {
      cx.check(mh_icp_align_batch_async(h.data(), n, R.data(), t.data(), gu.data(), &c, call.results_.get()), "mh_icp_align_batch_async");
      call.pending_ = true;
    } else {
      cx.check(mh_icp_align_batch(h.data(), n, R.data(), t.data(), gu.data(), &c, call.results_.get()), "mh_icp_align_batch");
    }
    return call;
  }
  ScoreCall scorePosesBegin(const std::vector<Pose3> & poses, const ScoreConfig & config, bool want_scores, bool async)
  {
    std::vector<double> R, t;
    flattenPoses(poses, R, t);  // (the library has copied the poses when the call returns)
    const mh_icp_score_config c = scoreConfig(config);
    ScoreCall call;
    call.owner_ = this;
    call.top_k_ = config.top_k;
    call.scores_.reset(new std::vector<mh_pose_score>(want_scores ? poses.size() : 0));
    call.best_.reset(new std::array<int32_t, MH_RELOC_MAX_REFINE>());
    call.best_->fill(-1);
    mh_pose_score * s = want_scores ? call.scores_->data() : nullptr;
    if (async) {
      ctx().check(mh_icp_score_poses_async(icp_, R.data(), t.data(), poses.size(), &c, s, call.best_->data()), "mh_icp_score_poses_async");
      call.pending_ = true;
    } else {
      ctx().check(mh_icp_score_poses(icp_, R.data(), t.data(), poses.size(), &c, s, call.best_->data()), "mh_icp_score_poses");
    }
    return call;
  }
  static std::unique_ptr<WindowCall> startWindow(const std::vector<Ptr> & factors, const std::vector<Pose3> & poses, const std::vector<WindowBetween> & between,
                                                 const Unit3 & g, const WindowConfig & config, bool blocking, const WindowRelin * relin = nullptr,
                                                 const std::vector<WindowLinear> * linear = nullptr, const std::vector<WindowEdge> * edges = nullptr,
                                                 bool marginal = false, const WindowJoint * joint = nullptr, bool joint_call = false)
  {
    const size_t n = factors.size();
    if (!n || poses.size() != n || between.size() != n) throw std::runtime_error("ICPFactor::optimiseWindow: one pose and one between entry per factor");
    std::unique_ptr<WindowCall> w(new WindowCall);
    w->factors_ = factors;
    w->h_.resize(n);
    w->R_.resize(9 * n);
    w->t_.resize(3 * n);
    w->ZR_.assign(9 * n, 0.0);
    w->Zt_.assign(3 * n, 0.0);
    w->has_Z_.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
      if (factors[i]->is_binary_) throw std::runtime_error("ICPFactor::optimiseWindow: unary factors only");
      w->h_[i] = factors[i]->icp_;
      const PoseRM T = rowMajor(poses[i]);
      std::memcpy(&w->R_[9 * i], T.R.data(), 72);
      std::memcpy(&w->t_[3 * i], T.t.data(), 24);
      if (i && between[i].present) {
        const PoseRM Z = rowMajor(between[i].Z);
        std::memcpy(&w->ZR_[9 * i], Z.R.data(), 72);
        std::memcpy(&w->Zt_[3 * i], Z.t.data(), 24);
        w->has_Z_[i] = 1;
      }
    }
    w->g_ = toArray(g.unitVector());
    w->c_.iters = config.iters;
    w->c_.check_every = config.check_every;
    std::memcpy(w->c_.between_info, config.between_info, sizeof(config.between_info));
    std::memcpy(w->c_.prior_info, config.prior_info, sizeof(config.prior_info));
    w->c_.damping = config.damping;
    w->c_.eps_rot = config.eps_rot;
    w->c_.eps_trans = config.eps_trans;
    w->r_.reset(new mh_icp_window_result);
    if (linear) {
      for (const WindowLinear & l : *linear) {
        mh_window_linear_factor q;
        std::memset(&q, 0, sizeof(q));
        q.pose = l.pose < n ? static_cast<int32_t>(l.pose) : -1;  // (out of range: the library's to refuse)
        const PoseRM L = rowMajor(l.at);
        std::memcpy(q.L_R, L.R.data(), 72);
        std::memcpy(q.L_t, L.t.data(), 24);
        for (int r = 0; r < 6; ++r) {
          for (int c = 0; c < 6; ++c) q.H[6 * r + c] = l.H(r, c);
          q.b[r] = l.b(r);
        }
        q.f = l.f;
        w->lin_.push_back(q);
      }
      if (relin) {
        w->relin_on_ = true;
        w->relin_.relin_rot = relin->rot;
        w->relin_.relin_trans = relin->trans;
        w->masks_.assign(static_cast<size_t>(config.iters > 0 ? config.iters : 0), 0u);
      }
      if (edges) {
        for (const WindowEdge & e : *edges) {
          mh_window_edge q;
          std::memset(&q, 0, sizeof(q));
          q.pose_a = e.a < n ? static_cast<int32_t>(e.a) : -1;  // (out of range: the library's to refuse)
          q.pose_b = e.b < n ? static_cast<int32_t>(e.b) : -1;
          const PoseRM Z = rowMajor(e.Z);
          std::memcpy(q.Z_R, Z.R.data(), 72);
          std::memcpy(q.Z_t, Z.t.data(), 24);
          for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) q.info[6 * r + c] = e.info(r, c);
          w->edges_.push_back(q);
        }
        if (joint) {
          const size_t nj = joint->poses.size();
          if (joint->at.size() != nj || joint->H.size() != 36 * nj * nj || joint->b.size() != 6 * nj)
            throw std::runtime_error("ICPFactor::optimiseWindowJoint: one linearization pose per member, H of 6n x 6n, b of 6n");
          w->joint_.reset(new mh_window_joint_factor);
          mh_window_joint_factor & q = *w->joint_;
          std::memset(&q, 0, sizeof(q));
          q.n_poses = static_cast<int32_t>(nj);  // (out of range: the library's to refuse)
          const size_t nm = nj < static_cast<size_t>(MH_WINDOW_JOINT_POSES) ? nj : static_cast<size_t>(MH_WINDOW_JOINT_POSES);
          for (size_t m = 0; m < nm; ++m) {
            q.pose[m] = joint->poses[m] < n ? static_cast<int32_t>(joint->poses[m]) : -1;
            const PoseRM L = rowMajor(joint->at[m]);
            std::memcpy(q.L_R + 9 * m, L.R.data(), 72);
            std::memcpy(q.L_t + 3 * m, L.t.data(), 24);
          }
          for (size_t r = 0; r < 6 * nm; ++r) {
            for (size_t c = 0; c < 6 * nm; ++c) q.H[24 * r + c] = joint->H[6 * nj * r + c];
            q.b[r] = joint->b[r];
          }
          q.f = joint->f;
        }
        if (marginal && joint_call) {
          w->jm_.reset(new mh_window_joint_marginal);
          const auto fm = blocking ? mh_icp_window_marginalise_joint : mh_icp_window_marginalise_joint_async;
          factors[0]->ctx().check(fm(w->h_.data(), n, w->R_.data(), w->t_.data(), w->has_Z_.data(), w->ZR_.data(), w->Zt_.data(), w->g_.data(), &w->c_,
                                     w->lin_.data(), w->lin_.size(), w->edges_.data(), w->edges_.size(), w->joint_.get(), w->jm_.get()),
                                  blocking ? "mh_icp_window_marginalise_joint" : "mh_icp_window_marginalise_joint_async");
          return w;
        }
        if (joint_call) {
          const auto fj = blocking ? mh_icp_window_optimise_joint : mh_icp_window_optimise_joint_async;
          factors[0]->ctx().check(fj(w->h_.data(), n, w->R_.data(), w->t_.data(), w->has_Z_.data(), w->ZR_.data(), w->Zt_.data(), w->g_.data(), &w->c_,
                                     relin ? &w->relin_ : nullptr, w->lin_.data(), w->lin_.size(), w->edges_.data(), w->edges_.size(), w->r_.get(), nullptr,
                                     relin ? w->masks_.data() : nullptr, w->joint_.get()),
                                  blocking ? "mh_icp_window_optimise_joint" : "mh_icp_window_optimise_joint_async");
          return w;
        }
        if (marginal) {
          w->m_.reset(new mh_window_marginal);
          const auto fm = blocking ? mh_icp_window_marginalise : mh_icp_window_marginalise_async;
          factors[0]->ctx().check(fm(w->h_.data(), n, w->R_.data(), w->t_.data(), w->has_Z_.data(), w->ZR_.data(), w->Zt_.data(), w->g_.data(), &w->c_,
                                     w->lin_.data(), w->lin_.size(), w->edges_.data(), w->edges_.size(), w->m_.get()),
                                  blocking ? "mh_icp_window_marginalise" : "mh_icp_window_marginalise_async");
          return w;
        }
        const auto fe = blocking ? mh_icp_window_optimise_edges : mh_icp_window_optimise_edges_async;
        factors[0]->ctx().check(fe(w->h_.data(), n, w->R_.data(), w->t_.data(), w->has_Z_.data(), w->ZR_.data(), w->Zt_.data(), w->g_.data(), &w->c_,
                                   relin ? &w->relin_ : nullptr, w->lin_.data(), w->lin_.size(), w->edges_.data(), w->edges_.size(), w->r_.get(), nullptr,
                                   relin ? w->masks_.data() : nullptr),
                                blocking ? "mh_icp_window_optimise_edges" : "mh_icp_window_optimise_edges_async");
        return w;
      }
      const auto fl = blocking ? mh_icp_window_optimise_lin : mh_icp_window_optimise_lin_async;
      factors[0]->ctx().check(fl(w->h_.data(), n, w->R_.data(), w->t_.data(), w->has_Z_.data(), w->ZR_.data(), w->Zt_.data(), w->g_.data(), &w->c_,
                                 relin ? &w->relin_ : nullptr, w->lin_.data(), w->lin_.size(), w->r_.get(), nullptr, relin ? w->masks_.data() : nullptr),
                              blocking ? "mh_icp_window_optimise_lin" : "mh_icp_window_optimise_lin_async");
      return w;
    }
    if (relin) {
      w->relin_on_ = true;
      w->relin_.relin_rot = relin->rot;
      w->relin_.relin_trans = relin->trans;
      w->masks_.assign(static_cast<size_t>(config.iters > 0 ? config.iters : 0), 0u);
      const auto fr = blocking ? mh_icp_window_optimise_relin : mh_icp_window_optimise_relin_async;
      factors[0]->ctx().check(fr(w->h_.data(), n, w->R_.data(), w->t_.data(), w->has_Z_.data(), w->ZR_.data(), w->Zt_.data(), w->g_.data(), &w->c_, &w->relin_,
                                 w->r_.get(), nullptr, w->masks_.data()),
                              blocking ? "mh_icp_window_optimise_relin" : "mh_icp_window_optimise_relin_async");
      return w;
    }
    const auto fn = blocking ? mh_icp_window_optimise : mh_icp_window_optimise_async;
    factors[0]->ctx().check(fn(w->h_.data(), n, w->R_.data(), w->t_.data(), w->has_Z_.data(), w->ZR_.data(), w->Zt_.data(), w->g_.data(), &w->c_, w->r_.get(), nullptr),
                            blocking ? "mh_icp_window_optimise" : "mh_icp_window_optimise_async");
    return w;
  }

  const bool is_binary_;
  IncrementalVoxelMapPCL::Ptr ivox_target_;
  size_t n_;
  mh_icp * icp_ = nullptr;
  mutable mh_icp_result last_;
  std::vector<Ptr> reloc_work_;  // relocaliseBatch: the clones its candidates are aligned on, made on first use
};

// ---------------------------------------------------------------------------------------------
// mimosa_msgs/msg/LidarGeometricDebug.msg counterpart (plain struct)
struct GeometricDebug
{
  size_t n_points_in = 0, n_points_in_sm_ds = 0;
  int n_status[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  V3D localizability_trans_comp{}, localizability_rot_comp{}, localizability_trans_final{}, localizability_rot_final{};
  bool degen_rot_bool[3] = {false, false, false}, degen_trans_bool[3] = {false, false, false};
  int n_linearize_calls = 0;
  bool map_updated = false;
  // GeometricConfig::map_keyframe_min_new_fraction > 0: n_added / n_points of the insert preview updateMap decided by, and its
  // counts; -1 and zeros when no preview ran (switch off, forced update, first keyframe)
  double map_new_fraction = -1;
  mh_map_insert_preview map_preview{};
  // GeometricConfig::map_carve_grid > 0: what the carve before this keyframe's insert removed; zeros when none ran
  bool map_carved = false;
  mh_map_carve_result map_carve{};
};

class Geometric
{
public:
  const GeometricConfig config;

  Geometric(const std::shared_ptr<Context> & ctx, const GeometricConfig & cfg) : config(cfg), ctx_(ctx)
  {
    // geometric.cpp:23-28
    ivox_map_ = std::make_shared<IncrementalVoxelMapPCL>(ctx_, config.scan_to_map.target_ivox_map_leaf_size);
    ivox_map_->set_lru_horizon(config.lru_horizon);
    ivox_map_->set_neighbor_voxel_mode(config.neighbor_voxel_mode);
    ivox_map_->set_min_dist_in_cell(config.scan_to_map.target_ivox_map_min_dist_in_voxel);
    initial_clouds_to_force_map_update_ = config.initial_clouds_to_force_map_update;
    if (config.map_keyframe_store_capacity > 0)
      keyframe_store_ = std::make_shared<KeyframeStore>(ctx_, config.map_keyframe_store_capacity, config.map_keyframe_store_points);
  }

  // geometric.cpp:128-183: subset -> body frame (f32, on the GPU) -> voxel down-sample (host, :55-126)
  void preprocess(const PointCloud & points_deskewed, const std::vector<size_t> & idxs, const double ts)
  {
    if (!config.enabled) return;
    ts_ = ts;
    Be_cloud_.clear();
    Be_cloud_.reserve(idxs.size());
    for (const size_t idx : idxs) Be_cloud_.push_back(points_deskewed[idx]);
    float Rt[12];
    toFloat12(config.T_B_L, Rt);
    if (!Be_cloud_.empty())
      ctx_->check(mh_transform_f32(ctx_->get(), Be_cloud_.data(), Be_cloud_.size(), Rt, Rt + 9), "mh_transform_f32");
    downsample(Be_cloud_, sm_Be_cloud_ds_, config.scan_to_map.source_voxel_grid_filter_leaf_size, 20,
               config.scan_to_map.source_voxel_grid_min_dist_in_voxel);
    device_scan_ = nullptr;
    debug_.n_points_in = points_deskewed.size();
    debug_.n_points_in_sm_ds = sm_Be_cloud_ds_.size();
  }

  // The same on a device-resident scan: subset + body transform + down-sampler run on the GPU; Be_cloud_ stays there
  // (updateMap inserts it into the map on the device, geometric.cpp:483-495).
  void preprocess(ScanFrontEnd & scan, const double ts)
  {
    if (!config.enabled) return;
    ts_ = ts;
    float Rt[12];
    toFloat12(config.T_B_L, Rt);
    ctx_->check(mh_scan_preprocess_geometric(scan.underlying(), Rt, Rt + 9, config.scan_to_map.source_voxel_grid_filter_leaf_size,
                                             20, config.scan_to_map.source_voxel_grid_min_dist_in_voxel, &scan.mutableInfo()),
                "mh_scan_preprocess_geometric");
    Be_cloud_.clear();
    sm_Be_cloud_ds_.clear();
    device_scan_ = &scan;
    debug_.n_points_in = scan.info().n_full;
    debug_.n_points_in_sm_ds = scan.info().n_downsampled;
  }

  // geometric.cpp:185-328
  void getFactors(const Key & key, const Values & values, NonlinearFactorGraph & graph, M66 & eigenvectors_block_matrix,
                  V6D & degen_directions)
  {
    if (!config.enabled) return;
    factor_ = device_scan_ ? std::make_shared<ICPFactor>(key, ivox_map_, *device_scan_, config.scan_to_map)
                           : std::make_shared<ICPFactor>(key, ivox_map_, sm_Be_cloud_ds_, config.scan_to_map);
    auto tmp = factor_->linearize(values);  // linearized right away so localizability is available (:196)
    (void)tmp;
    V3D tc, rc, tf, rf;
    M33 et, er;
    factor_->getLocalizabilities(tc, rc, tf, rf, et, er);
    eigenvectors_block_matrix.setZero();
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        eigenvectors_block_matrix(r, c) = er(r, c);
        eigenvectors_block_matrix(3 + r, 3 + c) = et(r, c);
      }
    for (int i = 0; i < 3; ++i) {  // :218-228
      degen_directions(i) = rc(i) < config.scan_to_map.degen_thresh_rot;
      degen_directions(3 + i) = tc(i) < config.scan_to_map.degen_thresh_trans;
      debug_.degen_rot_bool[i] = degen_directions(i) != 0;
      debug_.degen_trans_bool[i] = degen_directions(3 + i) != 0;
    }
    debug_.localizability_trans_comp = tc;
    debug_.localizability_rot_comp = rc;
    debug_.localizability_trans_final = tf;
    debug_.localizability_rot_final = rf;
    for (int i = 0; i < 9; ++i) debug_.n_status[i] = factor_->lastResult().status_hist[i];  // :280-323
    // nothing reads the components or the histogram of this factor again (the smoother only takes the HessianFactor):
    // its re-linearizations skip that pass
    factor_->computeComponents(false);
    graph.add(factor_);
  }

  // geometric.cpp:427-513
  void updateMap(const Key key, const Values & values)
  {
    if (!config.enabled) return;
    if (factor_) debug_.n_linearize_calls = factor_->getLinearizeCount();
    const Pose3 T_W_Be = values.at<Pose3>(key);
    bool update_map = true;
    debug_.map_new_fraction = -1;
    debug_.map_preview = mh_map_insert_preview{};
    if (config.map_keyframe_min_new_fraction > 0) {
      // the quantity the pose test is a proxy for (geometric.cpp:460-464): what the map would keep of this scan.  Forced updates
      // and the first keyframe need no preview; the pose test is not evaluated.
      if (!map_poses_.empty() && initial_clouds_to_force_map_update_ == 0) {
        mh_map_insert_preview pv{};
        if (device_scan_) {
          pv = ivox_map_->previewInsertBodyCloud(device_scan_->underlying(), T_W_Be);
        } else {
          PointCloud W = Be_cloud_;
          float Rt[12];
          toFloat12(T_W_Be, Rt);
          if (!W.empty()) ctx_->check(mh_transform_f32(ctx_->get(), W.data(), W.size(), Rt, Rt + 9), "mh_transform_f32");
          pv = ivox_map_->previewInsert(W);
        }
        debug_.map_preview = pv;
        debug_.map_new_fraction = pv.n_points > 0 ? static_cast<double>(pv.n_added) / static_cast<double>(pv.n_points) : 0.0;
        update_map = static_cast<double>(pv.n_added) >= config.map_keyframe_min_new_fraction * static_cast<double>(pv.n_points);
      }
    } else if (!map_poses_.empty()) {
      float min_diff_trans = std::numeric_limits<float>::max();
      size_t min_diff_index = 0;
      for (size_t i = 0; i < map_poses_.size(); ++i) {
        const Point3 & a = map_poses_[i].translation();
        const Point3 & b = T_W_Be.translation();
        const float d = static_cast<float>(std::sqrt((a(0) - b(0)) * (a(0) - b(0)) + (a(1) - b(1)) * (a(1) - b(1)) + (a(2) - b(2)) * (a(2) - b(2))));
        if (d < min_diff_trans) {
          min_diff_trans = d;
          min_diff_index = i;
        }
      }
      // rot_diff = R_B_L^-1 * between(R_kf, R_now) * R_B_L, yaw-pitch-roll magnitudes (:454-458)
      const Rot3 & RBL = config.T_B_L.rotation();
      const Rot3 dR = RBL.inverse() * map_poses_[min_diff_index].rotation().between(T_W_Be.rotation()) * RBL;
      const M33 d = dR.matrix();  // Rot3::ypr() spelled out
      const double yaw = std::atan2(d(1, 0), d(0, 0));
      const double pitch = std::atan2(-d(2, 0), std::sqrt(d(2, 1) * d(2, 1) + d(2, 2) * d(2, 2)));
      const double roll = std::atan2(d(2, 1), d(2, 2));
      const double ypr_max = std::max(std::fabs(yaw), std::max(std::fabs(pitch), std::fabs(roll)));
      if (min_diff_trans > config.map_keyframe_trans_thresh)
        update_map = true;
      else if (ypr_max > config.map_keyframe_rot_thresh_deg * 0.017453293)  // DEG2RAD = PCL's macro (x)*0.017453293
        update_map = true;
      else
        update_map = false;
    }
    if (initial_clouds_to_force_map_update_ > 0) {
      update_map = true;
      initial_clouds_to_force_map_update_--;
    }
    debug_.map_updated = update_map;
    debug_.map_carved = false;
    debug_.map_carve = mh_map_carve_result{};
    if (!update_map) return;
    // world transform in f32 (:483-490), then copy-then-insert so live factors keep their snapshot (:494-495)
    ivox_map_ = ivox_map_->fork();  // device-to-device copy; the previous map lives on in the factors that hold it
    if (config.map_carve_grid > 0) {
      // the fork has no factor yet, so the carve disturbs nothing in the window.  Be_cloud_ is in the body frame, where the
      // sensor sits at T_B_L's translation.
      mh_map_carve_config cc{};
      cc.grid = config.map_carve_grid;
      cc.ring = config.map_carve_ring;
      cc.range_min = config.map_carve_range_min;
      cc.range_max = config.map_carve_range_max;
      cc.margin_abs = config.map_carve_margin_abs;
      cc.margin_rel = config.map_carve_margin_rel;
      cc.apply = 1;
      const V3D origin_B = config.T_B_L.translation();
      debug_.map_carve = device_scan_ ? ivox_map_->carveFromScan(device_scan_->underlying(), 1, origin_B, T_W_Be, cc)
                                      : ivox_map_->carve(Be_cloud_, origin_B, T_W_Be, cc);
      debug_.map_carved = true;
    }
    if (device_scan_) {
      ivox_map_->insertBodyCloud(device_scan_->underlying(), T_W_Be);  // transform + insert on the device
    } else {
      PointCloud W = Be_cloud_;
      float Rt[12];
      toFloat12(T_W_Be, Rt);
      if (!W.empty()) ctx_->check(mh_transform_f32(ctx_->get(), W.data(), W.size(), Rt, Rt + 9), "mh_transform_f32");
      ivox_map_->insert(W);
    }
    if (keyframe_store_) {  // a full store throws: the caller sizes it (GeometricConfig::map_keyframe_store_*)
      const int64_t tag = static_cast<int64_t>(map_poses_.size());
      if (device_scan_)
        keyframe_store_->addBodyCloud(device_scan_->underlying(), tag);
      else
        keyframe_store_->add(Be_cloud_, tag);
    }
    map_poses_.push_back(T_W_Be);
  }

  // After a loop closure: ivox_map_ becomes the map that the stored keyframe clouds give at `corrected` (one pose per keyframe, in
  // map_poses_' order), map_poses_ becomes `corrected`.  The previous map lives on in the factors that hold it, as after updateMap.
  // Needs GeometricConfig::map_keyframe_store_capacity > 0.  Refused with map_carve_grid > 0: a carved map is not a pure insert
  // sequence, so the stored clouds do not reproduce it.
  mh_map_rebuild_result rebuildMap(const std::vector<Pose3> & corrected)
  {
    if (!keyframe_store_) throw std::runtime_error("Geometric::rebuildMap: no keyframe store (GeometricConfig::map_keyframe_store_capacity is 0)");
    if (config.map_carve_grid > 0) throw std::runtime_error("Geometric::rebuildMap: a carved map (map_carve_grid > 0) is not a pure insert sequence");
    if (corrected.size() != map_poses_.size() || corrected.size() != keyframe_store_->size())
      throw std::runtime_error("Geometric::rebuildMap: one corrected pose per keyframe");
    mh_map_rebuild_result res{};
    ivox_map_ = keyframe_store_->rebuild(corrected, ivox_map_->config(), {}, 0, &res);
    map_poses_ = corrected;
    return res;
  }
  const std::shared_ptr<KeyframeStore> & keyframeStore() const { return keyframe_store_; }
  const std::vector<Pose3> & mapPoses() const { return map_poses_; }

  const GeometricDebug & debug() const { return debug_; }
  const PointCloud & sourceCloud() const { return sm_Be_cloud_ds_; }
  const IncrementalVoxelMapPCL::Ptr & map() const { return ivox_map_; }
  const ICPFactor::Ptr & factor() const { return factor_; }

  // Geometric::downsample, geometric.cpp:55-126 with FlatContainerMinimal::add (lidar/utils.hpp:260-278):
  // greedy, input order; output = voxels in first-seen order, points in acceptance order.
  static void downsample(const PointCloud & in, PointCloud & out, const double leaf_size, const size_t max_points_per_voxel,
                         const double min_dist_in_voxel)
  {
    struct Key3
    {
      int x, y, z;
      bool operator==(const Key3 & o) const { return x == o.x && y == o.y && z == o.z; }
    };
    struct Hash
    {
      size_t operator()(const Key3 & k) const
      {  // XORVector3iHash, lidar/utils.hpp:228-238
        return static_cast<size_t>((k.x * 9132043225175502913ull) ^ (k.y * 7277549399757405689ull) ^
                                   (k.z * 6673468629021231217ull));
      }
    };
    auto ffloor = [](double v) {
      const int n = static_cast<int>(v);
      return n - (v < static_cast<double>(n) ? 1 : 0);
    };
    const double inv = 1.0 / leaf_size, min_sq = min_dist_in_voxel * min_dist_in_voxel;
    std::unordered_map<Key3, size_t, Hash> voxels;
    voxels.reserve(in.size() / 2 + 1);
    std::vector<std::vector<uint32_t>> kept;
    for (size_t i = 0; i < in.size(); ++i) {
      const double px = in[i].x, py = in[i].y, pz = in[i].z;
      const Key3 c{ffloor(px * inv), ffloor(py * inv), ffloor(pz * inv)};
      auto f = voxels.find(c);
      if (f == voxels.end()) {
        f = voxels.emplace(c, kept.size()).first;
        kept.emplace_back();
      }
      auto & cell = kept[f->second];
      if (cell.size() >= max_points_per_voxel) continue;
      bool close = false;
      for (const uint32_t j : cell) {
        const double dx = in[j].x - px, dy = in[j].y - py, dz = in[j].z - pz;
        if (dx * dx + (dy * dy + dz * dz) < min_sq) {
          close = true;
          break;
        }
      }
      if (!close) cell.push_back(static_cast<uint32_t>(i));
    }
    out.clear();
    for (const auto & cell : kept)
      for (const uint32_t j : cell) out.push_back(in[j]);
  }

private:
  std::shared_ptr<Context> ctx_;
  PointCloud Be_cloud_, sm_Be_cloud_ds_;
  ScanFrontEnd * device_scan_ = nullptr;  // set by the device preprocess: the factor takes its cloud from there
  ICPFactor::Ptr factor_;
  IncrementalVoxelMapPCL::Ptr ivox_map_;
  std::shared_ptr<KeyframeStore> keyframe_store_;  // null unless GeometricConfig::map_keyframe_store_capacity > 0
  std::vector<Pose3> map_poses_;
  size_t initial_clouds_to_force_map_update_ = 0;
  double ts_ = 0;
  GeometricDebug debug_;
};

// Manager::deskewPoints, pose part (manager.cpp:455-499), for callers that run their own IMU preintegration
// (gtsam::PreintegratedImuMeasurements stays the caller's: SURVEY.md §7).  Inputs are what that loop has in
// hand: the interpolated IMU samples (time, accelerometer, gyroscope — `imu_measurements`), the NavState the
// preintegrator predicted AT each sample time (nav[j] = state at imu_t[j]; nav[0] = the previous state), the
// bias, the gravity direction (unit) and magnitude, the scan's distinct timestamps and header time, and T_B_S.
// Output: T_Le_Lt per distinct timestamp, exactly the constant-acceleration / constant-rate extrapolation of
// :478-489 followed by T_Le_W * T_W_Bt * T_B_S (:493-497).  Timestamps after the last IMU sample get no pose
// (the reference's vector simply ends there).
using gtsam::NavState;

inline std::vector<Pose3> computeDeskewPoses(const std::vector<double> & imu_t, const std::vector<V3D> & imu_acc,
                                             const std::vector<V3D> & imu_gyro, const std::vector<NavState> & nav,
                                             const V3D & bias_acc, const V3D & bias_gyro, const V3D & gravity_unit,
                                             const double gravity_norm, const std::vector<uint32_t> & unique_ns,
                                             const double header_ts, const Pose3 & T_B_S)
{
  if (imu_t.size() < 2) throw std::runtime_error("Preintegration not possible as there are less than 2 measurements P1");  // :442-446
  if (imu_acc.size() != imu_t.size() || imu_gyro.size() != imu_t.size() || nav.size() != imu_t.size())
    throw std::runtime_error("computeDeskewPoses: one measurement and one state per IMU sample");
  std::vector<Pose3> T_W_Bts;
  T_W_Bts.reserve(unique_ns.size());
  size_t u = 0;
  for (size_t c = 0; c + 1 < imu_t.size(); ++c) {  // curr = c, next = c + 1 (:459-466)
    const NavState & curr = nav[c];
    const A9 Rc = rowMajor(curr.pose().rotation().matrix());
    const A3 pc = toArray(curr.pose().translation()), vc = toArray(curr.velocity());
    while (u < unique_ns.size()) {
      const double ts = header_ts + unique_ns[u] * 1.0e-9;  // globalTs, manager.hpp:94
      if (ts > imu_t[c + 1]) break;
      const double dt = ts - imu_t[c];
      double acc[3], omega[3];
      for (int i = 0; i < 3; ++i) {
        acc[i] = imu_acc[c](i) - bias_acc(i);     // ConstantBias::correctAccelerometer
        omega[i] = imu_gyro[c](i) - bias_gyro(i);  // ::correctGyroscope
      }
      // :478-489  R = R_c Exp(omega dt),  p = p_c + v dt + 1/2 R_c a dt^2 + 1/2 g_hat |g| dt^2
      const Rot3 R = curr.pose().rotation() * Rot3::Expmap(V3D(omega[0] * dt, omega[1] * dt, omega[2] * dt));
      double p[3];
      for (int i = 0; i < 3; ++i) {
        const double Ra = Rc[3 * i] * acc[0] + Rc[3 * i + 1] * acc[1] + Rc[3 * i + 2] * acc[2];
        p[i] = pc[i] + vc[i] * dt + 0.5 * Ra * dt * dt + 0.5 * gravity_unit(i) * gravity_norm * dt * dt;
      }
      T_W_Bts.push_back(Pose3(R, Point3(p[0], p[1], p[2])));
      ++u;
    }
  }
  const Pose3 T_Le_W = T_B_S.inverse() * nav.back().pose().inverse();  // propagated state = T_W_Be (:492-493)
  std::vector<Pose3> out;
  out.reserve(T_W_Bts.size());
  for (const Pose3 & T : T_W_Bts) out.push_back(T_Le_W * T * T_B_S);
  return out;
}

// The IMU intervals mh_scan_deskew_imu / ScanFrontEnd::deskewPointsFromImu take, from the same inputs as computeDeskewPoses:
// interval c = (imu_t[c], imu_t[c + 1]] with the state at imu_t[c] and the bias-corrected measurement of sample c (:459-492).
// The per-timestamp half of computeDeskewPoses then runs on the device.
inline std::vector<mh_imu_segment> imuSegments(const std::vector<double> & imu_t, const std::vector<V3D> & imu_acc, const std::vector<V3D> & imu_gyro,
                                               const std::vector<NavState> & nav, const V3D & bias_acc, const V3D & bias_gyro)
{
  if (imu_t.size() < 2) throw std::runtime_error("Preintegration not possible as there are less than 2 measurements P1");  // :442-446
  if (imu_acc.size() != imu_t.size() || imu_gyro.size() != imu_t.size() || nav.size() != imu_t.size())
    throw std::runtime_error("imuSegments: one measurement and one state per IMU sample");
  if (imu_t.size() - 1 > MH_MAX_IMU_SEGMENTS) throw std::runtime_error("imuSegments: more than MH_MAX_IMU_SEGMENTS IMU intervals in one scan");
  std::vector<mh_imu_segment> seg(imu_t.size() - 1);
  for (size_t c = 0; c + 1 < imu_t.size(); ++c) {
    mh_imu_segment & s = seg[c];
    s.t0 = imu_t[c];
    s.t1 = imu_t[c + 1];
    const A9 R = rowMajor(nav[c].pose().rotation().matrix());
    const A3 p = toArray(nav[c].pose().translation()), v = toArray(nav[c].velocity());
    for (int i = 0; i < 9; ++i) s.R[i] = R[static_cast<size_t>(i)];
    for (int i = 0; i < 3; ++i) {
      s.p[i] = p[static_cast<size_t>(i)];
      s.v[i] = v[static_cast<size_t>(i)];
      s.acc[i] = imu_acc[c](i) - bias_acc(i);      // ConstantBias::correctAccelerometer (:479)
      s.omega[i] = imu_gyro[c](i) - bias_gyro(i);  // ::correctGyroscope (:480)
    }
  }
  return seg;
}

// Manager::deskewPoints' per-point part (manager.cpp:496-509).  T_Le_Lt[g] is the pose of the sensor at
// unique timestamp g in the scan-end frame — computed by the caller's IMU propagation (:455-499), which
// stays on the CPU.  Points are transformed in place on the GPU.
inline void deskewPoints(const Context & ctx, PointCloud & points_full, const std::vector<uint32_t> & unique_ns,
                         const std::vector<Pose3> & T_Le_Lt, const Pose3 * T_B_L = nullptr)
{
  if (unique_ns.size() != T_Le_Lt.size()) throw std::runtime_error("deskewPoints: one pose per unique timestamp");
  std::vector<float> Rt12(12 * T_Le_Lt.size());
  for (size_t g = 0; g < T_Le_Lt.size(); ++g) toFloat12(T_Le_Lt[g], &Rt12[12 * g]);
  float Rb[12];
  if (T_B_L) toFloat12(*T_B_L, Rb);
  ctx.check(mh_deskew(ctx.get(), points_full.data(), points_full.size(), unique_ns.data(), Rt12.data(), unique_ns.size(),
                      T_B_L ? Rb : nullptr, T_B_L ? Rb + 9 : nullptr),
            "mh_deskew");
}

}  // namespace lidar
}  // namespace mimosa_hip
