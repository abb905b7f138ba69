/*
 * mimosa_hip.h — C ABI of libmimosa_hip.so: the MI355X-native (gfx950, HIP) implementation of the
 * LiDAR geometric-factor hot path of ntnu-arl/mimosa.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ / torch / GTSAM
 * types.  Every entry point names the reference interface it replaces (paths relative to the
 * reference's mimosa/ package).  The C++ host layer in mimosa_amd/host/ (ICPFactor, Geometric,
 * IncrementalVoxelMap, Manager) is a thin mirror of the reference classes over this ABI.
 *
 * Conventions
 *  - every function returns an mh_status (0 = MH_OK); nothing throws across the boundary; per-point
 *    failures are RejectStatus values (same enum values 0..8 as geometric_factor.hpp:35-46), never
 *    errors.
 *  - matrices are row-major doubles; poses are (R[9], t[3]).
 *  - caller-owned host buffers are only read/written for the duration of the call; device memory is
 *    owned by the library behind opaque handles.
 *  - handles are not individually thread-safe; different handles may be used from different host
 *    threads (the library sets the device per call; one HIP stream per context).
 */
#ifndef MIMOSA_HIP_H
#define MIMOSA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_ABI_VERSION 3  /* 3: mh_set_overlap is gone with the component server (round 6); 2: the caller-driven sharding entry points,
                           * mh_map_fork and mh_map_sync went (round 5) */

typedef enum mh_status {
  MH_OK = 0,
  MH_ERR_INVALID_ARG = 1,
  MH_ERR_HIP = 2,        /* a HIP runtime call failed; see mh_last_error() */
  MH_ERR_NO_DEVICE = 3,  /* no usable gfx950 device (the library never falls back to the CPU) */
  MH_ERR_OOM = 4,
  MH_ERR_UNSUPPORTED = 5
} mh_status;

/* ICPFactor::RejectStatus, include/mimosa/lidar/geometric_factor.hpp:35-46 */
typedef enum mh_reject_status {
  MH_UNPROCESSED = 0,
  MH_INSUFFICIENT_CORRES_POINTS = 1,
  MH_CORRES_MAX_DIST = 2,
  MH_EIGEN_SOLVER_FAIL = 3,
  MH_MIN_EIGEN_VALUE_LOW = 4,
  MH_LINE = 5,
  MH_CORRES_PLANE_INVALID = 6,
  MH_MAX_ERROR = 7,
  MH_VALID = 8
} mh_reject_status;

/* lidar::Point, include/mimosa/lidar/point.hpp:18-39 (32 bytes, 16-byte aligned) */
typedef struct mh_point32 {
  float x, y, z, pad;
  float intensity;
  uint32_t t;   /* ns since the beginning of the scan */
  uint32_t idx; /* index in the original cloud */
  float range;
} mh_point32;

/* lidar::PointOuster, include/mimosa/lidar/point.hpp:42-50 (32 bytes, 16-byte aligned): what
 * Manager::prepareInput<PointOuster> reads from the sensor_msgs::PointCloud2 (lidar/manager.cpp:155-157) */
typedef struct mh_ouster_point {
  float x, y, z, pad;
  float intensity;
  uint32_t t; /* ns since the beginning of the scan */
  uint16_t reflectivity;
  uint16_t ring;
  uint32_t pad2;
} mh_ouster_point;

/* The fields of lidar::ManagerConfig (include/mimosa/lidar/manager.hpp:24-41) and GeometricConfig
 * (geometric_config.hpp:43-44) that Manager::prepareInput reads. */
typedef struct mh_input_config {
  float range_min, range_max;         /* metres; compared as squares in float (manager.cpp:19-20, :281-282) */
  float intensity_min, intensity_max; /* manager.cpp:272-276 */
  float ns_max;                       /* manager.cpp:306 */
  float z_offset;                     /* -lidar_to_sensor_transform[11] / 1000 (manager.cpp:18, :313) */
  int32_t create_full_res_pointcloud; /* loop stride 1 instead of point_skip_divisor (manager.cpp:244-246) */
  int32_t point_skip_divisor;         /* geometric subset: raw index % divisor == 0 (manager.cpp:318) */
  int32_t ring_skip_divisor;          /* geometric subset: ring % divisor == 0 (manager.cpp:331) */
} mh_input_config;

typedef struct mh_scan_info {
  uint64_t n_in;          /* raw points given to mh_scan_prepare_input */
  uint64_t n_full;        /* points_full_: points that passed the filters */
  uint64_t n_geometric;   /* geometric_point_idxs_ */
  uint64_t n_unique_ns;   /* unique_ns_ */
  uint64_t n_body;        /* Be_cloud_ (after mh_scan_preprocess_geometric) */
  uint64_t n_downsampled; /* sm_Be_cloud_ds_ */
  uint32_t last_point_ns; /* corrected_ts_ = header_ts + last_point_ns * 1e-9 (manager.cpp:336) */
  uint32_t pad;
} mh_scan_info;

/* lidar::RegistrationConfig, include/mimosa/lidar/geometric_config.hpp:17-33 (same field order) */
typedef struct mh_reg_config {
  float source_voxel_grid_filter_leaf_size;
  float source_voxel_grid_min_dist_in_voxel;
  float target_ivox_map_leaf_size;
  float target_ivox_map_min_dist_in_voxel;
  uint64_t num_corres_points; /* 2..8 supported */
  float max_corres_distance;
  float plane_validity_distance;
  float lidar_point_noise_std_dev;
  int32_t use_huber;
  float huber_threshold;
  int32_t reg_4_dof;
  int32_t project_on_degneneracy; /* (sic) spelling follows the reference */
  float degen_thresh_rot;
  float degen_thresh_trans;
} mh_reg_config;

/* gtsam_points::iVox settings as configured by Geometric's constructor, src/lidar/geometric.cpp:23-28 */
typedef struct mh_map_config {
  double leaf_size;            /* scan_to_map.target_ivox_map_leaf_size */
  double min_dist_in_cell;     /* scan_to_map.target_ivox_map_min_dist_in_voxel */
  int32_t max_points_in_cell;  /* FlatContainer default 20 (<= 20 supported) */
  int32_t neighbor_voxel_mode; /* 1, 7, 19 or 27 */
  int64_t lru_horizon;         /* GeometricConfig::lru_horizon */
  int32_t lru_clear_cycle;     /* iVox default 10 */
  int32_t reserved;
} mh_map_config;

typedef struct mh_map_stats {
  int64_t n_voxels;
  int64_t n_points;
  int64_t n_blocks;          /* 4x4x4-voxel blocks in the device block table */
  int64_t device_bytes;      /* HBM held by this map */
  int64_t uploads;           /* insert calls so far */
  int64_t upload_bytes;      /* bytes of point batches pushed host->device (nothing else ever travels) */
  int64_t delta_uploads;     /* == uploads: an insert only ever moves its own batch */
  int64_t full_uploads;      /* always 0 since the map is maintained on the device (kept for ABI stability) */
} mh_map_stats;

/* What the next insert of a batch would do (mh_map_preview_insert*): the outcome of every point under the insert's sequential
 * per-voxel rule.  n_added + n_too_close + n_voxel_full == n_points.  48 bytes. */
typedef struct mh_map_insert_preview {
  int64_t n_points;          /* the batch */
  int64_t n_added;           /* points the insert would keep */
  int64_t n_too_close;       /* refused by the min-distance rule */
  int64_t n_voxel_full;      /* refused because their voxel holds max_points_in_cell */
  int64_t n_touched_voxels;  /* distinct voxels of the batch */
  int64_t n_new_voxels;      /* of those, voxels the map does not hold yet */
} mh_map_insert_preview;

/*
 * What gtsam::HessianFactor(key[, key2], G11, [G12,] g1, [G22, g2,] f) receives from
 * ICPFactor::linearize (geometric_factor.hpp:459-462, 559-560) plus every getter-visible side
 * output (getLocalizabilities :52-62, getDegenInfo :64-70, getLinearizeCount :72) and the status
 * histogram Geometric::getFactors builds (src/lidar/geometric.cpp:280-323).
 * The Hessian factor is HessianFactor(key, H_ss, -b_s, f).
 */
typedef struct mh_icp_result {
  double H_ss[36]; /* J_s^T J_s, row-major 6x6, rotation block first (GTSAM Pose3 tangent order) */
  double H_st[36]; /* binary factor only */
  double H_tt[36]; /* binary factor only */
  double b_s[6];   /* J_s^T e */
  double b_t[6];   /* binary factor only */
  double f;        /* sum e^2 */
  double loc_trans_comp[3], loc_rot_comp[3], loc_trans_final[3], loc_rot_final[3];
  double eigvec_trans[9], eigvec_rot[9]; /* eigenvectors in columns, row-major storage */
  double degen_rot[3], degen_trans[3], degen_eigvec_rot[9], degen_eigvec_trans[9];
  int32_t status_hist[9];
  int32_t linearize_count;
  double mean_candidates; /* mean number of map points in the occupied neighbour voxels of a query that ran k-NN
                             (what the reference scans; SURVEY.md §8(d)'s C_q) */
  double mean_scanned;    /* mean number the device actually scanned after exact box-distance pruning */
  int64_t n_knn;          /* queries that ran k-NN in this call (the rest hit the DA cache) */
  int64_t n_exact_fallback; /* of those, queries whose coarse f32 scan could not be proven exact and were redone in fp64 */
  /* device-side timing of this call, ms; -1 unless this call was timed (mh_set_profiling) */
  float gpu_ms_linearize; /* icp_linearize kernel (K3) */
  float gpu_ms_localizability; /* component-localizability kernel (K4) */
} mh_icp_result;

typedef struct mh_ctx mh_ctx;
typedef struct mh_map mh_map;
typedef struct mh_icp mh_icp;
typedef struct mh_scan mh_scan;

/* ---- context ------------------------------------------------------------------------------ */
int mh_abi_version(void);
/* Binds a context to HIP device `device` and creates its stream.  MH_ERR_NO_DEVICE if there is no
 * GPU: there is no CPU fallback. */
int mh_init(int device, mh_ctx ** out);
/* Sharded factors and communicators may outlive the context: see the teardown rule at mh_shard_icp_destroy. */
void mh_shutdown(mh_ctx * ctx);
/* Last error text for this context (or the calling thread when ctx == NULL). */
const char * mh_last_error(const mh_ctx * ctx);
/* Per-kernel HIP-event timing inside mh_icp_linearize / mh_icp_linearize_async: 0 = off (default), n >= 1 =
 * bracket the kernels of every n-th linearize call of a factor (each event record costs ~4 us of stream time,
 * so a throughput measurement samples).  Untimed calls report gpu_ms_* = -1. */
int mh_set_profiling(mh_ctx * ctx, int every);
/* hipStream_t of the context, for callers that want to order their own work / events on it. */
void * mh_stream(mh_ctx * ctx);
int mh_synchronize(mh_ctx * ctx);
/* Event pair on the context stream: begin/end bracket, returns elapsed ms (synchronises). */
int mh_timer_begin(mh_ctx * ctx);
int mh_timer_end(mh_ctx * ctx, float * ms);

/* ---- target map: IncrementalVoxelMapPCL / gtsam_points::iVox --------------------------------
 * replaces include/mimosa/lidar/incremental_voxel_map.hpp:22-54, src/lidar/incremental_voxel_map.cpp:14-62.
 * The map lives on the device and is maintained there: insertion (greedy first-come-first-kept per voxel, min-distance
 * rule, per-voxel cap, voxels numbered in creation order), the LRU purge, getCloud and the copy are kernels; the
 * host keeps counters.  Mutations are synchronous and drain the device first, so factors of any context that share
 * the map see either the old or the new state, never a half-written one. */
int mh_map_create(mh_ctx * ctx, const mh_map_config * cfg, mh_map ** out); /* ctor, geometric.cpp:23-28 */
/* IncrementalVoxelMapPCL::insert (incremental_voxel_map.cpp:19-24).  xyz: n host points, `stride_floats` floats apart
 * (3 for packed xyz, 8 for mh_point32).  MH_ERR_UNSUPPORTED if a point is NaN or farther than 2^20 voxels from the origin. */
int mh_map_insert(mh_map * map, const float * xyz, size_t n, size_t stride_floats);
/* The same for a batch that is already on the map's device (d_points: device pointer).  R, t (both or neither): the
 * f32 rigid transform p <- R p + t applied first — Geometric::updateMap's world transform (geometric.cpp:483-490),
 * Eigen's evaluation order, no FMA. */
int mh_map_insert_device(mh_map * map, const void * d_points, size_t n, size_t stride_floats, const float * R, const float * t);
/* Geometric::updateMap's insert (geometric.cpp:483-495) straight from a device-resident scan: Be_cloud_ (the body-frame
 * geometric subset of mh_scan_preprocess_geometric) transformed by T_W_Be in f32 and inserted, no host round trip. */
int mh_map_insert_from_scan(mh_map * map, const mh_scan * scan, const float R_W_Be[9], const float t_W_Be[3]);
/* Insert preview: what the three inserts above WOULD do to this batch, read-only.  The information content of a scan with respect
 * to the map, which Geometric::updateMap replaces by a pose test (geometric.cpp:460-464), without forking the map and inserting.
 * Arguments: those of mh_map_insert / mh_map_insert_device / mh_map_insert_from_scan (same f32 transform, Eigen's order, no FMA),
 *   then `out` (required) and `outcome` (n bytes of HOST memory, or NULL): outcome[i] of input point i is 1 = added, 2 = too
 *   close (a resident point or a point of the batch kept earlier lies within min_dist_in_cell), 3 = voxel full (the voxel holds
 *   max_points_in_cell points when the point's turn comes).  Without `outcome` nothing is stored per point.
 * Synchronous on the map's context.
 * Meaning: the counts describe the insertion step of the insert that would come next, before any LRU purge that insert might
 *   trigger.  When it triggers none: mh_map_get_stats' n_points after minus before == n_added, n_voxels after minus before ==
 *   n_new_voxels, and the points that appear in mh_map_get_cloud are exactly the points with outcome 1.
 * Nothing observable moves: the eight fields of mh_map_get_stats (uploads and upload_bytes included), mh_map_get_cloud,
 *   mh_map_knn, the LRU stamps and counter and every factor on the map are what they were; a later real insert gives the map
 *   that a never-previewed twin gets, bit for bit.  The call writes nothing that factors read, so — unlike the inserts — it does
 *   not wait for the streams of other contexts that hold factors on the map.
 * n == 0: MH_OK, all zeros.
 * Refusals, each with the map untouched and usable: MH_ERR_INVALID_ARG for a NULL map or `out` (mh_last_error(NULL) names the
 *   function), for R without t or the reverse; MH_ERR_UNSUPPORTED for a NaN point, a voxel coordinate beyond +-2^20, a batch too
 *   large or a total above 2^27 voxels, as the insert; MH_ERR_HIP on a map a failed mutation left inconsistent.
 * The sharded inserts (mh_map_insert_shard*) have no preview. */
int mh_map_preview_insert(mh_map * map, const float * xyz, size_t n, size_t stride_floats, mh_map_insert_preview * out, uint8_t * outcome);
int mh_map_preview_insert_device(mh_map * map, const void * d_points, size_t n, size_t stride_floats, const float * R, const float * t,
                                 mh_map_insert_preview * out, uint8_t * outcome);
int mh_map_preview_insert_from_scan(mh_map * map, const mh_scan * scan, const float R_W_Be[9], const float t_W_Be[3],
                                    mh_map_insert_preview * out, uint8_t * outcome);
/* Map carving: remove the map points a new scan sees through.  Not in the reference, whose map only grows or loses whole
 * voxels by age; a point a person, a door or a vehicle left in a voxel the robot keeps observing stays there for good.
 *
 * The rule is a visibility test on a direction grid (a cube map around the sensor), conservative on purpose, without any
 * transcendental function.  All arithmetic is fp64, in the written order, without FMA contraction, so a restatement in numpy
 * (tests/map_carve_ref.py) matches it decision for decision.
 *
 * Inputs: `obs`, n points (f32 xyz, `stride_floats` apart) in some frame F; origin_F[3], the sensor origin in F; R_W_F[9]
 *   (row-major), t_W_F[3], the pose of F in the map frame, in doubles; and a config:
 *     grid N, 4 .. 512;  ring, 0 .. 2;  range_min, with 0 < range_min < range_max;  range_max;  margin_abs >= 0;
 *     margin_rel >= 0;  apply, 0 or 1.  All real values must be finite.
 *
 * Direction cell of a vector s = (s0, s1, s2), a cube map:
 *   1. Let a_k = |s_k|.
 *   2. The major axis f is 0 if a0 >= a1 and a0 >= a2, else 1 if a1 >= a2, else 2.
 *   3. m = a_f.  A vector with m == 0 has no cell (nor has one with a component that is not finite).
 *   4. face = 2f + (s_f < 0).
 *   5. (u, v) = (s_{(f+1)%3} / m, s_{(f+2)%3} / m).
 *   6. i = min(N-1, (int)floor((u + 1.0) * (0.5 * N))).
 *   7. j is formed the same way from v.
 *   8. cell = (face * N + j) * N + i.
 *
 * Observation image, 6 N^2 doubles, initially "not hit":
 *   1. For each obs point with finite coordinates, s = p - origin_F.  The f32 coordinates are widened first.
 *   2. r2 = (s0*s0 + s1*s1) + s2*s2.
 *   3. If r2 >= range_min^2 (and s has a cell), the point's cell takes min(cell, r2).
 *   4. Points beyond range_max still count.  They prove free space up to themselves.
 *
 * Map point test, for a bucket point p (f32 widened):
 *   1. d = p - t_W_F.
 *   2. s_a = ((R[a]*d0 + R[3+a]*d1) + R[6+a]*d2) - origin_F[a].  That is R^T d, with R row-major.
 *   3. r2 is computed as above.  r = sqrt(r2).
 *   4. The point is TESTED iff range_min^2 <= r2 <= range_max^2 (and s has a cell).
 *   5. The point is SEEN THROUGH iff both conditions hold:
 *      - Every cell (i+di, j+dj) with |di|, |dj| <= ring that lies inside [0, N) on the point's own face is hit.  Cells off
 *        the face are ignored.
 *      - With q the minimum of those cells and lim = r + (margin_abs + margin_rel * r), lim * lim < q.
 *   ring = 0 trusts a single cell, whose nearest return may belong to a surface beside the ray: in a 20 x 16 x 5 m room scanned
 *   with 64 x 1024 beams it removed hundreds to thousands of static points, ring = 1 none (at N = 64 and 128, margin 0.3 m).  A
 *   grid finer than the scan (N = 256 for 64 rows) leaves cells unhit and removes nothing.
 *
 * apply = 1: seen-through points leave their buckets.  A bucket's survivors keep their relative order and move to the front;
 *   the coarse copies, the voxel's count and its cell word in every block table it sits in follow.  A voxel left with no
 *   point is erased (a cell word with count 0 does not exist).  The surviving voxels keep their order and their LRU stamps;
 *   ids, block table and cell words are rebuilt exactly as the LRU purge rebuilds them.  The LRU counter and mh_map_get_stats'
 *   uploads and upload_bytes do not move.  The call is a mutation like the insert: it waits for the streams of the contexts
 *   that hold factors on the map, is synchronous, and refuses a map a failed mutation left inconsistent.  Factors created
 *   before the call keep per-point association state that names the old map: mh_icp_reset them.
 * apply = 0 (preview): the same counts, and nothing observable moves — mh_map_preview_insert's contract, including not
 *   waiting for readers.
 *
 * n == 0: MH_OK, nothing removed.
 * Refusals, each with the map untouched and usable: MH_ERR_INVALID_ARG for a NULL argument, a stride below 3, a config
 *   outside the stated ranges, a pose entry or origin that is not finite, `which` outside 0 .. 1, a scan without that stage
 *   or on another device; MH_ERR_UNSUPPORTED for a batch too large, as the insert; MH_ERR_HIP on an inconsistent map. */
typedef struct mh_map_carve_config {
  int32_t grid;       /* N: cells per cube-face edge, 4 .. 512 */
  int32_t ring;       /* 0 .. 2: neighbour cells on the point's face that must agree */
  double range_min;   /* m; observations nearer than this are not used, map points nearer than this not tested */
  double range_max;   /* m; map points farther than this are not tested */
  double margin_abs;  /* m */
  double margin_rel;  /* per metre of range */
  int32_t apply;      /* 0 = preview, 1 = carve */
  int32_t reserved;   /* 0 */
} mh_map_carve_config; /* 48 bytes */

typedef struct mh_map_carve_result {
  int64_t n_obs_used;        /* observation points that entered the image */
  int64_t n_cells_hit;       /* cells of the image that are hit */
  int64_t n_tested;          /* map points inside the range gates */
  int64_t n_removed;         /* of those, seen through */
  int64_t n_voxels_touched;  /* voxels that lose at least one point */
  int64_t n_voxels_emptied;  /* of those, voxels that lose all of theirs */
} mh_map_carve_result; /* 48 bytes */

int mh_map_carve(mh_map * map, const float * xyz, size_t n, size_t stride_floats, const double origin_F[3], const double R_W_F[9],
                 const double t_W_F[3], const mh_map_carve_config * cfg, mh_map_carve_result * out);
/* The same for a batch that is already on the map's device (d_points: device pointer). */
int mh_map_carve_device(mh_map * map, const void * d_points, size_t n, size_t stride_floats, const double origin_F[3], const double R_W_F[9],
                        const double t_W_F[3], const mh_map_carve_config * cfg, mh_map_carve_result * out);
/* The same straight from a device-resident scan.  which = 0: points_full_, the deskewed cloud in the lidar frame (the origin is
 * usually zero; needs mh_scan_prepare_input*); which = 1: Be_cloud_, the body frame (the origin is the caller's t_B_L; needs
 * mh_scan_preprocess_geometric). */
int mh_map_carve_from_scan(mh_map * map, const mh_scan * scan, int which, const double origin_F[3], const double R_W_F[9],
                           const double t_W_F[3], const mh_map_carve_config * cfg, mh_map_carve_result * out);
/* Deep copy — IncrementalVoxelMapPCL copy ctor (incremental_voxel_map.hpp:33-42) used by Geometric::updateMap's
 * copy-then-insert (geometric.cpp:494): device to device, both maps stay writable. */
int mh_map_copy(const mh_map * map, mh_map ** out);
/* shared_ptr semantics: factors retain the map they were built with. */
int mh_map_retain(mh_map * map);
void mh_map_release(mh_map * map);
int mh_map_get_stats(const mh_map * map, mh_map_stats * out);
/* IncrementalVoxelMapPCL::getCloud (incremental_voxel_map.cpp:34-38): all points in voxel order.
 * xyz may be NULL to query the size; returns the number of points through n_out. */
int mh_map_get_cloud(const mh_map * map, float * xyz, size_t capacity_points, size_t * n_out);
/* IncrementalVoxelMapPCL::knn_search (incremental_voxel_map.cpp:26-32) for a batch of fp64 queries,
 * run on the device.  point_xyz (n*k*3 doubles) receives the neighbour coordinates
 * (ivox->point(id), geometric_factor.hpp:184), sq_dists n*k ascending, found[n] = number found
 * (the reference returns found == k). */
int mh_map_knn(mh_map * map, const double * queries, size_t n, int k, double * point_xyz,
               double * sq_dists, int32_t * found);

/* ---- ICPFactor ------------------------------------------------------------------------------
 * replaces include/mimosa/lidar/geometric_factor.hpp:25-563 */
/* ctor (:119-156): copies the source cloud to the device, retains the map, allocates the per-point
 * data-association state zero-initialised.  `map` may belong to another context of the same device
 * (several contexts = several HIP streams sharing one read-only map); while factors of other contexts
 * are linearizing, do not insert into that map. */
int mh_icp_create(mh_ctx * ctx, mh_map * map, const mh_point32 * source, size_t n,
                  const mh_reg_config * cfg, int is_binary, mh_icp ** out);
/* clone() (:160-164): deep-copies the per-point state, shares the map. */
int mh_icp_clone(const mh_icp * icp, mh_icp ** out);
void mh_icp_destroy(mh_icp * icp);
/* linearize(Values) (:231-562).  T_src = Values[keys[0]]; (R_tgt, t_tgt) = Values[keys[1]] for a
 * binary factor, NULL for unary; g_unit = Values[G(0)].unitVector() (read unconditionally, :257).
 * Blocks until the result is on the host. */
int mh_icp_linearize(mh_icp * icp, const double R_src[9], const double t_src[3],
                     const double * R_tgt, const double * t_tgt, const double g_unit[3],
                     mh_icp_result * out);
/* Same work enqueued on the context stream without waiting; the result is written to *out (which
 * must stay valid) when mh_icp_wait / mh_synchronize returns. Up to 64 calls may be in flight. */
int mh_icp_linearize_async(mh_icp * icp, const double R_src[9], const double t_src[3],
                           const double * R_tgt, const double * t_tgt, const double g_unit[3],
                           mh_icp_result * out);
int mh_icp_wait(mh_icp * icp);
/* Every live ICPFactor of the sliding window re-linearized in ONE pass: what graph::Manager::defineNoLock's
 * smoother_->update() + additional_update_iterations (src/graph/manager.cpp:585-588) make GTSAM do one factor at
 * a time.  icps[f] is linearized at (R_src + 9 f, t_src + 3 f[, R_tgt + 9 f, t_tgt + 3 f], g_unit + 3 f) into out[f];
 * the per-point results (status, cached mean / normal of every point) are bit-identical to n_factors separate
 * mh_icp_linearize calls, and so are the sums when the factor runs the same LAUNCH CLASS in both — the class follows the
 * points of the whole launch (two lanes per point for k = 5 launches of up to 32 768 points, one lane up to 65 536, the
 * 512-thread class above); where the window's total moves a factor to another class its rows are added in another order
 * (H, b, f agree to ~1e-13 relative).  Factors that share a kernel instantiation — launch class, num_corres_points == 5 or
 * not, the map's neighbour mode, unary / binary — form one launch group: one K3 launch and one K4 launch per group, so a
 * window of like factors (the usual case) is one launch pair and any mix is accepted.  All factors must belong to one context and have no call in flight;
 * at most 64 per call.  R_tgt / t_tgt may be NULL when no factor is binary.  Blocks until every result is on the host. */
int mh_icp_linearize_batch(mh_icp * const * icps, size_t n_factors, const double * R_src, const double * t_src,
                           const double * R_tgt, const double * t_tgt, const double * g_unit, mh_icp_result * out);
/* getStatuses / getCorresMeansTarget / getCorresNormalsTarget (:48-50); any pointer may be NULL. */
int mh_icp_get_state(const mh_icp * icp, int32_t * status, double * means, double * normals);
/* Forget all data associations (== a freshly constructed factor): enqueued, no host sync. */
int mh_icp_reset(mh_icp * icp);
/* The component localizabilities and the status histogram (geometric_factor.hpp:430-457, geometric.cpp:280-323) need a second
 * pass over the points in the eigenbasis of the finished H — a kernel of its own (K4), a fifth of a call.  The reference
 * computes them in every linearize() but reads them in ONE place: Geometric::getFactors, right after its own linearize
 * (geometric.cpp:205-214, getLocalizabilities / the status log); the re-linearizations ISAM2 drives afterwards
 * (graph/manager.cpp:585-588) never have them looked at.  enabled = 0 skips the pass for this factor's following calls
 * (also in mh_icp_linearize_batch when no factor of the batch wants it): loc_trans_comp / loc_rot_comp come back NaN and
 * status_hist -1; H, b, f, the final localizabilities, eigenvectors and degeneracy info are bit-identical either way.
 * Default: enabled (the reference's behaviour). */
int mh_icp_set_components(mh_icp * icp, int enabled);
size_t mh_icp_size(const mh_icp * icp);

/* ---- scan-to-map alignment: a Gauss-Newton loop on the device ----------------------------------
 * One scan, one map, a rough pose in; the aligned pose out.  What a caller otherwise writes around mh_icp_linearize — one
 * blocking call, a 6 x 6 solve on the host, a retraction, again — runs as ONE chain of launches on the context's stream: K3
 * (component pass off), a one-wave step kernel that does the host epilogue's part of the work, solves
 * (H_ss + diag(prior) + damping I) xi = -b_s, retracts (R <- R Exp(xi_r), t <- t + R xi_t) and writes the pose into the
 * argument block of the next K3, and so on; the host waits once (or once per `check_every` iterations).  The step is taken
 * with exactly the H_ss, b_s that mh_icp_linearize returns at that pose, the reference's degeneracy quirk included: an
 * iteration with a degenerate direction (project_on_degneneracy) has H = b = 0 and moves by prior / damping only, i.e. not
 * at all.  A system without a positive pivot (a degenerate iteration without prior and damping) takes no step and ends the
 * call: MH_OK, converged = 0, the pose of that iteration unchanged, bit 4 in the trace row.
 * Unary, unsharded, non-empty factors without a call in flight.  The per-point association state evolves as under repeated
 * mh_icp_linearize calls and is left as the last EVALUATED pose left it (iterations queued behind the stop evaluate nothing);
 * the linearize count advances by `iters`. */
typedef struct mh_icp_align_config {
  int32_t max_iters;           /* 1 .. 64 (the factor's ring holds 64 calls) */
  double eps_rot, eps_trans;   /* rad, m: stop when both step norms fall below (0 = never) */
  double damping;              /* >= 0, added to the diagonal */
  double prior_sigma_rot, prior_sigma_trans; /* 0 = no prior; else 1 / sigma^2 on the diagonal, pulling towards the step's own pose */
  int32_t check_every;         /* launches queued per host look at the stop flag; 0 = all max_iters at once.  The result does
                                  not depend on it (mh_icp_align_async always queues everything) */
} mh_icp_align_config;

typedef struct mh_icp_align_trace {
  double f;                    /* cost at the pose the iteration evaluated */
  double step_rot, step_trans; /* |xi_r|, |xi_t| of its step */
  double R[9], t[3];           /* the pose after the step */
  int64_t n_knn;               /* queries that ran k-NN in this iteration (the rest hit the association cache) */
  int32_t degenerate;          /* 1: a rotation direction below its threshold, 2: a translation direction, 4: singular system */
  int32_t reserved;
} mh_icp_align_trace;

typedef struct mh_icp_align_result {
  double R[9], t[3];
  int32_t iters, converged;
  mh_icp_align_trace trace[64]; /* one row per executed iteration */
  mh_icp_result first, last;    /* what mh_icp_linearize (components off) returns at the initial and at the last evaluated pose */
} mh_icp_align_result;

int mh_icp_align(mh_icp * icp, const double R0[9], const double t0[3], const double g_unit[3],
                 const mh_icp_align_config * cfg, mh_icp_align_result * out);
/* The same without waiting: *out (which must stay valid) is filled when mh_icp_wait returns.  No other call on the
 * factor until then. */
int mh_icp_align_async(mh_icp * icp, const double R0[9], const double t0[3], const double g_unit[3],
                       const mh_icp_align_config * cfg, mh_icp_align_result * out);

/* ---- several alignments side by side: one chain for B (factor, start pose) pairs ----------------
 * B independent alignments, member i from (R0 + 9 i, t0 + 3 i); out[i] is member i's result.  Each is exactly the
 * mh_icp_align chain of that factor under cfg: the same H_ss, b_s, the degeneracy quirk, the prior on the step's own pose,
 * damping, the singular rule and the trace rows.  One cfg serves all members; the degeneracy thresholds, reg_4_dof and
 * project_on_degneneracy are each factor's own.  Nothing ties the members to each other: this is not a window.
 * Per iteration: the batch's K3 launches (component pass off; launch groups and launch classes chosen as
 * mh_icp_window_optimise chooses them for the same factors, i.e. by the batch's total point count — where that moves a
 * member to another class than a call of its own, its rows are added in another order, see mh_icp_linearize_batch), then ONE
 * step launch of B one-wave workgroups.  Member i's workgroup advances member i alone, writes its next pose into its
 * argument block of the next iteration and publishes its sums and trace row to the factor's own pinned ring.
 * Stopping is per member: one that converged or met a singular system evaluates nothing more (its later K3 blocks get
 * n = 0), its association state stays as its last evaluated pose left it, its linearize count advances by its own iters, its
 * result is what mh_icp_align gives (a singular member: MH_OK, converged = 0, bit 4 in its last row); the others go on.
 * check_every: iterations queued per host look; the host stops queueing once EVERY member's row carries the stop bit.  The
 * result does not depend on it.  The return value is MH_OK or the first member's error (a HIP failure).
 * Refused with nothing enqueued and every factor usable afterwards — MH_ERR_INVALID_ARG: a NULL argument or member, B
 * outside 1 .. MH_ALIGN_BATCH_MAX, the same factor twice, factors of different contexts, a member with a call in flight or
 * without points, a batch call already in flight on the context, the cfg ranges of mh_icp_align; MH_ERR_UNSUPPORTED: binary
 * factors and the factors of the map-sharded path.
 * While a call is in flight its members hold their whole ring: mh_icp_reset and mh_icp_wait refuse them, every other entry
 * point refuses them as factors with calls in flight.  Destroying a member inside a call nobody waited for abandons the call
 * as a whole. */
#define MH_ALIGN_BATCH_MAX 16
int mh_icp_align_batch(mh_icp * const * icps, size_t B, const double * R0, const double * t0, const double g_unit[3],
                       const mh_icp_align_config * cfg, mh_icp_align_result * out);
/* The same without waiting: out[] (which must stay valid; the other arguments may go) is filled by
 * mh_icp_align_batch_wait.  No other call on a member until then. */
int mh_icp_align_batch_async(mh_icp * const * icps, size_t B, const double * R0, const double * t0, const double g_unit[3],
                             const mh_icp_align_config * cfg, mh_icp_align_result * out);
/* Collects the one batch call in flight on the context (MH_ERR_INVALID_ARG when there is none). */
int mh_icp_align_batch_wait(mh_ctx * ctx);

/* ---- relocalisation: score candidate poses against the map, refine the best ---------------------
 * Every call above wants a pose that already lies inside the association gate.  These two serve the caller who has none: up to
 * MH_RELOC_MAX_POSES candidate poses of the factor's cloud are scored against its map in one chain of launches and ranked on
 * the device; mh_icp_relocalise then refines the few best with mh_icp_align.  No reference counterpart.
 *
 * Score of a pose (R, t) with gate g and stride s, over the factor's points i with i % s == 0 (i counts in the order the
 * points were given to mh_icp_create*): q = R p + t in fp64, q_a = ((R[3a] x + R[3a+1] y) + R[3a+2] z) + t[a]; the point is
 * `occupied` when the voxel of q holds a map point, and an `inlier` when the nearest map point over the map's neighbour voxels —
 * the k = 1 answer of mh_map_knn for q, bit for bit in sq_dists[0] — exists and has d2 <= g * g; sum_sq adds d2 over the
 * inliers.  A point farther than 2^20 voxels from the origin (or not finite after the transform) is neither: a pose far
 * outside the map is ordinary input and scores zeros.  The sums are taken in a fixed order that does not depend on n_poses: a
 * pose gives the same bits alone, at any position of any batch and on every repeat.
 * Ranking: n_inliers descending, then sum_sq ascending, then pose index ascending.  best[] receives the top_k pose indices in
 * rank order, -1 behind the last pose (all MH_RELOC_MAX_REFINE entries are written).
 * The call reads the map and the source cloud only: association state, linearize count and results of the factor are untouched.
 * MH_ERR_INVALID_ARG: a NULL icp, R, t or cfg, best == NULL with top_k > 0, a factor with a call in flight or without points,
 * n_poses outside 1 .. MH_RELOC_MAX_POSES, a gate that is not finite and > 0, stride < 1, top_k outside 0 .. MH_RELOC_MAX_REFINE,
 * a pose with an entry that is not finite (the message names its index).  MH_ERR_UNSUPPORTED: binary factors and the factors
 * of the map-sharded path.  Nothing is enqueued then. */
#define MH_RELOC_MAX_POSES 65536
#define MH_RELOC_MAX_REFINE 8
typedef struct mh_pose_score {
  int32_t n_points;   /* points looked at: ceil(n / stride) */
  int32_t n_occupied, n_inliers, reserved;
  double sum_sq;      /* sum of d2 over the inliers */
} mh_pose_score;      /* 24 bytes */

typedef struct mh_icp_score_config {
  double gate;        /* m, finite and > 0 */
  int32_t stride;     /* >= 1 */
  int32_t top_k;      /* 0 .. MH_RELOC_MAX_REFINE: how many winners the device selects */
} mh_icp_score_config;

/* R: 9 n_poses doubles (row-major), t: 3 n_poses.  scores (n_poses entries) may be NULL: a caller who wants only the winners
 * downloads MH_RELOC_MAX_REFINE indices.  best (MH_RELOC_MAX_REFINE entries) may be NULL iff top_k == 0. */
int mh_icp_score_poses(mh_icp * icp, const double * R, const double * t, size_t n_poses, const mh_icp_score_config * cfg,
                       mh_pose_score * scores, int32_t * best);
/* The same without waiting: scores / best (which must stay valid; R and t may go) are filled when mh_icp_wait returns.  No
 * other call on the factor until then. */
int mh_icp_score_poses_async(mh_icp * icp, const double * R, const double * t, size_t n_poses, const mh_icp_score_config * cfg,
                             mh_pose_score * scores, int32_t * best);

typedef struct mh_icp_reloc_config {
  mh_icp_score_config score;  /* the coarse pass; top_k >= 1 candidates are refined */
  mh_icp_align_config align;  /* the refinement of each */
  double final_gate;          /* m, finite and > 0: the gate of the re-score of the aligned poses (stride 1) */
} mh_icp_reloc_config;

typedef struct mh_icp_reloc_candidate {
  int32_t index;              /* into the caller's poses */
  int32_t iters, converged, reserved; /* of its alignment */
  mh_pose_score coarse;       /* its score in the coarse pass */
  double R[9], t[3];          /* the aligned pose (the unaligned one where the alignment ended on the singular path at once) */
  mh_pose_score fine;         /* the score of the aligned pose: stride 1, gate final_gate */
} mh_icp_reloc_candidate;

typedef struct mh_icp_reloc_result {
  int32_t n_candidates;       /* min(top_k, n_poses) */
  int32_t best;               /* the first of cand[] under the ranking on `fine` (ties: the earlier candidate) */
  double R[9], t[3];          /* its aligned pose */
  mh_icp_reloc_candidate cand[MH_RELOC_MAX_REFINE]; /* in the rank order of the coarse pass */
} mh_icp_reloc_result;

/* Score and select (one wait); for each selected candidate in rank order mh_icp_reset and mh_icp_align from its pose; one more
 * score call over the aligned poses.  The refusals of mh_icp_score_poses and mh_icp_align apply, and further
 * MH_ERR_INVALID_ARG for a NULL g_unit or out, score.top_k == 0 and a final_gate that is not finite and > 0.
 * On return the factor is RESET (its association state is that of a freshly constructed factor) and its linearize count has
 * advanced by the sum of the candidates' iters. */
int mh_icp_relocalise(mh_icp * icp, const double * R, const double * t, size_t n_poses, const double g_unit[3],
                      const mh_icp_reloc_config * cfg, mh_icp_reloc_result * out);
/* mh_icp_relocalise with the candidates aligned side by side: candidate c, in rank order, is aligned on work[c], which the
 * call resets first, and all candidates run in ONE mh_icp_align_batch.  Score, re-score, ranking and *out are as above (a
 * candidate's launch class follows the batch's total point count, so its aligned pose agrees with mh_icp_relocalise's to
 * rounding, ~1e-13 relative in the sums, not in bits).
 * work[]: n_work >= min(score.top_k, n_poses) clones of icp made by the caller with mh_icp_clone (a clone carries the
 * identity of its source's cloud; every created factor has a fresh one).  MH_ERR_INVALID_ARG for too few, for a NULL entry, an
 * entry twice, icp itself, an entry whose cloud identity, size, map or mh_reg_config differ from icp's, and an entry with a
 * call in flight; the refusals of mh_icp_relocalise and mh_icp_align_batch apply.  Nothing is enqueued then.
 * The one difference from mh_icp_relocalise: icp is only READ — its association state, linearize count and results do not
 * move (it is not reset).  The work[] factors that took a candidate are left as their alignments left them, and their
 * linearize counts advance by their own iters. */
int mh_icp_relocalise_batch(mh_icp * icp, mh_icp * const * work, size_t n_work, const double * R, const double * t,
                            size_t n_poses, const double g_unit[3], const mh_icp_reloc_config * cfg, mh_icp_reloc_result * out);

/* ---- place recognition: scan descriptors and a keyframe database, searched on the device -----------
 * mh_icp_score_poses and mh_icp_relocalise* search the candidate poses a caller hands them, in practice a grid around a
 * guess.  This section answers "where in this map could this scan have been taken": a database of rotation-tolerant scan
 * descriptors (a ring x sector height image in the style of Scan Context), searched by brute force over every entry and every
 * column shift.  Its hits are the grid centres mh_icp_relocalise wants.  Not in the reference.
 *
 * The arithmetic uses no transcendental function.  It is fp64, every product and sum rounded on its own (no FMA contraction),
 * in the written order, so a restatement in numpy (tests/place_ref.py) matches the descriptor bit for bit and the distance to
 * rounding.  It is implemented once, in place_device.hpp, for the device and for the host.
 *
 * 1. The descriptor.  Input: n points (f32 xyz, `stride_floats` apart) in some frame F, and R_G_F[9], a row-major fp64 rotation
 *    from F into a gravity-levelled frame G with the same origin (identity: the cloud is level).  Config: r_min, r_max, z_min,
 *    z_max in metres.  For each point, widened to fp64:
 *      p'_a = (R[3a] * x + R[3a+1] * y) + R[3a+2] * z
 *      r2   = p'_x * p'_x + p'_y * p'_y
 *    The point counts iff r2 >= r_min * r_min && r2 < b2[20] && p'_z > z_min && p'_z < z_max (a NaN fails), with
 *      b2[i] = (i * w) * (i * w), w = r_max / 20, i = 0 .. 20, computed once on the host.
 *    ring   = the number of i in 1 .. 19 with r2 >= b2[i].
 *    sector = 15 * q + m, where the quadrant q is 0 for x' > 0, y' >= 0;  1 for x' <= 0, y' > 0;  2 for x' < 0, y' <= 0;  3
 *      otherwise;  (u, v) = (x', y'), (y', -x'), (-x', -y'), (-y', x') for q = 0, 1, 2, 3;  and m = the number of j in 1 .. 14
 *      with v * C[j] >= u * S[j], where C[j], S[j] = cos, sin(6 deg * j) are the 17-digit literals of place_device.hpp.  (The
 *      axes fall into sectors 0 / 15 / 30 / 45, the point (1, 1) into sector 7.)
 *    The value of a cell is the maximum over its points of (float)(p'_z - z_min); an empty cell is 0.0f.  A maximum does not
 *    depend on the order of the points, so the descriptor is exact whatever the launch shape.  The descriptor is
 *    MH_PLACE_RINGS x MH_PLACE_SECTORS floats, ring-major: desc[ring * 60 + sector].
 *
 * 2. The distance of a query Q to a candidate C:
 *      n_X[j]  = sqrt(sum_i X[i][j]^2), fp64, i ascending.
 *      Column j of Q is compared with column (j + s) % 60 of C; the pair is valid iff both norms are > 0.
 *      c(s, j) = (sum_i Q[i][j] * C[i][(j+s)%60]) / (n_Q[j] * n_C[(j+s)%60]), i ascending.
 *      N(s)    = the number of valid j.
 *      d(s)    = N(s) >= min_overlap ? 1 - (sum_j c(s, j)) / N(s) : 2.0, the valid j ascending.
 *      D       = min_s d(s);  shift = the smallest s that attains it;  no admissible shift: D = 2.0, shift = 0.
 *    Nothing is summed across lanes, waves or workgroups, so an entry's {D, shift} has the same bits alone, at any database
 *    size, at any position and on every repeat.
 *    Hits are ranked by D ascending, then database index ascending.  An entry with D == 2.0 is never a hit.  All top_k hits are
 *    written; those behind the last real one have index -1 (shift 0, dist 2.0, tag 0).
 *    A hit with shift s means  T_W_Fq ~ T_W_Fk * (R_G_Fk^T * Rz(+s * 6 deg) * R_G_Fq, 0):  yaw_q - yaw_k = s * 6 deg.
 *
 * 3. The database holds, per entry, the 1 200 floats, their 60 column norms (computed on the device by the same kernel for
 *    every way of adding) and an int64 tag of the caller's.  It holds no pose: poses stay with the caller, because a smoother
 *    moves them.  Capacity is fixed at creation, 1 .. 65 536 entries.  A database belongs to its context and works on that
 *    context's stream; after mh_shutdown of the context every call but mh_place_db_destroy refuses it.
 *
 * Refusals, each with nothing enqueued and the database unchanged: MH_ERR_INVALID_ARG for a NULL argument; config values that
 *   are not finite; r_min <= 0, r_max <= r_min, z_min >= z_max; min_overlap outside 1 .. 60; capacity outside 1 .. 65 536;
 *   top_k outside 1 .. MH_PLACE_MAX_HITS; n_search greater than the size; a query on an empty database; an add to a full
 *   database; an index past the size; a stride below 3; `which` outside 0 .. 1, a scan without that stage or on another
 *   device; a descriptor entry that is negative or not finite; an R_G_F entry that is not finite.  MH_ERR_UNSUPPORTED for more
 *   than 2^30 - 1 points.  Zero points are no error: they give the all-zero descriptor, which matches nothing. */
#define MH_PLACE_RINGS 20
#define MH_PLACE_SECTORS 60
#define MH_PLACE_MAX_HITS 16

typedef struct mh_place_db mh_place_db;

typedef struct mh_place_config {
  double r_min, r_max;   /* m, horizontal range in G: 0 < r_min < r_max */
  double z_min, z_max;   /* m, height in G: z_min < z_max */
  int32_t min_overlap;   /* 1 .. 60: valid column pairs a shift needs to be admissible */
  int32_t capacity;      /* 1 .. 65 536 entries */
} mh_place_config; /* 40 bytes */

typedef struct mh_place_hit {
  int32_t index;   /* database index, -1 behind the last real hit */
  int32_t shift;   /* 0 .. 59 */
  double dist;     /* D */
  int64_t tag;     /* the entry's tag */
} mh_place_hit; /* 24 bytes */

typedef struct mh_place_score {
  double dist;     /* D of one searched entry (2.0: no admissible shift) */
  int32_t shift;
  int32_t reserved; /* 0 */
} mh_place_score; /* 16 bytes */

int mh_place_db_create(mh_ctx * ctx, const mh_place_config * cfg, mh_place_db ** out);
void mh_place_db_destroy(mh_place_db * db);
/* entries in the database; 0 for NULL or a database whose context was shut down */
size_t mh_place_db_size(const mh_place_db * db);

/* The descriptor of n host points under the database's config: desc[1200].  Synchronous; the database is not changed. */
int mh_place_describe(mh_place_db * db, const float * xyz, size_t n, size_t stride_floats, const double R_G_F[9], float * desc);
/* The same for points that are already on the database's device (d_points: device pointer). */
int mh_place_describe_device(mh_place_db * db, const void * d_points, size_t n, size_t stride_floats, const double R_G_F[9], float * desc);
/* The same straight from a device-resident scan; `which` as in mh_map_carve_from_scan (0: points_full_, 1: Be_cloud_). */
int mh_place_describe_from_scan(mh_place_db * db, const mh_scan * scan, int which, const double R_G_F[9], float * desc);

/* Append a host descriptor (one saved in an earlier session, say) under `tag`; *index (may be NULL) receives its index. */
int mh_place_db_add(mh_place_db * db, const float * desc, int64_t tag, int32_t * index);
/* Describe a device-resident scan and append the result, on the device: no host round trip. */
int mh_place_db_add_from_scan(mh_place_db * db, const mh_scan * scan, int which, const double R_G_F[9], int64_t tag, int32_t * index);
/* Read entry `index` back: desc[1200] and *tag (either may be NULL). */
int mh_place_db_get(mh_place_db * db, int32_t index, float * desc, int64_t * tag);

/* Search entries 0 .. n_search - 1 (n_search == 0: all of them; a loop-closure caller leaves out the newest keyframes) for the
 * top_k nearest to `desc`: hits[top_k] in rank order; all (may be NULL) receives {D, shift} of every searched entry.  One chain
 * of launches on the context's stream — norms of the query, distances, selection — and one wait. */
int mh_place_db_query(mh_place_db * db, const float * desc, size_t n_search, int32_t top_k, mh_place_hit * hits, mh_place_score * all);
/* The same with the query described from a device-resident scan within the chain. */
int mh_place_db_query_from_scan(mh_place_db * db, const mh_scan * scan, int which, const double R_G_F[9], size_t n_search, int32_t top_k,
                                mh_place_hit * hits, mh_place_score * all);

/* ---- fixed-lag window: the smoother's Gauss-Newton loop on the device ---------------------------
 * W unary factors, one pose each, tied by between factors and a prior on the oldest pose: what a caller otherwise writes
 * around mh_icp_linearize_batch — one blocking batch call, a 6W x 6W system assembled and solved on the host, W retractions,
 * again — runs as ONE chain of launches on the context's stream.  Per iteration: the window's K3 batch launches (component
 * pass off; launch groups and launch classes chosen as mh_icp_linearize_batch chooses them for the same window) and a
 * one-workgroup step kernel, which does the host epilogue's part of the work for every factor, assembles
 *   A = blockdiag(H_ss,i) + sum_i J_i^T diag(between_info) J_i + diag(prior_info) on pose 0 + damping I,   g likewise,
 * with the between factor Z_i of poses i - 1, i (where has_Z[i] != 0; has_Z[0] is ignored): residual
 * [Log(Z.R^T R_ab), Z.R^T (t_ab - Z.t)], T_ab = T_{i-1}^-1 T_i, J_a = -Ad(T_ab^-1), J_b = I; solves A xi = -g (block
 * tridiagonal L D L^T with residual refinement), retracts every pose (R <- R Exp(xi_r), t <- t + R xi_t) and writes the poses
 * into the argument blocks of the next iteration's launches.  The host waits once (or once per `check_every` iterations).
 * Every factor's step uses exactly the H_ss, b_s that mh_icp_linearize returns at its pose (4-DoF projection and the
 * degeneracy quirk included).  A system without a positive pivot takes no step and ends the call: MH_OK, converged = 0, the
 * poses of that iteration unchanged, bit 4 in the trace row.
 * Factors: 1 .. MH_WINDOW_MAX, unary, unsharded, of one context, each at most once, none with a call in flight; an empty
 * factor is allowed and contributes nothing.  One window call per context at a time.  The per-point association state
 * evolves as under repeated mh_icp_linearize_batch calls and is left as the last EVALUATED poses left it; every factor's
 * linearize count advances by `iters` (the executed ones).  Until the call has been waited for, mh_icp_reset, mh_icp_linearize*,
 * mh_icp_align* and mh_icp_wait refuse its factors.  Bad arguments: MH_ERR_INVALID_ARG / MH_ERR_UNSUPPORTED, nothing
 * enqueued, the handles unchanged. */
#define MH_WINDOW_MAX 16

typedef struct mh_icp_window_config {
  int32_t iters;               /* 1 .. 64 iterations queued */
  int32_t check_every;         /* iterations queued per host look at the stop flag; 0 = all at once.  The result does not
                                  depend on it (mh_icp_window_optimise_async always queues everything) */
  double between_info[6];      /* diagonal weights of every between factor, (rotation, translation) order: 1 / sigma^2 */
  double prior_info[6];        /* on the diagonal of the oldest pose (0 = none), pulling towards the step's own pose */
  double damping;              /* >= 0, added to every diagonal entry */
  double eps_rot, eps_trans;   /* rad, m: stop when EVERY pose's step norms fall below (0 = never: a fixed iteration count) */
} mh_icp_window_config;

typedef struct mh_icp_window_trace {
  double f;                    /* cost at the poses the iteration evaluated: the factors' f plus the between terms */
  double step_rot, step_trans; /* max over the poses of |xi_r|, |xi_t| */
  int32_t flags;               /* 4: singular system (no step; the call ends here) */
  uint32_t degenerate;         /* 2 bits per pose: 1 a rotation direction of its factor below the threshold, 2 a translation one */
} mh_icp_window_trace;

typedef struct mh_icp_window_result {
  double R[MH_WINDOW_MAX * 9], t[MH_WINDOW_MAX * 3]; /* the final poses, W used */
  int32_t iters, converged;
  int32_t n_poses, reserved;
  mh_icp_window_trace trace[64];     /* one row per executed iteration */
  mh_icp_result first[MH_WINDOW_MAX], last[MH_WINDOW_MAX]; /* per factor: what mh_icp_linearize (components off) returns at the
                                        initial and at the last evaluated pose */
} mh_icp_window_result;

/* R[9 W], t[3 W]: the initial poses, oldest first; has_Z[W], Z_R[9 W], Z_t[3 W]: the between measurements (entry i ties poses
 * i - 1 and i; Z_R / Z_t may be NULL when no has_Z is set); g_unit[3]: the gravity direction every factor reads.
 * trace_poses: NULL, or cfg->iters x W x 12 doubles the caller owns — the poses (R row-major, then t) after every executed
 * step; rows of iterations that were not executed are left untouched.  Blocks until the result is on the host. */
int mh_icp_window_optimise(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                           const double * Z_R, const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg,
                           mh_icp_window_result * out, double * trace_poses);
/* The same without waiting: *out and trace_poses (which must stay valid) are filled when mh_icp_window_wait(ctx) returns, ctx
 * being the factors' context.  No other call on the factors until then. */
int mh_icp_window_optimise_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                 const double * Z_R, const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg,
                                 mh_icp_window_result * out, double * trace_poses);
int mh_icp_window_wait(mh_ctx * ctx);

/* The same chain with ISAM2's per-variable relinearization thresholds: a factor is evaluated again (K3 at the current pose)
 * only once its pose has left the neighbourhood of the pose L_i of its last evaluation.  At the start of an iteration, with
 * d_r = Log(L_i.R^T R_i), d_t = L_i.R^T (t_i - L_i.t): factor i is evaluated in iteration 0, and whenever any |d_r[k]| > relin_rot
 * or any |d_t[k]| > relin_trans (component-wise and strict: exactly at a threshold keeps).  Otherwise its K3 launch touches
 * none of its points and the step uses the H_ss, b_s, f of the evaluation at L_i, carried to the current pose to first order
 * under the chain's retraction: with M = blockdiag(Jr^-1(d_r), Exp(d_r)) and d = [d_r, d_t] the factor contributes M^T H M,
 * M^T (b + H d) and the cost f + 2 b^T d + d^T H d (at d = 0 the stored H, b, f as they are).  The step in front of an iteration
 * takes the decision on the device; between factors, prior, damping, solve, retraction and stopping are those of
 * mh_icp_window_optimise, at the current poses.  With both thresholds 0 every non-empty factor whose pose moved at all is
 * evaluated and the call computes, bit for bit, what mh_icp_window_optimise computes.
 * Per-point association state: as the factor's own last evaluation left it.  Linearize count: advances by the number of the
 * factor's evaluations (an empty factor's by the executed iterations, as above).  first / last in the result: the factor's
 * first and last evaluation.  trace[].degenerate carries a kept factor's bits of its last evaluation.
 * evaluated_mask: NULL, or cfg->iters words the caller owns — bit i of word j: factor i ran K3 in iteration j; words of
 * iterations that were not executed are left untouched.  Every restriction and error rule of mh_icp_window_optimise applies;
 * thresholds that are negative or not finite: MH_ERR_INVALID_ARG, nothing enqueued.  mh_icp_window_wait collects the _async
 * form as well (evaluated_mask must stay valid until then). */
typedef struct mh_icp_window_relin {
  double relin_rot, relin_trans;  /* rad, m; >= 0 */
} mh_icp_window_relin;
int mh_icp_window_optimise_relin(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                 const double * Z_R, const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg,
                                 const mh_icp_window_relin * relin, mh_icp_window_result * out, double * trace_poses,
                                 uint32_t * evaluated_mask);
int mh_icp_window_optimise_relin_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                       const double * Z_R, const double * Z_t, const double g_unit[3],
                                       const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                       mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask);

/* Either chain with Hessian factors the host linearized ONCE: whatever else a fixed-lag smoother puts on a pose (a photometric
 * factor, a marginal prior with its own linearization point and a dense information matrix, a radar or odometry term), each
 * on one pose of the window.  Factor j is the quadratic model f + 2 b^T x + x^T H x in the tangent of its linearization pose
 * L (R <- R Exp(x_r), t <- t + R x_t): the convention of mh_icp_result.H_ss / b_s / f and mh_photo_result.H_bb / b_b / f, what
 * HessianFactor(key, H, -b, f) receives.  Every iteration carries it from L to the current pose T of its variable as the
 * relin chain carries a kept ICP factor: d = [Log(L.R^T T.R), L.R^T (T.t - L.t)], M = blockdiag(Jr^-1(d_r), Exp(d_r)); the
 * factor contributes M^T H M, M^T (b + H d) and the cost f + 2 b^T d + d^T H d (at d = 0 the stored H, b, f as they are) — how
 * ISAM2 treats a factor whose variable stays inside its relinearization threshold.  Per entry the system adds the pose's ICP
 * factor, then its linear factors in list order, then between terms, prior and damping; trace[].f adds the ICP factors' f,
 * the linear factors' in list order, then the between terms.  H is read as given, all 36 entries.  A pose whose ICP factor
 * is empty may carry linear factors.
 * relin: NULL (every non-empty ICP factor is evaluated in every iteration: first / last, linearize counts and association
 * state as under mh_icp_window_optimise; evaluated_mask is not written) or the thresholds of mh_icp_window_optimise_relin
 * (all of that as there).  With n_lin == 0 the call computes, bit for bit, what the respective call computes.
 * Every restriction and error rule of mh_icp_window_optimise applies; n_lin > MH_WINDOW_LINEAR_MAX, lin == NULL with
 * n_lin > 0, a pose outside 0 .. W - 1, an entry of L_R, L_t, H, b or f that is not finite: MH_ERR_INVALID_ARG, nothing
 * enqueued, the handles unchanged.  lin is copied before the call returns.  mh_icp_window_wait collects the _async form. */
#define MH_WINDOW_LINEAR_MAX 32
typedef struct mh_window_linear_factor {
  int32_t pose, reserved;          /* 0 .. W-1 */
  double L_R[9], L_t[3];           /* where H, b, f were evaluated */
  double H[36], b[6], f;
} mh_window_linear_factor;
int mh_icp_window_optimise_lin(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                               const double * Z_R, const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg,
                               const mh_icp_window_relin * relin /* NULL: evaluate every factor */,
                               const mh_window_linear_factor * lin, size_t n_lin, mh_icp_window_result * out,
                               double * trace_poses, uint32_t * evaluated_mask);
int mh_icp_window_optimise_lin_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                     const double * Z_R, const double * Z_t, const double g_unit[3],
                                     const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                     const mh_window_linear_factor * lin, size_t n_lin, mh_icp_window_result * out,
                                     double * trace_poses, uint32_t * evaluated_mask);

/* mh_icp_window_optimise_lin (relin NULL or set, n_lin 0 .. 32; has_Z / Z / cfg->between_info exactly as there) with between
 * factors on ANY pair of poses, each with its own measurement and a dense information matrix: the odometry manager's
 * BetweenFactor<Pose3> beside the IMU tie, a tie across several poses, a second tie on one pair.  Every iteration evaluates
 * edge e of the poses a < b at the current poses as the has_Z factor is evaluated: with T_ab = T_a^-1 T_b the residual
 * r = [Log(Z.R^T R_ab), Z.R^T (t_ab - Z.t)], J_a = -Ad(T_ab^-1), J_b = I; with Om = info it adds J_a^T Om J_a to the diagonal
 * block of a, Om J_a to the block in block row b, block column a (its transpose above the diagonal), Om to the diagonal
 * block of b, J_a^T Om r and Om r to the gradients of a and b, r^T Om r to the cost.  info is read as given, all 36 entries.
 * Per entry the system adds the pose's ICP factor, its linear factors in list order, the has_Z between terms in window
 * order, the edges in list order, the prior, the damping; trace[].f adds the edges' terms behind the has_Z terms, in list
 * order.  Several edges may share a pair; an edge may lie parallel to a has_Z tie, span a has_Z gap, or end on a pose whose
 * ICP factor is empty.  The system is then not block-tridiagonal: it is solved by a block L D L^T over its row profile
 * (fill stays between a row's first block and the diagonal), every pivot block factorised and tested as in the other chains,
 * followed by the same two refinement steps.  Retraction, stopping, relin decisions, masks, first / last, linearize counts and
 * association state are those of the underlying chain; a system without a positive pivot takes no step and ends the call
 * (trace[].flags bit 4).  With n_edges == 0 the call computes, bit for bit, what mh_icp_window_optimise_lin computes.
 * Everything mh_icp_window_optimise_lin refuses is refused; n_edges > MH_WINDOW_EDGE_MAX, edges == NULL with n_edges > 0,
 * pose_a < 0, pose_b >= W, pose_a >= pose_b, an entry of Z_R, Z_t or info that is not finite, info[6 r + c] != info[6 c + r]:
 * MH_ERR_INVALID_ARG, nothing enqueued, the handles unchanged.  The edge arguments are checked first, before icps and W: a call
 * with several things wrong reports the edges' error.  edges is copied before the call returns.
 * mh_icp_window_wait collects the _async form. */
#define MH_WINDOW_EDGE_MAX 32
typedef struct mh_window_edge {
  int32_t pose_a, pose_b;          /* 0 <= pose_a < pose_b <= W - 1, any distance apart */
  double Z_R[9], Z_t[3];           /* the measured T_a^-1 T_b */
  double info[36];                 /* information matrix, (rotation, translation) order, row-major, symmetric */
} mh_window_edge;
int mh_icp_window_optimise_edges(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                 const double * Z_R, const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg,
                                 const mh_icp_window_relin * relin /* NULL: evaluate every factor */,
                                 const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges, size_t n_edges,
                                 mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask);
int mh_icp_window_optimise_edges_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                       const double * Z_R, const double * Z_t, const double g_unit[3],
                                       const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                       const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges,
                                       size_t n_edges, mh_icp_window_result * out, double * trace_poses,
                                       uint32_t * evaluated_mask);

/* What a fixed-lag smoother leaves behind when the oldest pose drops out of the window: the marginal of pose 0, as ONE dense
 * Gaussian on pose 1, in the shape mh_icp_window_optimise_lin takes.  Nothing is iterated: the poses are the caller's.  The
 * call evaluates every term that touches pose 0 at R / t, in the chains' own per-entry order — the ICP factor icps[0] (one
 * K3 launch, component pass off, the launch class mh_icp_linearize chooses for that factor alone; H_ss, b_s, f after the
 * 4-DoF projection and the degeneracy quirk; nothing if the factor is empty), the linear factors with pose == 0 in list order,
 * each carried from its L to T_0 as the lin chain carries it, the has_Z[1] tie with diag(cfg->between_info), the edges with
 * (pose_a, pose_b) == (0, 1) in list order, diag(cfg->prior_info) and cfg->damping on the block of pose 0 — accumulates
 *   A00 = H_u + sum J_a^T Om J_a + prior + damping,  g0 = b_u + sum J_a^T Om r,  A10 = sum Om J_a,  A11' = sum Om,
 *   g1' = sum Om r,  c = f_u + sum r^T Om r
 * and eliminates pose 0 in a one-workgroup kernel: A00 is factorised as the chains factorise a pivot block, then
 *   H_m = A11' - A10 A00^-1 A10^T (exactly symmetric),  b_m = g1' - A10 A00^-1 g0,  f_m = c - g0^T A00^-1 g0,
 * the model f + 2 b^T x + x^T H x in the tangent of L = pose 1 as given.  Linear factors on other poses, has_Z ties and edges
 * that do not touch pose 0 and the other ICP factors contribute nothing: they stay in the window.  Of cfg the call reads
 * between_info, prior_info and damping (iters, check_every and the eps are ignored, but checked).  A00 without a positive
 * pivot: MH_OK, valid = 0, prior.H / b / f zero.
 * The caller passes the arrays it holds for mh_icp_window_optimise_edges; every argument is checked as there, the edges first.
 * Further: an edge with pose_a == 0 and pose_b > 1 (the marginal would be a joint factor on several poses): MH_ERR_UNSUPPORTED,
 * reported with the edges' errors; W < 2: MH_ERR_INVALID_ARG.  Nothing is enqueued then, the handles unchanged.
 * Only icps[0] runs K3: its association state and linearize count advance as under one mh_icp_linearize; the other factors'
 * state and counts are untouched (they are held, like the factors of any window call, until the call has been waited for).
 * The call counts as the context's one window call in flight; mh_icp_window_wait collects the _async form (*out must stay
 * valid until then). */
typedef struct mh_window_marginal {
  mh_window_linear_factor prior;   /* pose = 1 (index in THIS window), L = pose 1 as given, H_m, b_m, f_m */
  int32_t valid;                   /* 0: A00 had no positive pivot; prior.H / b / f are zero */
  int32_t n_ties;                  /* has_Z[1] plus the edges on (0, 1) */
  mh_icp_result oldest;            /* what mh_icp_linearize (components off) returns for icps[0] at pose 0 */
} mh_window_marginal;
int mh_icp_window_marginalise(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                              const double * Z_R, const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg,
                              const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges, size_t n_edges,
                              mh_window_marginal * out);
int mh_icp_window_marginalise_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                    const double * Z_R, const double * Z_t, const double g_unit[3],
                                    const mh_icp_window_config * cfg, const mh_window_linear_factor * lin, size_t n_lin,
                                    const mh_window_edge * edges, size_t n_edges, mh_window_marginal * out);

/* ONE dense Gaussian on up to four poses of the window: what eliminating the oldest pose leaves when something ties it to
 * poses beyond pose 1 (an odometry edge (0, b), b > 1, or an earlier joint marginal).  The model is f + 2 b^T x + x^T H x,
 * x the stacked tangents of the member poses at their linearization poses L, in the convention of mh_window_linear_factor
 * (rotation first, R <- R Exp(x_r), t <- t + R x_t); member m owns rows / columns 6 m .. 6 m + 5 of H (row stride 24) and b.
 *
 * mh_icp_window_optimise_joint: mh_icp_window_optimise_edges (every argument as there) with one joint factor, or none
 * (joint == NULL: the call IS mh_icp_window_optimise_edges, the same kernels, bit for bit).  Every iteration carries the joint
 * factor to the current poses as a linear factor is carried, member by member: d_i = [Log(L_i.R^T T_i.R), L_i.R^T (T_i.t - L_i.t)],
 * M_i = blockdiag(Jr^-1(d_i,r), Exp(d_i,r)); with M = blockdiag(M_i) and d stacked it contributes M^T H M, M^T (b + H d) and the
 * cost f + 2 b^T d + d^T H d (every d zero: H, b, f as they are).  Per entry the system adds the pose's ICP factor, its linear
 * factors in list order, the joint factor's block, the has_Z terms, the edges, the prior, the damping; trace[].f adds the joint
 * factor's cost behind the linear factors' costs.  The blocks between two member poses lie off the diagonal, anywhere in the
 * window: they enter the row profile of the edges call's solve.  Solve, refinement, retraction, stopping, relin decisions,
 * masks, first / last, counts and the singular path are those of mh_icp_window_optimise_edges.  With n_poses == 1 the call
 * computes, bit for bit, what mh_icp_window_optimise_edges computes with the same L, H, b, f appended as the last linear factor.
 * Refused with MH_ERR_INVALID_ARG, nothing enqueued, the handles unchanged: n_poses outside 1 .. MH_WINDOW_JOINT_POSES, poses
 * not strictly ascending or outside 0 .. W - 1, a used entry of L_R, L_t, H, b or f that is not finite, used H not symmetric.
 * The joint factor is checked behind the edges and before icps and W.  joint is copied before the call returns;
 * mh_icp_window_wait collects the _async form. */
#define MH_WINDOW_JOINT_POSES 4
typedef struct mh_window_joint_factor {
  int32_t n_poses, reserved;                 /* 1 .. MH_WINDOW_JOINT_POSES */
  int32_t pose[MH_WINDOW_JOINT_POSES];       /* strictly ascending, 0 .. W-1; entries >= n_poses ignored */
  double L_R[MH_WINDOW_JOINT_POSES * 9], L_t[MH_WINDOW_JOINT_POSES * 3];   /* linearization pose of each member */
  double H[24 * 24], b[24], f;               /* leading 6 n_poses rows/cols used, row stride 24; rest ignored on input, zero on output */
} mh_window_joint_factor;
int mh_icp_window_optimise_joint(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                 const double * Z_R, const double * Z_t, const double g_unit[3], const mh_icp_window_config * cfg,
                                 const mh_icp_window_relin * relin /* NULL: evaluate every factor */,
                                 const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges, size_t n_edges,
                                 mh_icp_window_result * out, double * trace_poses, uint32_t * evaluated_mask,
                                 const mh_window_joint_factor * joint /* NULL: none */);
int mh_icp_window_optimise_joint_async(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                       const double * Z_R, const double * Z_t, const double g_unit[3],
                                       const mh_icp_window_config * cfg, const mh_icp_window_relin * relin,
                                       const mh_window_linear_factor * lin, size_t n_lin, const mh_window_edge * edges,
                                       size_t n_edges, mh_icp_window_result * out, double * trace_poses,
                                       uint32_t * evaluated_mask, const mh_window_joint_factor * joint);

/* mh_icp_window_marginalise for a pose 0 that is tied beyond pose 1: the marginal as one joint factor on the separator
 * S = {1} + {b of every edge (0, b)} + (the poses of `joint` other than 0), sorted; pose 1 is always a member, also without a
 * tie.  Every term on pose 0 is evaluated as mh_icp_window_marginalise evaluates it, in the same order, and additionally every
 * edge (0, b) at the poses 0 and b, and the joint factor (if given: it must contain pose 0), carried to the current poses, in
 * the chains' per-entry order (behind the linear factors, in front of the has_Z tie).  With A the accumulated system over
 * {0} + S, g its gradient and c its constant:
 *   H_m = A_SS' - A_S0 A00^-1 A_S0^T (exactly symmetric),  b_m = g_S' - A_S0 A00^-1 g0,  f_m = c - g0^T A00^-1 g0,
 * in the tangents of the separator poses as given.  A00 is factorised and tested as in mh_icp_window_marginalise; without a
 * positive pivot: MH_OK, valid = 0, prior.H / b / f zero — prior.n_poses, prior.pose and prior.L_R / L_t report the separator
 * and its poses as given also then (as mh_icp_window_marginalise reports pose and L).  With no edge beyond pose 1 and joint == NULL the leading 6 x 6 / 6 / f, valid, n_ties
 * and oldest are mh_icp_window_marginalise's, bit for bit.  Every argument is checked as in mh_icp_window_optimise_joint; a
 * separator of more than MH_WINDOW_JOINT_POSES poses, and a joint factor that does not contain pose 0 (it would have to stay in
 * the window as a second joint factor, which no chain takes): MH_ERR_UNSUPPORTED; W < 2: MH_ERR_INVALID_ARG.  Only icps[0] runs
 * K3, as in mh_icp_window_marginalise; mh_icp_window_wait collects the _async form (*out must stay valid until then). */
typedef struct mh_window_joint_marginal {
  mh_window_joint_factor prior;  /* poses as indices in THIS window, L = those poses as given */
  int32_t valid, n_ties;         /* n_ties: has_Z[1] plus every edge with pose_a == 0 */
  mh_icp_result oldest;
} mh_window_joint_marginal;
int mh_icp_window_marginalise_joint(mh_icp * const * icps, size_t W, const double * R, const double * t, const int32_t * has_Z,
                                    const double * Z_R, const double * Z_t, const double g_unit[3],
                                    const mh_icp_window_config * cfg, const mh_window_linear_factor * lin, size_t n_lin,
                                    const mh_window_edge * edges, size_t n_edges, const mh_window_joint_factor * joint,
                                    mh_window_joint_marginal * out);
int mh_icp_window_marginalise_joint_async(mh_icp * const * icps, size_t W, const double * R, const double * t,
                                          const int32_t * has_Z, const double * Z_R, const double * Z_t, const double g_unit[3],
                                          const mh_icp_window_config * cfg, const mh_window_linear_factor * lin, size_t n_lin,
                                          const mh_window_edge * edges, size_t n_edges, const mh_window_joint_factor * joint,
                                          mh_window_joint_marginal * out);

/* ---- pose graph over all keyframes: close loops on the device -----------------------------------
 * The fixed-lag window takes at most MH_WINDOW_MAX poses; a loop closure ties a keyframe to one hundreds of keyframes back.
 * A pose graph holds n poses (world from keyframe: R row-major, t), relative-pose edges in the shape the window takes them
 * (mh_window_edge, unchanged: one loop measurement serves both) and a fixed flag per pose, and runs Gauss-Newton over all
 * of them as ONE chain of launches on the context's stream and one wait.  The rule:
 *
 * 1. Edge e of the poses a < b at the current poses, exactly as mh_icp_window_optimise_edges evaluates it: with
 *    T_ab = T_a^-1 T_b the residual r = [Log(Z.R^T R_ab), Z.R^T (t_ab - Z.t)], J_a = -Ad(T_ab^-1), J_b = I; with Om = info (all 36
 *    entries read as given) it adds J_a^T Om J_a to the diagonal block of a, Om J_a to the block in block row b, block column
 *    a (its transpose above the diagonal), Om to the diagonal block of b, J_a^T Om r and Om r to the gradients, r^T Om r to f.
 * 2. A fixed pose takes no step: its block row and column are the identity, its right-hand side is zero, its edges act only
 *    on their other end.  `damping` is added to every diagonal entry of the free poses.  The system is A xi = -g.
 * 3. Every sum of a pose's block row is taken over the pose's edges in edge-list order; nothing is added by atomics.
 *    f = sum_{l < 256} (sum_k c[l + 256 k]), c[e] = r^T Om r of edge e, k and l ascending: the same bits whatever the launch.
 * 4. The edges are split into near ones (pose_b - pose_a == 1) and far ones (>= 2; at most MH_PGO_FAR_MAX of them on a graph of
 *    mh_pose_graph_create, at most max_far (1 .. MH_PGO_FAR_LIMIT) on a graph of mh_pose_graph_create_wide, else
 *    MH_ERR_UNSUPPORTED).  A = T + sum_f W_f^T Om_f W_f: T block-tridiagonal (near edges, damping, the identity rows), W_f the
 *    6 x 6n matrix with J_a in block column a and I in block column b of far edge f (the block column of a fixed pose
 *    zeroed).  With Y = T^-1 [W^T | -g] and C = blockdiag(Om_f^-1) + W Y (6F x 6F) the step is xi = y - Y C^-1 W y, followed by
 *    two refinement steps whose residual is taken against A itself in twice the working precision.  T is factorised by the
 *    window chains' block L D L^T, every Om_f and C by L D L^T; nothing pivots.
 * 5. Retraction R <- R Exp(xi_r), t <- t + R xi_t.  The call stops behind a step whose largest |xi_r| over the poses is below
 *    eps_rot and whose largest |xi_t| is below eps_trans (0: never), or behind `iters` iterations.
 * 6. A pivot of T, of an Om_f or of C that is not positive: no step, the poses unchanged, trace[].flags = 4, the call ends with
 *    MH_OK and converged = 0 — the window chains' rule.  LIMIT: T must be positive definite by itself, so every run of poses
 *    joined by near edges needs a fixed pose or damping; a gap in the chain bridged only by a far edge makes A regular but T
 *    singular and ends in flag 4, as does a far edge whose info is only positive semi-definite.
 * 7. A prior p on pose i (mh_pose_graph_set_priors) has a measured pose Z (world from keyframe) and a dense symmetric info[36]
 *    = Om in (rotation, translation) order.  Its residual is d = [Log(Z.R^T R_i), Z.R^T (t_i - Z.t)] (the window chains' local
 *    coordinates of T_i around Z), its Jacobian M = blockdiag(Jr^-1(d_r), Exp(d_r)), Jr^-1 the inverse right Jacobian of SO(3)
 *    (the matrix the window chains transport a factor with).  It adds M^T Om M to the diagonal block of i, M^T Om d to the
 *    gradient and d^T Om d to f.  A prior on a fixed pose acts on nothing but f.  A pose may carry several priors.  Priors
 *    belong to T: they make T positive definite for a run of poses that has no fixed pose, as far as their info reaches.
 * 8. Every edge and every prior may carry a loss {kind, param} (mh_pose_graph_set_loss).  With s = r^T Om r, its chi^2 as
 *    mh_pose_graph_residuals / mh_pose_graph_prior_residuals report it, the term has a weight w and a cost rho:
 *      0 none                 w = 1                                       rho = s
 *      1 Huber, param k > 0   w = 1 if s <= k^2, else k / sqrt(s)         rho = s if s <= k^2, else 2 k sqrt(s) - k^2
 *      2 Cauchy, param k > 0  w = 1 / (1 + s / k^2)                       rho = k^2 log(1 + s / k^2)
 *      3 DCS, param Phi > 0   w = c^2, c = min(1, 2 Phi / (Phi + s))      rho = c^2 s + Phi (1 - c)^2
 *    (kinds 1 .. 3 read an s that is not positive as 0).  A w below 1e-12 is taken as 1e-12, so that Om_f^-1 / w of a far edge
 *    stays far from the pivot test's 1e300.  The term enters the system with w times each of its contributions of 1. and 7.;
 *    f sums rho.  WHERE w is applied: the term's blocks and gradients are formed unweighted, and every entry of them is
 *    multiplied by w, once, as one rounded product w * entry, at the point where it is added into a sum of a pose's block row
 *    or right-hand side or is read as a matrix entry (w_f Om_f is what 4. factorises and inverts for a far edge; the refinement
 *    residual reads w_f times the edge's blocks).  With w = 1 that product is the entry itself.
 * 9. Order of sums: a pose's sums run over its edges in edge-list order, then over its priors in prior-list order, then the
 *    damping.  The cost fold of 3. runs over c[0 .. E + P), c[j] = rho of term j, edges then priors.  With no prior and every
 *    kind 0, every launch does what it does without 7. - 9. and the result has the same bits.
 * 10. Marginal covariances (mh_pose_graph_covariances).  At the stored poses A is assembled exactly as an iteration of
 *    mh_pose_graph_optimise with this `damping` assembles it (1., 2., 7. - 9.), the weights w of the losses at these poses and
 *    the fixed poses' identity rows included, and Sigma = A^-1 is reported in the tangent coordinates of the retraction of
 *    5.: rotation then translation, right perturbation, translation in the keyframe's frame.  cov[36 i ..] is block (i, i),
 *    row-major; its lower triangle is computed and mirrored, so it is symmetric to the bit.  joint[144 p ..] is the 12 x 12
 *    matrix [[S_ii, S_ij], [S_ij^T, S_jj]] of pair p = (i, j), i < j: its two diagonal blocks have the bits of cov, S_ij is
 *    block row i of the columns A^-1 E_j.  Every block of a fixed pose is zero (a fixed pose is known, not unit-variance),
 *    cross blocks with a fixed pose too.  How it is computed, which defines the bits: T's factors, Y and C are taken as an
 *    iteration takes them (the same launches, up to C's factorisation).  P_i = (T^-1)_ii by the backward recursion
 *    P_{n-1} = S_{n-1}^-1, P_i = S_i^-1 + G_{i+1} P_{i+1} G_{i+1}^T on the stored block factors S_i = L_i D_i L_i^T,
 *    G_{i+1} = S_i^-1 E_{i+1}^T (S_i^-1 column by column through the factor; M = G P, then the lower triangle of S_i^-1 + M G^T,
 *    mirrored).  S_ii = P_i - U_i^T D_C^-1 U_i with U_i = L_C^-1 Y_i^T, the pose's six rows of Y forward-substituted through
 *    C's factor (row k takes -= L_C[k][j] U[j] for j ascending); entry (a, b), a >= b, subtracts (U[k][a] U[k][b]) / D_C[k]
 *    for k ascending.  A pair's columns are Z = T^-1 E_j by the sweep of 4. with a unit source, X = Z - Y C^-1 W Z, then the
 *    chains' two refinement steps against A in twice the working precision, each column by itself.  With no far edge the
 *    correction terms are absent.  A pair's result does not depend on which other pairs are in the call, cov does not depend
 *    on `pairs`, and every output has the same bits on every repeat.  The call moves neither poses nor edges nor priors nor
 *    losses: a mh_pose_graph_optimise after it has the bits it has without it.  A pivot of T, of an Om_f or of C that is not
 *    positive (6.): info->flags = 4, no output byte is written, the return is MH_OK.  LIMIT, as in 6.: T must be positive
 *    definite by itself, and a run of poses anchored by damping alone has a T^-1 of size 1 / damping from which the
 *    correction subtracts almost all of it: the digits lost are log10 of (1 / damping) / |Sigma|.  Anchor a run with a fixed
 *    pose or a prior where its covariance matters.  The diagonal blocks are not refined (a pair's cross block is): their
 *    relative error is about cond(A) x 1e-16 — 2e-7 on an open chain of 4 096 poses whose largest variance is 3e3 m^2, where
 *    the joint of two neighbours far from the anchor is no longer positive semi-definite to rounding.  One chain of launches
 *    on the context's stream and one wait.
 * 11. A wide graph (mh_pose_graph_create_wide) is a graph like any other: every call takes it.  Whenever it holds a far edge it
 *    builds, factorises and solves C in blocks over many workgroups, with the same arithmetic.  Build: entry (i, k), i >= k, of C
 *    starts as the plain graph forms it: the row of W times column k of Y in the row's order, with the Om_f^-1 entry added in
 *    front on the diagonal blocks.  Factor: for j ascending, D_j = C[j][j], under the pivot test d > 0 && d < 1e300;
 *    U[j][i] = C[i][j] and L[i][j] = C[i][j] / D_j for i > j; C[i][k] -= L[i][j] * U[j][k] for i >= k > j, the product rounded
 *    first, then subtracted.  Solve: u[i] -= L[i][j] * u[j], j ascending; u[j] /= D_j; u[i] -= L[j][i] * u[j], j descending.
 *    Apply: s -= Y[row][c] * u[c], c ascending.  Every entry's operations therefore come in an order of their own, and any
 *    schedule that keeps that order per entry gives the same bits, whether blocked, tiled or spread over any number of
 *    workgroups.  A wide graph's result has the bits the unblocked phases give; on a graph of at most MH_PGO_FAR_MAX far edges
 *    it therefore has the bits of a plain graph.  No FMA contraction, no MFMA, no floating-point atomics, no sums across lanes.
 *    mh_pose_graph_covariances on a graph that holds more than MH_PGO_FAR_MAX far edges: MH_ERR_UNSUPPORTED, nothing written;
 *    on a wide graph that holds at most that many it gives the plain graph's bits.  An allocation that fails is an error of
 *    mh_pose_graph_create_wide with nothing kept: Y of a 4 096 x 512 graph is 604 MB, its C 75 MB.
 *
 * mh_pose_graph_set_poses copies n poses (1 .. max_poses); with an n other than the last one it also drops the edges, the
 * fixed flags, the priors and the losses.  mh_pose_graph_set_fixed: n flags (NULL: none fixed).  mh_pose_graph_set_edges replaces the edge list (n_edges
 * 0 .. max_edges; copied before the call returns) and drops the edges' losses.  mh_pose_graph_set_priors replaces the prior
 * list (0 .. max_poses entries, copied) and drops the priors' losses.  mh_pose_graph_set_loss replaces both lists of losses:
 * `edges` has one entry per edge, `priors` one per prior, each in list order; NULL: no loss on any of them.  mh_pose_graph_get_poses: the poses as the last call left them; capacity in
 * poses, *n_out (may be NULL) the count; R and t may each be NULL.  mh_pose_graph_residuals evaluates every edge at the stored
 * poses and moves nothing: r[6 E] the residuals, chi2[E] = r^T Om r per edge — what a caller needs to reject a false loop
 * before accepting it — and *f their sum in the order of 3.; each may be NULL.  mh_pose_graph_optimise: cfg->iters iterations
 * are queued, or check_every at a time with a look at the chain's stop word in between (the result does not depend on it);
 * launches behind a stopped iteration return at once.  With losses trace[].f is the sum of rho.  mh_pose_graph_prior_residuals
 * (d[6 P], chi2[P] = d^T Om d) and mh_pose_graph_weights (w_edges[E], w_priors[P], *f the sum of rho in the order of 9.) evaluate
 * at the stored poses and move nothing; each output may be NULL.  mh_pose_graph_residuals keeps reporting the edges' chi^2 and
 * their plain sum, whatever the losses.  trace_poses: NULL, or iters x n x 12 doubles the caller owns — the
 * poses (R, then t) behind every executed step; rows of iterations that were not executed are left untouched.
 *
 * Refusals, each with nothing enqueued and the graph unchanged — MH_ERR_INVALID_ARG: a NULL argument; max_poses outside
 * 1 .. MH_PGO_MAX_POSES, max_edges above MH_PGO_MAX_EDGES; n outside 1 .. max_poses; a pose entry that is not finite; a call
 * that needs poses before any were set; n_edges above max_edges; pose_a < 0, pose_a >= pose_b, pose_b >= n; an entry of Z_R,
 * Z_t or info that is not finite; info[6 r + c] != info[6 c + r]; capacity below n; iters outside 1 .. 64; a negative or
 * non-finite damping, eps or check_every; a prior whose pose is outside 0 .. n - 1, with an entry that is
 * not finite or an asymmetric info; more priors than max_poses; a loss kind outside 0 .. 3; a kind 1 .. 3 whose param is not
 * finite and positive; edge losses given before edges were set; mh_pose_graph_covariances with a NULL info, with cov and
 * joint both NULL, with n_pairs > 0 and pairs or joint NULL, n_pairs above MH_PGO_COV_PAIRS_MAX, a pair with i < 0, i >= j or
 * j >= n; max_far outside 1 .. MH_PGO_FAR_LIMIT.  MH_ERR_UNSUPPORTED: more than MH_PGO_FAR_MAX far edges (a wide graph: more
 * than its max_far, the message names max_far); covariances of a graph that holds more than MH_PGO_FAR_MAX.  A graph belongs to its
 * context; after mh_shutdown of the context every call but mh_pose_graph_destroy refuses it.
 * Not here: an asynchronous form, the sharded path. */
#define MH_PGO_MAX_POSES 4096
#define MH_PGO_MAX_EDGES 32768
#define MH_PGO_FAR_MAX 32 /* edges with pose_b - pose_a >= 2 */
#define MH_PGO_FAR_LIMIT 512 /* ... on a graph of mh_pose_graph_create_wide */

typedef struct mh_pose_graph mh_pose_graph;

typedef struct mh_pose_graph_config {
  int32_t iters;             /* 1 .. 64 iterations queued */
  int32_t check_every;       /* iterations queued per host look at the stop word; 0 = all at once */
  double damping;            /* >= 0, added to every diagonal entry of the free poses */
  double eps_rot, eps_trans; /* rad, m: stop when the largest step norms fall below (0 = never) */
} mh_pose_graph_config; /* 32 bytes */

typedef struct mh_pose_graph_trace {
  double f;                    /* sum of rho (r^T Om r where no loss is set) at the poses the iteration evaluated */
  double step_rot, step_trans; /* max over the poses of |xi_r|, |xi_t| */
  int32_t flags;               /* 4: a pivot was not positive (no step; the call ends here) */
  int32_t reserved;            /* 0 */
} mh_pose_graph_trace; /* 32 bytes */

typedef struct mh_pose_graph_result {
  int32_t iters, converged;
  int32_t n_poses, n_far;
  double f_first, f_last;          /* trace[0].f, trace[iters - 1].f */
  mh_pose_graph_trace trace[64];   /* one row per executed iteration */
} mh_pose_graph_result;

int mh_pose_graph_create(mh_ctx * ctx, size_t max_poses, size_t max_edges, mh_pose_graph ** out);
/* rule 11 */
int mh_pose_graph_create_wide(mh_ctx * ctx, size_t max_poses, size_t max_edges, size_t max_far /* 1 .. MH_PGO_FAR_LIMIT */, mh_pose_graph ** out);
void mh_pose_graph_destroy(mh_pose_graph * pg);
int mh_pose_graph_set_poses(mh_pose_graph * pg, const double * R /* 9 n */, const double * t /* 3 n */, size_t n);
int mh_pose_graph_set_fixed(mh_pose_graph * pg, const uint8_t * fixed /* n, NULL = none */);
int mh_pose_graph_set_edges(mh_pose_graph * pg, const mh_window_edge * edges, size_t n_edges);
int mh_pose_graph_get_poses(mh_pose_graph * pg, double * R, double * t, size_t capacity, size_t * n_out);
int mh_pose_graph_residuals(mh_pose_graph * pg, double * r /* 6 E or NULL */, double * chi2 /* E or NULL */, double * f);
int mh_pose_graph_optimise(mh_pose_graph * pg, const mh_pose_graph_config * cfg, mh_pose_graph_result * out,
                           double * trace_poses /* NULL or iters x n x 12 */);

#define MH_PGO_LOSS_NONE 0
#define MH_PGO_LOSS_HUBER 1
#define MH_PGO_LOSS_CAUCHY 2
#define MH_PGO_LOSS_DCS 3

typedef struct mh_pose_prior {
  int32_t pose, reserved;   /* 0 .. n - 1; 0 */
  double Z_R[9], Z_t[3];    /* the measured pose, world from keyframe */
  double info[36];          /* dense, symmetric, (rotation, translation) order */
} mh_pose_prior; /* 392 bytes */

typedef struct mh_pose_graph_loss {
  int32_t kind, reserved;   /* MH_PGO_LOSS_*; 0 */
  double param;             /* k (Huber, Cauchy) or Phi (DCS): finite and > 0; not read for kind 0 */
} mh_pose_graph_loss; /* 16 bytes */

int mh_pose_graph_set_priors(mh_pose_graph * pg, const mh_pose_prior * priors, size_t n /* 0 .. max_poses */);
int mh_pose_graph_set_loss(mh_pose_graph * pg, const mh_pose_graph_loss * edges /* E or NULL = none */,
                           const mh_pose_graph_loss * priors /* P or NULL = none */);
int mh_pose_graph_prior_residuals(mh_pose_graph * pg, double * d /* 6 P or NULL */, double * chi2 /* P or NULL */);
int mh_pose_graph_weights(mh_pose_graph * pg, double * w_edges /* E or NULL */, double * w_priors /* P or NULL */,
                          double * f /* sum of rho, rule order; or NULL */);

#define MH_PGO_COV_PAIRS_MAX 64

typedef struct mh_pose_graph_cov_info {
  int32_t n_poses, n_far, n_pairs;
  int32_t flags;   /* 0, or 4: a pivot of T, of an Om_f or of C was not positive (no output written) */
} mh_pose_graph_cov_info; /* 16 bytes */

/* rule 10.  The graph's far edges are within MH_PGO_FAR_MAX: a wide graph that holds more is refused (MH_ERR_UNSUPPORTED, rule 11). */
int mh_pose_graph_covariances(mh_pose_graph * pg, double damping, double * cov /* 36 n, or NULL */,
                              const int32_t * pairs /* 2 n_pairs: i, j with i < j; or NULL */, size_t n_pairs /* 0 .. MH_PGO_COV_PAIRS_MAX */,
                              double * joint /* 144 n_pairs, or NULL */, mh_pose_graph_cov_info * info);

/* ---- deskew / rigid transforms ----------------------------------------------------------------
 * Manager::deskewPoints hot loop (src/lidar/manager.cpp:496-509): every point whose t equals
 * unique_ns[g] gets p <- R_g p + t_g in float (no FMA, Eigen's evaluation order).  Rt12 = n_groups x
 * {R row-major 9 floats, t 3 floats}.  If R_B_L != NULL the Geometric::preprocess body transform
 * (src/lidar/geometric.cpp:154-161) is applied afterwards in the same kernel. In place, host buffers. */
int mh_deskew(mh_ctx * ctx, mh_point32 * pts, size_t n, const uint32_t * unique_ns,
              const float * Rt12, size_t n_groups, const float * R_B_L, const float * t_B_L);
/* p <- R p + t in float for a whole cloud (body transform geometric.cpp:154-161, world transform
 * geometric.cpp:483-490). In place, host buffers. */
int mh_transform_f32(mh_ctx * ctx, mh_point32 * pts, size_t n, const float R[9], const float t[3]);


/* ---- device-resident scan front end ------------------------------------------------------------
 * The raw cloud is uploaded once; input filter, deskew, body-frame subset and voxel down-sampler run on
 * the device and the ICP factor takes its source cloud from there (no host round trip between
 * Manager::prepareInput and the first linearize).  Every stage reproduces the reference's sequential
 * result exactly, including output order.  Call order: prepare_input -> (caller propagates the IMU over
 * unique_ns) -> deskew -> preprocess_geometric -> mh_icp_create_from_scan. */
int mh_scan_create(mh_ctx * ctx, mh_scan ** out);
void mh_scan_destroy(mh_scan * scan);
/* Manager::prepareInput<PointOuster> (lidar/manager.cpp:149-383): NaN / intensity / range / ns_max filters,
 * z offset, points_full_ (order preserved), geometric subset indices, distinct timestamps (ascending). */
int mh_scan_prepare_input(mh_scan * scan, const mh_ouster_point * raw, size_t n, const mh_input_config * cfg,
                          mh_scan_info * info);
/* Manager::prepareInput<PointT> for the reference's OTHER point types (include/mimosa/lidar/point.hpp:52-131:
 * PointOusterOdyssey, PointOusterR8, PointHesai, PointLivox, PointLivoxFromCustom2, PointVelodyne,
 * PointVelodyneAnybotics, PointRslidar) — and PointOuster itself — described by where the fields sit in a record,
 * i.e. what the sensor_msgs::PointCloud2 `fields` array says.  The per-type branches of the reference are selected by the
 * layout: time decoding (lidar/manager.cpp:285-304), reflectivity as intensity (:265-271), the Livox tag filter
 * (:256-262), whether the ring filter applies (:321-332); `transpose` (:177-203, RSAiry / VelodyneAnybotics) and
 * `organize_by_ring` (:205-241, applied when height == 1 and the layout has a ring field, as there; ring numbers must be
 * < 128, the size of the reference's tables, else MH_ERR_UNSUPPORTED) reorder the cloud first.  width * height = n.
 * The double -> uint32 time conversions follow the reference's x86-64 build (truncate to 64 bits, keep the low word). */
typedef enum mh_time_kind {
  MH_TIME_U32_NS = 0,     /* t_ns = t                                    PointOuster*, PointLivoxFromCustom2 */
  MH_TIME_F64_S_ABS = 1,  /* t_ns = (timestamp - header_ts) * 1e9        PointHesai, PointRslidar */
  MH_TIME_F64_NS_ABS = 2, /* t_ns = timestamp - header_ts * 1e9          PointLivox */
  MH_TIME_F32_S = 3       /* t_ns = time * 1e9                           PointVelodyne, PointVelodyneAnybotics */
} mh_time_kind;
typedef enum mh_ring_kind { MH_RING_NONE = 0, MH_RING_U16 = 1, MH_RING_U8 = 2, MH_RING_F32 = 3 } mh_ring_kind;
typedef struct mh_point_layout {
  uint32_t stride;                  /* bytes per record */
  uint32_t off_x, off_y, off_z;     /* float */
  uint32_t off_intensity;           /* float intensity, or uint16 reflectivity when intensity_is_u16 (PointOusterOdyssey) */
  int32_t intensity_is_u16;
  uint32_t off_time;
  int32_t time_kind;                /* mh_time_kind */
  uint32_t off_ring;
  int32_t ring_kind;                /* mh_ring_kind: the field organize_by_ring and the ring filter read */
  int32_t ring_filter;              /* 0: `ring % ring_skip_divisor` is not applied (Livox, VelodyneAnybotics, OusterOdyssey) */
  uint32_t off_tag;                 /* uint8 Livox tag */
  int32_t has_tag;                  /* keep only (tag & 0x30) == 0x10 or 0x00 */
} mh_point_layout;
int mh_scan_prepare_input_layout(mh_scan * scan, const void * raw, size_t n, const mh_point_layout * layout, uint32_t width,
                                 uint32_t height, int transpose, int organize_by_ring, double header_ts,
                                 const mh_input_config * cfg, mh_scan_info * info);
/* Same, for a raw cloud that is already in device memory (a driver that DMAs packets to the GPU, or a benchmark that
 * wants the figure without the PCIe upload): d_raw must stay valid and unchanged until the call returns. */
int mh_scan_prepare_input_device(mh_scan * scan, const mh_ouster_point * d_raw, size_t n, const mh_input_config * cfg,
                                 mh_scan_info * info);
/* Pipelined input.  mh_scan_prefetch stages the NEXT cloud while another scan is being processed: raw[n] is copied into the
 * handle's pinned staging buffer and the host-to-device copy is enqueued on a copy stream of the handle's own; it returns as
 * soon as the caller's buffer may go away.  It may be called from another host thread than the one that runs the pipeline,
 * on a handle no other call is using at that moment.  mh_scan_prepare_input_prefetched is mh_scan_prepare_input on the staged
 * cloud: the context stream waits for the copy on the device, the host does not. */
int mh_scan_prefetch(mh_scan * scan, const mh_ouster_point * raw, size_t n);
int mh_scan_prepare_input_prefetched(mh_scan * scan, const mh_input_config * cfg, mh_scan_info * info);
/* unique_ns_ (lidar/manager.cpp:344-368), ascending; the caller's IMU propagation needs them on the host. */
int mh_scan_get_unique_ns(const mh_scan * scan, uint32_t * out, size_t capacity, size_t * n_out);
/* Manager::deskewPoints' per-point part (lidar/manager.cpp:496-509) on points_full_, in place:
 * Rt12[g] = pose (row-major R, then t, float) of the group with timestamp unique_ns[g].  Rt12 is read before the call returns;
 * the kernel itself is only ENQUEUED (every later call on the handle is ordered behind it on the context's stream). */
int mh_scan_deskew(mh_scan * scan, const float * Rt12, size_t n_groups);
/* Manager::deskewPoints with its pose part (lidar/manager.cpp:455-499) on the device as well: the caller hands over the IMU
 * intervals the reference's loop walks, the device computes T_Le_Lt for every distinct timestamp (R = R_c Exp(omega dt),
 * p = p_c + v_c dt + 1/2 R_c acc dt^2 + 1/2 g dt^2, :478-489; T_Le_W * T_W_Bt * T_B_S, :493-499), casts it to float (:504-505)
 * and runs mh_scan_deskew's per-point kernel with it.  No timestamp comes back to the host, no pose table goes up. */
#define MH_MAX_IMU_SEGMENTS 64    /* a 10 Hz scan at 400 Hz IMU has 40 */
typedef struct mh_imu_segment {   /* one IMU interval (t0, t1] of manager.cpp:459-492 */
  double t0, t1;                  /* curr_itr->first, next_itr->first (global seconds) */
  double R[9], p[3], v[3];        /* curr_state: pose (R row-major) and velocity at t0 */
  double acc[3], omega[3];        /* bias-corrected measurement of curr_itr (:479-480) */
} mh_imu_segment;
/* Interval rule of the reference's while loop (:469-476): ts = header_ts + ns * 1e-9 belongs to the FIRST segment with
 * ts <= t1, dt = ts - t0 (negative before the first sample: extrapolated backwards, as there).  gravity = unit vector * |g|;
 * T_Le_W = (T_W_Be * T_B_S)^-1 (:492-496).  n_seg == 0 is the first, uninitialised cloud (:399-408): identity for every group,
 * the cloud is left as it is.  More than MH_MAX_IMU_SEGMENTS segments: MH_ERR_UNSUPPORTED.  The arguments are read before the
 * call returns; the kernels are only ENQUEUED on the context's stream, as with mh_scan_deskew.
 * A timestamp later than the last segment's t1 has no pose in the reference (its flat_map ends there; the host mirror throws
 * "IMU samples end before the last point of the cloud").  The device cannot throw: the pose kernel raises a flag and writes
 * identity for every group, so no point of that cloud is moved (the per-point kernel still runs, with identity: a finite
 * coordinate keeps its value, -0.0 becomes +0.0), and the next call on the scan that waits for the device anyway
 * (mh_scan_preprocess_geometric, mh_scan_get_points, mh_scan_get_deskew_poses, mh_photo_preprocess_commit,
 * mh_photo_preprocess_scan_resident) returns MH_ERR_INVALID_ARG with that message.  The flag belongs to the prepared cloud:
 * it stays up — also across another mh_scan_deskew_imu with a longer buffer — until the next mh_scan_prepare_input*. */
int mh_scan_deskew_imu(mh_scan * scan, const mh_imu_segment * seg, size_t n_seg, double header_ts, const double gravity[3],
                       const double R_Le_W[9], const double t_Le_W[3], const double R_B_S[9], const double t_B_S[3]);
/* interpolated_map_T_Le_Lt_ (lidar/manager.cpp:390-405, :501-503) as mh_scan_deskew_imu left it on the device: 12 doubles per
 * distinct timestamp (R row-major, then t), in the order of mh_scan_get_unique_ns.  T_Le_Lt == NULL: only *n_out. */
int mh_scan_get_deskew_poses(const mh_scan * scan, double * T_Le_Lt, size_t capacity, size_t * n_out);
/* Geometric::preprocess (geometric.cpp:128-183): Be_cloud_ = R_B_L * points_full_[geometric idx] + t_B_L
 * (f32), then Geometric::downsample (geometric.cpp:55-126) into sm_Be_cloud_ds_.  max_points_per_voxel <= 20
 * (the reference passes the literal 20). */
int mh_scan_preprocess_geometric(mh_scan * scan, const float R_B_L[9], const float t_B_L[3], double leaf_size,
                                 int max_points_per_voxel, double min_dist_in_voxel, mh_scan_info * info);
/* Copies a stage's cloud to the host.  which: 0 points_full_, 1 Be_cloud_, 2 sm_Be_cloud_ds_. */
int mh_scan_get_points(const mh_scan * scan, int which, mh_point32 * out, size_t capacity, size_t * n_out);
/* The DEVICE address of a stage's cloud (which as above; valid until the scan object is prepared again or destroyed) for callers
 * that hand it on without a copy — mh_shard_icp_create(points_on_device = 1) on a rank's share of sm_Be_cloud_ds_,
 * mh_map_insert_device.  No reference counterpart (the reference's clouds are host members of Manager / Geometric). */
int mh_scan_device_points(const mh_scan * scan, int which, const mh_point32 ** d_points, size_t * n_out);
/* geometric_point_idxs_ (indices into points_full_) / the indices into Be_cloud_ that the down-sampler kept. */
int mh_scan_get_indices(const mh_scan * scan, int which, uint32_t * out, size_t capacity, size_t * n_out);
/* ICPFactor ctor (geometric_factor.hpp:119-142) with sm_Be_cloud_ds_ taken from the device. */
int mh_icp_create_from_scan(mh_ctx * ctx, mh_map * map, const mh_scan * scan, const mh_reg_config * cfg,
                            int is_binary, mh_icp ** out);


/* ---- photometric path: lidar::Photometric + PhotometricFactor ---------------------------------------
 * replaces include/mimosa/lidar/photometric.hpp:22-86 (class Photometric), src/lidar/photometric.cpp,
 * include/mimosa/lidar/photometric_factor.hpp:22-357 and src/lidar/photometric_utils.cpp.
 * An mh_photo is one Photometric instance: configuration, the current Frame (device-resident images, yaw table,
 * proj_idx, pose table — photometric_utils.hpp:42-92) and the tracked features (map_Le_features_).  Frames are
 * reference-counted like the reference's shared_ptr<Frame>: a factor keeps the frame it was built on. */
typedef struct mh_photo mh_photo;
typedef struct mh_photo_factor mh_photo_factor;

/* lidar::PhotometricConfig, include/mimosa/lidar/photometric_config.hpp:15-87: the fields the arithmetic reads.
 * Arrays are copied by mh_photo_create.  The derived parameters fx, fy, cx, beam_offset_m
 * (src/lidar/photometric_config.cpp:98-110) are computed by the library. */
typedef struct mh_photo_config {
  int32_t rows, cols;                   /* sensor/lidar_data_format: pixels_per_column, columns_per_frame */
  int32_t destagger;
  const int32_t * pixel_shift_by_row;   /* rows entries */
  const float * beam_altitude_angles;   /* rows entries, degrees, descending */
  float range_min, range_max;
  int32_t erosion_buffer, patch_size, margin_size;
  float intensity_scale, intensity_gamma;
  int32_t remove_lines, filter_brightness, gaussian_blur, gaussian_blur_size; /* gaussian_blur_size: 3 supported */
  float gradient_threshold, max_dist_from_mean, max_dist_from_plane;
  int32_t nma_radius;
  int32_t num_features_detect;
  float occlusion_range_diff_threshold;
  int32_t max_feature_life_time;
  const double * high_pass_fir;         /* column kernel of removeLines (photometric.cpp:322-327) */
  int32_t n_high_pass;
  const double * low_pass_fir;          /* row kernel */
  int32_t n_low_pass;
  int32_t brightness_window_size[2];    /* cv::Size(width, height) */
  float lidar_origin_to_beam_origin_mm;
  int32_t rotate_patch_to_align_with_gradient; /* photometric.cpp:659-684: new features sample the pattern rotated into their edge frame */
  const int32_t * patch_offsets;        /* edgelet_patch_offsets: n_patch_offsets pairs (du, dv); <= 64 */
  int32_t n_patch_offsets;
  int32_t use_robust_cost_function;
  int32_t robust_cost_function;         /* 0 "huber", 1 "gemanmcclure" */
  double robust_cost_function_parameter, error_scale, max_error, sigma;
  double T_B_L_R[9], T_B_L_t[3];        /* lidar/T_B_S */
  const uint8_t * static_mask;          /* rows * cols, 0 = invalid, or NULL (static_mask_path == "") */
} mh_photo_config;

/* PhotometricFactor::RejectStatus, photometric_factor.hpp:36-47 */
typedef enum mh_photo_status {
  MH_PHOTO_UNPROCESSED = 0,
  MH_PHOTO_POINT_PROJECT_UNDISTORTED = 1,
  MH_PHOTO_POINT_RANGE = 2,
  MH_PHOTO_POINT_PROJECT = 3,
  MH_PHOTO_POINT_MASK = 4,
  MH_PHOTO_POINT_MASK_MARGIN = 5,
  MH_PHOTO_POINT_RANGE_DIFF = 6,
  MH_PHOTO_MAX_ERROR = 7,
  MH_PHOTO_VALID = 8
} mh_photo_status;

/* Feature, include/mimosa/lidar/photometric_utils.hpp:25-40 (per-point arrays travel separately) */
typedef struct mh_photo_feature {
  uint32_t id;
  int32_t life_time;
  int32_t n_points;
  int32_t pad;
  double center[2];
  double normal[3];
  double mean_intensity, sigma_intensity;
} mh_photo_feature;

/* What gtsam::HessianFactor receives from PhotometricFactor::linearize (photometric_factor.hpp:332-353):
 * unary HessianFactor(key, H_bb, -b_b, f); binary HessianFactor(key_b, key_a, H_bb, H_ba, -b_b, H_aa, -b_a, f). */
typedef struct mh_photo_result {
  double H_bb[36], H_ba[36], H_aa[36];
  double b_b[6], b_a[6];
  double f;
  double loc_trans_final[3], loc_rot_final[3], eigvec_trans[9], eigvec_rot[9]; /* getLocalizabilities :51-59 (unary) */
  int32_t status_hist[9];
  int32_t n_exceptions; /* features at which the reference would have THROWN (project(): invalid x coordinate,
                           photometric_utils.cpp:90-97; interpolated_map_T_Le_Lt.at()); reported as
                           PointProjectUndistorted, the host mirror turns a non-zero count into the exception */
  float gpu_ms;         /* kernel time of this call, -1 unless mh_set_profiling is on */
} mh_photo_result;

int mh_photo_create(mh_ctx * ctx, const mh_photo_config * cfg, mh_photo ** out); /* ctor, photometric.cpp:13-70 */
void mh_photo_destroy(mh_photo * photo);
/* Photometric::preprocess (photometric.cpp:92-320): yaw table from points_raw, image formation from points_deskewed,
 * proj_idx, intensity filter chain, Sobel, mask.  points_raw[i] / points_deskewed[i] are the same measurement before /
 * after Manager::deskewPoints; the corrected intensities are written back into points_deskewed (:307-314).
 * unique_ns / T_Le_Lt = interpolated_map_T_Le_Lt_ (lidar/manager.cpp:390-405, :501-503): n_groups ascending
 * timestamps, 12 doubles each (R row-major, then t).  Replaces the current frame. */
int mh_photo_preprocess(mh_photo * photo, const mh_point32 * points_raw, mh_point32 * points_deskewed, size_t n,
                        const uint32_t * unique_ns, const double * T_Le_Lt, size_t n_groups);
/* The same on a device-resident scan (mh_scan_*): points_raw = the scan's points_full_ as they were before
 * mh_scan_deskew (the scan keeps that copy once mh_scan_keep_raw(scan, 1) was called before mh_scan_deskew),
 * points_deskewed = its points_full_ now (corrected intensities are written there). */
int mh_scan_keep_raw(mh_scan * scan, int keep);
int mh_photo_preprocess_scan(mh_photo * photo, mh_scan * scan, const double * T_Le_Lt, size_t n_groups);
/* The same in two steps, for a caller that pipelines scans: _begin ENQUEUES the frame of scan k without making it current and
 * without waiting for anything (it queues behind the scan's deskew on the device, reads the scan, does not write it) — it touches
 * none of the state mh_photo_update_map / mh_photo_detect_features use (tracked features, current frame, their scratch), so one
 * host thread may run it while another is still inside mh_photo_update_map of scan k - 1 on the same object (the only concurrent
 * pair that is allowed; both enqueue on the object's context stream); _commit (after that update has returned) waits for the
 * frame, reports what _begin's kernels found (the project() error), writes the corrected intensities into the scan's cloud —
 * `scan` must still be alive and must not have been prepared again — and makes the frame current.
 * mh_photo_preprocess_scan == _begin + _commit.  A begun frame that is never committed is dropped by the next _begin or by
 * mh_photo_destroy. */
int mh_photo_preprocess_scan_begin(mh_photo * photo, mh_scan * scan, const double * T_Le_Lt, size_t n_groups);
int mh_photo_preprocess_commit(mh_photo * photo);
/* mh_photo_preprocess_scan / _begin with interpolated_map_T_Le_Lt_ (lidar/manager.cpp:501-503) read from the table
 * mh_scan_deskew_imu left on the device: no pose table crosses PCIe.  MH_ERR_INVALID_ARG on a scan whose current cloud was not
 * deskewed by mh_scan_deskew_imu.  _begin_resident is followed by mh_photo_preprocess_commit as _begin is.  When the scan's
 * IMU buffer ended too early (see mh_scan_deskew_imu) both forms return MH_ERR_INVALID_ARG and drop the frame; the current
 * frame stays what it was.  (The blocking form has by then written corrected intensities into the scan's cloud, which every
 * waiting call on that scan reports as failed until it is prepared again.) */
int mh_photo_preprocess_scan_resident(mh_photo * photo, mh_scan * scan);
int mh_photo_preprocess_scan_begin_resident(mh_photo * photo, mh_scan * scan);
/* One image of the current frame, rows * cols elements.  which: 0 img_intensity (float), 1 img_range (float),
 * 2 img_dx (float), 3 img_dy (float), 4 img_mask (uint8), 5 img_deskewed_cloud_idx (int32), 6 yaw_angles (float),
 * 7 proj_idx (int32, x 10 per pixel), 8 gradient magnitude (uint8, photometric.cpp:536-540), 9 detection mask
 * before the per-feature circles (uint8, :524-525). */
int mh_photo_get_image(mh_photo * photo, int which, void * out, size_t capacity_bytes);
/* tracked features (map_Le_features_).  Per-point arrays: n_points entries per feature, concatenated in feature
 * order: Le_ps (3 doubles per point), intensities, psi_intensities.  Any output pointer may be NULL. */
int mh_photo_num_features(const mh_photo * photo, size_t * n_features, size_t * n_points_total);
int mh_photo_get_features(const mh_photo * photo, mh_photo_feature * features, double * Le_ps, double * intensities,
                          double * psi);
int mh_photo_set_features(mh_photo * photo, const mh_photo_feature * features, size_t n_features, const double * Le_ps,
                          const double * intensities, const double * psi);
/* Photometric::detectFeatures (photometric.cpp:516-745) on the current frame: up to num_to_detect new features are
 * appended to the tracked ones.  T_W_Be = Values[frame key]; bias_directions: n_directions x 3 (the degenerate
 * directions Manager::postDefineUpdate passes, lidar/manager.cpp:568-581).  The candidate sort (std::sort's exact result, tie order included)
 * runs on up to four host threads of its own for the duration of the call (MH_SORT_THREADS=1: the plain library call). */
int mh_photo_detect_features(mh_photo * photo, int num_to_detect, const double R_W_Be[9], const double t_W_Be[3],
                             const double * bias_directions, size_t n_directions);
/* Photometric::updateMap (photometric.cpp:396-514): feature bookkeeping from the factor's statuses (drop the
 * non-Valid ones, new centres, life_time, max_feature_life_time), then detectFeatures for the missing ones.
 * factor may be NULL (no factor was built for this frame). */
int mh_photo_update_map(mh_photo * photo, mh_photo_factor * factor, const double R_W_Be[9], const double t_W_Be[3],
                        const double * bias_directions, size_t n_directions);
/* Optional: enqueues the part of the next mh_photo_detect_features / mh_photo_update_map that depends on the current frame
 * alone (gradient magnitude, detection mask, candidate compaction, read-back of the candidate list) and returns without
 * waiting; the next detection on this frame then only waits for those copies.  Results are the same with or without it. */
int mh_photo_detect_prefetch(mh_photo * photo);
/* PhotometricFactor ctor (photometric_factor.hpp:86-124) from the current frame and the tracked features (copied).
 * VSVt: 6x6 row-major = V S V^T of Photometric::getFactors (photometric.cpp:373-394), NULL = identity; ignored for
 * the binary form. */
int mh_photo_factor_create(mh_photo * photo, const double * VSVt, int is_binary, mh_photo_factor ** out);
/* clone() (photometric_factor.hpp:120-124): member-wise copy — same frame (shared), own feature list and statuses. */
int mh_photo_factor_clone(const mh_photo_factor * factor, mh_photo_factor ** out);
void mh_photo_factor_destroy(mh_photo_factor * factor);
/* linearize(Values) (:136-355): T_b = Values[keys[0]] (the frame's pose), T_a = Values[keys[1]] for the binary
 * form (NULL otherwise).  Blocks until the result is on the host. */
int mh_photo_factor_linearize(mh_photo_factor * factor, const double R_b[9], const double t_b[3], const double * R_a,
                              const double * t_a, mh_photo_result * out);
/* The same enqueued on the context stream without waiting: the smoother can queue it next to mh_icp_linearize_batch and
 * collect both; mh_photo_factor_wait blocks and fills *out.  One call in flight per factor. */
int mh_photo_factor_linearize_async(mh_photo_factor * factor, const double R_b[9], const double t_b[3], const double * R_a,
                                    const double * t_a);
int mh_photo_factor_wait(mh_photo_factor * factor, mh_photo_result * out);
/* The largest window mh_photo_factor_linearize_batch takes in one call. */
#define MH_PHOTO_MAX_BATCH 256
/* A window of factors linearized in ONE kernel launch (the smoother re-linearizes every live photometric factor per
 * update, src/graph/manager.cpp:585-588).  Factor i is linearized at T_b = (R_b + 9 i, t_b + 3 i) and, if it is binary,
 * T_a = (R_a + 9 i, t_a + 3 i); R_a / t_a may be NULL when no factor is binary.  out: n_factors results.  Blocks.
 * - Same bits as separate calls: every factor's result (H, b, f, localizabilities, status_hist, n_exceptions) and the state
 *   it leaves (statuses, centres, the features mh_photo_update_map reads, the rows of mh_photo_factor_get_state) are
 *   bit-identical to its own mh_photo_factor_linearize at the same poses: the per-feature arithmetic is shared, the
 *   feature-order fold and the unary epilogue run per factor on the host as in a single call, and each factor has its own
 *   exception counters.
 * - The factors come from one mh_photo (or are clones of its factors): one model, one context, one stream; their frames
 *   may differ.  Unary and binary factors may share a call; a factor without features costs nothing.
 * - MH_ERR_INVALID_ARG, with no factor left in flight: n_factors 0 or above MH_PHOTO_MAX_BATCH, a NULL array or factor,
 *   factors of different mh_photo objects, the same factor twice, a factor with a call in flight, a binary factor
 *   without R_a / t_a.
 * - gpu_ms (profiling on) is the kernel time of the whole launch, in every factor's result. */
int mh_photo_factor_linearize_batch(mh_photo_factor * const * factors, size_t n_factors, const double * R_b, const double * t_b,
                                    const double * R_a, const double * t_a, mh_photo_result * out);
/* The same enqueued without waiting; each factor is then collected with mh_photo_factor_wait, in any order.  Destroying a
 * member while the launch is in flight waits for the launch; the other members can still be collected. */
int mh_photo_factor_linearize_batch_async(mh_photo_factor * const * factors, size_t n_factors, const double * R_b,
                                          const double * t_b, const double * R_a, const double * t_a);
/* getStatuses / getFeatures().center after the last linearize; rows (optional, parity tooling): per feature and
 * patch point {whitened residual, J_b[6], valid} = 8 doubles, 64 points per feature. */
int mh_photo_factor_get_state(const mh_photo_factor * factor, int32_t * statuses, double * centers, double * rows);
size_t mh_photo_factor_size(const mh_photo_factor * factor);


/* ---- radar Doppler path: radar::Manager's front end + DopplerHessianFactor (SURVEY.md component #14) --------------------
 * replaces src/radar/manager.cpp:111-181 (Manager::preprocess), include/mimosa/radar/utils.hpp:17-69 (TargetData,
 * decodePointType), include/mimosa/radar/point.hpp (rioPoint, mmWavePoint) and include/mimosa/radar/factor.hpp:22-188
 * (DopplerHessianFactor).  The targets stay on the device from the raw cloud to the Hessian: mh_radar_prepare_input ->
 * mh_radar_factor_create_from_scan -> mh_radar_factor_linearize[_async | _batch].  What the caller supplies, as the
 * reference's constructor takes it: T_B_S (config_.base.T_B_S) and the mean gyro rate over the exposure (manager.cpp:56-75,
 * the IMU manager's job); keys are X(0), V(0), B(0) (manager.cpp:84-86).  The static / dynamic classification is not
 * computed: the reference never fills it (factor.hpp:135-138, :190-193 are commented out). */
typedef struct mh_radar_scan mh_radar_scan;
typedef struct mh_radar_factor mh_radar_factor;

/* radar::ManagerConfig, include/mimosa/radar/manager.hpp:20-33: the float fields the arithmetic reads (is_exposure_compensated
 * and frame_ms only move the timestamp, manager.cpp:34; the host mirror applies them). */
typedef struct mh_radar_config {
  float range_min, range_max;
  float threshold_azimuth_deg, threshold_elevation_deg;
  float filter_min_db;
  float noise_sigma;
} mh_radar_config;

/* radar::PType, include/mimosa/radar/utils.hpp:45-51 (Unknown has no value here: the caller has matched the fields) */
typedef enum mh_radar_kind {
  MH_RADAR_RIO = 0,                     /* rioPoint: x, y, z, snr_db, noise_db, v_doppler_mps (point.hpp:17-25) */
  MH_RADAR_MMWAVE = 1,                  /* mmWavePoint: x, y, z, intensity, velocity (point.hpp:27-32) */
  MH_RADAR_MMWAVE_DOPPLER_RESIDUAL = 2  /* recognised, but Manager::callback throws "Unsupported point type" (manager.cpp:43-54):
                                           MH_ERR_UNSUPPORTED */
} mh_radar_kind;
/* Where the fields sit in a sensor_msgs::PointCloud2 record: the radar counterpart of mh_point_layout.  Every field is a
 * float; point_step and the offsets are multiples of 4.  RIO: off_intensity = snr_db, off_velocity = v_doppler_mps. */
typedef struct mh_radar_layout {
  int32_t kind; /* mh_radar_kind */
  uint32_t point_step;
  uint32_t off_x, off_y, off_z, off_intensity, off_velocity;
} mh_radar_layout;

/* radar::TargetData, include/mimosa/radar/utils.hpp:17-41 (same field order) */
typedef struct mh_radar_target {
  double x, y, z, range, azimuth, elevation, radial_speed, intensity;
} mh_radar_target;

/* RadarManagerDebug's counts (manager.cpp:135, :81) */
typedef struct mh_radar_info {
  uint64_t n_points_in, n_points_valid;
} mh_radar_info;

/* What gtsam::HessianFactor(X, V, B, G11, G12, G13, g1, G22, G23, g2, G33, g3, f) receives from
 * DopplerHessianFactor::linearize (factor.hpp:185-186); blocks row-major: G11 6x6, G12 6x3, G13 6x6, G22 3x3, G23 3x6,
 * G33 6x6.  The translation columns of X and the accelerometer columns of B are exactly 0.0. */
typedef struct mh_radar_result {
  double G11[36], G12[18], G13[36], G22[9], G23[18], G33[36];
  double g1[6], g2[3], g3[6];
  double f;
  uint64_t n_targets;
  float gpu_ms; /* kernel time of this call (of the whole batch for mh_radar_factor_linearize_batch), -1 unless
                   mh_set_profiling is on */
} mh_radar_result;

/* The largest window mh_radar_factor_linearize_batch takes in one call. */
#define MH_RADAR_MAX_BATCH 1024

int mh_radar_scan_create(mh_ctx * ctx, mh_radar_scan ** out);
void mh_radar_scan_destroy(mh_radar_scan * scan); /* waits for a call in flight on the scan */
/* Manager::preprocess<rioPoint | mmWavePoint> (manager.cpp:111-181): raw = n host records laid out as `layout` says; the
 * rioPoint remap (x' = y, y' = -x, intensity = snr_db, velocity = v_doppler_mps), the NaN, filter_min_db, range and angle
 * gates and the order-preserving compaction into valid_targets_ run in one kernel, the targets stay on the device.  The
 * arithmetic is the reference's float arithmetic (radar_kernels.hip explains the one-ulp caveat of atan2f).
 * info (may be NULL): n_points_in, n_points_valid. */
int mh_radar_prepare_input(mh_radar_scan * scan, const void * raw, size_t n, const mh_radar_layout * layout,
                           const mh_radar_config * cfg, mh_radar_info * info);
/* valid_targets_ of the last mh_radar_prepare_input; out may be NULL to ask for the count. */
int mh_radar_get_targets(const mh_radar_scan * scan, mh_radar_target * out, size_t capacity, size_t * n_out);
/* DopplerHessianFactor ctor (factor.hpp:54-65) from a host TargetVector: targets (copied), pose_R_B = T_B_S (R row-major, t),
 * angular_velocity_B, noise_sigma (the manager passes its float config value, manager.cpp:84-86). */
int mh_radar_factor_create(mh_ctx * ctx, const mh_radar_target * targets, size_t n, const double R_B_S[9], const double t_B_S[3],
                           const double angular_velocity_B[3], double noise_sigma, mh_radar_factor ** out);
/* The same from the scan's valid_targets_, device to device (the scan may be prepared again or destroyed afterwards). */
int mh_radar_factor_create_from_scan(const mh_radar_scan * scan, const double R_B_S[9], const double t_B_S[3],
                                     const double angular_velocity_B[3], double noise_sigma, mh_radar_factor ** out);
/* clone() (factor.hpp:69-73): a copy with its own targets. */
int mh_radar_factor_clone(const mh_radar_factor * factor, mh_radar_factor ** out);
void mh_radar_factor_destroy(mh_radar_factor * factor); /* waits for a call in flight */
size_t mh_radar_factor_size(const mh_radar_factor * factor); /* targets_.size() */
/* linearize(Values) (factor.hpp:98-188): R_W_B = rotation of Values[X] (its translation is not read), v_W = Values[V],
 * bias_gyro = Values[B].gyroscope().  Blocks until the result is on the host.  No targets: all zeros. */
int mh_radar_factor_linearize(mh_radar_factor * factor, const double R_W_B[9], const double v_W[3], const double bias_gyro[3],
                              mh_radar_result * out);
/* The same enqueued on the context stream without waiting (next to mh_icp_linearize_batch / mh_photo_factor_linearize_async);
 * mh_radar_factor_wait blocks and fills *out.  One call in flight per factor. */
int mh_radar_factor_linearize_async(mh_radar_factor * factor, const double R_W_B[9], const double v_W[3], const double bias_gyro[3]);
int mh_radar_factor_wait(mh_radar_factor * factor, mh_radar_result * out);
/* Every live radar factor of the window re-linearized in ONE kernel launch (graph::Manager re-linearizes each of them per
 * update).  All factors on one context, none with a call in flight, 1 <= n_factors <= MH_RADAR_MAX_BATCH, else
 * MH_ERR_INVALID_ARG.  Arrays are n_factors long: R_W_B[9 n], v_W[3 n], bias_gyro[3 n], out[n].  A factor's result is
 * bit-identical to its own mh_radar_factor_linearize.  Blocks. */
int mh_radar_factor_linearize_batch(mh_radar_factor * const * factors, size_t n_factors, const double * R_W_B, const double * v_W,
                                    const double * bias_gyro, mh_radar_result * out);
/* Parity tooling: per target at the state of the last linearize, e_whitened = e / noise_sigma before the robust weight
 * (factor.hpp:157-160) and weight (:162-164); either pointer may be NULL.  MH_ERR_INVALID_ARG before the first linearize. */
int mh_radar_factor_get_residuals(const mh_radar_factor * factor, double * e_whitened, double * weight);


/* ---- map sharded across GPUs (BASELINE configs[2]): what both the library's own exchange (below) and a
 * framework that owns the stream need ------------------------------------------------------------------------------------
 * No reference counterpart: the reference is single-process.  The map is partitioned into shard blocks of 2^block_log2 voxels
 * per axis; block (bx, by, bz) = voxel coordinates >> block_log2 is owned by rank (bx + A[world] by + B[world] bz) mod world, a
 * lattice colouring of the block grid (neighbouring blocks never share a rank; tools/lattice_table.py derives the two tables;
 * rounds 3-4 used the reference's XORVector3iHash, include/mimosa/lidar/utils.hpp:228-238, which put neighbouring heavy blocks
 * on one rank at random).  A caller that partitions points itself asks mh_shard_owner_of_block instead of re-implementing the
 * rule.  Every rank also stores the one-voxel halo of its blocks, so a query on the owner of its centre voxel finds all
 * 1/7/19/27 neighbour voxels locally.  (ABI version 1 also exported a caller-driven form of the exchange — mh_icp_shard_plan / _pack /
 * _unpack, mh_icp_linearize_begin[_device] / _finish[_device], mh_icp_global_epilogue — with the collectives in the caller's
 * hands; version 2 keeps ONE implementation, the native one below.) */
/* The owner function: rank (0 .. world - 1) of shard block (bx, by, bz); -1 if world is outside 1 .. 64. */
int mh_shard_owner_of_block(int bx, int by, int bz, int world);
/* A context on an existing HIP stream (not owned): kernels, the caller's collectives and its tensor ops are ordered by it. */
int mh_init_on_stream(int device, void * hip_stream, mh_ctx ** out);
/* This rank's share of IncrementalVoxelMapPCL::insert: of the batch (identical on every rank) the points of owned shard
 * blocks plus their one-voxel halo are inserted, in the original order. */
int mh_map_insert_shard(mh_map * map, const float * xyz, size_t n, size_t stride_floats, int world, int rank, int block_log2);
/* The same for the resident scan's Be_cloud_ with Geometric::updateMap's f32 world transform (geometric.cpp:483-495) applied
 * first: mh_map_insert_from_scan for ONE RANK's shard — transform, shard filter and insert on the device, nothing crosses PCIe. */
int mh_map_insert_shard_from_scan(mh_map * map, const mh_scan * scan, const float R_W_Be[9], const float t_W_Be[3], int world, int rank, int block_log2);
/* ICPFactor ctor (geometric_factor.hpp:119-142) from a cloud that is already on the device; the point order is kept. */
int mh_icp_create_from_device(mh_ctx * ctx, mh_map * map, const mh_point32 * d_points, size_t n, const mh_reg_config * cfg,
                              int is_binary, mh_icp ** out);
/* ---- native map-sharded factor: the exchange inside the library (RCCL over xGMI) ------------------------------------
 * No reference counterpart (the reference is single-process): what it must preserve is that the sharded factor equals
 * ICPFactor::linearize (include/mimosa/lidar/geometric_factor.hpp:231-562) point for point.  Same partition as above
 * (shard blocks by the lattice owner function, mh_shard_owner_of_block; one-voxel halo stored by mh_map_insert_shard).
 * One process per GPU; a linearize is ONE chain of enqueues — route kernels, ncclAllToAll of fixed-size per-peer segments
 * [count | records], append, K3, ncclAllReduce of the Hessian sums, (K4 + ncclAllReduce when the components are on), publish —
 * and one wait at its end: no count ever crosses the host, the factor's slot count lives on the device.  A segment that
 * was too small (every rank reads the same maxima from the all-reduce vector) makes every rank repeat the call with larger
 * segments.  With world == 1 and force_collectives == 0 the call is mh_icp_linearize.  librccl is resolved at run time
 * (dlopen; a copy already in the process, e.g. PyTorch's, is used; MH_RCCL_LIB overrides). */
typedef struct mh_shard_comm mh_shard_comm;
typedef struct mh_shard_icp mh_shard_icp;
#define MH_SHARD_UNIQUE_ID_BYTES 128
typedef struct mh_shard_config {
  int32_t block_log2;        /* shard blocks of 2^block_log2 voxels per axis (the map must have been built with the same value) */
  int32_t force_collectives; /* run the full exchange protocol even with one rank (tests, overhead measurement) */
} mh_shard_config;
typedef struct mh_shard_stats {
  uint64_t n_live, n_slots, slot_capacity, n_total; /* points held; slots in use incl. tombstones; capacity; points of all ranks */
  uint32_t segment_records;   /* per-peer segment capacity the next call will use */
  uint32_t last_max_movers;   /* max over ranks and destinations of the points that wanted to move in the last call */
  uint32_t retries_total, retries_last, compactions_total;
  uint32_t collectives_last;  /* collectives the last call entered */
  int32_t world, rank, collective, linearize_count;
} mh_shard_stats;
/* ncclGetUniqueId: one rank creates it, the caller hands it to the others (any channel: a file, MPI, torch.distributed). */
int mh_shard_unique_id(void * id128);
/* ncclCommInitRank on ctx's device; collective over all ranks. */
int mh_shard_comm_init_rccl(mh_ctx * ctx, const void * id128, int world, int rank, mh_shard_comm ** out);
/* Test transport: `world` ranks inside ONE process (one host thread per rank, all on one device); out_array[world]. */
int mh_shard_comm_init_local(int world, mh_shard_comm ** out_array);
/* Any time, before or after its factors and contexts: see the teardown rule at mh_shard_icp_destroy. */
void mh_shard_comm_destroy(mh_shard_comm * comm);
int mh_shard_comm_world(const mh_shard_comm * comm);
int mh_shard_comm_rank(const mh_shard_comm * comm);
const char * mh_shard_comm_backend(const mh_shard_comm * comm); /* "rccl" | "local" */
/* The communicator as the transport itself reports it: ranks_in_communicator = ncclCommCount (world for the local transport),
 * rccl_version = ncclGetVersion (0 for the local transport).  Either pointer may be NULL. */
int mh_shard_comm_info(const mh_shard_comm * comm, int * ranks_in_communicator, int * rccl_version);
/* ICPFactor ctor (geometric_factor.hpp:119-142) for this rank's share of the scan (any split; the first linearize routes
 * every point to the owner of its centre voxel).  points: host buffer, or device buffer when points_on_device != 0.
 * shard_map: this rank's shard (mh_map_insert_shard with the same world / rank / block_log2).  Collective. */
int mh_shard_icp_create(mh_ctx * ctx, mh_shard_comm * comm, mh_map * shard_map, const mh_point32 * points, size_t n_local,
                        int points_on_device, const mh_reg_config * cfg, int is_binary, const mh_shard_config * scfg, mh_shard_icp ** out);
/* ICPFactor::linearize of the WHOLE scan against the WHOLE map: every rank gets the same global result (H, b, f,
 * localizabilities, degeneracy info; 4-DoF / degeneracy projection applied once, on the global sums).  Collective; blocks. */
int mh_shard_icp_linearize(mh_shard_icp * icp, const double R_src[9], const double t_src[3], const double * R_tgt,
                           const double * t_tgt, const double g_unit[3], mh_icp_result * out);
/* Throughput forms.  The reference's second caller re-linearizes EVERY live ICPFactor per smoother update
 * (src/graph/manager.cpp:585-588); the unsharded path answers that with mh_icp_linearize_async / _batch, these are the
 * sharded counterparts.  A protocol ROUND carries any number of factors of one communicator and context: their movers
 * interleaved per peer in ONE ncclAllToAll, one route / append / K3b (/ K4b) / publish launch each, ONE ncclAllReduce of
 * n_factors x 168 doubles (+ one of n_factors x 16 when a factor's components are on).  _async / _batch_async only enqueue
 * (up to 32 rounds in flight per communicator; a further one first completes the oldest); mh_shard_icp_wait completes
 * every round in flight on the factor's communicator, in order, and fills their results — `out` must stay valid until
 * then.  All of them are collective: every rank issues the same sequence of calls.  A call whose movers did not fit the
 * per-peer segments is repeated (larger segments, same pose) at the next wait, or when its round leaves the ring — and
 * the calls of that factor enqueued behind it are repeated behind its repeat, so results and association cache end as
 * if the calls had run one after the other (the k-NN counters of repeated calls are statistics: a point may be counted
 * by the attempt and by the repeat).
 * Arrays are n_factors long: R_src[9 n], t_src[3 n], R_tgt / t_tgt (NULL without binary factors), g_unit[3 n], out[n]. */
int mh_shard_icp_linearize_async(mh_shard_icp * icp, const double R_src[9], const double t_src[3], const double * R_tgt,
                                 const double * t_tgt, const double g_unit[3], mh_icp_result * out);
int mh_shard_icp_linearize_batch(mh_shard_icp * const * icps, size_t n_factors, const double * R_src, const double * t_src,
                                 const double * R_tgt, const double * t_tgt, const double * g_unit, mh_icp_result * out); /* blocks */
int mh_shard_icp_linearize_batch_async(mh_shard_icp * const * icps, size_t n_factors, const double * R_src, const double * t_src,
                                       const double * R_tgt, const double * t_tgt, const double * g_unit, mh_icp_result * out);
int mh_shard_icp_wait(mh_shard_icp * icp);
int mh_shard_icp_reset(mh_shard_icp * icp);                       /* as mh_icp_reset; points stay where they are; stream-ordered */
int mh_shard_icp_set_components(mh_shard_icp * icp, int enabled); /* as mh_icp_set_components; must agree on all ranks */
/* Per-point state of the points this rank holds now (origin = first rank << 32 | index there); n_out alone may be asked for. */
int mh_shard_icp_get_state(mh_shard_icp * icp, uint64_t * origin, int32_t * status, double * means, double * normals,
                           size_t capacity, size_t * n_out);
int mh_shard_icp_stats(const mh_shard_icp * icp, mh_shard_stats * out);
/* Teardown rule.  A context (mh_shutdown), a communicator (mh_shard_comm_destroy) and a sharded factor (mh_shard_icp_destroy)
 * may be torn down in any order.
 * - A sharded factor whose context was shut down gave its device memory back in mh_shutdown; afterwards it can only be
 *   destroyed and asked for mh_shard_icp_stats, every other call fails ("the factor's context was shut down").
 * - A sharded factor whose communicator was destroyed can no longer linearize or wait ("the factor's communicator was
 *   destroyed"); it is to be destroyed, mh_shard_icp_stats still answers.  With both gone, the context's message is the one.
 * - A communicator whose context was shut down lets go of it; its next factor's context takes its place.
 * - The rounds in flight of a communicator, and the calls waiting to be repeated, are dropped when the context they run on
 *   is shut down or the communicator is destroyed: their factors' results are never filled, and the factors can only be
 *   destroyed. */
void mh_shard_icp_destroy(mh_shard_icp * icp);

/* ---- keyframe cloud store, and the map rebuilt at corrected poses -------------------------------------------------------
 * No reference counterpart: the reference never moves a keyframe once it is in the map.  With mh_place_* (find a revisit),
 * mh_icp_relocalise* (measure it) and mh_pose_graph_* (correct every keyframe pose) a caller has corrected poses and a map whose
 * points still sit where the drifted poses put them.  The store keeps every keyframe's cloud on the device; the rebuild makes
 * the map those clouds give at any poses.
 *
 * 1. The store holds up to capacity_keyframes clouds (1 .. 65 536) and capacity_points points in total (>= 1), both fixed at
 *    creation.  An entry is a cloud in its own frame — the body frame for what Geometric::updateMap inserts — and an int64 tag of
 *    the caller's.  It holds no pose: poses live with the caller or the pose graph, and move.  The clouds are packed float4
 *    (x, y, z, 1) in one device arena; the offset table is kept on the host and on the device.  A cloud of 0 points is a valid
 *    entry.  A store belongs to its context and works on that context's stream; after mh_shutdown of the context every call but
 *    mh_keyframes_destroy refuses it.
 *    Refusals, each with MH_ERR_INVALID_ARG and the store as it was: a NULL argument; a full store, in keyframes or in points;
 *    stride_floats < 3; `which` outside 0 .. 1; a scan without that stage or of another context; a NULL cloud with n > 0; an
 *    index out of range; capacities outside their ranges. */
typedef struct mh_keyframes mh_keyframes;

typedef struct mh_keyframes_config {
  int32_t capacity_keyframes; /* 1 .. 65 536 */
  int32_t reserved;           /* 0 */
  int64_t capacity_points;    /* >= 1, all entries together */
} mh_keyframes_config; /* 16 bytes */

typedef struct mh_keyframes_info {
  int64_t keyframes;
  int64_t points;
  int64_t capacity_keyframes;
  int64_t capacity_points;
  int64_t device_bytes;       /* the arena and the offset table */
} mh_keyframes_info; /* 40 bytes */

int mh_keyframes_create(mh_ctx * ctx, const mh_keyframes_config * cfg, mh_keyframes ** out);
void mh_keyframes_destroy(mh_keyframes * kf);
/* entries in the store; 0 for NULL or a store whose context was shut down */
size_t mh_keyframes_size(const mh_keyframes * kf);
int mh_keyframes_get_info(const mh_keyframes * kf, mh_keyframes_info * out);
/* Append n host points, `stride_floats` floats apart, under `tag`; *index (may be NULL) receives the entry's index.  Synchronous. */
int mh_keyframes_add(mh_keyframes * kf, const float * xyz, size_t n, size_t stride_floats, int64_t tag, int32_t * index);
/* The same for points that are already on the store's device (d_points: device pointer), as mh_map_insert_device takes them. */
int mh_keyframes_add_device(mh_keyframes * kf, const void * d_points, size_t n, size_t stride_floats, int64_t tag, int32_t * index);
/* The same straight from a device-resident scan; `which` as in mh_map_carve_from_scan (0: points_full_, 1: Be_cloud_).  Device to
 * device on the context's stream; waits for nothing. */
int mh_keyframes_add_from_scan(mh_keyframes * kf, const mh_scan * scan, int which, int64_t tag, int32_t * index);
/* Read entry `index` back as packed xyz: at most capacity_points points into xyz (NULL: only the count), *n_out = the entry's
 * size, *tag its tag (either may be NULL). */
int mh_keyframes_get(mh_keyframes * kf, int32_t index, float * xyz, size_t capacity_points, size_t * n_out, int64_t * tag);
/* The device address of entry `index`, 4 floats per point — what mh_map_insert_device(..., stride_floats = 4, ...) takes — and its
 * size.  Valid until the store is destroyed (work enqueued on the store's context sees the entry's points). */
int mh_keyframes_device_points(mh_keyframes * kf, int32_t index, const float ** d_xyz1, size_t * n);

/* 2. mh_map_rebuild_from_keyframes creates a NEW map on the store's context and fills it.  Synchronous.  It reads the store and
 *    touches no existing map, so live factors keep the map they hold: the copy-then-insert discipline of Geometric::updateMap.
 *
 *    Contract.  The returned map is what mh_map_create(cfg) gives, followed by one mh_map_insert_device per listed keyframe, in
 *    list order.  Keyframe j uses the cloud cloud[order[j]], the stride 4, and the pose R_W_K + 9j, t_W_K + 3j.  The result is bit
 *    for bit the same in everything a caller can observe, now or later:
 *      - mh_map_get_cloud gives the same points in the same order.
 *      - mh_map_knn gives the same answers.
 *      - mh_icp_linearize on it gives the same result.
 *      - mh_map_get_stats gives the same values in every field but device_bytes.
 *      - Whatever later inserts, purges, previews and carves do to the two maps is the same.  That means the LRU stamps and
 *        lru_counter are the same too.
 *    The contract holds when LRU purges fall inside the sequence.  It also covers the case where a purge removes a voxel that a
 *    later keyframe creates again.
 *    The poses are f32.  The caller rounds them as toFloat12 does.  The per-point arithmetic is map_assign_kernel's expression,
 *    unchanged: (r0 x + (r1 y + r2 z)) + t, no FMA.
 *
 *    How.  The list is cut into chunks (csrc/rebuild_plan.hpp): a chunk ends where the insert count reaches a multiple of
 *    cfg->lru_clear_cycle, and before its point total would exceed chunk_points (0 = the default, 4 Mi points; a keyframe larger
 *    than the budget is a chunk of its own).  A chunk is ONE insert of its clouds laid end to end — the insert's rule couples only
 *    the points of one voxel, in input order, and numbers voxels in first-seen order — after which every voxel the chunk touched
 *    is stamped with the counter of the last keyframe of the chunk that put a point into it; the purge runs at the chunk ends
 *    that land on the cycle.  A keyframe of 0 points still counts as an insert.
 *
 *    order, n_order: the entries to insert, each at most once; NULL, 0: every entry in stored order.  R_W_K: 9 floats (row-major)
 *    and t_W_K: 3 floats per LISTED keyframe.  rc: NULL = defaults.  An empty store or an empty list gives an empty map.
 *    Refusals with MH_ERR_INVALID_ARG: a NULL kf, cfg, out or res; an invalid cfg (what mh_map_create refuses); an index out of
 *    range or listed twice; n_order > 0 with NULL order; NULL poses with a non-empty list; a pose entry that is not finite; chunk_points < 0; a non-zero reserved word.
 *    A point that lands as NaN or beyond +-2^20 voxels gives MH_ERR_UNSUPPORTED, as in the insert; the half-built map is released
 *    and *out stays NULL.  The store is never changed. */
typedef struct mh_map_rebuild_config {
  int64_t chunk_points; /* the point budget of a chunk; 0 = 4 Mi */
  int64_t reserved;     /* 0 */
} mh_map_rebuild_config; /* 16 bytes */

typedef struct mh_map_rebuild_result {
  int64_t keyframes;      /* keyframes inserted */
  int64_t points_offered; /* the points of their clouds */
  int64_t chunks;
  int64_t purges;         /* LRU purge passes run (the chunk ends that land on the cycle) */
  int64_t n_points;       /* of the finished map */
  int64_t n_voxels;
} mh_map_rebuild_result; /* 48 bytes */

int mh_map_rebuild_from_keyframes(mh_keyframes * kf, const mh_map_config * cfg, const int32_t * order, size_t n_order, const float * R_W_K,
                                  const float * t_W_K, const mh_map_rebuild_config * rc, mh_map ** out, mh_map_rebuild_result * res);

/* ---- diagnostics -------------------------------------------------------------------------------------------------------
 * With MH_ALLOC_CHECK=1 in the environment the device-allocation cache checks its hand-over rule (a block is re-used only
 * behind everything that was enqueued on it): freed blocks are poisoned behind their last use, verified when they are handed
 * out again.  blocks_verified / words_overwritten so far; MH_ERR_UNSUPPORTED when the check is off.  No reference counterpart. */
int mh_alloc_check_stats(unsigned long long * blocks_verified, unsigned long long * words_overwritten);

#ifdef __cplusplus
}
#endif
#endif /* MIMOSA_HIP_H */
