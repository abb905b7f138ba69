// Device-resident incremental voxel map: state and launcher declarations shared by map_kernels.hip and the C ABI.
//
// Replaces gtsam_points::iVox as used through IncrementalVoxelMapPCL (reference: include/mimosa/lidar/
// incremental_voxel_map.hpp:22-54, src/lidar/incremental_voxel_map.cpp:14-62; configuration src/lidar/geometric.cpp:23-28).
// The layout of voxel_map.hpp (buckets, packed coarse buckets, halo'd 4x4x4 block tables, block hash) is unchanged;
// what changed in round 2 is WHO maintains it: insertion, voxel / block creation, the LRU purge, get_cloud and the
// copy all run on the device, so a keyframe update moves the keyframe cloud to the device and nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "voxel_map.hpp"

namespace mh
{
constexpr int kVoxCoordBits = 21;                      // voxel / block coordinates must fit 21 bits (+-2^20 voxels)
constexpr int kVoxCoordBias = 1 << (kVoxCoordBits - 1);
constexpr uint64_t kEmptyKey = ~0ull;

#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t pack_coord_key(int x, int y, int z)
{
  const uint64_t m = (1ull << kVoxCoordBits) - 1;
  return ((static_cast<uint64_t>(x + kVoxCoordBias) & m) << (2 * kVoxCoordBits)) | ((static_cast<uint64_t>(y + kVoxCoordBias) & m) << kVoxCoordBits) |
         (static_cast<uint64_t>(z + kVoxCoordBias) & m);
}

// Counters the map kernels publish into mapped pinned host memory (read by the host after a stream synchronisation).
struct MapState
{
  uint32_t n_voxels;      // voxels in the map (creation order = iVox's flat_voxels order)
  uint32_t n_blocks;      // 4x4x4-voxel blocks with a table
  unsigned long long n_points;
  uint32_t n_segments;    // this insert: distinct voxels touched
  uint32_t n_new_voxels;  // this insert: voxels to create
  uint32_t bad_coord;     // a coordinate did not fit kVoxCoordBits
  uint32_t n_keep;        // LRU purge: voxels that survive
  uint32_t cloud_points;  // get_cloud: total points
  uint32_t preview[3];    // insert preview: points it would add / refuse as too close / refuse because their voxel is full
  unsigned long long carve[6];  // mh_map_carve*: the fields of mh_map_carve_result, in their order
};

// Everything the insert / purge kernels need to reach the map arrays.
struct MapArrays
{
  int4 * table;           // {key lo, key hi, block id, -}: 63-bit packed block coordinate, all-ones = empty
  uint32_t table_mask;
  uint32_t * cells;       // n_blocks x 216: voxel_id << 5 | count, ~0u empty
  float4 * buckets;       // n_voxels x 20
  uint32_t * qbuckets;    // n_voxels x 20, 3 x 10-bit voxel-relative
  int4 * vox;             // n_voxels: {cx, cy, cz, count}
  unsigned long long * lru;  // n_voxels: lru_counter at the last insert that touched the voxel
  MapState * state;       // device-visible (mapped pinned) counters
};

#if defined(__HIPCC__)
// block id of block (bx, by, bz), or -1.  The table's load is <= 0.5, so an empty slot ends every probe.
__device__ __forceinline__ int find_block(const MapArrays & m, int bx, int by, int bz)
{
  const uint64_t key = pack_coord_key(bx, by, bz);
  uint32_t h = block_hash(bx, by, bz) & m.table_mask;
  for (;;) {
    const int4 e = m.table[h];
    const uint64_t k = static_cast<uint64_t>(static_cast<uint32_t>(e.x)) | (static_cast<uint64_t>(static_cast<uint32_t>(e.y)) << 32);
    if (k == kEmptyKey) return -1;
    if (k == key) return e.z;
    h = (h + 1) & m.table_mask;
  }
}

// The <= 8 blocks whose halo'd table holds voxel (cx,cy,cz): its home block and, per axis, the neighbour it touches.
// which in [0, 8): bit a selects the second block of axis a.  Returns false when that combination does not exist.
__device__ __forceinline__ bool voxel_block(int cx, int cy, int cz, int which, int & bx, int & by, int & bz)
{
  const int c[3] = {cx, cy, cz};
  int b[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int l = c[a] & (kBlockDim - 1);
    b[a] = c[a] >> kBlockLog2;
    if ((which >> a) & 1) {
      if (l == 0)
        b[a] -= 1;
      else if (l == kBlockDim - 1)
        b[a] += 1;
      else
        return false;
    }
  }
  bx = b[0];
  by = b[1];
  bz = b[2];
  return true;
}

// Geometric::updateMap's world transform (geometric.cpp:483-490): f32 R p + t, Eigen's r0 x + (r1 y + r2 z) order, no FMA (the
// including kernels are compiled with -ffp-contract=off).  The one place the expression exists: map_assign_kernel and
// map_rebuild_assign_kernel both call it.
__device__ __forceinline__ void map_world_point(const float * Rt12, float px, float py, float pz, float & x, float & y, float & z)
{
  x = (Rt12[0] * px + (Rt12[1] * py + Rt12[2] * pz)) + Rt12[9];
  y = (Rt12[3] * px + (Rt12[4] * py + Rt12[5] * pz)) + Rt12[10];
  z = (Rt12[6] * px + (Rt12[7] * py + Rt12[8] * pz)) + Rt12[11];
}

// Voxel key of an insert's point.  A NaN or a coordinate beyond the key range raises MapState::bad_coord and is filed under
// voxel (0,0,0): the grouping stays well-formed, the host rejects the batch before anything is modified.
__device__ __forceinline__ uint64_t map_point_key(float x, float y, float z, double inv_leaf, MapState * st)
{
  const int cx = fast_floor(static_cast<double>(x) * inv_leaf), cy = fast_floor(static_cast<double>(y) * inv_leaf),
            cz = fast_floor(static_cast<double>(z) * inv_leaf);
  // one voxel of margin: the blocks a voxel touches must fit the key as well
  const int lim = kVoxCoordBias - 8;
  if (cx < -lim || cx >= lim || cy < -lim || cy >= lim || cz < -lim || cz >= lim || !(x == x) || !(y == y) || !(z == z)) {
    atomicOr(&st->bad_coord, 1u);
    return pack_coord_key(0, 0, 0);
  }
  return pack_coord_key(cx, cy, cz);
}
#endif

struct InsertScratch
{
  float4 * pts;           // n: the batch as float4 (after the optional f32 transform)
  void * group;           // voxel_group.hpp scratch of the batch (map_group_bytes(n)): hash, first-seen segments, index lists
  uint32_t * seg_vid;     // n: voxel id of segment s (existing, or n_voxels + creation rank)
  uint32_t * seg_added;   // n: points the insert added to segment s
  uint32_t * blk_new;     // (n + 255) / 256: per-block counts of segments that open a new voxel
};

size_t map_group_bytes(size_t n);
size_t map_temp_bytes(size_t n);
// phase A: voxel key per point -> first-seen grouping (voxel_group.hpp, no sort) -> which voxels exist / creation ranks
// of the new ones (first-seen order = the reference's creation order).  Publishes n_segments, n_new_voxels, bad_coord.  src: n points `stride_floats` apart (device memory); Rt12 != null applies the f32 rigid
// transform p <- R p + t first (Geometric::updateMap's world transform, geometric.cpp:483-490).
hipError_t launch_map_insert_prepare(const MapArrays & m, const float * src, uint32_t n, uint32_t stride_floats, const float * Rt12,
                                     double inv_leaf, const InsertScratch & s, hipStream_t stream);
// The two halves of launch_map_insert_prepare.  A.1: the batch hash cleared, then map_assign_kernel (s.pts, the keys).  A.2 to A.4:
// grouping, lookup, creation ranks — also what follows a caller's own phase A.1 (launch_map_rebuild_assign).
hipError_t launch_map_insert_assign(const MapArrays & m, const float * src, uint32_t n, uint32_t stride_floats, const float * Rt12, double inv_leaf,
                                    const InsertScratch & s, hipStream_t stream);
hipError_t launch_map_insert_group(const MapArrays & m, uint32_t n, const InsertScratch & s, hipStream_t stream);
// ---- mh_map_rebuild_from_keyframes (rebuild_kernels.hip): a chunk of keyframes as one insert ------------------------------
struct RebuildKeyframe
{
  unsigned long long src;  // first point of the keyframe's cloud in the store's arena (float4 per point)
  float Rt12[12];          // its pose: R row-major, then t
};
// phase A.1 of a chunk: point i of the n points of kc keyframes laid end to end (rel[j] = first point of keyframe j, rel[kc] = n)
// is loaded from the arena, moved by its keyframe's pose (map_world_point) and keyed, as map_assign_kernel does for one batch.
hipError_t launch_map_rebuild_assign(const MapArrays & m, const float4 * arena, const RebuildKeyframe * kf, const uint32_t * rel, uint32_t kc,
                                     uint32_t n, double inv_leaf, const InsertScratch & s, hipStream_t stream);
// after phase C: lru[voxel of segment s] = counter_start + (the last keyframe of the chunk with a point in the segment)
hipError_t launch_map_rebuild_stamp(const MapArrays & m, const uint32_t * rel, uint32_t kc, uint32_t n, unsigned long long counter_start,
                                    const InsertScratch & s, hipStream_t stream);
// a keyframe store's entry: n points `stride_floats` apart (device memory) -> float4 (x, y, z, 1); offsets[1] = offsets[0] + n
hipError_t launch_keyframes_pack(const float * src, uint32_t n, uint32_t stride_floats, float4 * dst, unsigned long long * offsets,
                                 unsigned long long end, hipStream_t stream);
// phase B: create the new voxels (coordinates, lru) and claim their blocks in the hash table; publishes n_blocks
hipError_t launch_map_create_voxels(const MapArrays & m, uint32_t n, uint32_t n_voxels_before, unsigned long long lru_counter,
                                    const InsertScratch & s, hipStream_t stream);
// phase C: FlatContainer::add per touched voxel, one wave each; cell words, counts, lru; publishes n_voxels, n_points
hipError_t launch_map_insert_points(const MapArrays & m, uint32_t n, uint32_t n_voxels_after, uint32_t max_pts, double min_sq,
                                    double inv_leaf, unsigned long long lru_counter, const InsertScratch & s, hipStream_t stream);
// insert preview, after phase A and INSTEAD of phases B and C: phase C's rule per touched voxel on a bucket held in registers,
// nothing of the map is written.  seg_close / seg_full: n words each; outcome: n bytes (1 added, 2 too close, 3 voxel full,
// at the point's input index) or null.  Publishes MapState::preview.
hipError_t launch_map_preview_points(const MapArrays & m, uint32_t n, uint32_t n_voxels_before, uint32_t max_pts, double min_sq,
                                     const InsertScratch & s, uint32_t * seg_close, uint32_t * seg_full, uint8_t * outcome, hipStream_t stream);
// hash table of a new capacity from the block coordinates stored in the old one
hipError_t launch_map_rehash(const int4 * old_table, uint32_t old_cap, int4 * new_table, uint32_t new_cap, hipStream_t stream);
// LRU purge (iVox: voxels with lru + horizon < counter are erased, the rest keep their order): flags + count,
// then compaction into fresh arrays and a rebuild of the block structure.
hipError_t launch_map_purge_flags(const MapArrays & m, uint32_t n_voxels, unsigned long long horizon, unsigned long long lru_counter,
                                  uint32_t * keep, uint32_t * pos, void * temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_map_purge_compact(const MapArrays & src, const MapArrays & dst, uint32_t n_voxels, const uint32_t * keep,
                                    const uint32_t * pos, hipStream_t stream);
// (re)build table + cells from the voxel coordinates: claim blocks, then write every voxel's word
hipError_t launch_map_claim_blocks(const MapArrays & m, uint32_t v0, uint32_t v1, hipStream_t stream);
hipError_t launch_map_write_words(const MapArrays & m, uint32_t v0, uint32_t v1, hipStream_t stream);
// positions of the kept voxels (exclusive scan of keep) and their number (MapState::n_keep): the second half of
// launch_map_purge_flags, for callers that wrote the flags themselves
hipError_t launch_map_keep_positions(const MapArrays & m, uint32_t n_voxels, const uint32_t * keep, uint32_t * pos, void * temp, size_t temp_bytes,
                                     hipStream_t stream);
// voxel_data(): all points in voxel order.  offsets: n_voxels + 1 scratch; out: packed xyz (3 floats per point)
hipError_t launch_map_cloud(const MapArrays & m, uint32_t n_voxels, uint32_t * counts, uint32_t * offsets, float * out, size_t out_capacity_points,
                            void * temp, size_t temp_bytes, hipStream_t stream);

// ---- map carving (carve_kernels.hip; the rule: carve_device.hpp) ------------------------------------------------
struct CarveParams;
size_t carve_image_bytes(int N);  // 6 N^2 cells + the call's observation counter
// the observation image of n points `stride_floats` apart (device memory): a clear, then the 64-bit atomic-minimum splat
hipError_t launch_carve_image(const float * src, uint32_t n, uint32_t stride_floats, const CarveParams & P, void * image, hipStream_t stream);
// every map point against the image, one wave per voxel; apply: survivors compacted in their buckets, counts and cell words
// follow.  per_voxel, keep: n_voxels words each (keep = 0 for a voxel left without a point).  Publishes MapState::carve, and
// with apply MapState::n_points.
hipError_t launch_carve_test(const MapArrays & m, uint32_t n_voxels, const CarveParams & P, const void * image, double leaf, const double sensor_W[3],
                             double range_max, bool apply, uint32_t * per_voxel, uint32_t * keep, hipStream_t stream);

}  // namespace mh
