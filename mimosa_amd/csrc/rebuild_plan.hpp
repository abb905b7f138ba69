// The host-side plan of mh_map_rebuild_from_keyframes: how a list of keyframes is cut into chunks, each of which is ONE insert of
// its clouds laid end to end.  Plain C++ (g++ compiles it: tests/test_map_rebuild_cpu.py compares it with tests/map_rebuild_ref.py).
//
// Keyframe j of the list is insert number counter0 + j of the map: it stamps the voxels it touches with that value, the map's
// counter is counter0 + j + 1 afterwards, and the LRU purge runs when that is a multiple of `cycle`.  One insert of several
// keyframes builds the same buckets and voxel ids as one insert each (the rule couples only the points of one voxel, in input
// order; voxels are numbered in first-seen order) as long as no purge falls between them, so:
//   - a chunk ends behind the keyframe whose insert makes the counter a multiple of `cycle` (purge_after: the purge runs there);
//   - a chunk ends in front of the keyframe with which its point total would pass `budget` (a keyframe larger than the budget is
//     a chunk of its own);
//   - a keyframe of 0 points is an insert like any other.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mh
{
struct RebuildChunk
{
  size_t k0, k1;           // keyframes [k0, k1) of the list
  uint64_t points;         // their point total
  uint64_t counter_start;  // the map's insert counter when the chunk begins = the stamp of keyframe k0
  bool purge_after;        // counter_start + (k1 - k0) is a multiple of the cycle
};

// sizes[n]: points per listed keyframe.  cycle >= 1, budget >= 1.
inline std::vector<RebuildChunk> rebuild_plan(const uint64_t * sizes, size_t n, uint64_t counter0, uint64_t cycle, uint64_t budget)
{
  std::vector<RebuildChunk> plan;
  size_t k = 0;
  while (k < n) {
    RebuildChunk c;
    c.k0 = k;
    c.points = 0;
    c.counter_start = counter0 + k;
    c.purge_after = false;
    while (k < n) {
      if (k > c.k0 && c.points + sizes[k] > budget) break;
      c.points += sizes[k];
      ++k;
      if ((counter0 + k) % cycle == 0) {
        c.purge_after = true;
        break;
      }
    }
    c.k1 = k;
    plan.push_back(c);
  }
  return plan;
}
}  // namespace mh
