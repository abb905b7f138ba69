// csrc/rebuild_plan.hpp under g++: the chunk plan of mh_map_rebuild_from_keyframes, for tests/test_map_rebuild_cpu.py to compare with
// tests/map_rebuild_ref.py.  Reads lines "counter0 cycle budget n size_0 ... size_{n-1}" and prints, per line, one JSON list of
// [k0, k1, points, counter_start, purge_after] per chunk.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rebuild_plan.hpp"

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint64_t counter0 = 0, cycle = 0, budget = 0;
    size_t n = 0;
    if (!(in >> counter0 >> cycle >> budget >> n) || cycle < 1 || budget < 1) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    std::vector<uint64_t> sizes(n);
    for (size_t i = 0; i < n; ++i)
      if (!(in >> sizes[i])) {
        std::fprintf(stderr, "short line: %s\n", line.c_str());
        return 2;
      }
    const std::vector<mh::RebuildChunk> plan = mh::rebuild_plan(sizes.data(), n, counter0, cycle, budget);
    std::printf("[");
    for (size_t c = 0; c < plan.size(); ++c)
      std::printf("%s[%zu, %zu, %" PRIu64 ", %" PRIu64 ", %d]", c ? ", " : "", plan[c].k0, plan[c].k1, plan[c].points, plan[c].counter_start,
                  plan[c].purge_after ? 1 : 0);
    std::printf("]\n");
  }
  return 0;
}
