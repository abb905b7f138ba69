// Drives the host-testable half of the relocalisation kernels (mimosa_amd/csrc/reloc_device.hpp, the header reloc_kernels.hip
// is built from) on the CPU for tests/test_icp_reloc_cpu.py.  stdin: commands, one after another, until the end of input:
//   select n top_k  then n pairs (n_inliers sum_sq)      -> the top_k indices, found the way the select kernel finds them:
//                                                           kRelocSelThreads lanes, their answers four at a time, those four
//                                                           at a time, then all sixteen
//   voxel k         then k values v                      -> per value: ok and the voxel of u = (v, 0.25, -0.25)
//   transform k     then k times R[9] t[3] x y z         -> q[3] per case, as 17 significant digits
//   fold n_waves n_chunks  then n_waves * n_chunks triples (n_occupied n_inliers sum_sq): every chunk's waves in wave order,
//                   then the chunks in chunk order       -> n_occupied n_inliers sum_sq
// stdout: one JSON list per command, one per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "reloc_device.hpp"

static bool rd(double & v) { return std::scanf("%lf", &v) == 1; }
static double need()
{
  double v = 0;
  if (!rd(v)) std::exit(2);
  return v;
}

static void do_select()
{
  const int n = static_cast<int>(need()), top_k = static_cast<int>(need());
  std::vector<mh::RelocScore> s(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    s[i].n_points = s[i].n_occupied = s[i].reserved = 0;
    s[i].n_inliers = static_cast<int32_t>(need());
    s[i].sum_sq = need();
  }
  constexpr int L = mh::kRelocSelThreads;
  std::vector<mh::RelocKey> key(L), key4(L / 4), key16(L / 16);
  mh::RelocKey prev = mh::reloc_no_key();
  std::printf("[");
  for (int r = 0; r < mh::kRelocMaxRefine; ++r) {
    int idx = -1;
    if (r < top_k) {
      for (int lane = 0; lane < L; ++lane) key[lane] = mh::reloc_select_lane(s.data(), n, lane, L, prev);
      for (int lane = 0; lane < L / 4; ++lane) key4[lane] = mh::reloc_best_of(key.data() + 4 * lane, 4);
      for (int lane = 0; lane < L / 16; ++lane) key16[lane] = mh::reloc_best_of(key4.data() + 4 * lane, 4);
      const mh::RelocKey w = mh::reloc_best_of(key16.data(), L / 16);
      if (w.index >= 0) prev = w;
      idx = w.index;
    }
    std::printf("%s%d", r ? ", " : "", idx);
  }
  std::printf("]\n");
}

static void do_voxel()
{
  const int k = static_cast<int>(need());
  std::printf("[");
  for (int i = 0; i < k; ++i) {
    const double u[3] = {need(), 0.25, -0.25};
    int c[3] = {12345, 12345, 12345};
    const bool ok = mh::reloc_voxel(u, c);
    std::printf("%s[%d, %d, %d, %d]", i ? ", " : "", ok ? 1 : 0, c[0], c[1], c[2]);
  }
  std::printf("]\n");
}

static void do_transform()
{
  const int k = static_cast<int>(need());
  std::printf("[");
  for (int i = 0; i < k; ++i) {
    double R[9], t[3], q[3];
    for (double & v : R) v = need();
    for (double & v : t) v = need();
    const float x = static_cast<float>(need()), y = static_cast<float>(need()), z = static_cast<float>(need());
    mh::reloc_transform(R, t, x, y, z, q);
    std::printf("%s[%.17g, %.17g, %.17g]", i ? ", " : "", q[0], q[1], q[2]);
  }
  std::printf("]\n");
}

static void do_fold()
{
  const int n_waves = static_cast<int>(need()), n_chunks = static_cast<int>(need());
  std::vector<mh::RelocPartial> chunks(static_cast<size_t>(n_chunks)), waves(static_cast<size_t>(n_waves));
  for (int c = 0; c < n_chunks; ++c) {
    for (int w = 0; w < n_waves; ++w) {
      waves[w].n_occupied = static_cast<int32_t>(need());
      waves[w].n_inliers = static_cast<int32_t>(need());
      waves[w].sum_sq = need();
    }
    chunks[c] = mh::reloc_fold_waves(waves.data(), n_waves);
  }
  const mh::RelocScore s = mh::reloc_fold_chunks(chunks.data(), n_chunks, 7);
  std::printf("[%d, %d, %d, %.17g]\n", s.n_points, s.n_occupied, s.n_inliers, s.sum_sq);
}

int main()
{
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "select"))
      do_select();
    else if (!std::strcmp(cmd, "voxel"))
      do_voxel();
    else if (!std::strcmp(cmd, "transform"))
      do_transform();
    else if (!std::strcmp(cmd, "fold"))
      do_fold();
    else
      return 3;
  }
  return 0;
}
