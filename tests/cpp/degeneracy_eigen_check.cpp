// Host side of the degeneracy zoo (tests/degeneracy_zoo.py, tests/test_degeneracy_zoo_cpu.py): runs the 3 x 3 solvers of math3.hpp
// and the device chains' degeneracy test of align_device.hpp, compiled for the host, on blocks read from a file, and prints what
// they return; the Python side holds every line to the multi-precision reference.  This covers the HOST branches of math3.hpp
// (1.0 / x, std::sqrt); the device branches are reached by tests/test_gpu_degeneracy_zoo.py with the same checks.
//
// usage: degeneracy_eigen_check IN OUT
// IN, one block per line, every number as a hexadecimal float:  block (0 rotation, 1 translation)  a00 .. a22 (row-major)  t0 t1 t2 t3
// OUT, one line per block:  w[3] V[9] (sym_eigen3)  accepted F[9] (sym_eigvec3_fast)  loc[3] E[9] (compute_localizability)
//                           d0 .. d3 (align_block_degenerate of the block in place in the 28 sums, at each threshold)
#include <cstdio>
#include <cstring>

#include "../../mimosa_amd/csrc/align_device.hpp"

int main(int argc, char ** argv)
{
  if (argc != 3) return 2;
  std::FILE * in = std::fopen(argv[1], "r");
  std::FILE * out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  long lines = 0;
  for (;;) {
    int block = 0;
    double A[9], t[4];
    if (std::fscanf(in, "%d", &block) != 1) break;
    bool ok = block == 0 || block == 1;
    for (int i = 0; i < 9; ++i) ok = ok && std::fscanf(in, "%la", &A[i]) == 1;
    for (int i = 0; i < 4; ++i) ok = ok && std::fscanf(in, "%la", &t[i]) == 1;
    if (!ok) return 3;
    double w[3], V[9], F[9], loc[3], E[9];
    mh::sym_eigen3(A, w, V);
    std::memset(F, 0, sizeof(F));
    const bool accepted = mh::sym_eigvec3_fast(A, F);
    mh::compute_localizability(A, loc, E);
    double sums[32];
    for (int i = 0; i < 32; ++i) sums[i] = 0.0;
    for (int r = 0; r < 3; ++r)
      for (int c = r; c < 3; ++c) sums[mh::align_ent(3 * block + r, 3 * block + c)] = A[3 * r + c];
    for (int i = 0; i < 3; ++i) std::fprintf(out, "%a ", w[i]);
    for (int i = 0; i < 9; ++i) std::fprintf(out, "%a ", V[i]);
    std::fprintf(out, "%d ", accepted ? 1 : 0);
    for (int i = 0; i < 9; ++i) std::fprintf(out, "%a ", F[i]);
    for (int i = 0; i < 3; ++i) std::fprintf(out, "%a ", loc[i]);
    for (int i = 0; i < 9; ++i) std::fprintf(out, "%a ", E[i]);
    for (int i = 0; i < 4; ++i) std::fprintf(out, "%d ", mh::align_block_degenerate(sums, block, t[i]) ? 1 : 0);
    std::fprintf(out, "\n");
    ++lines;
  }
  std::fclose(in);
  if (std::fclose(out) != 0) return 4;
  std::printf("OK %ld blocks\n", lines);
  return 0;
}
