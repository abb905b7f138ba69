// mimosa_amd/csrc/pose_graph_device.hpp compiled for the CPU, with priors and losses: the chain of mh_pose_graph_optimise with
// every launch a loop (pgo_iterate_host), as tests/cpp/pose_graph_step.cpp runs it without them.
// tests/test_pose_graph_robust_cpu.py feeds it the graphs of tests/pose_graph_robust_cases.py and compares with the numpy
// restatement.  Input (numbers as C hex floats), one graph per block:
//   graph N E P iters damping eps_rot eps_trans
//   N x (R[9] t[3])   N x fixed   E x (a b Z_R[9] Z_t[3] info[36] kind param)   P x (pose Z_R[9] Z_t[3] info[36] kind param)
// Output, one JSON line each: the terms at the given poses {"w", "pw", "d", "pchi2", "f"}, then per executed iteration
// {"f", "step_rot", "step_trans", "flags", "iters", "w", "pw", "poses"}, then {"iters", "converged", "n_far", "poses"}.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <iostream>
#include <string>
#include <vector>

#include "pose_graph_device.hpp"

namespace
{
bool next(std::string & tok) { return static_cast<bool>(std::cin >> tok); }
double num()
{
  std::string tok;
  if (!next(tok)) {
    std::fprintf(stderr, "pose_graph_robust_step: input ended early\n");
    std::exit(2);
  }
  return std::strtod(tok.c_str(), nullptr);
}
void put(const char * name, const double * v, size_t n, const char * tail)
{
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) std::printf("%s\"%a\"", i ? ", " : "", v[i]);
  std::printf("]%s", tail);
}
void put_poses(const mh::PgoGraph & g, const char * tail)
{
  std::printf("\"poses\": [");
  for (int i = 0; i < g.N; ++i) {
    for (int q = 0; q < 9; ++q) std::printf("%s\"%a\"", (i || q) ? ", " : "", g.R[9 * i + q]);
    for (int q = 0; q < 3; ++q) std::printf(", \"%a\"", g.t[3 * i + q]);
  }
  std::printf("]%s", tail);
}
bool loss_ok(int kind, double param) { return kind == 0 || (kind >= 1 && kind <= 3 && std::isfinite(param) && param > 0.0); }
}  // namespace

int main()
{
  std::string tok;
  while (next(tok)) {
    if (tok != "graph") {
      std::fprintf(stderr, "pose_graph_robust_step: unknown command %s\n", tok.c_str());
      return 2;
    }
    const int N = static_cast<int>(num()), E = static_cast<int>(num()), P = static_cast<int>(num()), iters = static_cast<int>(num());
    mh::PgoParams p{};
    p.damping = num();
    p.eps_rot = num();
    p.eps_trans = num();
    if (N < 1 || N > mh::kPgoMaxPoses || E < 0 || E > mh::kPgoMaxEdges || P < 0 || P > N || iters < 1 || iters > mh::kPgoMaxIters) return 2;
    size_t off[mh::kPgArrays];
    // sized to this graph exactly (the prior arrays by N, as the library sizes them by max_poses)
    const size_t bytes = mh::pgo_layout(static_cast<size_t>(N), static_cast<size_t>(E > 0 ? E : 1), off);
    std::vector<char> block(bytes, 0);
    mh::PgoGraph g{};
    mh::pgo_bind(g, block.data(), off);
    g.N = N;
    g.E = E;
    g.P = P;
    for (int i = 0; i < N; ++i) {
      for (int q = 0; q < 9; ++q) g.R[9 * i + q] = num();
      for (int q = 0; q < 3; ++q) g.t[3 * i + q] = num();
    }
    for (int i = 0; i < N; ++i) g.fixed[i] = num() != 0.0 ? 1 : 0;
    int n_far = 0;
    for (int e = 0; e < E; ++e) {
      g.ea[e] = static_cast<int>(num());
      g.eb[e] = static_cast<int>(num());
      if (g.ea[e] < 0 || g.ea[e] >= g.eb[e] || g.eb[e] >= N) return 2;
      n_far += g.eb[e] - g.ea[e] >= 2 ? 1 : 0;
      for (int q = 0; q < 9; ++q) g.ZR[9 * e + q] = num();
      for (int q = 0; q < 3; ++q) g.Zt[3 * e + q] = num();
      for (int q = 0; q < 36; ++q) g.Om[36 * e + q] = num();
      g.lkind[e] = static_cast<int>(num());
      g.lparam[e] = num();
      if (!loss_ok(g.lkind[e], g.lparam[e])) return 2;
    }
    if (n_far > mh::kPgoFarMax) return 2;
    for (int k = 0; k < P; ++k) {
      g.ppose[k] = static_cast<int>(num());
      if (g.ppose[k] < 0 || g.ppose[k] >= N) return 2;
      for (int q = 0; q < 9; ++q) g.pZR[9 * k + q] = num();
      for (int q = 0; q < 3; ++q) g.pZt[3 * k + q] = num();
      for (int q = 0; q < 36; ++q) g.pOm[36 * k + q] = num();
      g.plkind[k] = static_cast<int>(num());
      g.plparam[k] = num();
      if (!loss_ok(g.plkind[k], g.plparam[k])) return 2;
    }
    g.F = mh::pgo_index_edges(N, E, g.ea, g.eb, g.eslot, g.inc_off, g.inc, g.far);
    g.K = 6 * g.F + 1;
    mh::pgo_index_priors(N, P, g.ppose, g.pinc_off, g.pinc);

    mh::WindowSerial par;
    for (int j = 0; j < E + P; ++j) mh::pgo_term(g, j, false);
    double f = 0.0;
    mh::pgo_cost(g, &f, par);
    std::printf("{");
    put("w", g.w, static_cast<size_t>(E), ", ");
    put("pw", g.pw, static_cast<size_t>(P), ", ");
    put("d", g.pres, 6 * static_cast<size_t>(P), ", ");
    put("pchi2", g.pcz, static_cast<size_t>(P), ", ");
    std::printf("\"f\": \"%a\"}\n", f);

    double sm[114];
    for (int it = 0; it < iters && !g.st->stopped; ++it) {
      mh::pgo_iterate_host(g, p, it, nullptr, sm);
      const mh::PgoRow & row = g.rows[it];
      std::printf("{\"f\": \"%a\", \"step_rot\": \"%a\", \"step_trans\": \"%a\", \"flags\": %d, \"iters\": %d, ", row.f, row.step_rot, row.step_trans, row.flags,
                  row.iters);
      put("w", g.w, static_cast<size_t>(E), ", ");
      put("pw", g.pw, static_cast<size_t>(P), ", ");
      put_poses(g, "}\n");
    }
    std::printf("{\"iters\": %d, \"converged\": %d, \"n_far\": %d, ", g.st->iters, g.st->converged, g.F);
    put_poses(g, "}\n");
  }
  return 0;
}
