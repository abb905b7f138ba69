// mimosa_amd/csrc/pose_graph_device.hpp compiled for the CPU: the marginal covariances of mh_pose_graph_covariances with every
// launch a loop (pgo_cov_host).  tests/test_pose_graph_cov_cpu.py feeds it the graphs of tests/pose_graph_cases.py and
// tests/pose_graph_robust_cases.py and compares with the dense restatement (tests/pose_graph_cov_ref.py).
// Input (numbers as C hex floats), one graph per block:
//   graph N E P n_pairs damping
//   N x (R[9] t[3])   N x fixed   E x (a b Z_R[9] Z_t[3] info[36] kind param)   P x (pose Z_R[9] Z_t[3] info[36] kind param)
//   n_pairs x (i j)
// Output, one JSON line per graph: {"flags", "n_far", "cov": 36 N, "joint": 144 n_pairs} (the arrays empty with flags 4).
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
    std::fprintf(stderr, "pose_graph_cov_step: input ended early\n");
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
bool loss_ok(int kind, double param) { return kind == 0 || (kind >= 1 && kind <= 3 && std::isfinite(param) && param > 0.0); }
}  // namespace

int main()
{
  std::string tok;
  while (next(tok)) {
    if (tok != "graph") {
      std::fprintf(stderr, "pose_graph_cov_step: unknown command %s\n", tok.c_str());
      return 2;
    }
    const int N = static_cast<int>(num()), E = static_cast<int>(num()), P = static_cast<int>(num()), n_pairs = static_cast<int>(num());
    mh::PgoParams p{};
    p.damping = num();
    if (N < 1 || N > mh::kPgoMaxPoses || E < 0 || E > mh::kPgoMaxEdges || P < 0 || P > N || n_pairs < 0 || n_pairs > mh::kPgoCovPairsMax) return 2;
    size_t off[mh::kPgArrays];
    // sized to this graph exactly
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

    // the covariance block, every array sized to this call exactly
    const size_t ncols = 6 * static_cast<size_t>(n_pairs), rows = 6 * static_cast<size_t>(N);
    std::vector<double> Pd(36 * static_cast<size_t>(N)), S(36 * static_cast<size_t>(N)), X(rows * ncols), Z(rows * ncols), U(6 * static_cast<size_t>(g.F) * ncols),
      joint(144 * static_cast<size_t>(n_pairs));
    std::vector<int> pairs(2 * static_cast<size_t>(n_pairs));
    for (int k = 0; k < n_pairs; ++k) {
      pairs[2 * k] = static_cast<int>(num());
      pairs[2 * k + 1] = static_cast<int>(num());
      if (pairs[2 * k] < 0 || pairs[2 * k] >= pairs[2 * k + 1] || pairs[2 * k + 1] >= N) return 2;
    }
    mh::PgoCov cov{};
    cov.n_pairs = n_pairs;
    cov.ncols = static_cast<int>(ncols);
    cov.P = Pd.data();
    cov.S = S.data();
    cov.X = X.data();
    cov.Z = Z.data();
    cov.U = U.data();
    cov.joint = joint.data();
    cov.pairs = pairs.data();
    const int need = mh::pgo_cov_correct_sm(g.F);
    std::vector<double> sm(static_cast<size_t>(need > 114 ? need : 114));
    const int flags = mh::pgo_cov_host(g, p, cov, sm.data());
    std::printf("{\"flags\": %d, \"n_far\": %d, ", flags, g.F);
    put("cov", S.data(), flags ? 0 : S.size(), ", ");
    put("joint", joint.data(), flags ? 0 : joint.size(), "}\n");
  }
  return 0;
}
