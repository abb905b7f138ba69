// mimosa_amd/csrc/window_request.hpp under g++ (tests/test_icp_window_request_cpu.py): requests read from stdin, one JSON
// line per request with what window_check_request answers.  Every array has exactly the size its request states (n_edges
// edges, n_lin linear factors, 9 W doubles ...), on the heap, so that the sanitizer build sees a read behind any of them.  The
// factors are distinct dummy pointers that nothing dereferences; the factors' own checks are a hook that refuses on request.
//
// A request is a run of whitespace-separated tokens:
//   req kind W relin_required lin_call factors_refuse null_factor null_mask
//   cfg iters check_every between_info[6] prior_info[6] damping eps_rot eps_trans
//   has_Z v[W]
//   relin present [relin_rot relin_trans]
//   lin n_lin n_given { pose L_R[9] L_t[3] H[36] b[6] f }[n_given]
//   edges n_edges n_given { pose_a pose_b Z_R[9] Z_t[3] info[36] }[n_given]
//   joint present [n_poses pose[4] L_R[36] L_t[12] H[576] b[24] f]
// kind: 0 optimise, 1 marginal, 2 marginal_joint.  null_factor: the index of a NULL factor, or -1.  null_mask: bit 0 icps,
// 1 R, 2 t, 3 has_Z, 4 Z_R, 5 Z_t, 6 g_unit, 7 cfg, 8 the output of the request's kind, 9 lin, 10 edges.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>

#include "window_request.hpp"

static bool next(std::string & tok) { return static_cast<bool>(std::cin >> tok); }
static std::string word()
{
  std::string tok;
  if (!next(tok)) {
    std::fprintf(stderr, "window_request_check: the input ends inside a request\n");
    std::exit(2);
  }
  return tok;
}
static void expect(const char * what)
{
  const std::string tok = word();
  if (tok != what) {
    std::fprintf(stderr, "window_request_check: expected %s, got %s\n", what, tok.c_str());
    std::exit(2);
  }
}
static long integer() { return std::strtol(word().c_str(), nullptr, 10); }
static double real() { return std::strtod(word().c_str(), nullptr); }
template <size_t N>
static void reals(double (&a)[N])
{
  for (double & v : a) v = real();
}
template <typename T>
static std::unique_ptr<T[]> exactly(size_t n) { return std::unique_ptr<T[]>(new T[n]()); }

int main()
{
  static char factor_at[64];  // addresses for the dummy factors
  static mh_icp_window_result out;
  static mh_window_marginal marg;
  static mh_window_joint_marginal jmarg;
  std::string tok;
  while (next(tok)) {
    if (tok != "req") {
      std::fprintf(stderr, "window_request_check: expected req, got %s\n", tok.c_str());
      return 2;
    }
    WindowRequest q;
    q.kind = static_cast<WindowKind>(integer());
    q.W = static_cast<size_t>(integer());
    q.relin_required = integer() != 0;
    q.lin_call = integer() != 0;
    const bool factors_refuse = integer() != 0;
    const long null_factor = integer();
    const unsigned long null_mask = static_cast<unsigned long>(integer());
    auto null = [&](int bit) { return ((null_mask >> bit) & 1ul) != 0; };
    const size_t W = q.W;
    if (W > sizeof(factor_at)) return 2;

    auto icps = exactly<mh_icp *>(W);
    for (size_t f = 0; f < W; ++f) icps[f] = static_cast<long>(f) == null_factor ? nullptr : reinterpret_cast<mh_icp *>(factor_at + f);
    auto R = exactly<double>(9 * W), t = exactly<double>(3 * W), Z_R = exactly<double>(9 * W), Z_t = exactly<double>(3 * W);
    auto has_Z = exactly<int32_t>(W);
    const double g_unit[3] = {0.0, 0.0, -1.0};

    mh_icp_window_config cfg{};
    expect("cfg");
    cfg.iters = static_cast<int32_t>(integer());
    cfg.check_every = static_cast<int32_t>(integer());
    reals(cfg.between_info);
    reals(cfg.prior_info);
    cfg.damping = real();
    cfg.eps_rot = real();
    cfg.eps_trans = real();
    expect("has_Z");
    for (size_t f = 0; f < W; ++f) has_Z[f] = static_cast<int32_t>(integer());
    mh_icp_window_relin relin{};
    expect("relin");
    if (integer()) {
      relin.relin_rot = real();
      relin.relin_trans = real();
      q.relin = &relin;
    }
    expect("lin");
    q.n_lin = static_cast<size_t>(integer());
    const size_t lin_given = static_cast<size_t>(integer());
    auto lin = exactly<mh_window_linear_factor>(lin_given);
    for (size_t j = 0; j < lin_given; ++j) {
      lin[j].pose = static_cast<int32_t>(integer());
      reals(lin[j].L_R);
      reals(lin[j].L_t);
      reals(lin[j].H);
      reals(lin[j].b);
      lin[j].f = real();
    }
    expect("edges");
    q.n_edges = static_cast<size_t>(integer());
    const size_t edges_given = static_cast<size_t>(integer());
    auto edges = exactly<mh_window_edge>(edges_given);
    for (size_t e = 0; e < edges_given; ++e) {
      edges[e].pose_a = static_cast<int32_t>(integer());
      edges[e].pose_b = static_cast<int32_t>(integer());
      reals(edges[e].Z_R);
      reals(edges[e].Z_t);
      reals(edges[e].info);
    }
    auto joint = exactly<mh_window_joint_factor>(1);
    expect("joint");
    if (integer()) {
      joint[0].n_poses = static_cast<int32_t>(integer());
      for (int32_t & p : joint[0].pose) p = static_cast<int32_t>(integer());
      reals(joint[0].L_R);
      reals(joint[0].L_t);
      reals(joint[0].H);
      reals(joint[0].b);
      joint[0].f = real();
      q.joint = joint.get();
    }

    q.icps = null(0) ? nullptr : icps.get();
    q.R = null(1) ? nullptr : R.get();
    q.t = null(2) ? nullptr : t.get();
    q.has_Z = null(3) ? nullptr : has_Z.get();
    q.Z_R = null(4) ? nullptr : Z_R.get();
    q.Z_t = null(5) ? nullptr : Z_t.get();
    q.g_unit = null(6) ? nullptr : g_unit;
    q.cfg = null(7) ? nullptr : &cfg;
    if (!null(8)) {
      if (q.kind == WindowKind::optimise) q.outputs.out = &out;
      if (q.kind == WindowKind::marginal) q.outputs.marg = &marg;
      if (q.kind == WindowKind::marginal_joint) q.outputs.jmarg = &jmarg;
    }
    q.lin = null(9) ? nullptr : lin.get();
    q.edges = null(10) ? nullptr : edges.get();

    WindowChecked k;
    const Refusal no = window_check_request(q, k, [&]() -> Refusal {
      if (factors_refuse) return {MH_ERR_UNSUPPORTED, "the factors' own checks"};
      return {};
    });
    std::printf("{\"code\": %d, \"message\": \"%s\", \"sep\": [%d, %d, %d, %d], \"n_sep\": %d, \"zmask\": %u}\n", no.code, no.message.c_str(), k.sep[0], k.sep[1],
                k.sep[2], k.sep[3], k.n_sep, k.zmask);
  }
  return 0;
}
