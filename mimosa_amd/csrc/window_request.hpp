// What an mh_icp_window_* entry point was given (WindowRequest) and every check of it that needs neither a device nor a look
// inside a factor, in the order the ABI promises (include/mimosa_hip.h: "a call with several things wrong reports ...").
// HIP-free: chain_api.hip runs window_check_request at the start of a call, tests/cpp/window_request_check.cpp runs the same
// function under g++.  mh_icp stays opaque here; what is asked of the factors themselves is the caller's hook.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/mimosa_hip.h"

enum class WindowKind
{
  optimise,        // mh_icp_window_optimise and its _relin, _lin, _edges, _joint forms: iterations of K3 and a step kernel
  marginal,        // mh_icp_window_marginalise: K3 of icps[0] and the marginal kernel
  marginal_joint,  // mh_icp_window_marginalise_joint: ... and the joint marginal kernel, on a separator of up to four poses
};

// where a call's results go; the entry point's kind decides which it needs (optimise: out, marginal: marg, marginal_joint: jmarg)
struct WindowOutputs
{
  mh_icp_window_result * out = nullptr;
  double * trace_poses = nullptr;
  uint32_t * evaluated_mask = nullptr;
  mh_window_marginal * marg = nullptr;
  mh_window_joint_marginal * jmarg = nullptr;
};

struct WindowRequest
{
  WindowKind kind = WindowKind::optimise;
  bool blocking = true;
  mh_icp * const * icps = nullptr;
  size_t W = 0;
  const double * R = nullptr, * t = nullptr;
  const int32_t * has_Z = nullptr;
  const double * Z_R = nullptr, * Z_t = nullptr;
  const double * g_unit = nullptr;
  const mh_icp_window_config * cfg = nullptr;
  const mh_icp_window_relin * relin = nullptr;
  bool relin_required = false;  // the _relin entry points: their thresholds are not optional
  bool lin_call = false;        // the entry point has a list of linear factors (which may be empty)
  const mh_window_linear_factor * lin = nullptr;
  size_t n_lin = 0;
  const mh_window_edge * edges = nullptr;
  size_t n_edges = 0;
  const mh_window_joint_factor * joint = nullptr;
  WindowOutputs outputs;
};

// why a request is not run: code is MH_OK when it is
struct Refusal
{
  int code = MH_OK;
  std::string message;
  explicit operator bool() const { return code != MH_OK; }
};

// what the checks work out on their way and the staging needs
struct WindowChecked
{
  int sep[MH_WINDOW_JOINT_POSES] = {0, 0, 0, 0};  // marginal_joint: the separator of pose 0, ascending
  int n_sep = 0;
  unsigned int zmask = 0;  // bit f: pose f has a between measurement to pose f - 1
};

constexpr int kWindowItersMax = 64;  // the pending ring of a factor (kMaxPending of mh_internal.hpp)

// ---- the two predicates mh_pose_graph_set_edges shares ---------------------------------------------------------------------
inline bool window_edge_finite(const mh_window_edge & q)
{
  bool fin = true;
  for (double v : q.Z_R) fin = fin && std::isfinite(v);
  for (double v : q.Z_t) fin = fin && std::isfinite(v);
  for (double v : q.info) fin = fin && std::isfinite(v);
  return fin;
}

// the row-major n x n block at a, leading dimension ld: a[r][c] == a[c][r] exactly
inline bool exactly_symmetric(const double * a, int n, int ld)
{
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < r; ++c)
      if (a[ld * r + c] != a[ld * c + r]) return false;
  return true;
}

// ---- the checks, one per payload ---------------------------------------------------------------------------------------------
inline Refusal window_check_edges(const mh_window_edge * edges, size_t n_edges, size_t W)
{
  if (n_edges > static_cast<size_t>(MH_WINDOW_EDGE_MAX)) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_edges: at most 32 edges per call"};
  if (n_edges && !edges) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_edges: NULL edges"};
  for (size_t e = 0; e < n_edges; ++e) {
    const mh_window_edge & q = edges[e];
    if (q.pose_a < 0 || static_cast<size_t>(q.pose_b) >= W || q.pose_b < 0 || q.pose_a >= q.pose_b)
      return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_edges: an edge needs 0 <= pose_a < pose_b <= W - 1"};
    if (!window_edge_finite(q)) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_edges: an edge has an entry that is not finite"};
    if (!exactly_symmetric(q.info, 6, 6)) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_edges: an edge's info is not symmetric"};
  }
  return {};
}

// the plain marginal is a factor on pose 1 alone
inline Refusal window_check_marginal_edges(const mh_window_edge * edges, size_t n_edges)
{
  for (size_t e = 0; e < n_edges; ++e)
    if (edges[e].pose_a == 0 && edges[e].pose_b > 1)
      return {MH_ERR_UNSUPPORTED, "mh_icp_window_marginalise: an edge from pose 0 beyond pose 1 makes the marginal a joint factor on several poses"};
  return {};
}

inline Refusal window_check_joint(const mh_window_joint_factor & q, size_t W)
{
  if (q.n_poses < 1 || q.n_poses > MH_WINDOW_JOINT_POSES) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_joint: n_poses must be in 1..4"};
  const int n = q.n_poses;
  for (int m = 0; m < n; ++m)
    if (q.pose[m] < 0 || static_cast<size_t>(q.pose[m]) >= W || (m > 0 && q.pose[m] <= q.pose[m - 1]))
      return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_joint: the poses must be strictly ascending in 0 .. W - 1"};
  bool fin = std::isfinite(q.f);
  for (int k = 0; k < 9 * n; ++k) fin = fin && std::isfinite(q.L_R[k]);
  for (int k = 0; k < 3 * n; ++k) fin = fin && std::isfinite(q.L_t[k]);
  for (int r = 0; r < 6 * n; ++r) {
    fin = fin && std::isfinite(q.b[r]);
    for (int c = 0; c < 6 * n; ++c) fin = fin && std::isfinite(q.H[24 * r + c]);
  }
  if (!fin) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_joint: the joint factor has an entry that is not finite"};
  if (!exactly_symmetric(q.H, 6 * n, 24)) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_joint: the joint factor's H is not symmetric"};
  return {};
}

// the joint marginal absorbs the carried joint factor, which it can only when pose 0 is in it (joint: checked, or NULL)
inline Refusal window_check_joint_has_pose0(const mh_window_joint_factor * joint)
{
  if (joint && joint->pose[0] != 0)
    return {MH_ERR_UNSUPPORTED, "mh_icp_window_marginalise_joint: a joint factor without pose 0 would stay in the window as a second joint factor"};
  return {};
}

// The separator of pose 0: pose 1 (the between chain), every pose an edge from pose 0 reaches, the other poses of the joint
// factor; ascending into sep, at most four.  (Poses are inside the window by the checks above, but W itself is judged later:
// a window of more than 16 poses is refused there, hence the clamp.)
inline Refusal window_separator(const mh_window_edge * edges, size_t n_edges, const mh_window_joint_factor * joint, int sep[MH_WINDOW_JOINT_POSES],
                                int & n_sep)
{
  unsigned int smask = 2u;
  for (size_t e = 0; e < n_edges; ++e)
    if (edges[e].pose_a == 0) smask |= 1u << std::min(edges[e].pose_b, 31);
  for (int m = 1; joint && m < joint->n_poses; ++m) smask |= 1u << std::min(joint->pose[m], 31);
  n_sep = 0;
  for (int i = 1; i < 32; ++i)
    if ((smask >> i) & 1u) {
      if (n_sep < MH_WINDOW_JOINT_POSES) sep[n_sep] = i;
      ++n_sep;
    }
  if (n_sep > MH_WINDOW_JOINT_POSES) return {MH_ERR_UNSUPPORTED, "mh_icp_window_marginalise_joint: the separator of pose 0 has more than 4 poses"};
  return {};
}

inline Refusal window_check_arguments(const WindowRequest & q)
{
  const WindowOutputs & o = q.outputs;
  const bool no_out = q.kind == WindowKind::marginal_joint ? !o.jmarg : q.kind == WindowKind::marginal ? !o.marg : !o.out;
  if (!q.icps || !q.R || !q.t || !q.has_Z || !q.g_unit || !q.cfg || no_out) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise: NULL argument"};
  if (q.W < 1) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise: the window has no pose"};
  if (q.kind != WindowKind::optimise && q.W < 2) return {MH_ERR_INVALID_ARG, "mh_icp_window_marginalise: the window needs a pose behind the oldest"};
  if (q.W > static_cast<size_t>(MH_WINDOW_MAX)) return {MH_ERR_UNSUPPORTED, "mh_icp_window_optimise: at most 16 poses per call"};
  for (size_t f = 0; f < q.W; ++f)
    if (!q.icps[f]) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise: NULL factor"};
  return {};
}

inline Refusal window_check_config(const mh_icp_window_config & cfg)
{
  if (cfg.iters < 1 || cfg.iters > kWindowItersMax) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise: iters must be in 1..64"};
  bool ok = cfg.damping >= 0.0 && cfg.eps_rot >= 0.0 && cfg.eps_trans >= 0.0 && cfg.check_every >= 0;
  for (int i = 0; i < 6; ++i) ok = ok && cfg.between_info[i] >= 0.0 && cfg.prior_info[i] >= 0.0;
  if (!ok) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise: eps, damping, between_info, prior_info and check_every must be >= 0"};
  return {};
}

inline Refusal window_check_relin(const mh_icp_window_relin & r)
{
  constexpr double big = std::numeric_limits<double>::max();
  if (!(r.relin_rot >= 0.0 && r.relin_rot <= big && r.relin_trans >= 0.0 && r.relin_trans <= big))
    return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_relin: relin_rot and relin_trans must be finite and >= 0"};
  return {};
}

inline Refusal window_check_linear(const mh_window_linear_factor * lin, size_t n_lin, size_t W)
{
  if (n_lin > static_cast<size_t>(MH_WINDOW_LINEAR_MAX)) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_lin: at most 32 linear factors per call"};
  if (n_lin && !lin) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_lin: NULL linear factors"};
  for (size_t j = 0; j < n_lin; ++j) {
    const mh_window_linear_factor & q = lin[j];
    if (q.pose < 0 || static_cast<size_t>(q.pose) >= W) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_lin: a linear factor's pose is outside the window"};
    bool fin = std::isfinite(q.f);
    for (double v : q.L_R) fin = fin && std::isfinite(v);
    for (double v : q.L_t) fin = fin && std::isfinite(v);
    for (double v : q.H) fin = fin && std::isfinite(v);
    for (double v : q.b) fin = fin && std::isfinite(v);
    if (!fin) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_lin: a linear factor has an entry that is not finite"};
  }
  return {};
}

// which poses have a between measurement (pose 0 never), and that the measurements are there when one does
inline Refusal window_check_between(const int32_t * has_Z, const double * Z_R, const double * Z_t, size_t W, unsigned int & zmask)
{
  zmask = 0;
  for (size_t f = 1; f < W; ++f)
    if (has_Z[f]) zmask |= 1u << f;
  if (zmask && (!Z_R || !Z_t)) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise: NULL between measurements"};
  return {};
}

// ---- all of them, in the order that is part of the ABI's behaviour ---------------------------------------------------------
// check_factors() is the caller's look at the factors themselves (none is NULL by then), between the arguments and the
// config; it returns a Refusal as well.  The first refusal ends the checks.  Most messages say mh_icp_window_optimise
// whichever entry point was called: callers match them, they stay.
template <typename CheckFactors>
inline Refusal window_check_request(const WindowRequest & q, WindowChecked & k, CheckFactors check_factors)
{
  Refusal no;
  if (q.relin_required && !q.relin) return {MH_ERR_INVALID_ARG, "mh_icp_window_optimise_relin: NULL argument"};
  // the edges first, then the joint factor: what is wrong with them is told apart without a factor
  if ((no = window_check_edges(q.edges, q.n_edges, q.W))) return no;
  if (q.kind == WindowKind::marginal && (no = window_check_marginal_edges(q.edges, q.n_edges))) return no;
  if (q.joint && (no = window_check_joint(*q.joint, q.W))) return no;
  if (q.kind == WindowKind::marginal_joint) {
    if ((no = window_check_joint_has_pose0(q.joint))) return no;
    if ((no = window_separator(q.edges, q.n_edges, q.joint, k.sep, k.n_sep))) return no;
  }
  if ((no = window_check_arguments(q))) return no;
  if ((no = check_factors())) return no;
  if ((no = window_check_config(*q.cfg))) return no;
  if (q.relin && (no = window_check_relin(*q.relin))) return no;
  if (q.lin_call && (no = window_check_linear(q.lin, q.n_lin, q.W))) return no;
  return window_check_between(q.has_Z, q.Z_R, q.Z_t, q.W, k.zmask);
}
