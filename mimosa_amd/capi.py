"""ctypes binding over libmimosa_hip.so (include/mimosa_hip.h) — test / bench tooling.

Thin and literal: one Python method per C entry point, numpy arrays for the plain buffers.  There is
no fallback of any kind: if the library is missing, or no GPU is present, these raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None

MH_OK, MH_ERR_INVALID_ARG, MH_ERR_HIP, MH_ERR_NO_DEVICE, MH_ERR_OOM, MH_ERR_UNSUPPORTED = range(6)

# every symbol include/mimosa_hip.h declares
EXPORTS = [
    "mh_abi_version", "mh_init", "mh_shutdown", "mh_last_error", "mh_set_profiling",
    "mh_stream", "mh_synchronize", "mh_timer_begin", "mh_timer_end",
    "mh_map_create", "mh_map_insert", "mh_map_insert_device", "mh_map_insert_from_scan", "mh_map_preview_insert", "mh_map_preview_insert_device", "mh_map_preview_insert_from_scan", "mh_map_carve", "mh_map_carve_device", "mh_map_carve_from_scan", "mh_map_copy", "mh_map_retain", "mh_map_release", "mh_map_get_stats",
    "mh_map_get_cloud", "mh_map_knn",
    "mh_icp_create", "mh_icp_clone", "mh_icp_destroy", "mh_icp_linearize", "mh_icp_linearize_async",
    "mh_icp_wait", "mh_icp_linearize_batch", "mh_icp_get_state", "mh_icp_reset", "mh_icp_set_components", "mh_icp_size",
    "mh_icp_align", "mh_icp_align_async",
    "mh_icp_align_batch", "mh_icp_align_batch_async", "mh_icp_align_batch_wait",
    "mh_icp_score_poses", "mh_icp_score_poses_async", "mh_icp_relocalise", "mh_icp_relocalise_batch",
    "mh_place_db_create", "mh_place_db_destroy", "mh_place_db_size", "mh_place_describe", "mh_place_describe_device", "mh_place_describe_from_scan",
    "mh_place_db_add", "mh_place_db_add_from_scan", "mh_place_db_get", "mh_place_db_query", "mh_place_db_query_from_scan",
    "mh_pose_graph_create", "mh_pose_graph_destroy", "mh_pose_graph_set_poses", "mh_pose_graph_set_fixed", "mh_pose_graph_set_edges",
    "mh_pose_graph_get_poses", "mh_pose_graph_residuals", "mh_pose_graph_optimise",
    "mh_pose_graph_set_priors", "mh_pose_graph_set_loss", "mh_pose_graph_prior_residuals", "mh_pose_graph_weights",
    "mh_pose_graph_covariances", "mh_pose_graph_create_wide",
    "mh_keyframes_create", "mh_keyframes_destroy", "mh_keyframes_size", "mh_keyframes_get_info", "mh_keyframes_add", "mh_keyframes_add_device",
    "mh_keyframes_add_from_scan", "mh_keyframes_get", "mh_keyframes_device_points", "mh_map_rebuild_from_keyframes",
    "mh_icp_window_optimise", "mh_icp_window_optimise_async", "mh_icp_window_wait",
    "mh_icp_window_optimise_relin", "mh_icp_window_optimise_relin_async",
    "mh_icp_window_optimise_lin", "mh_icp_window_optimise_lin_async",
    "mh_icp_window_optimise_edges", "mh_icp_window_optimise_edges_async",
    "mh_icp_window_marginalise", "mh_icp_window_marginalise_async",
    "mh_icp_window_optimise_joint", "mh_icp_window_optimise_joint_async", "mh_icp_window_marginalise_joint", "mh_icp_window_marginalise_joint_async",
    "mh_deskew", "mh_transform_f32",
    "mh_scan_create", "mh_scan_destroy", "mh_scan_prepare_input", "mh_scan_prepare_input_device", "mh_scan_prefetch", "mh_scan_prepare_input_prefetched", "mh_scan_prepare_input_layout", "mh_scan_get_unique_ns", "mh_scan_deskew",
    "mh_scan_deskew_imu", "mh_scan_get_deskew_poses", "mh_photo_preprocess_scan_resident", "mh_photo_preprocess_scan_begin_resident",
    "mh_scan_preprocess_geometric", "mh_scan_get_points", "mh_scan_get_indices", "mh_icp_create_from_scan",
    "mh_init_on_stream", "mh_map_insert_shard", "mh_icp_create_from_device", 
    "mh_shard_unique_id", "mh_shard_comm_init_rccl", "mh_shard_comm_init_local", "mh_shard_comm_destroy", "mh_shard_comm_world", "mh_shard_comm_rank",
    "mh_shard_comm_backend", "mh_shard_comm_info", "mh_shard_owner_of_block", "mh_map_insert_shard_from_scan", "mh_scan_device_points", "mh_shard_icp_create", "mh_shard_icp_linearize", "mh_shard_icp_linearize_async", "mh_shard_icp_linearize_batch",
    "mh_shard_icp_linearize_batch_async", "mh_shard_icp_wait", "mh_shard_icp_reset", "mh_shard_icp_set_components", "mh_shard_icp_get_state",
    "mh_shard_icp_stats", "mh_shard_icp_destroy", "mh_alloc_check_stats",
    "mh_photo_create", "mh_photo_destroy", "mh_photo_preprocess", "mh_scan_keep_raw", "mh_photo_preprocess_scan", "mh_photo_preprocess_scan_begin", "mh_photo_preprocess_commit", "mh_photo_detect_prefetch", "mh_photo_get_image",
    "mh_photo_num_features", "mh_photo_get_features", "mh_photo_set_features", "mh_photo_detect_features", "mh_photo_update_map",
    "mh_photo_factor_create", "mh_photo_factor_clone", "mh_photo_factor_destroy", "mh_photo_factor_linearize", "mh_photo_factor_linearize_async", "mh_photo_factor_wait", "mh_photo_factor_get_state", "mh_photo_factor_size",
    "mh_photo_factor_linearize_batch", "mh_photo_factor_linearize_batch_async",
    "mh_radar_scan_create", "mh_radar_scan_destroy", "mh_radar_prepare_input", "mh_radar_get_targets", "mh_radar_factor_create",
    "mh_radar_factor_create_from_scan", "mh_radar_factor_clone", "mh_radar_factor_destroy", "mh_radar_factor_size", "mh_radar_factor_linearize",
    "mh_radar_factor_linearize_async", "mh_radar_factor_wait", "mh_radar_factor_linearize_batch", "mh_radar_factor_get_residuals",
]


class MhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mimosa_hip error {code}: {msg}")
        self.code = code


class RegConfig(C.Structure):
    _fields_ = [
        ("source_voxel_grid_filter_leaf_size", C.c_float),
        ("source_voxel_grid_min_dist_in_voxel", C.c_float),
        ("target_ivox_map_leaf_size", C.c_float),
        ("target_ivox_map_min_dist_in_voxel", C.c_float),
        ("num_corres_points", C.c_uint64),
        ("max_corres_distance", C.c_float),
        ("plane_validity_distance", C.c_float),
        ("lidar_point_noise_std_dev", C.c_float),
        ("use_huber", C.c_int32),
        ("huber_threshold", C.c_float),
        ("reg_4_dof", C.c_int32),
        ("project_on_degneneracy", C.c_int32),
        ("degen_thresh_rot", C.c_float),
        ("degen_thresh_trans", C.c_float),
    ]


class MapConfig(C.Structure):
    _fields_ = [
        ("leaf_size", C.c_double), ("min_dist_in_cell", C.c_double), ("max_points_in_cell", C.c_int32),
        ("neighbor_voxel_mode", C.c_int32), ("lru_horizon", C.c_int64), ("lru_clear_cycle", C.c_int32),
        ("reserved", C.c_int32),
    ]


class MapStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_voxels", "n_points", "n_blocks", "device_bytes", "uploads", "upload_bytes",
                                         "delta_uploads", "full_uploads")]


class MapInsertPreview(C.Structure):
    """mh_map_insert_preview: what the next insert of a batch would do (48 bytes)."""
    _fields_ = [(n, C.c_int64) for n in ("n_points", "n_added", "n_too_close", "n_voxel_full", "n_touched_voxels", "n_new_voxels")]


class MapCarveConfig(C.Structure):
    """mh_map_carve_config (48 bytes)."""
    _fields_ = [("grid", C.c_int32), ("ring", C.c_int32), ("range_min", C.c_double), ("range_max", C.c_double), ("margin_abs", C.c_double),
                ("margin_rel", C.c_double), ("apply", C.c_int32), ("reserved", C.c_int32)]


class MapCarveResult(C.Structure):
    """mh_map_carve_result (48 bytes)."""
    _fields_ = [(n, C.c_int64) for n in ("n_obs_used", "n_cells_hit", "n_tested", "n_removed", "n_voxels_touched", "n_voxels_emptied")]


def make_carve_config(grid=64, ring=1, range_min=0.5, range_max=60.0, margin_abs=0.3, margin_rel=0.0, apply=True) -> MapCarveConfig:
    return MapCarveConfig(int(grid), int(ring), float(range_min), float(range_max), float(margin_abs), float(margin_rel), int(apply), 0)


class IcpResult(C.Structure):
    _fields_ = [
        ("H_ss", C.c_double * 36), ("H_st", C.c_double * 36), ("H_tt", C.c_double * 36),
        ("b_s", C.c_double * 6), ("b_t", C.c_double * 6), ("f", C.c_double),
        ("loc_trans_comp", C.c_double * 3), ("loc_rot_comp", C.c_double * 3),
        ("loc_trans_final", C.c_double * 3), ("loc_rot_final", C.c_double * 3),
        ("eigvec_trans", C.c_double * 9), ("eigvec_rot", C.c_double * 9),
        ("degen_rot", C.c_double * 3), ("degen_trans", C.c_double * 3),
        ("degen_eigvec_rot", C.c_double * 9), ("degen_eigvec_trans", C.c_double * 9),
        ("status_hist", C.c_int32 * 9), ("linearize_count", C.c_int32),
        ("mean_candidates", C.c_double), ("mean_scanned", C.c_double), ("n_knn", C.c_int64), ("n_exact_fallback", C.c_int64),
        ("gpu_ms_linearize", C.c_float), ("gpu_ms_localizability", C.c_float),
    ]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = np.array(v) if hasattr(v, "__len__") else v
        for k in ("H_ss", "H_st", "H_tt"):
            d[k] = d[k].reshape(6, 6)
        for k in ("eigvec_trans", "eigvec_rot", "degen_eigvec_rot", "degen_eigvec_trans"):
            d[k] = d[k].reshape(3, 3)
        return d


class AlignConfig(C.Structure):
    """mh_icp_align_config"""
    _fields_ = [("max_iters", C.c_int32), ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("damping", C.c_double),
                ("prior_sigma_rot", C.c_double), ("prior_sigma_trans", C.c_double), ("check_every", C.c_int32)]


class AlignTrace(C.Structure):
    """mh_icp_align_trace"""
    _fields_ = [("f", C.c_double), ("step_rot", C.c_double), ("step_trans", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("n_knn", C.c_int64), ("degenerate", C.c_int32), ("reserved", C.c_int32)]


class AlignResult(C.Structure):
    """mh_icp_align_result"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("iters", C.c_int32), ("converged", C.c_int32),
                ("trace", AlignTrace * 64), ("first", IcpResult), ("last", IcpResult)]

    def as_dict(self):
        n = int(self.iters)
        tr = [self.trace[i] for i in range(n)]
        return {
            "R": np.array(self.R).reshape(3, 3), "t": np.array(self.t), "iters": n, "converged": int(self.converged),
            "trace": [{"f": r.f, "step_rot": r.step_rot, "step_trans": r.step_trans, "R": np.array(r.R).reshape(3, 3), "t": np.array(r.t),
                       "n_knn": int(r.n_knn), "degenerate": int(r.degenerate)} for r in tr],
            "first": self.first.as_dict(), "last": self.last.as_dict(),
        }


def make_align_config(max_iters=10, eps_rot=1e-6, eps_trans=1e-6, damping=0.0, prior_sigma_rot=0.0, prior_sigma_trans=0.0,
                      check_every=0) -> AlignConfig:
    return AlignConfig(max_iters, eps_rot, eps_trans, damping, prior_sigma_rot, prior_sigma_trans, check_every)


MH_ALIGN_BATCH_MAX = 16
MH_RELOC_MAX_POSES = 65536
MH_RELOC_MAX_REFINE = 8


class PoseScore(C.Structure):
    """mh_pose_score"""
    _fields_ = [("n_points", C.c_int32), ("n_occupied", C.c_int32), ("n_inliers", C.c_int32), ("reserved", C.c_int32), ("sum_sq", C.c_double)]

    def as_dict(self):
        return {"n_points": int(self.n_points), "n_occupied": int(self.n_occupied), "n_inliers": int(self.n_inliers), "sum_sq": float(self.sum_sq)}


# the same record as a numpy dtype: ICPFactor.score_poses returns its scores as such an array
POSE_SCORE_DTYPE = np.dtype([("n_points", np.int32), ("n_occupied", np.int32), ("n_inliers", np.int32), ("reserved", np.int32), ("sum_sq", np.float64)])


class ScoreConfig(C.Structure):
    """mh_icp_score_config"""
    _fields_ = [("gate", C.c_double), ("stride", C.c_int32), ("top_k", C.c_int32)]


class RelocConfig(C.Structure):
    """mh_icp_reloc_config"""
    _fields_ = [("score", ScoreConfig), ("align", AlignConfig), ("final_gate", C.c_double)]


class RelocCandidate(C.Structure):
    """mh_icp_reloc_candidate"""
    _fields_ = [("index", C.c_int32), ("iters", C.c_int32), ("converged", C.c_int32), ("reserved", C.c_int32), ("coarse", PoseScore),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("fine", PoseScore)]


class RelocResult(C.Structure):
    """mh_icp_reloc_result"""
    _fields_ = [("n_candidates", C.c_int32), ("best", C.c_int32), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("cand", RelocCandidate * MH_RELOC_MAX_REFINE)]

    def as_dict(self):
        n = int(self.n_candidates)
        return {
            "n_candidates": n, "best": int(self.best), "R": np.array(self.R).reshape(3, 3), "t": np.array(self.t),
            "cand": [{"index": int(c.index), "iters": int(c.iters), "converged": int(c.converged), "coarse": c.coarse.as_dict(),
                      "R": np.array(c.R).reshape(3, 3), "t": np.array(c.t), "fine": c.fine.as_dict()} for c in (self.cand[i] for i in range(n))],
        }


def make_reloc_config(gate=1.0, stride=1, top_k=4, align: AlignConfig = None, final_gate=0.3) -> RelocConfig:
    return RelocConfig(ScoreConfig(gate, stride, top_k), align if align is not None else make_align_config(), final_gate)


def score_key(scores):
    """The ranking of mh_icp_score_poses as a numpy sort: n_inliers descending, sum_sq ascending, pose index ascending.
    Returns the pose indices in rank order."""
    idx = np.arange(len(scores))
    return np.lexsort((idx, scores["sum_sq"], -scores["n_inliers"].astype(np.int64)))


def pose_grid(R0, t0, half_xy, step_xy, half_yaw, step_yaw):
    """Candidate poses around (R0, t0): translations t0 + (ix * step_xy, iy * step_xy, 0) for ix, iy in -nx .. nx with
    nx = floor(half_xy / step_xy + 1e-9), and rotations Rz(iw * step_yaw) @ R0 (a yaw about the WORLD z axis, radians) for iw in
    -nw .. nw with nw = floor(half_yaw / step_yaw + 1e-9).  A step <= 0 gives that axis its centre node alone.
    Order (the pose index is part of the ranking): yaw slowest, then x, then y fastest, each ascending from its negative end:
    index = (iw + nw) * (2 nx + 1)^2 + (ix + nx) * (2 nx + 1) + (iy + nx).  Returns (R [n, 3, 3], t [n, 3])."""
    R0 = np.asarray(R0, np.float64).reshape(3, 3)
    t0 = np.asarray(t0, np.float64).reshape(3)
    nx = int(np.floor(half_xy / step_xy + 1e-9)) if step_xy > 0 else 0
    nw = int(np.floor(half_yaw / step_yaw + 1e-9)) if step_yaw > 0 else 0
    side = 2 * nx + 1
    n = (2 * nw + 1) * side * side
    R = np.empty((n, 3, 3))
    t = np.empty((n, 3))
    i = 0
    for iw in range(-nw, nw + 1):
        a = iw * step_yaw
        c, s = np.cos(a), np.sin(a)
        Rw = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ R0
        for ix in range(-nx, nx + 1):
            for iy in range(-nx, nx + 1):
                R[i] = Rw
                t[i] = (t0[0] + ix * step_xy, t0[1] + iy * step_xy, t0[2])
                i += 1
    return R, t


MH_WINDOW_MAX = 16


class WindowConfig(C.Structure):
    """mh_icp_window_config"""
    _fields_ = [("iters", C.c_int32), ("check_every", C.c_int32), ("between_info", C.c_double * 6), ("prior_info", C.c_double * 6),
                ("damping", C.c_double), ("eps_rot", C.c_double), ("eps_trans", C.c_double)]


class WindowTrace(C.Structure):
    """mh_icp_window_trace"""
    _fields_ = [("f", C.c_double), ("step_rot", C.c_double), ("step_trans", C.c_double), ("flags", C.c_int32), ("degenerate", C.c_uint32)]


class WindowResult(C.Structure):
    """mh_icp_window_result"""
    _fields_ = [("R", C.c_double * (9 * MH_WINDOW_MAX)), ("t", C.c_double * (3 * MH_WINDOW_MAX)), ("iters", C.c_int32), ("converged", C.c_int32),
                ("n_poses", C.c_int32), ("reserved", C.c_int32), ("trace", WindowTrace * 64), ("first", IcpResult * MH_WINDOW_MAX),
                ("last", IcpResult * MH_WINDOW_MAX)]

    def as_dict(self):
        n, W = int(self.iters), int(self.n_poses)
        return {
            "R": np.array(self.R).reshape(MH_WINDOW_MAX, 3, 3)[:W], "t": np.array(self.t).reshape(MH_WINDOW_MAX, 3)[:W], "iters": n,
            "converged": int(self.converged),
            "trace": [{"f": r.f, "step_rot": r.step_rot, "step_trans": r.step_trans, "flags": int(r.flags), "degenerate": int(r.degenerate)}
                      for r in (self.trace[i] for i in range(n))],
            "first": [self.first[i].as_dict() for i in range(W)], "last": [self.last[i].as_dict() for i in range(W)],
        }


class WindowRelin(C.Structure):
    """mh_icp_window_relin"""
    _fields_ = [("relin_rot", C.c_double), ("relin_trans", C.c_double)]


MH_WINDOW_LINEAR_MAX = 32


class WindowLinearFactor(C.Structure):
    """mh_window_linear_factor"""
    _fields_ = [("pose", C.c_int32), ("reserved", C.c_int32), ("L_R", C.c_double * 9), ("L_t", C.c_double * 3), ("H", C.c_double * 36), ("b", C.c_double * 6),
                ("f", C.c_double)]


def make_window_linear(linear):
    """an array of mh_window_linear_factor from dicts {"pose": i, "at": (R, t), "H": 6 x 6, "b": 6, "f": float}"""
    arr = (WindowLinearFactor * max(len(linear), 1))()
    for q, l in zip(arr, linear):
        q.pose = int(l["pose"])
        q.L_R[:] = [float(v) for v in np.asarray(l["at"][0], np.float64).reshape(9)]
        q.L_t[:] = [float(v) for v in np.asarray(l["at"][1], np.float64).reshape(3)]
        q.H[:] = [float(v) for v in np.asarray(l["H"], np.float64).reshape(36)]
        q.b[:] = [float(v) for v in np.asarray(l["b"], np.float64).reshape(6)]
        q.f = float(l["f"])
    return arr


MH_WINDOW_EDGE_MAX = 32


class WindowEdge(C.Structure):
    """mh_window_edge"""
    _fields_ = [("pose_a", C.c_int32), ("pose_b", C.c_int32), ("Z_R", C.c_double * 9), ("Z_t", C.c_double * 3), ("info", C.c_double * 36)]


def make_window_edge(edges):
    """an array of mh_window_edge from dicts {"a": i, "b": j, "Z": (R, t) the measured T_a^-1 T_b, "info": 6 x 6}"""
    arr = (WindowEdge * max(len(edges), 1))()
    for q, e in zip(arr, edges):
        q.pose_a, q.pose_b = int(e["a"]), int(e["b"])
        q.Z_R[:] = [float(v) for v in np.asarray(e["Z"][0], np.float64).reshape(9)]
        q.Z_t[:] = [float(v) for v in np.asarray(e["Z"][1], np.float64).reshape(3)]
        q.info[:] = [float(v) for v in np.asarray(e["info"], np.float64).reshape(36)]
    return arr


class WindowMarginal(C.Structure):
    """mh_window_marginal"""
    _fields_ = [("prior", WindowLinearFactor), ("valid", C.c_int32), ("n_ties", C.c_int32), ("oldest", IcpResult)]

    def as_dict(self):
        """"linear": the marginal as optimise_window(linear=[...]) takes it, on pose 0 of the window without its oldest pose"""
        q = self.prior
        lin = {"pose": int(q.pose) - 1, "at": (np.array(q.L_R).reshape(3, 3), np.array(q.L_t)), "H": np.array(q.H).reshape(6, 6), "b": np.array(q.b),
               "f": float(q.f)}
        return {"valid": int(self.valid), "n_ties": int(self.n_ties), "oldest": self.oldest.as_dict(), "linear": lin}


MH_WINDOW_JOINT_POSES = 4


class WindowJointFactor(C.Structure):
    """mh_window_joint_factor"""
    _fields_ = [("n_poses", C.c_int32), ("reserved", C.c_int32), ("pose", C.c_int32 * MH_WINDOW_JOINT_POSES), ("L_R", C.c_double * (9 * MH_WINDOW_JOINT_POSES)),
                ("L_t", C.c_double * (3 * MH_WINDOW_JOINT_POSES)), ("H", C.c_double * (24 * 24)), ("b", C.c_double * 24), ("f", C.c_double)]

    def as_dict(self, shift=0):
        """{"poses": [...], "at": [(R, t)] per member, "H": 6n x 6n, "b": 6n, "f"}; shift is subtracted from every pose index"""
        n = int(self.n_poses)
        LR, Lt = np.array(self.L_R).reshape(MH_WINDOW_JOINT_POSES, 3, 3), np.array(self.L_t).reshape(MH_WINDOW_JOINT_POSES, 3)
        return {"poses": [int(self.pose[m]) - shift for m in range(n)], "at": [(LR[m].copy(), Lt[m].copy()) for m in range(n)],
                "H": np.array(self.H).reshape(24, 24)[:6 * n, :6 * n].copy(), "b": np.array(self.b)[:6 * n].copy(), "f": float(self.f)}


def make_window_joint(joint) -> WindowJointFactor:
    """mh_window_joint_factor from a dict {"poses": ascending indices, "at": [(R, t)] per member, "H": 6n x 6n, "b": 6n, "f": float}"""
    q = WindowJointFactor()
    n = len(joint["poses"])
    q.n_poses = n
    m = min(n, MH_WINDOW_JOINT_POSES)  # (a bad n_poses is the library's to refuse)
    H = np.zeros((24, 24))
    H[:6 * m, :6 * m] = np.asarray(joint["H"], np.float64).reshape(6 * n, 6 * n)[:6 * m, :6 * m]
    b = np.zeros(24)
    b[:6 * m] = np.asarray(joint["b"], np.float64).reshape(6 * n)[:6 * m]
    for k in range(m):
        q.pose[k] = int(joint["poses"][k])
        q.L_R[9 * k:9 * k + 9] = [float(v) for v in np.asarray(joint["at"][k][0], np.float64).reshape(9)]
        q.L_t[3 * k:3 * k + 3] = [float(v) for v in np.asarray(joint["at"][k][1], np.float64).reshape(3)]
    q.H[:] = [float(v) for v in H.reshape(-1)]
    q.b[:] = [float(v) for v in b]
    q.f = float(joint["f"])
    return q


class WindowJointMarginal(C.Structure):
    """mh_window_joint_marginal"""
    _fields_ = [("prior", WindowJointFactor), ("valid", C.c_int32), ("n_ties", C.c_int32), ("oldest", IcpResult)]

    def as_dict(self):
        """"joint_here": the marginal with the pose indices of the window it was computed in; "joint": rebased to the window
        without its oldest pose (every index minus one), as optimise_window(joint=...) takes it there"""
        return {"valid": int(self.valid), "n_ties": int(self.n_ties), "oldest": self.oldest.as_dict(), "joint_here": self.prior.as_dict(0),
                "joint": self.prior.as_dict(1)}


def make_window_config(iters=6, between_sigma_rot=2e-3, between_sigma_trans=1e-2, prior_sigma_rot=1e-4, prior_sigma_trans=1e-4, damping=1e-9,
                       eps_rot=0.0, eps_trans=0.0, check_every=0, between_info=None, prior_info=None) -> WindowConfig:
    """the defaults are the replay's smoother: six fixed iterations, its between sigmas, the tight prior marginalisation leaves"""
    bi = [1.0 / between_sigma_rot ** 2] * 3 + [1.0 / between_sigma_trans ** 2] * 3 if between_info is None else list(between_info)
    pi = ([1.0 / prior_sigma_rot ** 2 if prior_sigma_rot > 0 else 0.0] * 3 + [1.0 / prior_sigma_trans ** 2 if prior_sigma_trans > 0 else 0.0] * 3
          if prior_info is None else list(prior_info))
    return WindowConfig(iters, check_every, (C.c_double * 6)(*bi), (C.c_double * 6)(*pi), damping, eps_rot, eps_trans)


class ShardConfig(C.Structure):
    _fields_ = [("block_log2", C.c_int32), ("force_collectives", C.c_int32)]


class ShardStats(C.Structure):
    _fields_ = [("n_live", C.c_uint64), ("n_slots", C.c_uint64), ("slot_capacity", C.c_uint64), ("n_total", C.c_uint64),
                ("segment_records", C.c_uint32), ("last_max_movers", C.c_uint32), ("retries_total", C.c_uint32), ("retries_last", C.c_uint32),
                ("compactions_total", C.c_uint32), ("collectives_last", C.c_uint32),
                ("world", C.c_int32), ("rank", C.c_int32), ("collective", C.c_int32), ("linearize_count", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


SHARD_UNIQUE_ID_BYTES = 128


class InputConfig(C.Structure):
    """mh_input_config: the ManagerConfig / GeometricConfig fields Manager::prepareInput reads."""
    _fields_ = [
        ("range_min", C.c_float), ("range_max", C.c_float), ("intensity_min", C.c_float), ("intensity_max", C.c_float),
        ("ns_max", C.c_float), ("z_offset", C.c_float), ("create_full_res_pointcloud", C.c_int32),
        ("point_skip_divisor", C.c_int32), ("ring_skip_divisor", C.c_int32),
    ]


class PointLayout(C.Structure):
    """mh_point_layout: where the fields of a sensor's point record sit (what PointCloud2.fields says)."""
    _fields_ = [
        ("stride", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32), ("off_z", C.c_uint32), ("off_intensity", C.c_uint32),
        ("intensity_is_u16", C.c_int32), ("off_time", C.c_uint32), ("time_kind", C.c_int32), ("off_ring", C.c_uint32),
        ("ring_kind", C.c_int32), ("ring_filter", C.c_int32), ("off_tag", C.c_uint32), ("has_tag", C.c_int32),
    ]


TIME_U32_NS, TIME_F64_S_ABS, TIME_F64_NS_ABS, TIME_F32_S = 0, 1, 2, 3
RING_NONE, RING_U16, RING_U8, RING_F32 = 0, 1, 2, 3


def _dt(stride, **fields):
    names, formats, offsets = zip(*[(k, f, o) for k, (f, o) in fields.items()])
    return np.dtype({"names": list(names), "formats": list(formats), "offsets": list(offsets), "itemsize": stride})


# The reference's point types (include/mimosa/lidar/point.hpp:40-131, EIGEN_ALIGN16 structs): numpy record dtype with the
# members at their C++ offsets, and the mh_point_layout that selects the same branches of Manager::prepareInput<PointT>.
POINT_TYPES = {
    "ouster": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), intensity=("f4", 16), t=("u4", 20), reflectivity=("u2", 24), ring=("u2", 26)),
               dict(off_intensity=16, off_time=20, time_kind=TIME_U32_NS, off_ring=26, ring_kind=RING_U16, ring_filter=1)),
    "ouster_odyssey": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), t=("u4", 16), reflectivity=("u2", 20), near_ir=("u2", 22)),
                       dict(off_intensity=20, intensity_is_u16=1, off_time=16, time_kind=TIME_U32_NS)),
    "ouster_r8": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), intensity=("f4", 16), t=("u4", 20), reflectivity=("u2", 24), ring=("u1", 26)),
                  dict(off_intensity=16, off_time=20, time_kind=TIME_U32_NS, off_ring=26, ring_kind=RING_U8, ring_filter=1)),
    "hesai": (_dt(48, x=("f4", 0), y=("f4", 4), z=("f4", 8), intensity=("f4", 16), timestamp=("f8", 24), ring=("u2", 32)),
              dict(off_intensity=16, off_time=24, time_kind=TIME_F64_S_ABS, off_ring=32, ring_kind=RING_U16, ring_filter=1)),
    "livox": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), intensity=("f4", 16), tag=("u1", 20), line=("u1", 21), timestamp=("f8", 24)),
              dict(off_intensity=16, off_time=24, time_kind=TIME_F64_NS_ABS, off_tag=20, has_tag=1)),
    "livox_custom2": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), t=("u4", 12), intensity=("f4", 16), tag=("u1", 20), line=("u1", 21)),
                      dict(off_intensity=16, off_time=12, time_kind=TIME_U32_NS, off_tag=20, has_tag=1)),
    "velodyne": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), intensity=("f4", 16), ring=("u2", 20), time=("f4", 24)),
                 dict(off_intensity=16, off_time=24, time_kind=TIME_F32_S, off_ring=20, ring_kind=RING_U16, ring_filter=1)),
    "velodyne_anybotics": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), intensity=("f4", 16), ring=("f4", 20), time=("f4", 24)),
                           dict(off_intensity=16, off_time=24, time_kind=TIME_F32_S, off_ring=20, ring_kind=RING_F32, ring_filter=0)),
    "rslidar": (_dt(32, x=("f4", 0), y=("f4", 4), z=("f4", 8), intensity=("f4", 16), ring=("u2", 20), timestamp=("f8", 24)),
                dict(off_intensity=16, off_time=24, time_kind=TIME_F64_S_ABS, off_ring=20, ring_kind=RING_U16, ring_filter=1)),
}


def point_dtype(kind: str) -> np.dtype:
    return POINT_TYPES[kind][0]


def point_layout(kind: str) -> PointLayout:
    dt, f = POINT_TYPES[kind]
    return PointLayout(stride=dt.itemsize, off_x=0, off_y=4, off_z=8, **f)


class ScanInfo(C.Structure):
    _fields_ = [
        ("n_in", C.c_uint64), ("n_full", C.c_uint64), ("n_geometric", C.c_uint64), ("n_unique_ns", C.c_uint64),
        ("n_body", C.c_uint64), ("n_downsampled", C.c_uint64), ("last_point_ns", C.c_uint32), ("pad", C.c_uint32),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}



class PhotoConfig(C.Structure):
    """mh_photo_config (lidar::PhotometricConfig, include/mimosa/lidar/photometric_config.hpp:15-87)."""
    _fields_ = [
        ("rows", C.c_int32), ("cols", C.c_int32), ("destagger", C.c_int32),
        ("pixel_shift_by_row", C.c_void_p), ("beam_altitude_angles", C.c_void_p),
        ("range_min", C.c_float), ("range_max", C.c_float),
        ("erosion_buffer", C.c_int32), ("patch_size", C.c_int32), ("margin_size", C.c_int32),
        ("intensity_scale", C.c_float), ("intensity_gamma", C.c_float),
        ("remove_lines", C.c_int32), ("filter_brightness", C.c_int32), ("gaussian_blur", C.c_int32), ("gaussian_blur_size", C.c_int32),
        ("gradient_threshold", C.c_float), ("max_dist_from_mean", C.c_float), ("max_dist_from_plane", C.c_float),
        ("nma_radius", C.c_int32), ("num_features_detect", C.c_int32), ("occlusion_range_diff_threshold", C.c_float),
        ("max_feature_life_time", C.c_int32),
        ("high_pass_fir", C.c_void_p), ("n_high_pass", C.c_int32), ("low_pass_fir", C.c_void_p), ("n_low_pass", C.c_int32),
        ("brightness_window_size", C.c_int32 * 2), ("lidar_origin_to_beam_origin_mm", C.c_float),
        ("rotate_patch_to_align_with_gradient", C.c_int32),
        ("patch_offsets", C.c_void_p), ("n_patch_offsets", C.c_int32),
        ("use_robust_cost_function", C.c_int32), ("robust_cost_function", C.c_int32),
        ("robust_cost_function_parameter", C.c_double), ("error_scale", C.c_double), ("max_error", C.c_double), ("sigma", C.c_double),
        ("T_B_L_R", C.c_double * 9), ("T_B_L_t", C.c_double * 3),
        ("static_mask", C.c_void_p),
    ]


class PhotoFeature(C.Structure):
    _fields_ = [("id", C.c_uint32), ("life_time", C.c_int32), ("n_points", C.c_int32), ("pad", C.c_int32),
                ("center", C.c_double * 2), ("normal", C.c_double * 3), ("mean_intensity", C.c_double), ("sigma_intensity", C.c_double)]


class PhotoResult(C.Structure):
    _fields_ = [
        ("H_bb", C.c_double * 36), ("H_ba", C.c_double * 36), ("H_aa", C.c_double * 36), ("b_b", C.c_double * 6), ("b_a", C.c_double * 6),
        ("f", C.c_double), ("loc_trans_final", C.c_double * 3), ("loc_rot_final", C.c_double * 3),
        ("eigvec_trans", C.c_double * 9), ("eigvec_rot", C.c_double * 9), ("status_hist", C.c_int32 * 9),
        ("n_exceptions", C.c_int32), ("gpu_ms", C.c_float),
    ]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = np.array(v) if hasattr(v, "__len__") else v
        for k in ("H_bb", "H_ba", "H_aa"):
            d[k] = d[k].reshape(6, 6)
        for k in ("eigvec_trans", "eigvec_rot"):
            d[k] = d[k].reshape(3, 3)
        return d


MH_RADAR_RIO, MH_RADAR_MMWAVE, MH_RADAR_MMWAVE_DOPPLER_RESIDUAL = range(3)
MH_RADAR_MAX_BATCH = 1024


class RadarConfig(C.Structure):
    """radar::ManagerConfig's float fields (include/mimosa/radar/manager.hpp:20-33)"""
    _fields_ = [(n, C.c_float) for n in ("range_min", "range_max", "threshold_azimuth_deg", "threshold_elevation_deg",
                                          "filter_min_db", "noise_sigma")]


class RadarLayout(C.Structure):
    _fields_ = [("kind", C.c_int32), ("point_step", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32), ("off_z", C.c_uint32),
                ("off_intensity", C.c_uint32), ("off_velocity", C.c_uint32)]


class RadarTarget(C.Structure):
    """radar::TargetData (include/mimosa/radar/utils.hpp:17-41)"""
    _fields_ = [(n, C.c_double) for n in ("x", "y", "z", "range", "azimuth", "elevation", "radial_speed", "intensity")]


MH_MAX_IMU_SEGMENTS = 64
# mh_imu_segment: one IMU interval (t0, t1] of Manager::deskewPoints (src/lidar/manager.cpp:459-492)
IMU_SEGMENT_DTYPE = np.dtype([("t0", np.float64), ("t1", np.float64), ("R", np.float64, (9,)), ("p", np.float64, (3,)), ("v", np.float64, (3,)),
                              ("acc", np.float64, (3,)), ("omega", np.float64, (3,))])


def imu_segments(imu_t, imu_acc, imu_gyro, nav_R, nav_p, nav_v, bias_acc=(0, 0, 0), bias_gyro=(0, 0, 0)):
    """The segments mh_scan_deskew_imu takes, from what Manager::deskewPoints has in hand: sample times, raw measurements, the
    state at each sample time and the bias (interval c: state and bias-corrected measurement of sample c, manager.cpp:459-492)."""
    m = len(imu_t)
    seg = np.zeros(max(m - 1, 0), IMU_SEGMENT_DTYPE)
    for c in range(m - 1):
        seg[c] = (imu_t[c], imu_t[c + 1], np.asarray(nav_R[c], np.float64).ravel(), nav_p[c], nav_v[c],
                  np.asarray(imu_acc[c], np.float64) - np.asarray(bias_acc, np.float64),
                  np.asarray(imu_gyro[c], np.float64) - np.asarray(bias_gyro, np.float64))
    return seg


RADAR_TARGET_DTYPE = np.dtype([(n, np.float64) for n, _ in RadarTarget._fields_])


class RadarInfo(C.Structure):
    _fields_ = [("n_points_in", C.c_uint64), ("n_points_valid", C.c_uint64)]


class RadarResult(C.Structure):
    _fields_ = [
        ("G11", C.c_double * 36), ("G12", C.c_double * 18), ("G13", C.c_double * 36), ("G22", C.c_double * 9),
        ("G23", C.c_double * 18), ("G33", C.c_double * 36), ("g1", C.c_double * 6), ("g2", C.c_double * 3), ("g3", C.c_double * 6),
        ("f", C.c_double), ("n_targets", C.c_uint64), ("gpu_ms", C.c_float),
    ]
    SHAPES = {"G11": (6, 6), "G12": (6, 3), "G13": (6, 6), "G22": (3, 3), "G23": (3, 6), "G33": (6, 6)}

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = np.array(v) if hasattr(v, "__len__") else v
        for k, shp in self.SHAPES.items():
            d[k] = d[k].reshape(shp)
        return d


def make_radar_config(range_min=0.1, range_max=20.0, threshold_azimuth_deg=60.0, threshold_elevation_deg=60.0,
                      filter_min_db=5.0, noise_sigma=0.1) -> RadarConfig:
    """Defaults of radar::ManagerConfig (manager.hpp:24-32)."""
    return RadarConfig(range_min, range_max, threshold_azimuth_deg, threshold_elevation_deg, filter_min_db, noise_sigma)


def radar_layout(kind: int, point_step: int, off_x: int, off_y: int, off_z: int, off_intensity: int, off_velocity: int) -> RadarLayout:
    return RadarLayout(kind, point_step, off_x, off_y, off_z, off_intensity, off_velocity)


PHOTO_IMAGES = {"intensity": (0, np.float32, 1), "range": (1, np.float32, 1), "dx": (2, np.float32, 1), "dy": (3, np.float32, 1),
                "mask": (4, np.uint8, 1), "idx": (5, np.int32, 1), "yaw": (6, np.float32, 1), "proj_idx": (7, np.int32, 10),
                "grad": (8, np.uint8, 1), "detection_mask": (9, np.uint8, 1)}


def make_photo_config(d: dict):
    """Build an mh_photo_config from a dict (mimosa_amd.synth_photo.photo_config()); returns (struct, keep-alive list)."""
    c = PhotoConfig()
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    for k, _ in PhotoConfig._fields_:
        if k in ("pixel_shift_by_row", "patch_offsets"):
            setattr(c, k, arr(d[k], np.int32))
        elif k == "beam_altitude_angles":
            setattr(c, k, arr(d[k], np.float32))
        elif k in ("high_pass_fir", "low_pass_fir"):
            setattr(c, k, arr(d[k], np.float64) if d.get(k) is not None and len(d[k]) else None)
        elif k == "static_mask":
            setattr(c, k, arr(d[k], np.uint8) if d.get(k) is not None else None)
        elif k == "brightness_window_size":
            c.brightness_window_size[0], c.brightness_window_size[1] = int(d[k][0]), int(d[k][1])
        elif k == "T_B_L_R":
            for i, v in enumerate(np.asarray(d[k], float).ravel()):
                c.T_B_L_R[i] = v
        elif k == "T_B_L_t":
            for i, v in enumerate(np.asarray(d[k], float).ravel()):
                c.T_B_L_t[i] = v
        elif k == "n_high_pass":
            c.n_high_pass = len(d["high_pass_fir"]) if d.get("high_pass_fir") is not None else 0
        elif k == "n_low_pass":
            c.n_low_pass = len(d["low_pass_fir"]) if d.get("low_pass_fir") is not None else 0
        elif k == "n_patch_offsets":
            c.n_patch_offsets = len(np.asarray(d["patch_offsets"]).reshape(-1, 2))
        else:
            setattr(c, k, d[k])
    return c, keep


def make_input_config(**kw) -> InputConfig:
    """ENWIDE manager block (config/enwide/params.yaml:66-72) + geometric skip divisors (:79-80) by default."""
    d = dict(range_min=0.2, range_max=100.0, intensity_min=0.0, intensity_max=1.0e10, ns_max=1.0e9, z_offset=0.0,
             create_full_res_pointcloud=1, point_skip_divisor=4, ring_skip_divisor=1)
    d.update(kw)
    c = InputConfig()
    for k, v in d.items():
        setattr(c, k, v)
    return c


def make_reg_config(**kw) -> RegConfig:
    c = RegConfig()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True):
    """Load libmimosa_hip.so.  Raises if it cannot be built / found — never substitutes anything."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB
    if not os.path.exists(path):
        if not build_if_missing:
            raise FileNotFoundError(path)
        _build.build()
    # kernel-tuning experiments (tools/variant.sh) load a differently compiled build of the SAME library
    path = os.environ.get("MH_LIB_OVERRIDE", path)
    L = C.CDLL(path)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    pvp = C.POINTER(C.c_void_p)
    L.mh_abi_version.restype = i32
    L.mh_shard_owner_of_block.argtypes = [i32, i32, i32, i32]
    L.mh_shard_owner_of_block.restype = i32
    L.mh_init.argtypes = [i32, pvp]
    L.mh_shutdown.argtypes = [vp]
    L.mh_shutdown.restype = None
    L.mh_last_error.argtypes = [vp]
    L.mh_last_error.restype = C.c_char_p
    L.mh_set_profiling.argtypes = [vp, i32]
    L.mh_stream.argtypes = [vp]
    L.mh_stream.restype = vp
    L.mh_synchronize.argtypes = [vp]
    L.mh_timer_begin.argtypes = [vp]
    L.mh_timer_end.argtypes = [vp, C.POINTER(C.c_float)]
    L.mh_map_create.argtypes = [vp, C.POINTER(MapConfig), pvp]
    L.mh_map_insert.argtypes = [vp, vp, sz, sz]
    L.mh_map_insert_device.argtypes = [vp, vp, sz, sz, vp, vp]
    L.mh_map_insert_from_scan.argtypes = [vp, vp, vp, vp]
    L.mh_map_preview_insert.argtypes = [vp, vp, sz, sz, C.POINTER(MapInsertPreview), vp]
    L.mh_map_preview_insert_device.argtypes = [vp, vp, sz, sz, vp, vp, C.POINTER(MapInsertPreview), vp]
    L.mh_map_preview_insert_from_scan.argtypes = [vp, vp, vp, vp, C.POINTER(MapInsertPreview), vp]
    L.mh_map_carve.argtypes = [vp, vp, sz, sz, vp, vp, vp, C.POINTER(MapCarveConfig), C.POINTER(MapCarveResult)]
    L.mh_map_carve_device.argtypes = [vp, vp, sz, sz, vp, vp, vp, C.POINTER(MapCarveConfig), C.POINTER(MapCarveResult)]
    L.mh_map_carve_from_scan.argtypes = [vp, vp, i32, vp, vp, vp, C.POINTER(MapCarveConfig), C.POINTER(MapCarveResult)]
    L.mh_map_copy.argtypes = [vp, pvp]
    L.mh_map_retain.argtypes = [vp]
    L.mh_map_release.argtypes = [vp]
    L.mh_map_release.restype = None
    L.mh_map_get_stats.argtypes = [vp, C.POINTER(MapStats)]
    L.mh_map_get_cloud.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.mh_map_knn.argtypes = [vp, vp, sz, i32, vp, vp, vp]
    L.mh_icp_create.argtypes = [vp, vp, vp, sz, C.POINTER(RegConfig), i32, pvp]
    L.mh_icp_clone.argtypes = [vp, pvp]
    L.mh_icp_destroy.argtypes = [vp]
    L.mh_icp_destroy.restype = None
    L.mh_icp_linearize.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(IcpResult)]
    L.mh_icp_linearize_async.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(IcpResult)]
    L.mh_icp_wait.argtypes = [vp]
    L.mh_icp_linearize_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.mh_icp_get_state.argtypes = [vp, vp, vp, vp]
    L.mh_icp_reset.argtypes = [vp]
    L.mh_icp_set_components.argtypes = [vp, C.c_int]
    L.mh_icp_size.argtypes = [vp]
    L.mh_icp_align.argtypes = [vp, vp, vp, vp, C.POINTER(AlignConfig), C.POINTER(AlignResult)]
    L.mh_icp_align_async.argtypes = [vp, vp, vp, vp, C.POINTER(AlignConfig), C.POINTER(AlignResult)]
    L.mh_icp_score_poses.argtypes = [vp, vp, vp, sz, C.POINTER(ScoreConfig), vp, vp]
    L.mh_icp_score_poses_async.argtypes = [vp, vp, vp, sz, C.POINTER(ScoreConfig), vp, vp]
    L.mh_icp_relocalise.argtypes = [vp, vp, vp, sz, vp, C.POINTER(RelocConfig), C.POINTER(RelocResult)]
    L.mh_icp_align_batch.argtypes = [vp, sz, vp, vp, vp, C.POINTER(AlignConfig), vp]
    L.mh_icp_align_batch_async.argtypes = L.mh_icp_align_batch.argtypes
    L.mh_icp_align_batch_wait.argtypes = [vp]
    L.mh_icp_relocalise_batch.argtypes = [vp, vp, sz, vp, vp, sz, vp, C.POINTER(RelocConfig), C.POINTER(RelocResult)]
    L.mh_place_db_create.argtypes = [vp, C.POINTER(PlaceConfig), pvp]
    L.mh_place_db_destroy.argtypes = [vp]
    L.mh_place_db_destroy.restype = None
    L.mh_place_db_size.argtypes = [vp]
    L.mh_place_db_size.restype = sz
    L.mh_place_describe.argtypes = [vp, vp, sz, sz, vp, vp]
    L.mh_place_describe_device.argtypes = [vp, vp, sz, sz, vp, vp]
    L.mh_place_describe_from_scan.argtypes = [vp, vp, i32, vp, vp]
    L.mh_place_db_add.argtypes = [vp, vp, C.c_int64, vp]
    L.mh_place_db_add_from_scan.argtypes = [vp, vp, i32, vp, C.c_int64, vp]
    L.mh_place_db_get.argtypes = [vp, C.c_int32, vp, vp]
    L.mh_place_db_query.argtypes = [vp, vp, sz, C.c_int32, vp, vp]
    L.mh_place_db_query_from_scan.argtypes = [vp, vp, i32, vp, sz, C.c_int32, vp, vp]
    L.mh_pose_graph_create.argtypes = [vp, sz, sz, pvp]
    L.mh_pose_graph_create_wide.argtypes = [vp, sz, sz, sz, pvp]
    L.mh_pose_graph_destroy.argtypes = [vp]
    L.mh_pose_graph_destroy.restype = None
    L.mh_pose_graph_set_poses.argtypes = [vp, vp, vp, sz]
    L.mh_pose_graph_set_fixed.argtypes = [vp, vp]
    L.mh_pose_graph_set_edges.argtypes = [vp, C.POINTER(WindowEdge), sz]
    L.mh_pose_graph_get_poses.argtypes = [vp, vp, vp, sz, C.POINTER(sz)]
    L.mh_pose_graph_residuals.argtypes = [vp, vp, vp, vp]
    L.mh_pose_graph_optimise.argtypes = [vp, C.POINTER(PoseGraphConfig), C.POINTER(PoseGraphResult), vp]
    L.mh_pose_graph_set_priors.argtypes = [vp, C.POINTER(PosePrior), sz]
    L.mh_pose_graph_set_loss.argtypes = [vp, C.POINTER(PoseGraphLoss), C.POINTER(PoseGraphLoss)]
    L.mh_pose_graph_prior_residuals.argtypes = [vp, vp, vp]
    L.mh_pose_graph_weights.argtypes = [vp, vp, vp, vp]
    L.mh_pose_graph_covariances.argtypes = [vp, C.c_double, vp, vp, sz, vp, C.POINTER(PoseGraphCovInfo)]
    L.mh_keyframes_create.argtypes = [vp, C.POINTER(KeyframesConfig), pvp]
    L.mh_keyframes_destroy.argtypes = [vp]
    L.mh_keyframes_destroy.restype = None
    L.mh_keyframes_size.argtypes = [vp]
    L.mh_keyframes_size.restype = sz
    L.mh_keyframes_get_info.argtypes = [vp, C.POINTER(KeyframesInfo)]
    L.mh_keyframes_add.argtypes = [vp, vp, sz, sz, C.c_int64, vp]
    L.mh_keyframes_add_device.argtypes = [vp, vp, sz, sz, C.c_int64, vp]
    L.mh_keyframes_add_from_scan.argtypes = [vp, vp, i32, C.c_int64, vp]
    L.mh_keyframes_get.argtypes = [vp, C.c_int32, vp, sz, C.POINTER(sz), vp]
    L.mh_keyframes_device_points.argtypes = [vp, C.c_int32, C.POINTER(vp), C.POINTER(sz)]
    L.mh_map_rebuild_from_keyframes.argtypes = [vp, C.POINTER(MapConfig), vp, sz, vp, vp, C.POINTER(MapRebuildConfig), pvp, C.POINTER(MapRebuildResult)]
    L.mh_icp_window_optimise.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(WindowConfig), C.POINTER(WindowResult), vp]
    L.mh_icp_window_optimise_async.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(WindowConfig), C.POINTER(WindowResult), vp]
    L.mh_icp_window_wait.argtypes = [vp]
    L.mh_icp_window_optimise_relin.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(WindowConfig), C.POINTER(WindowRelin), C.POINTER(WindowResult), vp, vp]
    L.mh_icp_window_optimise_relin_async.argtypes = L.mh_icp_window_optimise_relin.argtypes
    L.mh_icp_window_optimise_lin.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(WindowConfig), C.POINTER(WindowRelin), C.POINTER(WindowLinearFactor), sz,
                                             C.POINTER(WindowResult), vp, vp]
    L.mh_icp_window_optimise_lin_async.argtypes = L.mh_icp_window_optimise_lin.argtypes
    L.mh_icp_window_optimise_edges.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(WindowConfig), C.POINTER(WindowRelin), C.POINTER(WindowLinearFactor), sz,
                                               C.POINTER(WindowEdge), sz, C.POINTER(WindowResult), vp, vp]
    L.mh_icp_window_optimise_edges_async.argtypes = L.mh_icp_window_optimise_edges.argtypes
    L.mh_icp_window_marginalise.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(WindowConfig), C.POINTER(WindowLinearFactor), sz, C.POINTER(WindowEdge), sz,
                                            C.POINTER(WindowMarginal)]
    L.mh_icp_window_marginalise_async.argtypes = L.mh_icp_window_marginalise.argtypes
    L.mh_icp_window_optimise_joint.argtypes = L.mh_icp_window_optimise_edges.argtypes + [C.POINTER(WindowJointFactor)]
    L.mh_icp_window_optimise_joint_async.argtypes = L.mh_icp_window_optimise_joint.argtypes
    L.mh_icp_window_marginalise_joint.argtypes = L.mh_icp_window_marginalise.argtypes[:-1] + [C.POINTER(WindowJointFactor), C.POINTER(WindowJointMarginal)]
    L.mh_icp_window_marginalise_joint_async.argtypes = L.mh_icp_window_marginalise_joint.argtypes
    L.mh_icp_size.restype = sz
    L.mh_deskew.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp]
    L.mh_transform_f32.argtypes = [vp, vp, sz, vp, vp]
    L.mh_scan_create.argtypes = [vp, pvp]
    L.mh_scan_destroy.argtypes = [vp]
    L.mh_scan_destroy.restype = None
    L.mh_scan_prepare_input.argtypes = [vp, vp, sz, C.POINTER(InputConfig), C.POINTER(ScanInfo)]
    L.mh_scan_prepare_input_layout.argtypes = [vp, vp, sz, C.POINTER(PointLayout), C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_double,
                                               C.POINTER(InputConfig), C.POINTER(ScanInfo)]
    L.mh_scan_prepare_input_device.argtypes = [vp, vp, sz, C.POINTER(InputConfig), C.POINTER(ScanInfo)]
    L.mh_scan_prefetch.argtypes = [vp, vp, sz]
    L.mh_scan_prepare_input_prefetched.argtypes = [vp, C.POINTER(InputConfig), C.POINTER(ScanInfo)]
    L.mh_scan_get_unique_ns.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.mh_scan_deskew.argtypes = [vp, vp, sz]
    L.mh_scan_deskew_imu.argtypes = [vp, vp, sz, C.c_double, vp, vp, vp, vp, vp]
    L.mh_scan_get_deskew_poses.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.mh_scan_preprocess_geometric.argtypes = [vp, vp, vp, C.c_double, i32, C.c_double, C.POINTER(ScanInfo)]
    L.mh_scan_get_points.argtypes = [vp, i32, vp, sz, C.POINTER(sz)]
    L.mh_scan_get_indices.argtypes = [vp, i32, vp, sz, C.POINTER(sz)]
    L.mh_icp_create_from_scan.argtypes = [vp, vp, vp, C.POINTER(RegConfig), i32, pvp]
    L.mh_init_on_stream.argtypes = [i32, vp, pvp]
    L.mh_map_insert_shard.argtypes = [vp, vp, sz, sz, i32, i32, i32]
    L.mh_map_insert_shard_from_scan.argtypes = [vp, vp, vp, vp, i32, i32, i32]
    L.mh_scan_device_points.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz)]
    L.mh_icp_create_from_device.argtypes = [vp, vp, vp, sz, C.POINTER(RegConfig), i32, pvp]
    L.mh_shard_unique_id.argtypes = [vp]
    L.mh_shard_comm_init_rccl.argtypes = [vp, vp, i32, i32, pvp]
    L.mh_shard_comm_init_local.argtypes = [i32, pvp]
    L.mh_shard_comm_destroy.argtypes = [vp]
    L.mh_shard_comm_destroy.restype = None
    L.mh_shard_comm_world.argtypes = [vp]
    L.mh_shard_comm_rank.argtypes = [vp]
    L.mh_shard_comm_backend.argtypes = [vp]
    L.mh_shard_comm_backend.restype = C.c_char_p
    L.mh_shard_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mh_shard_icp_create.argtypes = [vp, vp, vp, vp, sz, i32, C.POINTER(RegConfig), i32, C.POINTER(ShardConfig), pvp]
    L.mh_shard_icp_linearize.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(IcpResult)]
    L.mh_shard_icp_linearize_async.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(IcpResult)]
    L.mh_shard_icp_linearize_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.mh_shard_icp_linearize_batch_async.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.mh_shard_icp_wait.argtypes = [vp]
    L.mh_shard_icp_reset.argtypes = [vp]
    L.mh_shard_icp_set_components.argtypes = [vp, C.c_int]
    L.mh_shard_icp_get_state.argtypes = [vp, vp, vp, vp, vp, sz, C.POINTER(sz)]
    L.mh_shard_icp_stats.argtypes = [vp, C.POINTER(ShardStats)]
    L.mh_alloc_check_stats.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.mh_shard_icp_destroy.argtypes = [vp]
    L.mh_shard_icp_destroy.restype = None
    L.mh_photo_create.argtypes = [vp, C.POINTER(PhotoConfig), pvp]
    L.mh_photo_destroy.argtypes = [vp]
    L.mh_photo_destroy.restype = None
    L.mh_photo_preprocess.argtypes = [vp, vp, vp, sz, vp, vp, sz]
    L.mh_scan_keep_raw.argtypes = [vp, i32]
    L.mh_photo_preprocess_scan.argtypes = [vp, vp, vp, sz]
    L.mh_photo_preprocess_scan_begin.argtypes = [vp, vp, vp, sz]
    L.mh_photo_preprocess_commit.argtypes = [vp]
    L.mh_photo_preprocess_scan_resident.argtypes = [vp, vp]
    L.mh_photo_preprocess_scan_begin_resident.argtypes = [vp, vp]
    L.mh_photo_detect_prefetch.argtypes = [vp]
    L.mh_photo_get_image.argtypes = [vp, i32, vp, sz]
    L.mh_photo_num_features.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.mh_photo_get_features.argtypes = [vp, vp, vp, vp, vp]
    L.mh_photo_set_features.argtypes = [vp, vp, sz, vp, vp, vp]
    L.mh_photo_detect_features.argtypes = [vp, i32, vp, vp, vp, sz]
    L.mh_photo_update_map.argtypes = [vp, vp, vp, vp, vp, sz]
    L.mh_photo_factor_create.argtypes = [vp, vp, i32, pvp]
    L.mh_photo_factor_clone.argtypes = [vp, pvp]
    L.mh_photo_factor_linearize_async.argtypes = [vp, vp, vp, vp, vp]
    L.mh_photo_factor_wait.argtypes = [vp, vp]
    L.mh_photo_factor_destroy.argtypes = [vp]
    L.mh_photo_factor_destroy.restype = None
    L.mh_photo_factor_linearize.argtypes = [vp, vp, vp, vp, vp, C.POINTER(PhotoResult)]
    L.mh_photo_factor_get_state.argtypes = [vp, vp, vp, vp]
    L.mh_photo_factor_linearize_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.mh_photo_factor_linearize_batch_async.argtypes = [vp, sz, vp, vp, vp, vp]
    L.mh_photo_factor_size.argtypes = [vp]
    L.mh_photo_factor_size.restype = sz
    L.mh_radar_scan_create.argtypes = [vp, pvp]
    L.mh_radar_scan_destroy.argtypes = [vp]
    L.mh_radar_scan_destroy.restype = None
    L.mh_radar_prepare_input.argtypes = [vp, vp, sz, C.POINTER(RadarLayout), C.POINTER(RadarConfig), C.POINTER(RadarInfo)]
    L.mh_radar_get_targets.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.mh_radar_factor_create.argtypes = [vp, vp, sz, vp, vp, vp, C.c_double, pvp]
    L.mh_radar_factor_create_from_scan.argtypes = [vp, vp, vp, vp, C.c_double, pvp]
    L.mh_radar_factor_clone.argtypes = [vp, pvp]
    L.mh_radar_factor_destroy.argtypes = [vp]
    L.mh_radar_factor_destroy.restype = None
    L.mh_radar_factor_size.argtypes = [vp]
    L.mh_radar_factor_size.restype = sz
    L.mh_radar_factor_linearize.argtypes = [vp, vp, vp, vp, C.POINTER(RadarResult)]
    L.mh_radar_factor_linearize_async.argtypes = [vp, vp, vp, vp]
    L.mh_radar_factor_wait.argtypes = [vp, C.POINTER(RadarResult)]
    L.mh_radar_factor_linearize_batch.argtypes = [vp, sz, vp, vp, vp, vp]
    L.mh_radar_factor_get_residuals.argtypes = [vp, vp, vp]
    _LIB = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Context:
    def __init__(self, device: int = 0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.mh_init(device, C.byref(h))
        if rc != MH_OK:
            raise MhError(rc, (self.L.mh_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        self._children = 0
        self._closing = False

    def _child_released(self):
        self._children -= 1
        if self._closing and self._children == 0:
            self.close()

    def check(self, rc):
        if rc != MH_OK:
            raise MhError(rc, (self.L.mh_last_error(self.h) or b"").decode())

    def set_profiling(self, every):
        """0/False = off, n = HIP events around the kernels of every n-th linearize call (True = every call)."""
        self.check(self.L.mh_set_profiling(self.h, int(every)))

    def synchronize(self):
        self.check(self.L.mh_synchronize(self.h))

    def timer_begin(self):
        self.check(self.L.mh_timer_begin(self.h))

    def timer_end(self) -> float:
        ms = C.c_float()
        self.check(self.L.mh_timer_end(self.h, C.byref(ms)))
        return ms.value

    def deskew(self, pts, unique_ns, Rt12, R_B_L=None, t_B_L=None):
        pts = np.ascontiguousarray(pts).copy()
        u = np.ascontiguousarray(unique_ns, dtype=np.uint32)
        P = np.ascontiguousarray(Rt12, dtype=np.float32)
        Rb = np.ascontiguousarray(R_B_L, dtype=np.float32) if R_B_L is not None else None
        tb = np.ascontiguousarray(t_B_L, dtype=np.float32) if t_B_L is not None else None
        self.check(self.L.mh_deskew(self.h, _p(pts), len(pts), _p(u), _p(P), len(u), _p(Rb), _p(tb)))
        return pts

    def transform_f32(self, pts, R, t):
        pts = np.ascontiguousarray(pts).copy()
        R = np.ascontiguousarray(R, dtype=np.float32)
        t = np.ascontiguousarray(t, dtype=np.float32)
        self.check(self.L.mh_transform_f32(self.h, _p(pts), len(pts), _p(R), _p(t)))
        return pts

    def close(self):
        """Shut the context down; deferred until every map / factor created on it is released."""
        if getattr(self, "h", None):
            if self._children > 0:
                self._closing = True
                return
            self.L.mh_shutdown(self.h)
            self.h = None


class VoxelMap:
    """IncrementalVoxelMapPCL counterpart (include/mimosa/lidar/incremental_voxel_map.hpp:22-54)."""

    def __init__(self, ctx: Context, leaf=0.5, min_dist=0.15, max_pts=20, mode=19, lru_horizon=1000,
                 lru_clear_cycle=10, _h=None):
        self.ctx, self.L = ctx, ctx.L
        ctx._children += 1
        if _h is not None:
            self.h = _h
            return
        cfg = MapConfig(leaf, min_dist, max_pts, mode, lru_horizon, lru_clear_cycle, 0)
        h = C.c_void_p()
        ctx.check(self.L.mh_map_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def insert(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self.ctx.check(self.L.mh_map_insert(self.h, _p(xyz), xyz.shape[0], 3))

    def insert_from_scan(self, scan, R_W_Be, t_W_Be):
        R = np.ascontiguousarray(R_W_Be, np.float32)
        t = np.ascontiguousarray(t_W_Be, np.float32)
        self.ctx.check(self.L.mh_map_insert_from_scan(self.h, scan.h, _p(R), _p(t)))

    @staticmethod
    def _preview_dict(pv, outcome):
        d = {n: getattr(pv, n) for n, _ in pv._fields_}
        if outcome is not None:
            d["outcome"] = outcome
        return d

    def preview_insert(self, xyz, want_outcome=False):
        """mh_map_preview_insert: what insert(xyz) would do, read-only.  The six counts, plus `outcome` (uint8 per point:
        1 added, 2 too close, 3 voxel full) when asked for."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        pv = MapInsertPreview()
        oc = np.zeros(xyz.shape[0], np.uint8) if want_outcome else None
        self.ctx.check(self.L.mh_map_preview_insert(self.h, _p(xyz), xyz.shape[0], 3, C.byref(pv), _p(oc)))
        return self._preview_dict(pv, oc)

    def preview_insert_device(self, d_points, n, stride_floats, R=None, t=None, want_outcome=False):
        """mh_map_preview_insert_device: the same for n points at a device address, optionally through the f32 transform."""
        R = np.ascontiguousarray(R, np.float32) if R is not None else None
        t = np.ascontiguousarray(t, np.float32) if t is not None else None
        pv = MapInsertPreview()
        oc = np.zeros(n, np.uint8) if want_outcome else None
        self.ctx.check(self.L.mh_map_preview_insert_device(self.h, d_points, n, stride_floats, _p(R), _p(t), C.byref(pv), _p(oc)))
        return self._preview_dict(pv, oc)

    def preview_insert_from_scan(self, scan, R_W_Be, t_W_Be, want_outcome=False):
        """mh_map_preview_insert_from_scan: what insert_from_scan(scan, R, t) would do, read-only."""
        R = np.ascontiguousarray(R_W_Be, np.float32)
        t = np.ascontiguousarray(t_W_Be, np.float32)
        pv = MapInsertPreview()
        oc = None
        if want_outcome:
            d, n = C.c_void_p(), C.c_size_t()
            self.ctx.check(self.L.mh_scan_device_points(scan.h, Scan.BODY, C.byref(d), C.byref(n)))
            oc = np.zeros(n.value, np.uint8)
        self.ctx.check(self.L.mh_map_preview_insert_from_scan(self.h, scan.h, _p(R), _p(t), C.byref(pv), _p(oc)))
        return self._preview_dict(pv, oc)

    @staticmethod
    def _carve_args(origin_F, R_W_F, t_W_F, cfg):
        o, R, t = _f64(origin_F).reshape(3), _f64(R_W_F).reshape(9), _f64(t_W_F).reshape(3)
        return o, R, t, (cfg if isinstance(cfg, MapCarveConfig) else make_carve_config(**cfg)), MapCarveResult()

    def carve(self, obs_xyz, origin_F, R_W_F, t_W_F, cfg) -> dict:
        """mh_map_carve: remove (cfg.apply) or count (preview) the map points the observations see through.  obs_xyz: points in a
        frame F whose pose in the map frame is (R_W_F, t_W_F), sensor at origin_F in F.  cfg: MapCarveConfig or the keywords of
        make_carve_config.  Returns the six counters."""
        xyz = np.ascontiguousarray(obs_xyz, dtype=np.float32).reshape(-1, 3)
        o, R, t, cfg, out = self._carve_args(origin_F, R_W_F, t_W_F, cfg)
        self.ctx.check(self.L.mh_map_carve(self.h, _p(xyz), xyz.shape[0], 3, _p(o), _p(R), _p(t), C.byref(cfg), C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def carve_device(self, d_points, n, stride_floats, origin_F, R_W_F, t_W_F, cfg) -> dict:
        """mh_map_carve_device: the same for n points at a device address."""
        o, R, t, cfg, out = self._carve_args(origin_F, R_W_F, t_W_F, cfg)
        self.ctx.check(self.L.mh_map_carve_device(self.h, d_points, n, stride_floats, _p(o), _p(R), _p(t), C.byref(cfg), C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def carve_from_scan(self, scan, which, origin_F, R_W_F, t_W_F, cfg) -> dict:
        """mh_map_carve_from_scan: the same from a device-resident scan; which = Scan.FULL (lidar frame) or Scan.BODY (body frame)."""
        o, R, t, cfg, out = self._carve_args(origin_F, R_W_F, t_W_F, cfg)
        self.ctx.check(self.L.mh_map_carve_from_scan(self.h, scan.h, int(which), _p(o), _p(R), _p(t), C.byref(cfg), C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def copy(self):
        h = C.c_void_p()
        self.ctx.check(self.L.mh_map_copy(self.h, C.byref(h)))
        return VoxelMap(self.ctx, _h=h)

    def stats(self) -> dict:
        s = MapStats()
        self.ctx.check(self.L.mh_map_get_stats(self.h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in s._fields_}

    def get_cloud(self):
        n = C.c_size_t()
        self.ctx.check(self.L.mh_map_get_cloud(self.h, None, 0, C.byref(n)))
        xyz = np.empty((n.value, 3), np.float32)
        self.ctx.check(self.L.mh_map_get_cloud(self.h, _p(xyz), n.value, C.byref(n)))
        return xyz

    def knn(self, q, k=5):
        q = _f64(q).reshape(-1, 3)
        n = q.shape[0]
        pts = np.empty((n, k, 3))
        sq = np.empty((n, k))
        found = np.empty(n, np.int32)
        self.ctx.check(self.L.mh_map_knn(self.h, _p(q), n, k, _p(pts), _p(sq), _p(found)))
        return pts, sq, found

    def release(self):
        if getattr(self, "h", None):
            self.L.mh_map_release(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Scan:
    """Device-resident scan front end: Manager::prepareInput -> deskewPoints -> Geometric::preprocess
    (src/lidar/manager.cpp:149-512, src/lidar/geometric.cpp:55-183) with the cloud staying on the GPU."""
    FULL, BODY, DOWNSAMPLED = 0, 1, 2

    def __init__(self, ctx: Context):
        self.ctx, self.L = ctx, ctx.L
        ctx._children += 1
        h = C.c_void_p()
        ctx.check(self.L.mh_scan_create(ctx.h, C.byref(h)))
        self.h = h

    def prepare_input(self, raw, cfg: InputConfig) -> dict:
        raw = np.ascontiguousarray(raw)
        assert raw.dtype.itemsize == 32
        info = ScanInfo()
        self.ctx.check(self.L.mh_scan_prepare_input(self.h, _p(raw), len(raw), C.byref(cfg), C.byref(info)))
        return info.as_dict()

    def prepare_input_layout(self, raw, layout: PointLayout, cfg: InputConfig, width=None, height=1, transpose=False, organize_by_ring=False,
                             header_ts=0.0) -> dict:
        """Manager::prepareInput<PointT> for any point record described by `layout` (see POINT_TYPES)."""
        raw = np.ascontiguousarray(raw)
        assert raw.dtype.itemsize == layout.stride
        n = len(raw)
        width = n if width is None else width
        info = ScanInfo()
        self.ctx.check(self.L.mh_scan_prepare_input_layout(self.h, _p(raw), n, C.byref(layout), width, height, int(transpose),
                                                           int(organize_by_ring), header_ts, C.byref(cfg), C.byref(info)))
        return info.as_dict()

    def prefetch(self, raw):
        """stage the next cloud: pinned copy + host-to-device copy on the handle's copy stream (returns before the copy is done)"""
        raw = np.ascontiguousarray(raw)
        assert raw.dtype.itemsize == 32
        self.ctx.check(self.L.mh_scan_prefetch(self.h, _p(raw), len(raw)))

    def prepare_input_prefetched(self, cfg: InputConfig) -> dict:
        info = ScanInfo()
        self.ctx.check(self.L.mh_scan_prepare_input_prefetched(self.h, C.byref(cfg), C.byref(info)))
        return info.as_dict()

    def prepare_input_device(self, d_raw_ptr: int, n: int, cfg: InputConfig) -> dict:
        """raw cloud (32-byte Ouster records) already in device memory at address d_raw_ptr"""
        info = ScanInfo()
        self.ctx.check(self.L.mh_scan_prepare_input_device(self.h, C.c_void_p(d_raw_ptr), n, C.byref(cfg), C.byref(info)))
        return info.as_dict()

    def unique_ns(self):
        n = C.c_size_t()
        self.ctx.check(self.L.mh_scan_get_unique_ns(self.h, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint32)
        self.ctx.check(self.L.mh_scan_get_unique_ns(self.h, _p(out), out.size, C.byref(n)))
        return out

    def deskew(self, Rt12):
        P = np.ascontiguousarray(Rt12, dtype=np.float32).reshape(-1, 12)
        self.ctx.check(self.L.mh_scan_deskew(self.h, _p(P), len(P)))

    def deskew_imu(self, segments, header_ts, gravity, T_Le_W, T_B_S):
        """Manager::deskewPoints with the per-timestamp poses computed on the device (src/lidar/manager.cpp:455-509).
        segments: IMU_SEGMENT_DTYPE records (imu_segments builds them); gravity = unit vector * |g|; T_* = (R 3x3, t 3)."""
        seg = np.ascontiguousarray(segments, dtype=IMU_SEGMENT_DTYPE)
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        g, Rl, tl, Rb, tb = d(gravity), d(T_Le_W[0]), d(T_Le_W[1]), d(T_B_S[0]), d(T_B_S[1])
        self.ctx.check(self.L.mh_scan_deskew_imu(self.h, _p(seg) if len(seg) else None, len(seg), float(header_ts), _p(g), _p(Rl), _p(tl),
                                                 _p(Rb), _p(tb)))

    def deskew_poses(self):
        """T_Le_Lt per distinct timestamp as mh_scan_deskew_imu left it on the device: (n, 12) doubles, R row-major then t."""
        n = C.c_size_t()
        self.ctx.check(self.L.mh_scan_get_deskew_poses(self.h, None, 0, C.byref(n)))
        out = np.empty((n.value, 12), np.float64)
        self.ctx.check(self.L.mh_scan_get_deskew_poses(self.h, _p(out), n.value, C.byref(n)))
        return out

    def preprocess_geometric(self, R_B_L, t_B_L, leaf=0.5, max_pts=20, min_dist=0.15) -> dict:
        R = np.ascontiguousarray(R_B_L, dtype=np.float32)
        t = np.ascontiguousarray(t_B_L, dtype=np.float32)
        info = ScanInfo()
        self.ctx.check(self.L.mh_scan_preprocess_geometric(self.h, _p(R), _p(t), float(leaf), int(max_pts), float(min_dist),
                                                           C.byref(info)))
        return info.as_dict()

    def points(self, which):
        from .synth import POINT_DTYPE
        n = C.c_size_t()
        self.ctx.check(self.L.mh_scan_get_points(self.h, which, None, 0, C.byref(n)))
        out = np.zeros(n.value, POINT_DTYPE)
        self.ctx.check(self.L.mh_scan_get_points(self.h, which, _p(out), out.size, C.byref(n)))
        return out

    def indices(self, which):
        n = C.c_size_t()
        self.ctx.check(self.L.mh_scan_get_indices(self.h, which, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint32)
        self.ctx.check(self.L.mh_scan_get_indices(self.h, which, _p(out), out.size, C.byref(n)))
        return out

    def make_factor(self, map_, cfg: RegConfig, binary=False):
        h = C.c_void_p()
        self.ctx.check(self.L.mh_icp_create_from_scan(self.ctx.h, map_.h, self.h, C.byref(cfg), int(binary), C.byref(h)))
        n = int(self.L.mh_icp_size(h))
        f = ICPFactor(self.ctx, map_, None, None, _h=h, _n=n)
        f._keep = []
        return f

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_scan_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def linearize_batch(factors, Rs, ts, g_units=None, R_tgts=None, t_tgts=None) -> list:
    """mh_icp_linearize_batch: every factor of `factors` linearized at its own pose in one K3 + one K4 launch."""
    n = len(factors)
    ctx = factors[0].ctx
    R = np.ascontiguousarray(np.asarray(Rs, np.float64).reshape(n, 9))
    t = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(n, 3))
    g = np.ascontiguousarray(np.tile(np.array([0.0, 0.0, -1.0]), (n, 1)) if g_units is None else np.asarray(g_units, np.float64).reshape(n, 3))
    Rt = None if R_tgts is None else np.ascontiguousarray(np.asarray(R_tgts, np.float64).reshape(n, 9))
    tt = None if t_tgts is None else np.ascontiguousarray(np.asarray(t_tgts, np.float64).reshape(n, 3))
    handles = (C.c_void_p * n)(*[f.h for f in factors])
    out = (IcpResult * n)()
    ctx.check(ctx.L.mh_icp_linearize_batch(handles, n, _p(R), _p(t), _p(Rt), _p(tt), _p(g), out))
    return [out[i].as_dict() for i in range(n)]


class AlignBatchCall:
    """an mh_icp_align_batch_async call in flight: wait() collects it and returns the list of results"""

    def __init__(self, ctx, keep, out):
        self.ctx, self._keep, self.out = ctx, keep, out

    def wait(self) -> list:
        self.ctx.check(self.ctx.L.mh_icp_align_batch_wait(self.ctx.h))
        res = [r.as_dict() for r in self.out]
        self._keep = None
        return res


def align_batch(factors, poses, cfg: AlignConfig, g_unit=(0.0, 0.0, -1.0), wait=True):
    """mh_icp_align_batch: the alignments of `factors`, member i from poses[i] = (R, t), side by side in one chain of launches.
    Returns the list of the dicts ICPFactor.align returns, one per member.  wait=False: mh_icp_align_batch_async; returns an
    AlignBatchCall whose wait() gives the same list."""
    B = len(factors)
    if B == 0:
        raise ValueError("align_batch: no factor")
    if len(poses) != B:
        raise ValueError("align_batch: one start pose per factor")
    ctx = factors[0].ctx
    R = np.ascontiguousarray(np.array([np.asarray(p[0], np.float64).reshape(9) for p in poses]))
    t = np.ascontiguousarray(np.array([np.asarray(p[1], np.float64).reshape(3) for p in poses]))
    g = _f64(g_unit)
    handles = (C.c_void_p * B)(*[f.h for f in factors])
    out = (AlignResult * B)()
    if not wait:
        ctx.check(ctx.L.mh_icp_align_batch_async(handles, B, _p(R), _p(t), _p(g), C.byref(cfg), out))
        return AlignBatchCall(ctx, (handles, R, t, g, cfg), out)
    ctx.check(ctx.L.mh_icp_align_batch(handles, B, _p(R), _p(t), _p(g), C.byref(cfg), out))
    return [r.as_dict() for r in out]


class WindowCall:
    """an mh_icp_window_optimise_async call in flight: wait() collects it and returns the result"""

    def __init__(self, ctx, keep, out, trace, masks=None):
        self.ctx, self._keep, self.out, self.trace, self.masks = ctx, keep, out, trace, masks

    def wait(self) -> dict:
        self.ctx.check(self.ctx.L.mh_icp_window_wait(self.ctx.h))
        d = self.out.as_dict()
        if self.trace is not None:
            d["poses"] = self.trace[:d["iters"]]
        if self.masks is not None:
            d["evaluated"] = self.masks[:d["iters"]].copy()
        self._keep = None
        return d


def optimise_window(factors, poses, cfg: WindowConfig, has_Z=None, Z=None, g_unit=(0.0, 0.0, -1.0), trace_poses=False, wait=True, relin=None, linear=None,
                    edges=None, joint=None):
    """mh_icp_window_optimise: the fixed-lag Gauss-Newton loop over `factors` (oldest first) as one chain of launches.
    poses: (R, t) per factor; Z: (R, t) per factor, entry i the measured T_{i-1}^-1 T_i where has_Z[i] (entry 0 unused).
    trace_poses: also return "poses", (iters, W, 12) — R row-major then t after every executed step.
    wait=False: mh_icp_window_optimise_async; returns a WindowCall whose wait() gives the same dict.
    relin=(rot, trans): mh_icp_window_optimise_relin — a factor is evaluated again only once its pose has moved past these
    thresholds (rad, m) from the pose of its last evaluation; also returns "evaluated", per executed iteration the mask of the
    factors that ran K3.
    linear=[...]: mh_icp_window_optimise_lin (with or without relin) — Hessian factors the host linearized once, each a dict
    {"pose": index, "at": (R, t) of its linearization, "H": 6 x 6, "b": 6, "f": float} (make_window_linear); an empty list takes
    the same entry point with no factor.
    edges=[...]: mh_icp_window_optimise_edges (with or without relin and linear) — between factors on any pair of poses, each a
    dict {"a": i, "b": j, "Z": (R, t) the measured T_a^-1 T_b, "info": 6 x 6} (make_window_edge); an empty list takes the same
    entry point with no edge.  None: the dispatch above, untouched.
    joint={...}: mh_icp_window_optimise_joint (with or without relin, linear and edges) — one dense factor on up to four poses, a
    dict {"poses": ascending indices, "at": [(R, t)] per member, "H": 6n x 6n, "b": 6n, "f": float} (make_window_joint), what
    marginalise_window_joint returns as "joint".  None: the dispatch above, untouched."""
    W = len(factors)
    ctx = factors[0].ctx
    R = np.ascontiguousarray(np.array([np.asarray(p[0], np.float64).reshape(9) for p in poses]))
    t = np.ascontiguousarray(np.array([np.asarray(p[1], np.float64).reshape(3) for p in poses]))
    hz = np.zeros(W, np.int32) if has_Z is None else np.ascontiguousarray(np.asarray(has_Z).astype(np.int32))
    ZR = Zt = None
    if Z is not None:
        ZR = np.ascontiguousarray(np.array([np.asarray(z[0], np.float64).reshape(9) for z in Z]))
        Zt = np.ascontiguousarray(np.array([np.asarray(z[1], np.float64).reshape(3) for z in Z]))
    g = _f64(g_unit)
    handles = (C.c_void_p * W)(*[f.h for f in factors])
    out = WindowResult()
    trace = np.full((int(cfg.iters), W, 12), np.nan) if trace_poses else None
    if joint is not None:
        rl = None if relin is None else WindowRelin(float(relin[0]), float(relin[1]))
        masks = None if relin is None else np.zeros(max(int(cfg.iters), 1), np.uint32)
        lin, ed, jt = make_window_linear(linear or []), make_window_edge(edges or []), make_window_joint(joint)
        args = (handles, W, _p(R), _p(t), _p(hz), _p(ZR), _p(Zt), _p(g), C.byref(cfg), None if rl is None else C.byref(rl), lin, len(linear or []), ed,
                len(edges or []), C.byref(out), _p(trace), _p(masks), C.byref(jt))
        if not wait:
            ctx.check(ctx.L.mh_icp_window_optimise_joint_async(*args))
            return WindowCall(ctx, (handles, R, t, hz, ZR, Zt, g, cfg, rl, lin, ed, jt), out, trace, masks)
        ctx.check(ctx.L.mh_icp_window_optimise_joint(*args))
        d = out.as_dict()
        if trace is not None:
            d["poses"] = trace[:d["iters"]]
        if masks is not None:
            d["evaluated"] = masks[:d["iters"]].copy()
        return d
    if edges is not None:
        rl = None if relin is None else WindowRelin(float(relin[0]), float(relin[1]))
        masks = None if relin is None else np.zeros(max(int(cfg.iters), 1), np.uint32)
        lin = make_window_linear(linear or [])
        ed = make_window_edge(edges)
        args = (handles, W, _p(R), _p(t), _p(hz), _p(ZR), _p(Zt), _p(g), C.byref(cfg), None if rl is None else C.byref(rl), lin, len(linear or []), ed, len(edges),
                C.byref(out), _p(trace), _p(masks))
        if not wait:
            ctx.check(ctx.L.mh_icp_window_optimise_edges_async(*args))
            return WindowCall(ctx, (handles, R, t, hz, ZR, Zt, g, cfg, rl, lin, ed), out, trace, masks)
        ctx.check(ctx.L.mh_icp_window_optimise_edges(*args))
        d = out.as_dict()
        if trace is not None:
            d["poses"] = trace[:d["iters"]]
        if masks is not None:
            d["evaluated"] = masks[:d["iters"]].copy()
        return d
    if linear is not None:
        rl = None if relin is None else WindowRelin(float(relin[0]), float(relin[1]))
        masks = None if relin is None else np.zeros(max(int(cfg.iters), 1), np.uint32)
        lin = make_window_linear(linear)
        args = (handles, W, _p(R), _p(t), _p(hz), _p(ZR), _p(Zt), _p(g), C.byref(cfg), None if rl is None else C.byref(rl), lin, len(linear), C.byref(out),
                _p(trace), _p(masks))
        if not wait:
            ctx.check(ctx.L.mh_icp_window_optimise_lin_async(*args))
            return WindowCall(ctx, (handles, R, t, hz, ZR, Zt, g, cfg, rl, lin), out, trace, masks)
        ctx.check(ctx.L.mh_icp_window_optimise_lin(*args))
        d = out.as_dict()
        if trace is not None:
            d["poses"] = trace[:d["iters"]]
        if masks is not None:
            d["evaluated"] = masks[:d["iters"]].copy()
        return d
    if relin is not None:
        rl = WindowRelin(float(relin[0]), float(relin[1]))
        masks = np.zeros(max(int(cfg.iters), 1), np.uint32)  # (a bad iters is the library's to refuse)
        args = (handles, W, _p(R), _p(t), _p(hz), _p(ZR), _p(Zt), _p(g), C.byref(cfg), C.byref(rl), C.byref(out), _p(trace), _p(masks))
        if not wait:
            ctx.check(ctx.L.mh_icp_window_optimise_relin_async(*args))
            return WindowCall(ctx, (handles, R, t, hz, ZR, Zt, g, cfg, rl), out, trace, masks)
        ctx.check(ctx.L.mh_icp_window_optimise_relin(*args))
        d = out.as_dict()
        if trace is not None:
            d["poses"] = trace[:d["iters"]]
        d["evaluated"] = masks[:d["iters"]].copy()
        return d
    args = (handles, W, _p(R), _p(t), _p(hz), _p(ZR), _p(Zt), _p(g), C.byref(cfg), C.byref(out), _p(trace))
    if not wait:
        ctx.check(ctx.L.mh_icp_window_optimise_async(*args))
        return WindowCall(ctx, (handles, R, t, hz, ZR, Zt, g, cfg), out, trace)
    ctx.check(ctx.L.mh_icp_window_optimise(*args))
    d = out.as_dict()
    if trace is not None:
        d["poses"] = trace[:d["iters"]]
    return d


def marginalise_window(factors, poses, cfg: WindowConfig, has_Z=None, Z=None, g_unit=(0.0, 0.0, -1.0), linear=None, edges=None, wait=True):
    """mh_icp_window_marginalise: what eliminating the oldest pose of the window leaves on pose 1, at `poses` (nothing is
    iterated).  The arguments are optimise_window's (of cfg: between_info, prior_info, damping).  Returns {"valid", "n_ties",
    "oldest": the oldest factor linearized at pose 0, "linear": the marginal as optimise_window(linear=[...]) takes it, its
    pose rebased to 0 for the window without its oldest pose}.  wait=False: mh_icp_window_marginalise_async; returns a
    WindowCall whose wait() gives the same dict."""
    W = len(factors)
    ctx = factors[0].ctx
    R = np.ascontiguousarray(np.array([np.asarray(p[0], np.float64).reshape(9) for p in poses]))
    t = np.ascontiguousarray(np.array([np.asarray(p[1], np.float64).reshape(3) for p in poses]))
    hz = np.zeros(W, np.int32) if has_Z is None else np.ascontiguousarray(np.asarray(has_Z).astype(np.int32))
    ZR = Zt = None
    if Z is not None:
        ZR = np.ascontiguousarray(np.array([np.asarray(z[0], np.float64).reshape(9) for z in Z]))
        Zt = np.ascontiguousarray(np.array([np.asarray(z[1], np.float64).reshape(3) for z in Z]))
    g = _f64(g_unit)
    handles = (C.c_void_p * W)(*[f.h for f in factors])
    out = WindowMarginal()
    lin, ed = make_window_linear(linear or []), make_window_edge(edges or [])
    args = (handles, W, _p(R), _p(t), _p(hz), _p(ZR), _p(Zt), _p(g), C.byref(cfg), lin, len(linear or []), ed, len(edges or []), C.byref(out))
    if not wait:
        ctx.check(ctx.L.mh_icp_window_marginalise_async(*args))
        return WindowCall(ctx, (handles, R, t, hz, ZR, Zt, g, cfg, lin, ed), out, None)
    ctx.check(ctx.L.mh_icp_window_marginalise(*args))
    return out.as_dict()


def marginalise_window_joint(factors, poses, cfg: WindowConfig, has_Z=None, Z=None, g_unit=(0.0, 0.0, -1.0), linear=None, edges=None, joint=None, wait=True):
    """mh_icp_window_marginalise_joint: marginalise_window for an oldest pose that is tied beyond pose 1 — by edges (0, b) or by
    the carried joint factor `joint` (a dict as optimise_window(joint=...) takes it; it must contain pose 0).  Returns {"valid",
    "n_ties", "oldest", "joint_here": the marginal on its separator with this window's pose indices, "joint": the same rebased to
    the window without its oldest pose, every index minus one}.  wait=False: the _async form; returns a WindowCall."""
    W = len(factors)
    ctx = factors[0].ctx
    R = np.ascontiguousarray(np.array([np.asarray(p[0], np.float64).reshape(9) for p in poses]))
    t = np.ascontiguousarray(np.array([np.asarray(p[1], np.float64).reshape(3) for p in poses]))
    hz = np.zeros(W, np.int32) if has_Z is None else np.ascontiguousarray(np.asarray(has_Z).astype(np.int32))
    ZR = Zt = None
    if Z is not None:
        ZR = np.ascontiguousarray(np.array([np.asarray(z[0], np.float64).reshape(9) for z in Z]))
        Zt = np.ascontiguousarray(np.array([np.asarray(z[1], np.float64).reshape(3) for z in Z]))
    g = _f64(g_unit)
    handles = (C.c_void_p * W)(*[f.h for f in factors])
    out = WindowJointMarginal()
    lin, ed = make_window_linear(linear or []), make_window_edge(edges or [])
    jt = None if joint is None else make_window_joint(joint)
    args = (handles, W, _p(R), _p(t), _p(hz), _p(ZR), _p(Zt), _p(g), C.byref(cfg), lin, len(linear or []), ed, len(edges or []),
            None if jt is None else C.byref(jt), C.byref(out))
    if not wait:
        ctx.check(ctx.L.mh_icp_window_marginalise_joint_async(*args))
        return WindowCall(ctx, (handles, R, t, hz, ZR, Zt, g, cfg, lin, ed, jt), out, None)
    ctx.check(ctx.L.mh_icp_window_marginalise_joint(*args))
    return out.as_dict()


class ICPFactor:
    """lidar::ICPFactor counterpart (include/mimosa/lidar/geometric_factor.hpp:25-563)."""

    def __init__(self, ctx: Context, map_: VoxelMap, pts, cfg: RegConfig, binary=False, _h=None, _n=None):
        self.ctx, self.L, self.map = ctx, ctx.L, map_
        self._reloc_work = []  # relocalise(batch=True): the clones its candidates are aligned on
        ctx._children += 1
        if _h is not None:
            self.h, self.n = _h, _n
            return
        pts = np.ascontiguousarray(pts)
        assert pts.dtype.itemsize == 32
        h = C.c_void_p()
        ctx.check(self.L.mh_icp_create(ctx.h, map_.h, _p(pts), len(pts), C.byref(cfg), int(binary), C.byref(h)))
        self.h, self.n = h, len(pts)
        self._keep = []

    def clone(self):
        h = C.c_void_p()
        self.ctx.check(self.L.mh_icp_clone(self.h, C.byref(h)))
        c = ICPFactor(self.ctx, self.map, None, None, _h=h, _n=self.n)
        c._keep = []
        return c

    def linearize(self, R, t, g_unit=(0.0, 0.0, -1.0), R_tgt=None, t_tgt=None) -> dict:
        out = IcpResult()
        R, t, g = _f64(R), _f64(t), _f64(g_unit)
        Rt = _f64(R_tgt) if R_tgt is not None else None
        tt = _f64(t_tgt) if t_tgt is not None else None
        self.ctx.check(self.L.mh_icp_linearize(self.h, _p(R), _p(t), _p(Rt), _p(tt), _p(g), C.byref(out)))
        return out.as_dict()

    def linearize_async(self, R, t, g_unit=(0.0, 0.0, -1.0)) -> IcpResult:
        out = IcpResult()
        R, t, g = _f64(R), _f64(t), _f64(g_unit)
        self._keep.append((out, R, t, g))
        self.ctx.check(self.L.mh_icp_linearize_async(self.h, _p(R), _p(t), None, None, _p(g), C.byref(out)))
        return out

    def wait(self):
        self.ctx.check(self.L.mh_icp_wait(self.h))
        self._keep = []

    def reset(self):
        self.ctx.check(self.L.mh_icp_reset(self.h))

    def align(self, R0, t0, cfg: AlignConfig, g_unit=(0.0, 0.0, -1.0)) -> dict:
        """mh_icp_align: the Gauss-Newton loop from (R0, t0) as one chain of launches; pose, trace, first / last results."""
        out = AlignResult()
        R, t, g = _f64(R0), _f64(t0), _f64(g_unit)
        self.ctx.check(self.L.mh_icp_align(self.h, _p(R), _p(t), _p(g), C.byref(cfg), C.byref(out)))
        return out.as_dict()

    def align_async(self, R0, t0, cfg: AlignConfig, g_unit=(0.0, 0.0, -1.0)) -> AlignResult:
        """mh_icp_align_async: collected by wait(); the returned struct is filled then (as_dict())."""
        out = AlignResult()
        R, t, g = _f64(R0), _f64(t0), _f64(g_unit)
        self._keep.append((out, R, t, g, cfg))
        self.ctx.check(self.L.mh_icp_align_async(self.h, _p(R), _p(t), _p(g), C.byref(cfg), C.byref(out)))
        return out

    def _score_args(self, R, t, gate, stride, top_k, want_scores):
        R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 9))
        t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1, 3))
        assert len(R) == len(t)
        cfg = ScoreConfig(gate, stride, top_k)
        scores = np.zeros(len(R), POSE_SCORE_DTYPE) if want_scores else None
        best = np.full(MH_RELOC_MAX_REFINE, -2, np.int32) if top_k > 0 else None
        return R, t, cfg, scores, best

    def score_poses(self, R, t, gate, stride=1, top_k=0, want_scores=True):
        """mh_icp_score_poses: R [n, 3, 3], t [n, 3].  Returns (scores, best): scores a POSE_SCORE_DTYPE array (None without
        want_scores: scores = NULL, nothing but the winners is downloaded), best the top_k pose indices in rank order (None for
        top_k == 0; -1 behind the last pose)."""
        R, t, cfg, scores, best = self._score_args(R, t, gate, stride, top_k, want_scores)
        self.ctx.check(self.L.mh_icp_score_poses(self.h, _p(R), _p(t), len(R), C.byref(cfg), _p(scores), _p(best)))
        return scores, (best[:top_k] if best is not None else None)

    def score_poses_async(self, R, t, gate, stride=1, top_k=0, want_scores=True):
        """mh_icp_score_poses_async: collected by wait(); the returned arrays (scores, all MH_RELOC_MAX_REFINE entries of best) are
        filled then."""
        R, t, cfg, scores, best = self._score_args(R, t, gate, stride, top_k, want_scores)
        self._keep.append((R, t, cfg, scores, best))
        self.ctx.check(self.L.mh_icp_score_poses_async(self.h, _p(R), _p(t), len(R), C.byref(cfg), _p(scores), _p(best)))
        return scores, best

    def relocalise(self, R, t, cfg: RelocConfig, g_unit=(0.0, 0.0, -1.0), batch=False) -> dict:
        """mh_icp_relocalise: score the poses, align the cfg.score.top_k best, re-score; the factor is left reset.
        batch=True: mh_icp_relocalise_batch — the candidates are aligned side by side on clones of this factor, which are made
        on first use, kept on this object and destroyed with it (or by release_reloc_work()); this factor is only read."""
        R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 9))
        t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1, 3))
        assert len(R) == len(t)
        g = _f64(g_unit)
        out = RelocResult()
        if batch:
            work = self._reloc_work
            while len(work) < min(int(cfg.score.top_k), len(R)):
                work.append(self.clone())
            handles = (C.c_void_p * max(len(work), 1))(*[w.h for w in work])
            self.ctx.check(self.L.mh_icp_relocalise_batch(self.h, handles, len(work), _p(R), _p(t), len(R), _p(g), C.byref(cfg), C.byref(out)))
            return out.as_dict()
        self.ctx.check(self.L.mh_icp_relocalise(self.h, _p(R), _p(t), len(R), _p(g), C.byref(cfg), C.byref(out)))
        return out.as_dict()

    def set_components(self, enabled: bool):
        """component localizabilities + status histogram (K4) on / off for the following linearize calls"""
        self.ctx.check(self.L.mh_icp_set_components(self.h, int(bool(enabled))))

    def state(self):
        st = np.empty(self.n, np.int32)
        means = np.empty((self.n, 3))
        normals = np.empty((self.n, 3))
        self.ctx.check(self.L.mh_icp_get_state(self.h, _p(st), _p(means), _p(normals)))
        return st, means, normals

    def release_reloc_work(self):
        """destroy the clones relocalise(batch=True) made; the next such call makes new ones"""
        work, self._reloc_work = getattr(self, "_reloc_work", []), []
        for w in work:
            w.destroy()

    def destroy(self):
        self.release_reloc_work()
        if getattr(self, "h", None):
            self.L.mh_icp_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class ShardComm:
    """mh_shard_comm: the communicator of the native map-sharded factor.  rccl(): one process per GPU, the 128-byte
    ncclUniqueId travels through whatever channel the caller has (torch.distributed in bench.py); local(): `world` ranks inside
    this process, one host thread each (tests on a one-GPU box)."""

    def __init__(self, L, h):
        self.L, self.h = L, h

    @staticmethod
    def unique_id() -> bytes:
        L = load()
        buf = C.create_string_buffer(SHARD_UNIQUE_ID_BYTES)
        rc = L.mh_shard_unique_id(buf)
        if rc != MH_OK:
            raise MhError(rc, (L.mh_last_error(None) or b"").decode())
        return buf.raw

    @staticmethod
    def rccl(ctx: "Context", unique_id: bytes, world: int, rank: int) -> "ShardComm":
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), SHARD_UNIQUE_ID_BYTES)
        ctx.check(ctx.L.mh_shard_comm_init_rccl(ctx.h, buf, world, rank, C.byref(h)))
        return ShardComm(ctx.L, h)

    @staticmethod
    def local(world: int) -> list:
        L = load()
        arr = (C.c_void_p * world)()
        rc = L.mh_shard_comm_init_local(world, arr)
        if rc != MH_OK:
            raise MhError(rc, (L.mh_last_error(None) or b"").decode())
        return [ShardComm(L, C.c_void_p(arr[r])) for r in range(world)]

    @property
    def world(self):
        return int(self.L.mh_shard_comm_world(self.h))

    @property
    def rank(self):
        return int(self.L.mh_shard_comm_rank(self.h))

    @property
    def backend(self):
        return self.L.mh_shard_comm_backend(self.h).decode()

    def info(self) -> dict:
        n, v = C.c_int(0), C.c_int(0)
        self.L.mh_shard_comm_info(self.h, C.byref(n), C.byref(v))
        return {"ranks_in_communicator": n.value, "rccl_version": v.value}

    def destroy(self):
        if self.h:
            self.L.mh_shard_comm_destroy(self.h)
            self.h = None


class ShardedICPFactor:
    """mh_shard_icp: this rank's part of a scan-to-map factor whose map is sharded across GPUs; linearize() is collective
    and returns the GLOBAL result on every rank."""

    def __init__(self, ctx: Context, comm: ShardComm, shard_map: VoxelMap, pts, cfg: RegConfig, binary=False, block_log2=3, force_collectives=False,
                 d_points_ptr=None, n_device=0):
        self.ctx, self.L, self.comm, self.map = ctx, ctx.L, comm, shard_map
        ctx._children += 1
        sc = ShardConfig(block_log2, int(bool(force_collectives)))
        h = C.c_void_p()
        if d_points_ptr is not None:
            ctx.check(self.L.mh_shard_icp_create(ctx.h, comm.h, shard_map.h, C.c_void_p(d_points_ptr), n_device, 1, C.byref(cfg), int(binary), C.byref(sc), C.byref(h)))
        else:
            pts = np.ascontiguousarray(pts)
            assert pts.dtype.itemsize == 32
            ctx.check(self.L.mh_shard_icp_create(ctx.h, comm.h, shard_map.h, _p(pts), len(pts), 0, C.byref(cfg), int(binary), C.byref(sc), C.byref(h)))
        self.h = h

    def linearize(self, R, t, g_unit=(0.0, 0.0, -1.0), R_tgt=None, t_tgt=None) -> dict:
        out = IcpResult()
        R, t, g = _f64(R), _f64(t), _f64(g_unit)
        Rt = _f64(R_tgt) if R_tgt is not None else None
        tt = _f64(t_tgt) if t_tgt is not None else None
        self.ctx.check(self.L.mh_shard_icp_linearize(self.h, _p(R), _p(t), _p(Rt), _p(tt), _p(g), C.byref(out)))
        return out.as_dict()

    def linearize_async(self, R, t, g_unit=(0.0, 0.0, -1.0), R_tgt=None, t_tgt=None) -> IcpResult:
        """mh_shard_icp_linearize_async: enqueue only; the returned IcpResult is filled by wait() (collective, like linearize)."""
        out = IcpResult()
        R, t, g = _f64(R), _f64(t), _f64(g_unit)
        Rt = _f64(R_tgt) if R_tgt is not None else None
        tt = _f64(t_tgt) if t_tgt is not None else None
        self.ctx.check(self.L.mh_shard_icp_linearize_async(self.h, _p(R), _p(t), _p(Rt), _p(tt), _p(g), C.byref(out)))
        self._pending = getattr(self, "_pending", [])
        self._pending.append(out)  # the library writes into it at wait()
        return out

    def wait(self):
        """mh_shard_icp_wait: completes every round in flight on this factor's communicator."""
        self.ctx.check(self.L.mh_shard_icp_wait(self.h))
        self._pending = []

    def reset(self):
        self.ctx.check(self.L.mh_shard_icp_reset(self.h))

    def set_components(self, enabled: bool):
        self.ctx.check(self.L.mh_shard_icp_set_components(self.h, int(bool(enabled))))

    def stats(self) -> dict:
        s = ShardStats()
        self.ctx.check(self.L.mh_shard_icp_stats(self.h, C.byref(s)))
        return s.as_dict()

    def state(self):
        """(origin, status, mean, normal) of the points this rank holds now."""
        n = C.c_size_t()
        self.ctx.check(self.L.mh_shard_icp_get_state(self.h, None, None, None, None, 0, C.byref(n)))
        n = int(n.value)
        origin, st = np.empty(n, np.uint64), np.empty(n, np.int32)
        mean, nrm = np.empty((n, 3)), np.empty((n, 3))
        m = C.c_size_t()
        self.ctx.check(self.L.mh_shard_icp_get_state(self.h, _p(origin), _p(st), _p(mean), _p(nrm), n, C.byref(m)))
        assert int(m.value) == n
        return origin, st, mean, nrm

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_shard_icp_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class _ShardBatchArgs:
    """Marshalled arguments of a sharded batch call (kept alive until the results are in)."""

    def __init__(self, factors, Rs, ts, g_units, R_tgts, t_tgts):
        n = len(factors)
        self.n = n
        self.R = np.ascontiguousarray(np.asarray(Rs, np.float64).reshape(n, 9))
        self.t = np.ascontiguousarray(np.asarray(ts, np.float64).reshape(n, 3))
        self.g = np.ascontiguousarray(np.tile(np.array([0.0, 0.0, -1.0]), (n, 1)) if g_units is None else np.asarray(g_units, np.float64).reshape(n, 3))
        self.Rt = None if R_tgts is None else np.ascontiguousarray(np.asarray(R_tgts, np.float64).reshape(n, 9))
        self.tt = None if t_tgts is None else np.ascontiguousarray(np.asarray(t_tgts, np.float64).reshape(n, 3))
        self.handles = (C.c_void_p * n)(*[f.h for f in factors])
        self.out = (IcpResult * n)()

    def args(self):
        return (self.handles, self.n, _p(self.R), _p(self.t), _p(self.Rt), _p(self.tt), _p(self.g), self.out)

    def results(self) -> list:
        return [self.out[i].as_dict() for i in range(self.n)]


def sharded_linearize_batch(factors, Rs, ts, g_units=None, R_tgts=None, t_tgts=None) -> list:
    """mh_shard_icp_linearize_batch: the sharded factors of `factors` (one communicator) in ONE protocol round; blocks; collective."""
    a = _ShardBatchArgs(factors, Rs, ts, g_units, R_tgts, t_tgts)
    factors[0].ctx.check(factors[0].L.mh_shard_icp_linearize_batch(*a.args()))
    return a.results()


def sharded_linearize_batch_async(factors, Rs, ts, g_units=None, R_tgts=None, t_tgts=None) -> _ShardBatchArgs:
    """mh_shard_icp_linearize_batch_async: enqueue one round; `.results()` of the returned object is valid after factors[0].wait()."""
    a = _ShardBatchArgs(factors, Rs, ts, g_units, R_tgts, t_tgts)
    factors[0].ctx.check(factors[0].L.mh_shard_icp_linearize_batch_async(*a.args()))
    return a


def alloc_check_stats():
    """(blocks verified at hand-out, words found overwritten) of the allocation cache's MH_ALLOC_CHECK mode; None when it is off."""
    a, b = C.c_ulonglong(), C.c_ulonglong()
    if load().mh_alloc_check_stats(C.byref(a), C.byref(b)) != 0:
        return None
    return int(a.value), int(b.value)


def map_insert_shard_from_scan(ctx: Context, vmap: VoxelMap, scan, R_W_Be, t_W_Be, world: int, rank: int, block_log2: int = 3):
    """mh_map_insert_shard_from_scan: one rank's share of Geometric::updateMap's insert of the resident scan's Be_cloud_, on the device."""
    R = np.ascontiguousarray(R_W_Be, np.float32)
    t = np.ascontiguousarray(t_W_Be, np.float32)
    ctx.check(ctx.L.mh_map_insert_shard_from_scan(vmap.h, scan.h, _p(R), _p(t), world, rank, block_log2))


def map_insert_shard(ctx: Context, vmap: VoxelMap, xyz, world: int, rank: int, block_log2: int = 3):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    ctx.check(ctx.L.mh_map_insert_shard(vmap.h, _p(xyz), len(xyz), 3, world, rank, block_log2))


class _PhotoBase:
    """Shared marshalling of the photometric entry points: the product (libmimosa_hip.so, prefix mh_photo) and the
    checker (oracle/photo_ref.py, prefix refphoto) export the same shapes."""

    def _features_from(self, nf, npt, get):
        feats = (PhotoFeature * max(nf, 1))()
        Le, I, psi = np.zeros((max(npt, 1), 3)), np.zeros(max(npt, 1)), np.zeros(max(npt, 1))
        get(feats, _p(Le), _p(I), _p(psi))
        out, o = [], 0
        for i in range(nf):
            m = feats[i].n_points
            out.append(dict(id=int(feats[i].id), life_time=int(feats[i].life_time), center=np.array(feats[i].center),
                            normal=np.array(feats[i].normal), mean_intensity=feats[i].mean_intensity,
                            sigma_intensity=feats[i].sigma_intensity, Le_ps=Le[o:o + m].copy(), intensities=I[o:o + m].copy(),
                            psi=psi[o:o + m].copy()))
            o += m
        return out

    @staticmethod
    def _features_to(features):
        nf = len(features)
        feats = (PhotoFeature * max(nf, 1))()
        Le, I, psi = [], [], []
        for i, f in enumerate(features):
            feats[i].id, feats[i].life_time, feats[i].n_points = f["id"], f["life_time"], len(f["Le_ps"])
            feats[i].center[0], feats[i].center[1] = f["center"]
            for k in range(3):
                feats[i].normal[k] = f["normal"][k]
            feats[i].mean_intensity, feats[i].sigma_intensity = f["mean_intensity"], f["sigma_intensity"]
            Le.append(np.asarray(f["Le_ps"], float).reshape(-1, 3))
            I.append(np.asarray(f["intensities"], float))
            psi.append(np.asarray(f["psi"], float))
        Le = np.ascontiguousarray(np.concatenate(Le)) if nf else np.zeros((1, 3))
        I = np.ascontiguousarray(np.concatenate(I)) if nf else np.zeros(1)
        psi = np.ascontiguousarray(np.concatenate(psi)) if nf else np.zeros(1)
        return feats, Le, I, psi


class Photo(_PhotoBase):
    """lidar::Photometric counterpart (include/mimosa/lidar/photometric.hpp:22-86) over mh_photo_*."""

    def __init__(self, ctx: Context, cfg: dict):
        self.ctx, self.L = ctx, ctx.L
        self.cfgd = cfg
        self.c, self._keep = make_photo_config(cfg)
        self.rows, self.cols = cfg["rows"], cfg["cols"]
        h = C.c_void_p()
        ctx.check(self.L.mh_photo_create(ctx.h, C.byref(self.c), C.byref(h)))
        self.h = h
        ctx._children += 1

    def preprocess(self, raw, desk, unique_ns, T_Le_Lt):
        """Returns the deskewed cloud with the corrected intensities (a copy)."""
        raw, desk = np.ascontiguousarray(raw), np.array(desk, copy=True)
        ns = np.ascontiguousarray(unique_ns, np.uint32)
        T = np.ascontiguousarray(np.asarray(T_Le_Lt, np.float64).reshape(len(ns), 12))
        self.ctx.check(self.L.mh_photo_preprocess(self.h, _p(raw), _p(desk), len(desk), _p(ns), _p(T), len(ns)))
        return desk

    def preprocess_scan(self, scan, T_Le_Lt):
        T = np.ascontiguousarray(np.asarray(T_Le_Lt, np.float64).reshape(-1, 12))
        self.ctx.check(self.L.mh_photo_preprocess_scan(self.h, scan.h, _p(T), len(T)))

    def preprocess_scan_begin(self, scan, T_Le_Lt):
        """Builds the frame without making it current (may overlap update_map of the previous scan on another thread)."""
        T = np.ascontiguousarray(np.asarray(T_Le_Lt, np.float64).reshape(-1, 12))
        self.ctx.check(self.L.mh_photo_preprocess_scan_begin(self.h, scan.h, _p(T), len(T)))

    def preprocess_commit(self):
        self.ctx.check(self.L.mh_photo_preprocess_commit(self.h))

    def preprocess_scan_resident(self, scan):
        """preprocess_scan with T_Le_Lt read from the table Scan.deskew_imu left on the device."""
        self.ctx.check(self.L.mh_photo_preprocess_scan_resident(self.h, scan.h))

    def preprocess_scan_begin_resident(self, scan):
        self.ctx.check(self.L.mh_photo_preprocess_scan_begin_resident(self.h, scan.h))

    def detect_prefetch(self):
        self.ctx.check(self.L.mh_photo_detect_prefetch(self.h))

    def image(self, name):
        which, dt, k = PHOTO_IMAGES[name]
        out = np.empty((self.rows, self.cols, k) if k > 1 else (self.rows, self.cols), dt)
        self.ctx.check(self.L.mh_photo_get_image(self.h, which, _p(out), out.nbytes))
        return out

    def features(self):
        nf, npt = C.c_size_t(), C.c_size_t()
        self.ctx.check(self.L.mh_photo_num_features(self.h, C.byref(nf), C.byref(npt)))
        return self._features_from(nf.value, npt.value,
                                   lambda f, a, b, c: self.ctx.check(self.L.mh_photo_get_features(self.h, f, a, b, c)))

    def set_features(self, features):
        feats, Le, I, psi = self._features_to(features)
        self.ctx.check(self.L.mh_photo_set_features(self.h, feats, len(features), _p(Le), _p(I), _p(psi)))

    def detect(self, num, R_W_Be, t_W_Be, bias_directions):
        R, t, b = _f64(R_W_Be), _f64(t_W_Be), np.ascontiguousarray(np.asarray(bias_directions, np.float64).reshape(-1, 3))
        self.ctx.check(self.L.mh_photo_detect_features(self.h, int(num), _p(R), _p(t), _p(b), len(b)))

    def update_map(self, factor, R_W_Be, t_W_Be, bias_directions):
        R, t, b = _f64(R_W_Be), _f64(t_W_Be), np.ascontiguousarray(np.asarray(bias_directions, np.float64).reshape(-1, 3))
        self.ctx.check(self.L.mh_photo_update_map(self.h, factor.h if factor is not None else None, _p(R), _p(t), _p(b), len(b)))

    def make_factor(self, VSVt=None, binary=False):
        return PhotoFactor(self, VSVt, binary)

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_photo_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class PhotoFactor:
    """lidar::PhotometricFactor counterpart (include/mimosa/lidar/photometric_factor.hpp:22-357)."""

    def __init__(self, photo: Photo, VSVt=None, binary=False, _clone_of=None):
        self.photo, self.ctx, self.L = photo, photo.ctx, photo.L
        V = _f64(VSVt) if VSVt is not None else None
        h = C.c_void_p()
        if _clone_of is not None:
            self.ctx.check(self.L.mh_photo_factor_clone(_clone_of.h, C.byref(h)))
        else:
            self.ctx.check(self.L.mh_photo_factor_create(photo.h, _p(V), int(binary), C.byref(h)))
        self.h = h
        self.n = int(self.L.mh_photo_factor_size(h))
        self.ctx._children += 1

    def linearize(self, R_b, t_b, R_a=None, t_a=None) -> dict:
        out = PhotoResult()
        Rb, tb = _f64(R_b), _f64(t_b)
        Ra = _f64(R_a) if R_a is not None else None
        ta = _f64(t_a) if t_a is not None else None
        self.ctx.check(self.L.mh_photo_factor_linearize(self.h, _p(Rb), _p(tb), _p(Ra), _p(ta), C.byref(out)))
        return out.as_dict()

    def linearize_async(self, R_b, t_b, R_a=None, t_a=None):
        Rb, tb = _f64(R_b), _f64(t_b)
        Ra = _f64(R_a) if R_a is not None else None
        ta = _f64(t_a) if t_a is not None else None
        self.ctx.check(self.L.mh_photo_factor_linearize_async(self.h, _p(Rb), _p(tb), _p(Ra), _p(ta)))

    def wait(self) -> dict:
        out = PhotoResult()
        self.ctx.check(self.L.mh_photo_factor_wait(self.h, C.byref(out)))
        return out.as_dict()

    def clone(self) -> "PhotoFactor":
        """clone() (photometric_factor.hpp:120-124)"""
        return PhotoFactor(self.photo, _clone_of=self)

    def state(self, rows=True):
        st = np.empty(self.n, np.int32)
        ce = np.empty((self.n, 2))
        rw = np.empty((self.n, 64, 8)) if rows else None
        self.ctx.check(self.L.mh_photo_factor_get_state(self.h, _p(st), _p(ce), _p(rw)))
        return st, ce, rw

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_photo_factor_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class RadarScan:
    """radar::Manager's front end (src/radar/manager.cpp:111-181) with valid_targets_ kept on the device."""

    def __init__(self, ctx: Context):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        ctx.check(self.L.mh_radar_scan_create(ctx.h, C.byref(h)))
        self.h = h
        ctx._children += 1

    def prepare_input(self, raw: np.ndarray, layout: RadarLayout, cfg: RadarConfig, n: int | None = None) -> dict:
        """raw: the records as bytes (any numpy array, C-contiguous); n: number of records (default: raw.nbytes // point_step)."""
        raw = np.ascontiguousarray(raw)
        n = raw.nbytes // layout.point_step if n is None else n
        info = RadarInfo()
        self.ctx.check(self.L.mh_radar_prepare_input(self.h, _p(raw), n, C.byref(layout), C.byref(cfg), C.byref(info)))
        return {"n_points_in": int(info.n_points_in), "n_points_valid": int(info.n_points_valid)}

    def targets(self) -> np.ndarray:
        n = C.c_size_t()
        self.ctx.check(self.L.mh_radar_get_targets(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, RADAR_TARGET_DTYPE)
        self.ctx.check(self.L.mh_radar_get_targets(self.h, _p(out), n.value, C.byref(n)))
        return out

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_radar_scan_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class RadarFactor:
    """radar::DopplerHessianFactor counterpart (include/mimosa/radar/factor.hpp:22-188).  targets: a structured array of
    RADAR_TARGET_DTYPE (or n x 8 doubles in TargetData's field order), or a prepared RadarScan (device to device)."""

    def __init__(self, ctx: Context, targets, R_B_S, t_B_S, angular_velocity_B, noise_sigma, _clone_of=None):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        if _clone_of is not None:
            ctx.check(self.L.mh_radar_factor_clone(_clone_of.h, C.byref(h)))
        else:
            R, t, w = _f64(R_B_S), _f64(t_B_S), _f64(angular_velocity_B)
            if isinstance(targets, RadarScan):
                ctx.check(self.L.mh_radar_factor_create_from_scan(targets.h, _p(R), _p(t), _p(w), float(noise_sigma), C.byref(h)))
            else:
                tg = np.ascontiguousarray(targets)
                tg = tg.view(np.float64).reshape(-1, 8) if tg.dtype.names else np.ascontiguousarray(tg, np.float64).reshape(-1, 8)
                ctx.check(self.L.mh_radar_factor_create(ctx.h, _p(tg), tg.shape[0], _p(R), _p(t), _p(w), float(noise_sigma), C.byref(h)))
        self.h = h
        self.n = int(self.L.mh_radar_factor_size(h))
        ctx._children += 1

    def linearize(self, R_W_B, v_W, bias_gyro) -> dict:
        """linearize(Values) (:98-188): R_W_B = Values[X].rotation(), v_W = Values[V], bias_gyro = Values[B].gyroscope()."""
        out = RadarResult()
        R, v, b = _f64(R_W_B), _f64(v_W), _f64(bias_gyro)
        self.ctx.check(self.L.mh_radar_factor_linearize(self.h, _p(R), _p(v), _p(b), C.byref(out)))
        return out.as_dict()

    def linearize_async(self, R_W_B, v_W, bias_gyro):
        R, v, b = _f64(R_W_B), _f64(v_W), _f64(bias_gyro)
        self.ctx.check(self.L.mh_radar_factor_linearize_async(self.h, _p(R), _p(v), _p(b)))

    def wait(self) -> dict:
        out = RadarResult()
        self.ctx.check(self.L.mh_radar_factor_wait(self.h, C.byref(out)))
        return out.as_dict()

    def clone(self) -> "RadarFactor":
        """clone() (factor.hpp:69-73)"""
        return RadarFactor(self.ctx, None, None, None, None, None, _clone_of=self)

    def residuals(self):
        """(e_whitened before the robust weight, weight) per target at the state of the last linearize."""
        e, w = np.empty(self.n), np.empty(self.n)
        self.ctx.check(self.L.mh_radar_factor_get_residuals(self.h, _p(e), _p(w)))
        return e, w

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_radar_factor_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def radar_linearize_batch(factors, R_W_Bs, v_Ws, bias_gyros) -> list:
    """Every factor re-linearized in ONE kernel launch (mh_radar_factor_linearize_batch); the factors share one context."""
    n = len(factors)
    L = factors[0].L if n else load()
    hs = (C.c_void_p * max(n, 1))(*[f.h for f in factors])
    R = _f64(R_W_Bs).reshape(-1)
    v = _f64(v_Ws).reshape(-1)
    b = _f64(bias_gyros).reshape(-1)
    out = (RadarResult * max(n, 1))()
    rc = L.mh_radar_factor_linearize_batch(hs, n, _p(R), _p(v), _p(b), out)
    if rc != MH_OK:
        ctx = factors[0].ctx if n else None
        raise MhError(rc, (L.mh_last_error(ctx.h if ctx else None) or b"").decode())
    return [out[i].as_dict() for i in range(n)]


def _photo_batch_call(name, factors, R_bs, t_bs, R_as, t_as, *out):
    n = len(factors)
    L = factors[0].L if n else load()
    hs = (C.c_void_p * max(n, 1))(*[f.h for f in factors])
    Rb = _f64(R_bs).reshape(-1)
    tb = _f64(t_bs).reshape(-1)
    Ra = _f64(R_as).reshape(-1) if R_as is not None else None
    ta = _f64(t_as).reshape(-1) if t_as is not None else None
    rc = getattr(L, name)(hs, n, _p(Rb), _p(tb), _p(Ra), _p(ta), *out)
    if rc != MH_OK:
        ctx = factors[0].ctx if n else None
        raise MhError(rc, (L.mh_last_error(ctx.h if ctx else None) or b"").decode())


def photo_linearize_batch(factors, R_bs, t_bs, R_as=None, t_as=None) -> list:
    """Every photometric factor linearized at its own pose in ONE kernel launch (mh_photo_factor_linearize_batch); the
    factors come from one Photo.  R_as / t_as: the T_a of binary factors (None when no factor is binary)."""
    out = (PhotoResult * max(len(factors), 1))()
    _photo_batch_call("mh_photo_factor_linearize_batch", factors, R_bs, t_bs, R_as, t_as, out)
    return [out[i].as_dict() for i in range(len(factors))]


def photo_linearize_batch_async(factors, R_bs, t_bs, R_as=None, t_as=None) -> None:
    """The same enqueued without waiting: each PhotoFactor.wait() then returns its result, in any order."""
    _photo_batch_call("mh_photo_factor_linearize_batch_async", factors, R_bs, t_bs, R_as, t_as)


# ---- place recognition (mh_place_*) -------------------------------------------------------------------------------------------
MH_PLACE_RINGS, MH_PLACE_SECTORS, MH_PLACE_MAX_HITS = 20, 60, 16
PLACE_CELLS = MH_PLACE_RINGS * MH_PLACE_SECTORS


class PlaceConfig(C.Structure):
    """mh_place_config (40 bytes)."""
    _fields_ = [("r_min", C.c_double), ("r_max", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double), ("min_overlap", C.c_int32),
                ("capacity", C.c_int32)]


class PlaceHit(C.Structure):
    """mh_place_hit (24 bytes)."""
    _fields_ = [("index", C.c_int32), ("shift", C.c_int32), ("dist", C.c_double), ("tag", C.c_int64)]


class PlaceScore(C.Structure):
    """mh_place_score (16 bytes)."""
    _fields_ = [("dist", C.c_double), ("shift", C.c_int32), ("reserved", C.c_int32)]


# the same records as numpy dtypes: what PlaceDatabase.query returns
PLACE_HIT_DTYPE = np.dtype([("index", np.int32), ("shift", np.int32), ("dist", np.float64), ("tag", np.int64)])
PLACE_SCORE_DTYPE = np.dtype([("dist", np.float64), ("shift", np.int32), ("reserved", np.int32)])


def make_place_config(r_min=0.5, r_max=40.0, z_min=-2.0, z_max=30.0, min_overlap=30, capacity=1024) -> PlaceConfig:
    return PlaceConfig(r_min, r_max, z_min, z_max, min_overlap, capacity)


class PlaceDatabase:
    """A keyframe database of ring x sector scan descriptors, searched on the device (mh_place_db_*).  It stores a tag per
    entry and no pose: poses stay with the caller."""

    def __init__(self, ctx: Context, cfg=None, **kw):
        self.ctx, self.L = ctx, ctx.L
        self.cfg = cfg if isinstance(cfg, PlaceConfig) else make_place_config(**(cfg or kw))
        h = C.c_void_p()
        ctx.check(self.L.mh_place_db_create(ctx.h, C.byref(self.cfg), C.byref(h)))
        self.h = h
        ctx._children += 1

    @staticmethod
    def _R(R_G_F):
        return _f64(np.eye(3) if R_G_F is None else R_G_F).reshape(9)

    def size(self) -> int:
        return int(self.L.mh_place_db_size(self.h))

    def describe(self, xyz, R_G_F=None):
        """mh_place_describe: the descriptor (1 200 floats, ring-major) of host points in a frame F, R_G_F levelling it."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        R, desc = self._R(R_G_F), np.empty(PLACE_CELLS, np.float32)
        self.ctx.check(self.L.mh_place_describe(self.h, _p(xyz) if len(xyz) else None, xyz.shape[0], 3, _p(R), _p(desc)))
        return desc

    def describe_device(self, d_points, n, stride_floats, R_G_F=None):
        """mh_place_describe_device: the same for n points at a device address."""
        R, desc = self._R(R_G_F), np.empty(PLACE_CELLS, np.float32)
        self.ctx.check(self.L.mh_place_describe_device(self.h, d_points, n, stride_floats, _p(R), _p(desc)))
        return desc

    def describe_from_scan(self, scan, which, R_G_F=None):
        """mh_place_describe_from_scan: the same from a device-resident scan; which = Scan.FULL or Scan.BODY."""
        R, desc = self._R(R_G_F), np.empty(PLACE_CELLS, np.float32)
        self.ctx.check(self.L.mh_place_describe_from_scan(self.h, scan.h, int(which), _p(R), _p(desc)))
        return desc

    def add(self, desc, tag=0) -> int:
        """mh_place_db_add: append a host descriptor; returns its index."""
        desc = np.ascontiguousarray(desc, dtype=np.float32).reshape(PLACE_CELLS)
        idx = C.c_int32(-1)
        self.ctx.check(self.L.mh_place_db_add(self.h, _p(desc), int(tag), C.byref(idx)))
        return int(idx.value)

    def add_from_scan(self, scan, which, R_G_F=None, tag=0) -> int:
        """mh_place_db_add_from_scan: describe and append on the device; returns the index."""
        R, idx = self._R(R_G_F), C.c_int32(-1)
        self.ctx.check(self.L.mh_place_db_add_from_scan(self.h, scan.h, int(which), _p(R), int(tag), C.byref(idx)))
        return int(idx.value)

    def get(self, index):
        """mh_place_db_get: (descriptor, tag) of an entry."""
        desc, tag = np.empty(PLACE_CELLS, np.float32), C.c_int64(0)
        self.ctx.check(self.L.mh_place_db_get(self.h, int(index), _p(desc), C.byref(tag)))
        return desc, int(tag.value)

    def _query_out(self, n_search, top_k, want_all):
        hits = np.zeros(max(int(top_k), 0), PLACE_HIT_DTYPE)
        m = int(n_search) if n_search else self.size()
        return hits, (np.zeros(m, PLACE_SCORE_DTYPE) if want_all else None)

    def query(self, desc, top_k=4, n_search=0, want_all=False):
        """mh_place_db_query: (hits, all) — hits a PLACE_HIT_DTYPE array in rank order (index -1 behind the last real hit), all a
        PLACE_SCORE_DTYPE array over the searched entries (None unless asked for).  n_search = 0 searches every entry."""
        desc = np.ascontiguousarray(desc, dtype=np.float32).reshape(PLACE_CELLS)
        hits, all_ = self._query_out(n_search, top_k, want_all)
        self.ctx.check(self.L.mh_place_db_query(self.h, _p(desc), int(n_search), int(top_k), _p(hits), _p(all_)))
        return hits, all_

    def query_from_scan(self, scan, which, R_G_F=None, top_k=4, n_search=0, want_all=False):
        """mh_place_db_query_from_scan: the same with the query described from a device-resident scan."""
        R = self._R(R_G_F)
        hits, all_ = self._query_out(n_search, top_k, want_all)
        self.ctx.check(self.L.mh_place_db_query_from_scan(self.h, scan.h, int(which), _p(R), int(n_search), int(top_k), _p(hits), _p(all_)))
        return hits, all_

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_place_db_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def level_rotation(g_unit_F):
    """R_G_F for a gravity direction measured in F: the smallest rotation that takes -g to +z (the antipodal case: a turn by pi
    about x)."""
    g = np.asarray(g_unit_F, np.float64).reshape(3)
    a = -g / np.linalg.norm(g)
    c = a[2]
    if c <= -1.0 + 1e-12:
        return np.diag([1.0, -1.0, -1.0])
    v = np.array([a[1], -a[0], 0.0])                     # a x z
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + K + (K @ K) / (1.0 + c)


def place_candidate_pose(T_k, R_G_Fk, R_G_Fq, shift):
    """The pose a hit proposes for the query's frame: T_W_Fq = T_W_Fk * (R_G_Fk^T Rz(+shift * 6 deg) R_G_Fq, 0).  T_k = (R 3x3, t 3).
    Returns (R, t)."""
    R_k, t_k = np.asarray(T_k[0], np.float64).reshape(3, 3), np.asarray(T_k[1], np.float64).reshape(3)
    a = np.deg2rad(360.0 / MH_PLACE_SECTORS) * int(shift)
    c, s = np.cos(a), np.sin(a)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    Rk = np.eye(3) if R_G_Fk is None else np.asarray(R_G_Fk, np.float64).reshape(3, 3)
    Rq = np.eye(3) if R_G_Fq is None else np.asarray(R_G_Fq, np.float64).reshape(3, 3)
    return R_k @ (Rk.T @ Rz @ Rq), t_k.copy()


def place_relocalise(factor, hits, keyframe_poses, cfg: RelocConfig = None, R_G_Fk=None, R_G_Fq=None, g_unit=(0.0, 0.0, -1.0), half_xy=1.5, step_xy=0.5,
                     half_yaw=np.deg2rad(6.0), step_yaw=np.deg2rad(3.0)):
    """From place-recognition hits to a pose: for each real hit in rank order a pose_grid round its candidate pose (+-1.5 m in
    0.5 m steps, +-6 deg in 3 deg steps by default) and ONE factor.relocalise call on that grid; the winner is the call whose best
    candidate's `fine` score ranks first under the relocalisation ranking (ties: the earlier hit).
    keyframe_poses: indexable by a hit's database index (or a dict by it), each (R 3x3, t 3) of the keyframe's frame in the map.
    R_G_Fk: None, one rotation for every keyframe, or indexable like keyframe_poses.
    Returns None without a real hit, else {"hit": rank of the winning hit, "index": its database index, "R", "t": the pose,
    "fine": its score, "results": every call's result}."""
    cfg = cfg if cfg is not None else make_reloc_config()
    best, results = None, []
    for rank, h in enumerate(hits):
        k = int(h["index"])
        if k < 0:
            break
        Rk = R_G_Fk
        if Rk is not None and np.ndim(Rk) != 2:
            Rk = Rk[k]
        R0, t0 = place_candidate_pose(keyframe_poses[k], Rk, R_G_Fq, int(h["shift"]))
        Rg, tg = pose_grid(R0, t0, half_xy, step_xy, half_yaw, step_yaw)
        res = factor.relocalise(Rg, tg, cfg, g_unit=g_unit)
        results.append(res)
        if res["best"] < 0:
            continue
        fine = res["cand"][res["best"]]["fine"]
        key = (-fine["n_inliers"], fine["sum_sq"], rank)
        if best is None or key < best[0]:
            best = (key, dict(hit=rank, index=k, R=res["R"], t=res["t"], fine=fine))
    if best is None:
        return None
    return dict(best[1], results=results)


# ---- pose graph over all keyframes (mh_pose_graph_*) ----------------------------------------------------------------------------
MH_PGO_MAX_POSES, MH_PGO_MAX_EDGES, MH_PGO_FAR_MAX = 4096, 32768, 32
MH_PGO_FAR_LIMIT = 512


class PoseGraphConfig(C.Structure):
    """mh_pose_graph_config (32 bytes)."""
    _fields_ = [("iters", C.c_int32), ("check_every", C.c_int32), ("damping", C.c_double), ("eps_rot", C.c_double), ("eps_trans", C.c_double)]


class PoseGraphTrace(C.Structure):
    """mh_pose_graph_trace (32 bytes)."""
    _fields_ = [("f", C.c_double), ("step_rot", C.c_double), ("step_trans", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32)]


class PoseGraphResult(C.Structure):
    """mh_pose_graph_result"""
    _fields_ = [("iters", C.c_int32), ("converged", C.c_int32), ("n_poses", C.c_int32), ("n_far", C.c_int32), ("f_first", C.c_double), ("f_last", C.c_double),
                ("trace", PoseGraphTrace * 64)]


MH_PGO_LOSS_NONE, MH_PGO_LOSS_HUBER, MH_PGO_LOSS_CAUCHY, MH_PGO_LOSS_DCS = 0, 1, 2, 3
PGO_LOSS_KINDS = {None: 0, "none": 0, "huber": 1, "cauchy": 2, "dcs": 3}


class PosePrior(C.Structure):
    """mh_pose_prior (392 bytes)."""
    _fields_ = [("pose", C.c_int32), ("reserved", C.c_int32), ("Z_R", C.c_double * 9), ("Z_t", C.c_double * 3), ("info", C.c_double * 36)]


class PoseGraphLoss(C.Structure):
    """mh_pose_graph_loss (16 bytes)."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("param", C.c_double)]


MH_PGO_COV_PAIRS_MAX = 64


class PoseGraphCovInfo(C.Structure):
    """mh_pose_graph_cov_info (16 bytes)."""
    _fields_ = [("n_poses", C.c_int32), ("n_far", C.c_int32), ("n_pairs", C.c_int32), ("flags", C.c_int32)]


def _gate_edge_terms(Ra, ta, Rb, tb, ZR, Zt):
    """an edge's residual [Log(Z.R^T R_ab), Z.R^T (t_ab - Z.t)] and J_a = -Ad(T_ab^-1) (J_b = I): rule 1 of the pose graph"""
    hat = lambda v: np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    abR, abt = Ra.T @ Rb, Ra.T @ (tb - ta)
    Re = ZR.T @ abR
    th = np.arccos(min(1.0, max(-1.0, (np.trace(Re) - 1.0) / 2.0)))
    k = 0.5 if th < 1e-9 else th / (2.0 * np.sin(th))
    r = np.concatenate([np.array([Re[2, 1] - Re[1, 2], Re[0, 2] - Re[2, 0], Re[1, 0] - Re[0, 1]]) * k, ZR.T @ (abt - Zt)])
    Ri, ti = abR.T, -(abR.T @ abt)
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = Ri
    Ad[3:, :3] = hat(ti) @ Ri
    return r, -Ad


def make_pose_prior(priors):
    """an array of mh_pose_prior from dicts {"pose": i, "Z": (R, t) the measured pose (world from keyframe), "info": 6 x 6}"""
    arr = (PosePrior * max(len(priors), 1))()
    for q, e in zip(arr, priors):
        q.pose = int(e["pose"])
        q.Z_R[:] = [float(v) for v in np.asarray(e["Z"][0], np.float64).reshape(9)]
        q.Z_t[:] = [float(v) for v in np.asarray(e["Z"][1], np.float64).reshape(3)]
        q.info[:] = [float(v) for v in np.asarray(e["info"], np.float64).reshape(36)]
    return arr


def make_pose_graph_loss(losses):
    """an array of mh_pose_graph_loss from (kind, param) pairs; kind a number or "none" / "huber" / "cauchy" / "dcs", or None"""
    arr = (PoseGraphLoss * max(len(losses), 1))()
    for q, e in zip(arr, losses):
        kind, param = (0, 0.0) if e is None else e
        q.kind, q.param = int(PGO_LOSS_KINDS.get(kind, kind)), float(param)
    return arr


def make_pose_graph_config(iters=16, check_every=0, damping=0.0, eps_rot=1e-9, eps_trans=1e-9) -> PoseGraphConfig:
    return PoseGraphConfig(int(iters), int(check_every), float(damping), float(eps_rot), float(eps_trans))


class PoseGraph:
    """A pose graph over all keyframes, optimised on the device (mh_pose_graph_*): poses (world from keyframe), relative-pose
    edges in the shape the window chains take them, a fixed flag per pose.  max_far (1 .. MH_PGO_FAR_LIMIT): a wide graph
    (mh_pose_graph_create_wide), which takes that many far edges; None: at most MH_PGO_FAR_MAX."""

    def __init__(self, ctx: Context, max_poses, max_edges, max_far=None):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        if max_far is None:
            ctx.check(self.L.mh_pose_graph_create(ctx.h, int(max_poses), int(max_edges), C.byref(h)))
        else:
            ctx.check(self.L.mh_pose_graph_create_wide(ctx.h, int(max_poses), int(max_edges), int(max_far), C.byref(h)))
        self.h = h
        self.n = self.n_edges = self.n_priors = 0
        ctx._children += 1

    def set_poses(self, R, t):
        """mh_pose_graph_set_poses: R n x 3 x 3, t n x 3.  Another n than before drops the edges, the fixed flags, the priors and
        the losses."""
        R, t = _f64(R).reshape(-1, 9), _f64(t).reshape(-1, 3)
        self.ctx.check(self.L.mh_pose_graph_set_poses(self.h, _p(R), _p(t), R.shape[0]))
        if R.shape[0] != self.n:
            self.n, self.n_edges, self.n_priors = R.shape[0], 0, 0

    def set_fixed(self, fixed=None):
        """mh_pose_graph_set_fixed: n flags, or None for no fixed pose."""
        f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, dtype=np.uint8).reshape(self.n)
        self.ctx.check(self.L.mh_pose_graph_set_fixed(self.h, _p(f)))

    def set_edges(self, edges):
        """mh_pose_graph_set_edges: dicts as make_window_edge takes them, or an array it made."""
        n = len(edges)
        arr = edges if isinstance(edges, C.Array) else make_window_edge(edges)
        self.ctx.check(self.L.mh_pose_graph_set_edges(self.h, arr, n))
        self.n_edges = n

    def set_priors(self, priors):
        """mh_pose_graph_set_priors: dicts as make_pose_prior takes them, or an array it made.  Drops the priors' losses."""
        n = len(priors)
        arr = priors if isinstance(priors, C.Array) else make_pose_prior(priors)
        self.ctx.check(self.L.mh_pose_graph_set_priors(self.h, arr, n))
        self.n_priors = n

    def set_loss(self, edges=None, priors=None):
        """mh_pose_graph_set_loss: one (kind, param) per edge and per prior as make_pose_graph_loss takes them; None: no loss."""
        def arr(v, n, what):
            if v is None or isinstance(v, C.Array):
                return v
            if len(v) != n:
                raise ValueError("set_loss: %d %s losses for %d %ss" % (len(v), what, n, what))
            return make_pose_graph_loss(v)
        self.ctx.check(self.L.mh_pose_graph_set_loss(self.h, arr(edges, self.n_edges, "edge"), arr(priors, self.n_priors, "prior")))

    def prior_residuals(self):
        """mh_pose_graph_prior_residuals: (d P x 6, chi2 P) at the stored poses; nothing moves."""
        d, chi2 = np.empty((self.n_priors, 6)), np.empty(self.n_priors)
        self.ctx.check(self.L.mh_pose_graph_prior_residuals(self.h, _p(d) if self.n_priors else None, _p(chi2) if self.n_priors else None))
        return d, chi2

    def weights(self):
        """mh_pose_graph_weights: (w per edge, w per prior, f = the sum of rho) at the stored poses; nothing moves."""
        we, wp, f = np.empty(self.n_edges), np.empty(self.n_priors), C.c_double(0.0)
        self.ctx.check(self.L.mh_pose_graph_weights(self.h, _p(we) if self.n_edges else None, _p(wp) if self.n_priors else None, C.byref(f)))
        return we, wp, float(f.value)

    def poses(self):
        """mh_pose_graph_get_poses: (R n x 3 x 3, t n x 3) as the last call left them."""
        R, t, n = np.empty((self.n, 3, 3)), np.empty((self.n, 3)), C.c_size_t(0)
        self.ctx.check(self.L.mh_pose_graph_get_poses(self.h, _p(R), _p(t), self.n, C.byref(n)))
        assert n.value == self.n
        return R, t

    def residuals(self):
        """mh_pose_graph_residuals: (r E x 6, chi2 E, f) at the stored poses; nothing moves."""
        r, chi2, f = np.empty((self.n_edges, 6)), np.empty(self.n_edges), C.c_double(0.0)
        self.ctx.check(self.L.mh_pose_graph_residuals(self.h, _p(r) if self.n_edges else None, _p(chi2) if self.n_edges else None, C.byref(f)))
        return r, chi2, float(f.value)

    def covariances(self, damping=0.0, pairs=None):
        """mh_pose_graph_covariances: (cov n x 6 x 6, joint p x 12 x 12, info {"n_poses", "n_far", "n_pairs", "flags"}) at the stored
        poses; nothing moves.  pairs: up to 64 (i, j) with i < j.  With flags == 4 (a pivot was not positive) the library writes
        nothing, and both arrays come back filled with NaN."""
        pr = np.ascontiguousarray(np.asarray(pairs if pairs is not None else [], np.int32).reshape(-1, 2))
        cov, joint, info = np.full((self.n, 6, 6), np.nan), np.full((len(pr), 12, 12), np.nan), PoseGraphCovInfo()
        self.ctx.check(self.L.mh_pose_graph_covariances(self.h, float(damping), _p(cov), _p(pr) if len(pr) else None, len(pr), _p(joint) if len(pr) else None,
                                                        C.byref(info)))
        return cov, joint, {"n_poses": int(info.n_poses), "n_far": int(info.n_far), "n_pairs": int(info.n_pairs), "flags": int(info.flags)}

    def gate(self, candidates, damping=0.0):
        """Up to 64 candidate edges that are NOT in the graph (dicts as make_window_edge takes them), each tested against the
        joint marginal of its two poses: {"r": c x 6 the residual at the stored poses, "chi2": r^T Om r as mh_pose_graph_residuals
        would report it, "d2": r^T (J S J^T + Om^-1)^-1 r with J = [J_a | I] and S the pair's 12 x 12 joint covariance, "flags"}.
        d2 is chi^2 with 6 degrees of freedom for a true loop, whatever the drift between the two poses.  Host arithmetic on
        covariances()."""
        R, t = self.poses()
        pairs = [(int(e["a"]), int(e["b"])) for e in candidates]
        _, joint, info = self.covariances(damping, pairs)
        r, chi2, d2 = np.zeros((len(pairs), 6)), np.zeros(len(pairs)), np.full(len(pairs), np.nan)
        for k, ((a, b), e) in enumerate(zip(pairs, candidates)):
            Om = np.asarray(e["info"], np.float64).reshape(6, 6)
            r[k], Ja = _gate_edge_terms(R[a], t[a], R[b], t[b], np.asarray(e["Z"][0], np.float64).reshape(3, 3), np.asarray(e["Z"][1], np.float64).reshape(3))
            chi2[k] = r[k] @ Om @ r[k]
            if info["flags"] == 0:
                J = np.hstack([Ja, np.eye(6)])
                d2[k] = r[k] @ np.linalg.solve(J @ joint[k] @ J.T + np.linalg.inv(Om), r[k])
        return {"r": r, "chi2": chi2, "d2": d2, "flags": info["flags"]}

    def optimise(self, cfg: PoseGraphConfig = None, trace_poses=False, **kw):
        """mh_pose_graph_optimise: {"iters", "converged", "n_poses", "n_far", "f_first", "f_last", "trace": [{"f", "step_rot",
        "step_trans", "flags"}], "R", "t": the final poses, "trace_poses": iters x n x 12 (R, then t) when asked for}."""
        cfg = cfg if cfg is not None else make_pose_graph_config(**kw)
        res = PoseGraphResult()
        tp = np.full((cfg.iters, self.n, 12), np.nan) if trace_poses else None
        self.ctx.check(self.L.mh_pose_graph_optimise(self.h, C.byref(cfg), C.byref(res), _p(tp)))
        R, t = self.poses()
        out = {"iters": int(res.iters), "converged": int(res.converged), "n_poses": int(res.n_poses), "n_far": int(res.n_far), "f_first": float(res.f_first),
               "f_last": float(res.f_last), "R": R, "t": t,
               "trace": [{"f": float(q.f), "step_rot": float(q.step_rot), "step_trans": float(q.step_trans), "flags": int(q.flags)} for q in res.trace[:res.iters]]}
        if trace_poses:
            out["trace_poses"] = tp[:res.iters]
        return out

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_pose_graph_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class KeyframesConfig(C.Structure):
    """mh_keyframes_config (16 bytes)."""
    _fields_ = [("capacity_keyframes", C.c_int32), ("reserved", C.c_int32), ("capacity_points", C.c_int64)]


class KeyframesInfo(C.Structure):
    """mh_keyframes_info (40 bytes)."""
    _fields_ = [("keyframes", C.c_int64), ("points", C.c_int64), ("capacity_keyframes", C.c_int64), ("capacity_points", C.c_int64),
                ("device_bytes", C.c_int64)]


class MapRebuildConfig(C.Structure):
    """mh_map_rebuild_config (16 bytes)."""
    _fields_ = [("chunk_points", C.c_int64), ("reserved", C.c_int64)]


class MapRebuildResult(C.Structure):
    """mh_map_rebuild_result (48 bytes)."""
    _fields_ = [("keyframes", C.c_int64), ("points_offered", C.c_int64), ("chunks", C.c_int64), ("purges", C.c_int64), ("n_points", C.c_int64),
                ("n_voxels", C.c_int64)]


class KeyframeStore:
    """The clouds of the keyframes on the device, each in its own frame, with a tag and no pose (mh_keyframes_*), and the map they
    give at any poses (rebuild_map: mh_map_rebuild_from_keyframes)."""

    def __init__(self, ctx: Context, capacity_keyframes=1024, capacity_points=1 << 24):
        self.ctx, self.L = ctx, ctx.L
        cfg = KeyframesConfig(int(capacity_keyframes), 0, int(capacity_points))
        h = C.c_void_p()
        ctx.check(self.L.mh_keyframes_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        ctx._children += 1

    def size(self) -> int:
        return int(self.L.mh_keyframes_size(self.h))

    def info(self) -> dict:
        out = KeyframesInfo()
        self.ctx.check(self.L.mh_keyframes_get_info(self.h, C.byref(out)))
        return {n: getattr(out, n) for n, _ in out._fields_}

    def add(self, xyz, tag=0) -> int:
        """mh_keyframes_add: append host points (n x 3, or n x s with s >= 3: the first three columns); returns the index."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        xyz = xyz.reshape(-1, 3) if xyz.ndim != 2 else xyz
        idx = C.c_int32(-1)
        self.ctx.check(self.L.mh_keyframes_add(self.h, _p(xyz) if len(xyz) else None, xyz.shape[0], xyz.shape[1], int(tag), C.byref(idx)))
        return int(idx.value)

    def add_device(self, d_points, n, stride_floats, tag=0) -> int:
        """mh_keyframes_add_device: the same for n points at a device address."""
        idx = C.c_int32(-1)
        self.ctx.check(self.L.mh_keyframes_add_device(self.h, d_points, int(n), int(stride_floats), int(tag), C.byref(idx)))
        return int(idx.value)

    def add_from_scan(self, scan, which, tag=0) -> int:
        """mh_keyframes_add_from_scan: device to device from a scan; which = Scan.FULL or Scan.BODY.  Waits for nothing."""
        idx = C.c_int32(-1)
        self.ctx.check(self.L.mh_keyframes_add_from_scan(self.h, scan.h, int(which), int(tag), C.byref(idx)))
        return int(idx.value)

    def get(self, index):
        """mh_keyframes_get: (xyz as n x 3 float32, tag) of an entry."""
        n, tag = C.c_size_t(0), C.c_int64(0)
        self.ctx.check(self.L.mh_keyframes_get(self.h, int(index), None, 0, C.byref(n), C.byref(tag)))
        xyz = np.empty((n.value, 3), np.float32)
        self.ctx.check(self.L.mh_keyframes_get(self.h, int(index), _p(xyz), n.value, C.byref(n), C.byref(tag)))
        return xyz, int(tag.value)

    def device_points(self, index):
        """mh_keyframes_device_points: (device address, n) of an entry, 4 floats per point; valid until the store is destroyed."""
        d, n = C.c_void_p(), C.c_size_t(0)
        self.ctx.check(self.L.mh_keyframes_device_points(self.h, int(index), C.byref(d), C.byref(n)))
        return d, int(n.value)

    def rebuild_map(self, poses, order=None, chunk_points=0, **map_cfg):
        """mh_map_rebuild_from_keyframes: (VoxelMap, result dict).  poses: (R, t) with R of shape K x 3 x 3 and t of shape K x 3 for
        the K listed keyframes (any float arrays, cast to float32 once); order: the entries to insert (None: all, in stored
        order); map_cfg: the keywords of VoxelMap (leaf, min_dist, max_pts, mode, lru_horizon, lru_clear_cycle), with its defaults."""
        d = dict(leaf=0.5, min_dist=0.15, max_pts=20, mode=19, lru_horizon=1000, lru_clear_cycle=10)
        unknown = set(map_cfg) - set(d)
        if unknown:
            raise TypeError(f"rebuild_map: unknown map settings {sorted(unknown)}")
        d.update(map_cfg)
        cfg = MapConfig(d["leaf"], d["min_dist"], d["max_pts"], d["mode"], d["lru_horizon"], d["lru_clear_cycle"], 0)
        order = None if order is None else np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        K = self.size() if order is None else len(order)
        R = np.ascontiguousarray(np.asarray(poses[0], dtype=np.float32).reshape(K, 9))
        t = np.ascontiguousarray(np.asarray(poses[1], dtype=np.float32).reshape(K, 3))
        rc, res, h = MapRebuildConfig(int(chunk_points), 0), MapRebuildResult(), C.c_void_p()
        self.ctx.check(self.L.mh_map_rebuild_from_keyframes(self.h, C.byref(cfg), _p(order), 0 if order is None else len(order), _p(R) if K else None,
                                                            _p(t) if K else None, C.byref(rc), C.byref(h), C.byref(res)))
        return VoxelMap(self.ctx, _h=h), {n: getattr(res, n) for n, _ in res._fields_}

    def destroy(self):
        if getattr(self, "h", None):
            self.L.mh_keyframes_destroy(self.h)
            self.h = None
            self.ctx._child_released()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
