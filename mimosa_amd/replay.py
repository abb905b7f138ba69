"""Sequence replay harness (SURVEY.md §8 "next" row f-4, BASELINE configs[4]): deskew + geometric + photometric factors
per scan in a fixed-lag window, end to end through the C ABI, on a synthetic trajectory (ENWIDE bags and ROS are absent).

Every scan goes through the reference's LiDAR call order (src/lidar/manager.cpp:45-147):

    prepareInput -> [IMU propagation over the distinct timestamps] -> deskewPoints -> Photometric::preprocess ->
    Geometric::preprocess -> getFactors (ICPFactor ctor, PhotometricFactor ctor) -> define: smoother update +
    additional_update_iterations, EVERY live ICPFactor re-linearized each time (src/graph/manager.cpp:585-588) ->
    Geometric::updateMap (keyframe test on max |yaw, pitch, roll|, copy-then-insert) + Photometric::updateMap

What stands in for the parts that are out of scope (GTSAM / ISAM2, the IMU manager):
  * IMU: gyro / specific-force samples of the true constant-twist motion (+ noise) at `imu_rate`; propagated on the host
    exactly as Manager::deskewPoints does between samples (constant acc / omega extrapolation, manager.cpp:478-489) to get
    the per-timestamp deskew poses T_Le_Lt AND the relative-pose measurement between consecutive scans;
  * smoother: a dense Gauss-Newton over the `window` most recent poses: one unary ICP Hessian factor per live scan (all of
    them re-linearized per iteration through ONE mh_icp_linearize_batch call), the photometric factor on the newest pose
    (photo_window: every live scan's photometric factor, on its own pose, through ONE mh_photo_factor_linearize_batch call),
    between-factors from the IMU propagation, a prior on the oldest pose (what marginalisation leaves behind).  Retraction
    T <- T Exp(xi), xi = (omega, v) in the body frame: the perturbation the reference's Jacobians are taken against
    (geometric_factor.hpp:341-355, photometric_factor.hpp:262-279).

`backend` does the numerical work: HipBackend drives the C ABI; tests/ run the same loop on the CPU oracle
(oracle/replay_backend.py) and require the same trajectory.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from . import synth, synth_photo

GRAVITY = np.array([0.0, 0.0, -9.81])


def _photo_cfg(rows, cols):
    return synth_photo.photo_config(rows=rows, cols=cols, T_B_L_R=np.eye(3), T_B_L_t=np.zeros(3))


@dataclass
class ReplayConfig:
    n_scans: int = 20
    rows: int = 128
    cols: int = 1024
    dt: float = 0.1                                   # 10 Hz
    v: tuple = (1.2, 0.2, 0.0)                        # body-frame twist of the platform
    w: tuple = (0.0, 0.0, 0.35)
    room: tuple = tuple(synth_photo.ROOM)
    window: int = 5                                   # smoother lag 0.5 s at 10 Hz (config/enwide/params.yaml:30)
    update_iters: int = 6                             # smoother_->update + additional_update_iterations: 5 (:52)
    imu_rate: float = 200.0
    imu_gyro_noise: float = 2e-4                      # rad/s, per sample
    imu_acc_noise: float = 5e-3                       # m/s^2
    prior_trans_noise: float = 0.03                   # error of the very first pose guess, metres
    prior_rot_noise_deg: float = 0.3
    between_sigma_rot: float = 2e-3                   # weight of the IMU relative-pose factor
    between_sigma_trans: float = 1e-2
    keyframe_trans_thresh: float = 1.0                # ENWIDE: map_keyframe_trans_thresh
    keyframe_rot_thresh_deg: float = 20.0
    # > 0: the keyframe decision is made by what the pose test stands in for (geometric.cpp:460-464) — a scan becomes a keyframe when an
    # insert preview of its body cloud at the estimated pose (mh_map_preview_insert_from_scan) says the map would keep at least this
    # fraction of its points; the first scan always is one.  0: the reference's pose test.  HipBackend only; not in the native replay
    keyframe_new_fraction: float = 0.0
    # the forked map is carved by the keyframe's own scan at the estimated pose before the insert (mh_map_carve_from_scan on the body
    # cloud): map points the scan sees through are removed.  Off: the reference's map, which only grows.  HipBackend only; not in the
    # native replay.  The fields after it are mh_map_carve_config's.
    carve_keyframes: bool = False
    carve_grid: int = 64
    carve_ring: int = 1
    carve_range_min: float = 0.5
    carve_range_max: float = 60.0
    carve_margin_abs: float = 0.3
    carve_margin_rel: float = 0.0
    photometric: bool = True
    # every scan's photometric factor stays in the window on its own pose (released with the pose) and all of them are
    # re-linearized per iteration, as the reference's smoother does; off: the photometric factor on the newest pose only
    photo_window: bool = False
    # the per-timestamp deskew poses (src/lidar/manager.cpp:468-499) are computed on the device (mh_scan_deskew_imu): no
    # timestamp is read back, no pose table uploaded, the photometric frame reads the scan's device table.  HIP backend and the
    # native replay only (the CPU backend has no device to keep a table on)
    device_poses: bool = False
    # the first scan after the map is seeded is aligned to the map (mh_icp_align: the Gauss-Newton loop on the device, from the
    # propagated first guess) before its factor goes to the smoother.  HIP backend and the native FixedLagReplay only
    init_align: bool = False
    init_align_iters: int = 10
    # the first scan's pose comes from mh_icp_relocalise instead of from first_state's truth-based guess: the propagated first
    # guess is displaced by relocalise_guess_offset (m, world frame) and relocalise_guess_yaw_deg (about the world z axis) — further
    # than the association gate reaches — and candidate poses on a grid around THAT pose (capi.pose_grid: +-half_xy in steps of
    # step_xy, +-half_yaw in steps of step_yaw) are scored against the map, the best aligned and re-scored.  The sweep itself is
    # deskewed from first_state as before (the motion within a sweep, not where it is); every later scan is unchanged.
    # HipBackend only; the native replay has no such switch
    relocalise_first: bool = False
    relocalise_half_xy: float = 2.0
    relocalise_step_xy: float = 0.5
    relocalise_half_yaw_deg: float = 30.0
    relocalise_step_yaw_deg: float = 7.5
    relocalise_guess_offset: tuple = (1.2, -0.9, 0.0)   # 1.5 m
    relocalise_guess_yaw_deg: float = 20.0
    # with relocalise_first: the candidates are aligned side by side in one chain of launches (mh_icp_relocalise_batch, on clones of
    # the scan's factor that live for the call) instead of one after another.  Refused without relocalise_first
    relocalise_batch: bool = False
    # the smoother's update_iters iterations run as ONE chain of launches on the device (mh_icp_window_optimise: linearize,
    # assembly, block-tridiagonal solve, retraction) instead of a batched linearize, a numpy solve and the retractions per
    # iteration.  Without the photometric factor only; HIP backend and the native FixedLagReplay
    device_window: bool = False
    # with device_window: (rot, trans) in rad and m — a factor of the window is evaluated again only once its pose has moved past
    # these thresholds from the pose of its last evaluation within the call (mh_icp_window_optimise_relin; the reference's ISAM2
    # runs with 1.75e-2, 5e-3).  None: every factor every iteration.  Refused without device_window
    window_relin: tuple = None
    # with device_window: the photometric factor is accepted — before each window call the host linearizes it once at the call's
    # initial poses (photo_window: every live one, through the batch call) and passes the results as linear factors on their poses
    # (mh_icp_window_optimise_lin), which the chain carries along instead of evaluating them again.  Refused without device_window
    window_photo_linear: bool = False
    # > 0: a synthetic external odometry source delivers, at every odometry_every-th scan, the true pose with noise from a fixed
    # seed and a covariance; the message goes through the odometry manager's rules (OdometryManager; the reference:
    # src/odometry/manager.cpp:22-67) and becomes a between factor with these sigmas on the window poses of scans
    # k - odometry_every and k, beside the IMU ties; it is dropped once its older pose has left the window.  With device_window
    # the edges go to mh_icp_window_optimise_edges.  Unlike the reference's source, this one reports at scan times.  0: off
    odometry_every: int = 0
    # with device_window: when a scan's arrival pushes the oldest pose out of the window, that pose is marginalised on the device
    # (mh_icp_window_marginalise, at the current poses, before it is dropped) and the dense Gaussian this leaves on the next pose
    # is carried as a linear factor on the window's pose 0 instead of the 1e-4 rad / 1e-4 m pin; a marginal that is not valid
    # falls back to the pin for that window.  Refused without device_window, and with odometry_every > 1 (an odometry edge would
    # reach from pose 0 beyond pose 1: the marginal would be a joint factor on several poses)
    window_marginal: bool = False
    # window_marginal for a window whose oldest pose is tied beyond pose 1 by odometry edges: the pose that leaves is marginalised
    # with every live edge from it (mh_icp_window_marginalise_joint) and the dense Gaussian this leaves on its separator — up to
    # four poses — is carried as the one joint prior of the window calls (mh_icp_window_optimise_joint, prior_info = 0), absorbed
    # by the next marginalisation.  A marginal that is not valid falls back to the pin for that window.  Offered only with
    # device_window and odometry_every 1 .. 4 (a separator of at most four poses), refused otherwise; not together with window_marginal
    window_marginal_joint: bool = False
    odometry_sigma_rot_deg: float = 1.0
    odometry_sigma_trans_m: float = 0.5
    reg: dict = field(default_factory=synth.enwide_config)
    photo: dict = None

    def __post_init__(self):
        if self.photo is None:
            self.photo = _photo_cfg(self.rows, self.cols)


# ---- external odometry (ReplayConfig.odometry_every) ---------------------------------------------------------------------
ODOMETRY_SEED = 11
ODOMETRY_NOISE = (1e-3, 5e-3)  # rad, m: the synthetic source's own error, which its covariance states


def odometry_messages(cfg, scans):
    """[(k, R, t, covariance 6 x 6)]: at every odometry_every-th scan the true pose with noise from a fixed seed"""
    if cfg.odometry_every <= 0:
        return []
    rng = np.random.default_rng(ODOMETRY_SEED)
    cov = np.diag([ODOMETRY_NOISE[0] ** 2] * 3 + [ODOMETRY_NOISE[1] ** 2] * 3)
    out = []
    for k in range(0, len(scans), cfg.odometry_every):
        R = scans[k]["R_gt"] @ synth.so3_exp(ODOMETRY_NOISE[0] * rng.standard_normal(3))
        out.append((k, R, scans[k]["t_gt"] + ODOMETRY_NOISE[1] * rng.standard_normal(3), cov))
    return out


class OdometryManager:
    """odometry::Manager::callback (src/odometry/manager.cpp:22-67) without ROS, T_B_S = identity: the D-optimality gate
    (utils.hpp:21 as written; a negative determinant gives NaN, which passes), the first accepted message only initialises, every
    later one gives (previous key, Z = T_km1^-1 T_k, information matrix from the configured sigmas)."""

    def __init__(self, sigma_rot_deg, sigma_trans_m, d_opt_thresh=1.0):
        sr = float(sigma_rot_deg) * np.pi / 180.0
        self.info = np.diag([1.0 / (sr * sr)] * 3 + [1.0 / (float(sigma_trans_m) * float(sigma_trans_m))] * 3)
        self.thresh, self.prev = d_opt_thresh, None

    def callback(self, key, R, t, cov):
        with np.errstate(invalid="ignore"):
            d_opt = np.exp(np.log(np.power(np.float64(np.linalg.det(np.asarray(cov, float))), 1.0 / 6.0)))
        if d_opt > self.thresh:
            return None
        out = None
        if self.prev is not None:
            pk, Rp, tp = self.prev
            out = (pk, _between(Rp, tp, R, t), self.info)
        self.prev = (key, R, t)
        return out


# ---- SE(3) helpers (Pose3 tangent order: rotation first) ---------------------------------------------------------
def _hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def _so3_log(R):
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return w * (0.5 if th < 1e-9 else th / (2.0 * np.sin(th)))


def _retract(R, t, xi):
    """T <- T * Exp(xi), xi = (omega, v), first order in the translation (as in round 1)."""
    return R @ synth.so3_exp(np.asarray(xi[:3])), t + R @ np.asarray(xi[3:])


def _between(Ra, ta, Rb, tb):
    return Ra.T @ Rb, Ra.T @ (tb - ta)


def _adjoint(R, t):
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = _hat(t) @ R
    return A


def trajectory(cfg: ReplayConfig):
    """Ground-truth scan-END sensor poses (what synth_photo.make_frame integrates)."""
    R, t = synth.rot_z(synth.SENSOR_YAW), synth.room_origin(0, 0) + synth_photo.SENSOR_LOCAL
    v, w = np.asarray(cfg.v, float), np.asarray(cfg.w, float)
    out = []
    for _ in range(cfg.n_scans):
        out.append((R.copy(), t.copy()))
        t = t + R @ (v * cfg.dt)
        R = R @ synth.so3_exp(w * cfg.dt)
    return out


def imu_samples(cfg: ReplayConfig, R_end, k, seed=5):
    """Gyro / accelerometer samples over the sweep of scan k: times tau_k - dt + j h, j = 0..M (scan-end time tau_k = k dt).
    Constant body twist: omega = w, specific force f = w x v - R(t)^T g."""
    M = int(round(cfg.imu_rate * cfg.dt))
    h = cfg.dt / M
    v, w = np.asarray(cfg.v, float), np.asarray(cfg.w, float)
    ts = k * cfg.dt - cfg.dt + h * np.arange(M + 1)
    rng = np.random.default_rng(seed * 7919 + k)
    gyro = np.tile(w, (M + 1, 1)) + cfg.imu_gyro_noise * rng.standard_normal((M + 1, 3))
    acc = np.empty((M + 1, 3))
    for j, tj in enumerate(ts):
        Rj = R_end @ synth.so3_exp(w * (tj - k * cfg.dt))
        acc[j] = np.cross(w, v) - Rj.T @ GRAVITY
    acc += cfg.imu_acc_noise * rng.standard_normal((M + 1, 3))
    return ts, gyro, acc


def make_scans(cfg: ReplayConfig):
    """Per scan: the raw Ouster grid the driver publishes (NaN where there was no return), the frame of
    synth_photo.make_frame (ground truth, exact deskew poses — used by tests only), and the IMU samples of the sweep."""
    scans = []
    pc = cfg.photo
    for k in range(cfg.n_scans):
        fr = synth_photo.make_frame(pc, frame=k, v=cfg.v, w=cfg.w, room=np.asarray(cfg.room), dt_frame=cfg.dt)
        grid = np.zeros(cfg.rows * cfg.cols, dtype=synth.OUSTER_DTYPE)
        grid["x"] = np.nan
        sub = np.zeros(len(fr["raw"]), dtype=synth.OUSTER_DTYPE)
        for name in ("x", "y", "z", "intensity", "t"):
            sub[name] = fr["raw"][name]
        grid[fr["raw"]["idx"]] = sub
        grid["ring"] = (np.arange(len(grid)) // cfg.cols).astype(np.uint16)
        grid["t"] = np.tile(fr["unique_ns"], cfg.rows)
        scans.append(dict(raw=grid, frame=fr, imu=imu_samples(cfg, fr["R_W_L"], k), R_gt=fr["R_W_L"], t_gt=fr["t_W_L"],
                          header_ts=k * cfg.dt - float(fr["unique_ns"][-1]) * 1e-9))
    return scans


def propagate(R, p, vel, imu, header_ts, unique_ns):
    """Manager::deskewPoints' host part (src/lidar/manager.cpp:455-499): states at the IMU sample times by integrating
    sample to sample, then constant-acc / omega extrapolation to every distinct timestamp.  (R, p, vel) = state at the
    first sample.  Returns (T_W_Bt per timestamp as (n, 12), state at the last sample)."""
    ts, gyro, acc = imu
    states = [(R, p, vel)]
    for c in range(len(ts) - 1):
        Rc, pc, vc = states[-1]
        d = ts[c + 1] - ts[c]
        aw = Rc @ acc[c] + GRAVITY
        states.append((Rc @ synth.so3_exp(gyro[c] * d), pc + vc * d + 0.5 * aw * d * d, vc + aw * d))
    # every distinct timestamp: sample interval c with ts[c] < tq <= ts[c + 1] (manager.cpp:470-476), vectorised
    tq = header_ts + np.asarray(unique_ns, np.float64) * 1e-9
    ci = np.clip(np.searchsorted(ts[1:-1], tq, side="left"), 0, len(ts) - 2)
    Rs = np.stack([s_[0] for s_ in states])[ci]
    ps = np.stack([s_[1] for s_ in states])[ci]
    vs = np.stack([s_[2] for s_ in states])[ci]
    d = (tq - ts[ci])[:, None]
    wv = gyro[ci] * d
    th = np.linalg.norm(wv, axis=1)
    th2 = th * th
    with np.errstate(invalid="ignore", divide="ignore"):
        A = np.where(th < 1e-12, 1.0 - th2 / 6.0, np.sin(th) / th)
        B = np.where(th < 1e-12, 0.5 - th2 / 24.0, (1.0 - np.cos(th)) / th2)
    K = np.zeros((len(tq), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -wv[:, 2], wv[:, 1], wv[:, 2], -wv[:, 0], -wv[:, 1], wv[:, 0]
    E = np.eye(3)[None] + A[:, None, None] * K + B[:, None, None] * (K @ K)
    out = np.empty((len(tq), 12))
    out[:, :9] = (Rs @ E).reshape(-1, 9)
    out[:, 9:] = ps + vs * d + 0.5 * np.einsum("nij,nj->ni", Rs, acc[ci]) * d * d + 0.5 * GRAVITY * d * d
    return out, states[-1]


def imu_segments(R, p, vel, imu):
    """propagate()'s sample-to-sample half alone, as the IMU intervals mh_scan_deskew_imu takes; like propagate(), the last
    interval also serves timestamps behind the last sample.  Returns (segments, state at the last sample)."""
    from . import capi
    ts, gyro, acc = imu
    states = [(R, p, vel)]
    for c in range(len(ts) - 1):
        Rc, pc, vc = states[-1]
        d = ts[c + 1] - ts[c]
        aw = Rc @ acc[c] + GRAVITY
        states.append((Rc @ synth.so3_exp(gyro[c] * d), pc + vc * d + 0.5 * aw * d * d, vc + aw * d))
    seg = capi.imu_segments(ts, acc, gyro, [s_[0] for s_ in states], [s_[1] for s_ in states], [s_[2] for s_ in states])
    seg["t1"][-1] = np.inf
    return seg, states[-1]


class HipBackend:
    """The C ABI: device-resident front end, voxel map, ICP factors (batched re-linearization), photometric path."""

    def __init__(self, ctx, cfg: ReplayConfig, mode=synth.ENWIDE_NEIGHBOR_MODE):
        from . import capi
        self.capi, self.ctx, self.cfg = capi, ctx, cfg
        reg = cfg.reg
        self.reg = capi.make_reg_config(**reg)
        self.regd = reg
        self.map = capi.VoxelMap(ctx, leaf=reg["target_ivox_map_leaf_size"], min_dist=reg["target_ivox_map_min_dist_in_voxel"], mode=mode)
        self.scan = capi.Scan(ctx)
        self.icfg = capi.make_input_config()
        self.I3, self.z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        # the photometric path on its own context (stream): see host/mimosa_hip/replay.hpp
        self.photo_ctx = capi.Context(ctx.device) if cfg.photometric else None
        self.photo = capi.Photo(self.photo_ctx, cfg.photo) if cfg.photometric else None
        if self.photo is not None:
            ctx.check(ctx.L.mh_scan_keep_raw(self.scan.h, 1))

    def seed_map(self, xyz):
        self.map.insert(xyz)

    def prepare(self, raw):
        self.scan.prepare_input(raw, self.icfg)
        return self.scan.unique_ns()

    def deskew_and_preprocess(self, T_Le_Lt):
        self.scan.deskew(T_Le_Lt.astype(np.float32))
        if self.photo is not None:
            self.photo.preprocess_scan(self.scan, T_Le_Lt)
        info = self.scan.preprocess_geometric(self.I3, self.z3, self.regd["source_voxel_grid_filter_leaf_size"], 20,
                                              self.regd["source_voxel_grid_min_dist_in_voxel"])
        return info["n_downsampled"]

    def prepare_resident(self, raw):
        self.scan.prepare_input(raw, self.icfg)     # the distinct timestamps stay on the device

    def deskew_imu_and_preprocess(self, segments, header_ts, R_end, p_end):
        """deskew_and_preprocess with the poses computed on the device from the IMU intervals (body = sensor frame here)."""
        self.scan.deskew_imu(segments, header_ts, GRAVITY, (R_end.T, -R_end.T @ p_end), (np.eye(3), np.zeros(3)))
        if self.photo is not None:
            self.photo.preprocess_scan_resident(self.scan)
        info = self.scan.preprocess_geometric(self.I3, self.z3, self.regd["source_voxel_grid_filter_leaf_size"], 20,
                                              self.regd["source_voxel_grid_min_dist_in_voxel"])
        return info["n_downsampled"]

    def make_factor(self):
        f = self.scan.make_factor(self.map, self.reg)
        f.set_components(False)  # the loop takes H, b, f only (mh_icp_set_components)
        return f

    def align_first(self, f, R, t, max_iters):
        """init_align: the factor's scan aligned to the map from (R, t); the association state the loop leaves stays with f"""
        r = f.align(R, t, self.capi.make_align_config(max_iters=max_iters, eps_rot=1e-6, eps_trans=1e-6, damping=1e-9))
        return r["R"], r["t"]

    def relocalise_first(self, f, R, t, cfg: "ReplayConfig"):
        """relocalise_first: the pose of the factor's scan from a grid of candidates around the (wrong) guess (R, t); the factor
        comes back reset, as fresh as make_factor left it.  Returns (R, t, the call's result)"""
        Rs, ts = self.capi.pose_grid(R, t, cfg.relocalise_half_xy, cfg.relocalise_step_xy, np.deg2rad(cfg.relocalise_half_yaw_deg),
                                     np.deg2rad(cfg.relocalise_step_yaw_deg))
        align = self.capi.make_align_config(max_iters=30, eps_rot=1e-6, eps_trans=1e-6, damping=1e-9)
        rc = self.capi.make_reloc_config(gate=self.regd["max_corres_distance"], stride=4, top_k=4, align=align, final_gate=0.1)
        r = f.relocalise(Rs, ts, rc, batch=cfg.relocalise_batch)
        f.release_reloc_work()  # relocalise_batch: the clones the candidates were aligned on
        return r["R"], r["t"], r

    def make_photo_factor(self):
        return self.photo.make_factor() if self.photo is not None and self.photo.features() else None

    def linearize_window(self, factors, poses):
        """Every live ICP factor at its current pose: ONE batched call."""
        rs = self.capi.linearize_batch(factors, [p[0] for p in poses], [p[1] for p in poses])
        return [(np.asarray(r["H_ss"]).reshape(6, 6), np.asarray(r["b_s"]), float(r["f"])) for r in rs]

    def optimise_window(self, factors, poses, Zs, iters, between_info, prior_info, damping, relin=None, linear=None, edges=None, joint=None):
        """device_window: the smoother's loop over the window as one call; the poses after it and the cost before each iteration.
        linear: host-linearized Hessian factors on poses of the window (capi.optimise_window)"""
        cfg = self.capi.make_window_config(iters=iters, between_info=between_info, prior_info=prior_info, damping=damping)
        I3, z3 = np.eye(3), np.zeros(3)
        kw = {} if relin is None else dict(relin=relin)
        if linear is not None:
            kw["linear"] = linear
        if edges is not None:  # mh_icp_window_optimise_edges, also with an empty list
            kw["edges"] = edges
        if joint is not None:  # mh_icp_window_optimise_joint
            kw["joint"] = joint
        r = self.capi.optimise_window(factors, poses, cfg, has_Z=[Z is not None for Z in Zs], Z=[(I3, z3) if Z is None else Z for Z in Zs], **kw)
        if r["iters"] != iters:
            raise np.linalg.LinAlgError("Singular matrix")
        return [(r["R"][i], r["t"][i]) for i in range(len(factors))], [row["f"] for row in r["trace"]]

    def marginalise_window(self, factors, poses, Zs, between_info, prior_info, damping, linear, edges):
        """window_marginal: what eliminating the oldest pose leaves on the next one (capi.marginalise_window's dict)"""
        cfg = self.capi.make_window_config(iters=1, between_info=between_info, prior_info=prior_info, damping=damping)
        I3, z3 = np.eye(3), np.zeros(3)
        return self.capi.marginalise_window(factors, poses, cfg, has_Z=[Z is not None for Z in Zs], Z=[(I3, z3) if Z is None else Z for Z in Zs],
                                            linear=linear, edges=edges)

    def marginalise_window_joint(self, factors, poses, Zs, between_info, prior_info, damping, linear, edges, joint):
        """window_marginal_joint: what eliminating the oldest pose leaves on its separator (capi.marginalise_window_joint's dict)"""
        cfg = self.capi.make_window_config(iters=1, between_info=between_info, prior_info=prior_info, damping=damping)
        I3, z3 = np.eye(3), np.zeros(3)
        return self.capi.marginalise_window_joint(factors, poses, cfg, has_Z=[Z is not None for Z in Zs], Z=[(I3, z3) if Z is None else Z for Z in Zs],
                                                  linear=linear, edges=edges, joint=joint)

    def linearize_photo(self, pf, R, t):
        r = pf.linearize(R, t)
        return np.asarray(r["H_bb"]).reshape(6, 6), np.asarray(r["b_b"]), float(r["f"]), int(r["status_hist"][8])

    def linearize_photo_window(self, pfs, poses):
        """Every photometric factor of the window at its own pose: ONE batched call."""
        rs = self.capi.photo_linearize_batch(pfs, [p[0] for p in poses], [p[1] for p in poses])
        return [(np.asarray(r["H_bb"]).reshape(6, 6), np.asarray(r["b_b"]), float(r["f"]), int(r["status_hist"][8])) for r in rs]

    def update_map(self, R, t):
        # Geometric::updateMap: copy-then-insert (geometric.cpp:494-495), f32 world transform (:483-490) on the device
        new = self.map.copy()
        new.insert_from_scan(self.scan, R, t)
        self.map.release()
        self.map = new

    def update_map_carved(self, R, t, carve_cfg):
        """carve_keyframes: update_map with the fork carved by the scan's body cloud first (the replay's body frame is the lidar
        frame: the sensor sits at its origin); returns the carve's six counters"""
        new = self.map.copy()
        counters = new.carve_from_scan(self.scan, self.capi.Scan.BODY, np.zeros(3), R, t, dict(carve_cfg, apply=True))
        new.insert_from_scan(self.scan, R, t)
        self.map.release()
        self.map = new
        return counters

    def map_points(self):
        return self.map.stats()["n_points"]

    def preview_map(self, R, t):
        """keyframe_new_fraction: what update_map(R, t) would add to the map, without the copy and the insert (the six counts)"""
        return self.map.preview_insert_from_scan(self.scan, R, t)

    def photo_update_map(self, pf, R, t):
        self.photo.update_map(pf, R, t, synth_photo.BIAS_DIRECTIONS)

    def release(self, f):
        f.destroy()


def first_state(cfg: ReplayConfig, scan0, rng_seed=7):
    """State at the first IMU sample of the first sweep: ground truth + the prior error (the caller's first guess)."""
    rng = np.random.default_rng(rng_seed)
    Rs = scan0["R_gt"] @ synth.so3_exp(np.deg2rad(cfg.prior_rot_noise_deg) * rng.standard_normal(3))
    ps = scan0["t_gt"] + cfg.prior_trans_noise * rng.standard_normal(3)
    w_, v_body = np.asarray(cfg.w, float), np.asarray(cfg.v, float)
    R_start = Rs @ synth.so3_exp(-w_ * cfg.dt)
    p_start = ps - R_start @ (v_body * cfg.dt)
    return R_start, p_start, R_start @ v_body


def write_native_input(path, cfg: ReplayConfig, scans, rng_seed=7, mode=synth.ENWIDE_NEIGHBOR_MODE):
    """The input file of the native harness (mimosa_amd/host/replay_main.cpp): length-prefixed little-endian vectors."""
    import struct
    from . import capi
    with open(path, "wb") as f:
        def w(arr, dtype=None):
            arr = np.ascontiguousarray(arr if dtype is None else np.asarray(arr, dtype))
            f.write(struct.pack("<Q", len(arr) if arr.dtype.itemsize == 32 else arr.size))
            f.write(arr.tobytes())
        w([cfg.window, cfg.update_iters, int(cfg.photometric), mode, 1000] + ([1] if cfg.photo_window and not cfg.init_align else [])
          + ([int(cfg.photo_window), cfg.init_align_iters] if cfg.init_align else []), np.int32)
        w([cfg.between_sigma_rot, cfg.between_sigma_trans, cfg.keyframe_trans_thresh, cfg.keyframe_rot_thresh_deg, *GRAVITY], np.float64)
        w(np.frombuffer(bytes(capi.make_reg_config(**cfg.reg)), np.uint8))
        w(np.frombuffer(bytes(capi.make_input_config()), np.uint8))
        if cfg.photometric:
            pc = cfg.photo
            w([pc["rows"], pc["cols"], pc["destagger"], pc["erosion_buffer"], pc["patch_size"], pc["margin_size"], pc["remove_lines"],
               pc["filter_brightness"], pc["gaussian_blur"], pc["gaussian_blur_size"], pc["nma_radius"], pc["num_features_detect"],
               pc["max_feature_life_time"], pc["rotate_patch_to_align_with_gradient"], pc["use_robust_cost_function"],
               pc["robust_cost_function"], pc["brightness_window_size"][0], pc["brightness_window_size"][1]], np.int32)
            w([pc["range_min"], pc["range_max"], pc["intensity_scale"], pc["intensity_gamma"], pc["gradient_threshold"],
               pc["max_dist_from_mean"], pc["max_dist_from_plane"], pc["occlusion_range_diff_threshold"],
               pc["lidar_origin_to_beam_origin_mm"], pc["robust_cost_function_parameter"], pc["error_scale"], pc["max_error"],
               pc["sigma"]], np.float64)
            w(pc["pixel_shift_by_row"], np.int32)
            w(pc["beam_altitude_angles"], np.float32)
            w(pc["high_pass_fir"], np.float64)
            w(pc["low_pass_fir"], np.float64)
            w(np.asarray(pc["patch_offsets"], np.int32).ravel())
            w(np.concatenate([np.asarray(pc["T_B_L_R"], float).ravel(), np.asarray(pc["T_B_L_t"], float)]))
        w(np.asarray(synth_photo.BIAS_DIRECTIONS, np.float64).ravel())
        w(synth.make_room(synth.BASE_SEED, 0, 0, room=np.asarray(cfg.room)).astype(np.float32).ravel())
        R0, p0, v0 = first_state(cfg, scans[0], rng_seed)
        w(np.concatenate([R0.ravel(), p0, v0]))
        w([len(scans)], np.int32)
        for sc in scans:
            ts, gyro, acc = sc["imu"]
            w(sc["raw"])
            w(ts, np.float64)
            w(np.asarray(gyro, np.float64).ravel())
            w(np.asarray(acc, np.float64).ravel())
            w([sc["header_ts"]], np.float64)
        if cfg.odometry_every > 0:  # the trailing section the driver reads behind its `odometry` word
            w([cfg.odometry_every], np.int32)
            w([cfg.odometry_sigma_rot_deg, cfg.odometry_sigma_trans_m], np.float64)
            msgs = odometry_messages(cfg, scans)
            w(np.concatenate([np.concatenate([[float(k)], R.ravel(), t, cov.ravel()]) for k, R, t, cov in msgs]) if msgs else np.zeros(0), np.float64)


def _check_window_marginal(cfg, error):
    if cfg.window_marginal_joint:
        if not cfg.device_window:
            raise error("window_marginal_joint is only offered with device_window")
        if cfg.window_marginal:
            raise error("window_marginal_joint is not offered together with window_marginal")
        if not 1 <= cfg.odometry_every <= 4:
            raise error("window_marginal_joint is offered with odometry_every 1 .. 4: the separator of the oldest pose may have at most four poses")
        if cfg.window < 2:
            raise error("window_marginal_joint needs a window of at least two poses")
    if not cfg.window_marginal:
        return
    if not cfg.device_window:
        raise error("window_marginal is only offered with device_window")
    if cfg.odometry_every > 1:
        raise error("window_marginal is not offered with odometry_every > 1: an odometry edge would reach from pose 0 beyond pose 1")
    if cfg.window < 2:
        raise error("window_marginal needs a window of at least two poses")


def run_native(cfg: ReplayConfig, scans, workdir, repeats=1, rng_seed=7, visible_device=None, through_manager=False, sequential=False,
               sharded_world=0, sharded_rccl=False, timeout=900):
    """The same replay through the C++ host mirror (host/mimosa_hip/replay.hpp): no Python between the library calls.
    visible_device: run the driver with HIP_VISIBLE_DEVICES set to it (one replay per GPU of a node).
    through_manager: every scan goes through lidar::Manager::callback (host/mimosa_hip/manager.hpp: the reference's method
    names and call order, the first cloud initialises instead of being registered) instead of FixedLagReplay's own loop.
    sharded_world = W > 0: the map sharded over W ranks inside the driver process (host/mimosa_hip/sharded_replay.hpp, one host
    thread per rank, in-process transport); sharded_rccl: the driver is one rank of the launch this process belongs to (RANK /
    WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT in the environment), RCCL inside the library."""
    import json
    import os
    import subprocess
    import sys
    from . import build
    if cfg.window_relin is not None and not cfg.device_window:
        raise RuntimeError("window_relin is only offered with device_window")
    if cfg.window_photo_linear and not cfg.device_window:
        raise RuntimeError("window_photo_linear is only offered with device_window")
    _check_window_marginal(cfg, RuntimeError)
    if cfg.relocalise_first:
        raise RuntimeError("relocalise_first is only offered by the python replay with HipBackend")
    if cfg.keyframe_new_fraction > 0:
        raise RuntimeError("keyframe_new_fraction is only offered by the python replay with HipBackend")
    if cfg.carve_keyframes:
        raise RuntimeError("carve_keyframes is only offered by the python replay with HipBackend")
    exe = build.build_replay_native()
    path = os.path.join(workdir, "replay_input.bin")
    write_native_input(path, cfg, scans, rng_seed)
    env = dict(os.environ)
    if visible_device is not None:
        env["HIP_VISIBLE_DEVICES"] = str(visible_device)
    mode = ["manager"] if through_manager else (["sequential"] if sequential else [])
    if sharded_world:
        mode = ["sharded", str(sharded_world)]
    if sharded_rccl:
        mode = ["sharded-rccl"]
    if cfg.device_window:
        word = "device-window" if cfg.window_relin is None else "device-window-relin=%r,%r" % (float(cfg.window_relin[0]), float(cfg.window_relin[1]))
        mode = mode + [word + ("+photo-linear" if cfg.window_photo_linear else "") + ("+marginal" if cfg.window_marginal else "")
                       + ("+marginal-joint" if cfg.window_marginal_joint else "")]
    if cfg.odometry_every > 0:
        mode = mode + ["odometry"]
    if cfg.device_poses:
        mode = mode + ["device-poses"]
    out = subprocess.run([exe, path, str(repeats)] + mode, capture_output=True, text=True, timeout=timeout, env=env)
    os.remove(path)
    if out.returncode != 0:
        raise RuntimeError("replay_native failed: " + out.stderr[-2000:])
    if out.stderr and (os.environ.get("MH_ALLOC_TRACE") or os.environ.get("MH_DETECT_TRACE")):
        sys.stderr.write(out.stderr)   # the library's diagnostic traces
    r = json.loads(out.stdout)
    r["poses_est"] = [(np.array(p[:9]).reshape(3, 3), np.array(p[9:])) for p in r.pop("poses")]
    return r


def run(cfg: ReplayConfig, backend, scans=None, rng_seed=7):
    """Replay: returns dict(poses_est, errors, keyframes, per-stage seconds, ...)."""
    scans = scans if scans is not None else make_scans(cfg)
    if cfg.device_poses and not hasattr(backend, "deskew_imu_and_preprocess"):
        raise ValueError("device_poses needs a backend that keeps the pose table on the device (HipBackend)")
    if cfg.window_relin is not None and not cfg.device_window:
        raise ValueError("window_relin is only offered with device_window")
    if cfg.window_photo_linear and not cfg.device_window:
        raise ValueError("window_photo_linear is only offered with device_window")
    _check_window_marginal(cfg, ValueError)
    if cfg.device_window and cfg.photometric and not cfg.window_photo_linear:
        raise ValueError("device_window is not offered with the photometric factor enabled")
    if cfg.device_window and not hasattr(backend, "optimise_window"):
        raise ValueError("device_window needs a backend with mh_icp_window_optimise (HipBackend)")
    if cfg.init_align and not hasattr(backend, "align_first"):
        raise ValueError("init_align needs a backend with mh_icp_align (HipBackend)")
    if cfg.relocalise_first and not hasattr(backend, "relocalise_first"):
        raise ValueError("relocalise_first needs a backend with mh_icp_relocalise (HipBackend)")
    if cfg.relocalise_first and cfg.init_align:
        raise ValueError("relocalise_first aligns the first scan itself: not offered together with init_align")
    if cfg.relocalise_batch and not cfg.relocalise_first:
        raise ValueError("relocalise_batch is only offered with relocalise_first")
    if cfg.keyframe_new_fraction > 0 and not hasattr(backend, "preview_map"):
        raise ValueError("keyframe_new_fraction needs a backend with mh_map_preview_insert (HipBackend)")
    if cfg.carve_keyframes and not hasattr(backend, "update_map_carved"):
        raise ValueError("carve_keyframes needs a backend with mh_map_carve (HipBackend)")
    carve_cfg = dict(grid=cfg.carve_grid, ring=cfg.carve_ring, range_min=cfg.carve_range_min, range_max=cfg.carve_range_max,
                     margin_abs=cfg.carve_margin_abs, margin_rel=cfg.carve_margin_rel)
    relocalised = None
    new_fraction, kf_scans, carved, map_points = [], [], [], []
    backend.seed_map(synth.make_room(synth.BASE_SEED, 0, 0, room=np.asarray(cfg.room)))
    stage = {"front_end": 0.0, "imu": 0.0, "factor_create": 0.0, "optimise": 0.0, "update_map": 0.0}
    v_body = np.asarray(cfg.v, float)
    Wb = np.diag([1.0 / cfg.between_sigma_rot**2] * 3 + [1.0 / cfg.between_sigma_trans**2] * 3)
    odo = OdometryManager(cfg.odometry_sigma_rot_deg, cfg.odometry_sigma_trans_m) if cfg.odometry_every > 0 else None
    odo_msgs = {m[0]: m for m in odometry_messages(cfg, scans)}
    edges = []        # live odometry edges: dicts(ka, kb, Z, info), ka < kb scan indices
    win = []          # live window: dicts(k, R, t, factor, Z (relative pose to the previous scan), fresh)
    est, kf_poses, n_kf, costs, n_photo_valid, n_photo_window = [], [], 0, [], [], []
    carried, marginal_valid = None, []  # window_marginal: the marginal prior on the window's pose 0 (None: the pin), every marginal's valid flag
    carried_joint, separator_sizes = None, []  # window_marginal_joint: the joint prior (None: the pin), the separator of every marginal
    pin = [1.0 / 1e-4**2] * 6
    loose_info = [1.0 / np.deg2rad(1.0)**2] * 3 + [1.0 / 0.1**2] * 3
    R_prev = t_prev = vel_prev = None
    t0 = time.perf_counter()
    for k, sc in enumerate(scans):
        a0 = time.perf_counter()
        if cfg.device_poses:
            backend.prepare_resident(sc["raw"])
            uns = np.zeros(0, np.uint32)
        else:
            uns = backend.prepare(sc["raw"])
        a1 = time.perf_counter()
        # IMU propagation from the previous scan's estimate (first scan: ground truth + the prior error)
        if R_prev is None:
            R_start, p_start, vel_start = first_state(cfg, sc, rng_seed)   # state at the first IMU sample of this sweep
        else:
            R_start, p_start, vel_start = R_prev, t_prev, vel_prev
        if cfg.device_poses:
            segments, (R_pred, p_pred, vel_pred) = imu_segments(R_start, p_start, vel_start, sc["imu"])
            a2 = time.perf_counter()
            backend.deskew_imu_and_preprocess(segments, sc["header_ts"], R_pred, p_pred)
        else:
            T_W_Bt, (R_pred, p_pred, vel_pred) = propagate(R_start, p_start, vel_start, sc["imu"], sc["header_ts"], uns)
            T_Le_Lt = np.empty_like(T_W_Bt)
            T_Le_Lt[:, :9] = (R_pred.T @ T_W_Bt[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
            T_Le_Lt[:, 9:] = (T_W_Bt[:, 9:] - p_pred) @ R_pred
            a2 = time.perf_counter()
            backend.deskew_and_preprocess(T_Le_Lt)
        a3 = time.perf_counter()
        f = backend.make_factor()
        pf = backend.make_photo_factor() if cfg.photometric else None
        Z = _between(R_start, p_start, R_pred, p_pred) if R_prev is not None else None
        R_w, t_w = R_pred, p_pred
        if cfg.init_align and R_prev is None:
            R_w, t_w = backend.align_first(f, R_pred, p_pred, cfg.init_align_iters)
        if cfg.relocalise_first and R_prev is None:
            R_guess = synth.rot_z(np.deg2rad(cfg.relocalise_guess_yaw_deg)) @ R_pred
            t_guess = p_pred + np.asarray(cfg.relocalise_guess_offset, float)
            R_w, t_w, rr = backend.relocalise_first(f, R_guess, t_guess, cfg)
            relocalised = dict(guess=(R_guess, t_guess), pose=(R_w, t_w), predicted=(R_pred, p_pred), best=rr["best"],
                               candidates=[c["index"] for c in rr["cand"]], fine=[c["fine"] for c in rr["cand"]])
        win.append(dict(k=k, R=R_w, t=t_w, f=f, Z=Z, pf=pf if cfg.photo_window else None))
        if len(win) > cfg.window:
            if cfg.window_marginal or cfg.window_marginal_joint:
                # the window as it was optimised (without the scan that just arrived), at its current poses, with the carried
                # prior and, where the window call passes it, the oldest pose's photometric factor as a linear factor on pose 0;
                # the live edges as edges (window_marginal_joint: those from pose 0 reach beyond pose 1)
                live = win[:-1]
                mlin = [] if carried is None else [carried]
                if cfg.window_photo_linear and cfg.photo_window and live[0]["pf"] is not None:
                    T0 = (live[0]["R"], live[0]["t"])
                    Hp, bp, fp, nv = backend.linearize_photo_window([live[0]["pf"]], [T0])[0]
                    if nv and np.all(np.isfinite(Hp)) and np.all(np.isfinite(bp)) and np.isfinite(fp):
                        mlin.append(dict(pose=0, at=T0, H=Hp, b=bp, f=fp))
                medges = [dict(a=e["ka"] - live[0]["k"], b=e["kb"] - live[0]["k"], Z=e["Z"], info=e["info"]) for e in edges]
                has_prior = carried is not None or carried_joint is not None
                prior = [0.0] * 6 if has_prior else (loose_info if live[0]["k"] == 0 else pin)
                margs = ([w["f"] for w in live], [(w["R"], w["t"]) for w in live], [None] + [w["Z"] for w in live[1:]], list(np.diag(Wb)), prior, 1e-9, mlin, medges)
                if cfg.window_marginal:
                    m = backend.marginalise_window(*margs)
                    carried = m["linear"] if m["valid"] else None
                else:  # the carried joint prior goes in and is absorbed
                    m = backend.marginalise_window_joint(*margs, carried_joint)
                    separator_sizes.append(len(m["joint"]["poses"]))
                    carried_joint = m["joint"] if m["valid"] else None
                marginal_valid.append(int(m["valid"]))
            old = win.pop(0)
            backend.release(old["f"])
            if old["pf"] is not None:
                backend.release(old["pf"])
        if odo is not None:
            if k in odo_msgs:
                got = odo.callback(k, *odo_msgs[k][1:])
                if got is not None:
                    edges.append(dict(ka=got[0], kb=k, Z=got[1], info=got[2]))
            edges = [e for e in edges if e["ka"] >= win[0]["k"]]  # dropped once the older pose has left the window
        if cfg.photo_window:
            n_photo_window.append(sum(w["pf"] is not None for w in win))
        a4 = time.perf_counter()
        # ---- smoother update: every live factor re-linearized per iteration -------------------------------------
        nW = len(win)
        fs = []
        if cfg.device_window:
            loose = win[0]["k"] == 0 and k < cfg.window
            sr, st = (np.deg2rad(1.0), 0.1) if loose else (1e-4, 1e-4)
            kw = {} if cfg.window_relin is None else dict(relin=tuple(cfg.window_relin))
            if cfg.window_photo_linear:
                # the photometric factors of this call (as the host loop below chooses them), linearized once at the call's initial
                # poses; one without valid features or with a non-finite entry is skipped, as that loop skips it
                if cfg.photo_window:
                    at = [i for i, w in enumerate(win) if w["pf"] is not None]
                else:
                    at = [nW - 1] if pf is not None else []
                pfs = [win[i]["pf"] if cfg.photo_window else pf for i in at]
                poses = [(win[i]["R"], win[i]["t"]) for i in at]
                if len(at) > 1 or (at and cfg.photo_window):
                    plin = backend.linearize_photo_window(pfs, poses)
                else:
                    plin = [backend.linearize_photo(p, R_, t_) for p, (R_, t_) in zip(pfs, poses)]
                kw["linear"] = [dict(pose=i, at=T, H=Hp, b=bp, f=fp) for i, T, (Hp, bp, fp, nv) in zip(at, poses, plin)
                                if nv and np.all(np.isfinite(Hp)) and np.all(np.isfinite(bp)) and np.isfinite(fp)]
            if odo is not None:
                kw["edges"] = [dict(a=e["ka"] - win[0]["k"], b=e["kb"] - win[0]["k"], Z=e["Z"], info=e["info"]) for e in edges]
            prior = [1.0 / sr**2] * 3 + [1.0 / st**2] * 3
            if carried is not None:  # the marginal prior stands in for the pin
                kw["linear"] = kw.get("linear", []) + [carried]
                prior = [0.0] * 6
            if carried_joint is not None:  # ... or the joint prior
                kw["joint"] = carried_joint
                prior = [0.0] * 6
            new_poses, fs = backend.optimise_window([w["f"] for w in win], [(w["R"], w["t"]) for w in win], [None] + [w["Z"] for w in win[1:]],
                                                    cfg.update_iters, list(np.diag(Wb)), prior, 1e-9, **kw)
            for w, (R_n, t_n) in zip(win, new_poses):
                w["R"], w["t"] = R_n, t_n
        else:
            for it in range(cfg.update_iters):
                lin = backend.linearize_window([w["f"] for w in win], [(w["R"], w["t"]) for w in win])
                A = np.zeros((6 * nW, 6 * nW))
                g = np.zeros(6 * nW)
                cost = 0.0
                for i, (H, b, fv) in enumerate(lin):
                    A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += H
                    g[6 * i:6 * i + 6] += b
                    cost += fv
                if cfg.photo_window:
                    at = [i for i, w in enumerate(win) if w["pf"] is not None]
                    pfs, poses = [win[i]["pf"] for i in at], [(win[i]["R"], win[i]["t"]) for i in at]
                    if not at:
                        plin = []
                    elif hasattr(backend, "linearize_photo_window"):
                        plin = backend.linearize_photo_window(pfs, poses)
                    else:
                        plin = [backend.linearize_photo(p, R_, t_) for p, (R_, t_) in zip(pfs, poses)]
                else:
                    at = [nW - 1] if pf is not None else []
                    plin = [backend.linearize_photo(pf, win[-1]["R"], win[-1]["t"])] if pf is not None else []
                for i, (Hp, bp, fp, nv) in zip(at, plin):
                    if nv and np.all(np.isfinite(Hp)) and np.all(np.isfinite(bp)):
                        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] += Hp
                        g[6 * i:6 * i + 6] += bp
                        cost += fp
                for i in range(1, nW):
                    if win[i]["Z"] is None:
                        continue
                    Rz, tz = win[i]["Z"]
                    Rab, tab = _between(win[i - 1]["R"], win[i - 1]["t"], win[i]["R"], win[i]["t"])
                    Re, te = Rz.T @ Rab, Rz.T @ (tab - tz)                     # Z^-1 * between(X_{i-1}, X_i)
                    r = np.concatenate([_so3_log(Re), te])
                    Jb = np.eye(6)
                    Ja = -_adjoint(Rab.T, -Rab.T @ tab)                         # -Ad(between^-1)
                    J = np.zeros((6, 6 * nW))
                    J[:, 6 * (i - 1):6 * i] = Ja
                    J[:, 6 * i:6 * i + 6] = Jb
                    A += J.T @ Wb @ J
                    g += J.T @ Wb @ r
                    cost += float(r @ Wb @ r)
                for e in edges:  # the odometry edges, behind the IMU ties
                    ia, ib = e["ka"] - win[0]["k"], e["kb"] - win[0]["k"]
                    Rz, tz = e["Z"]
                    Rab, tab = _between(win[ia]["R"], win[ia]["t"], win[ib]["R"], win[ib]["t"])
                    r = np.concatenate([_so3_log(Rz.T @ Rab), Rz.T @ (tab - tz)])
                    J = np.zeros((6, 6 * nW))
                    J[:, 6 * ia:6 * ia + 6] = -_adjoint(Rab.T, -Rab.T @ tab)
                    J[:, 6 * ib:6 * ib + 6] = np.eye(6)
                    A += J.T @ e["info"] @ J
                    g += J.T @ e["info"] @ r
                    cost += float(r @ e["info"] @ r)
                # what marginalisation leaves on the oldest pose; loose while that pose has never been optimised
                loose = win[0]["k"] == 0 and k < cfg.window
                sr, st = (np.deg2rad(1.0), 0.1) if loose else (1e-4, 1e-4)
                A[:6, :6] += np.diag([1.0 / sr**2] * 3 + [1.0 / st**2] * 3)
                xi = np.linalg.solve(A + 1e-9 * np.eye(6 * nW), -g)
                for i, w in enumerate(win):
                    w["R"], w["t"] = _retract(w["R"], w["t"], xi[6 * i:6 * i + 6])
                fs.append(cost)
        costs.append(fs)
        a5 = time.perf_counter()
        R, t = win[-1]["R"], win[-1]["t"]
        # ---- Geometric::updateMap's keyframe test (geometric.cpp:445-478): nearest stored pose by translation, then
        # the largest of |yaw|, |pitch|, |roll| of the relative rotation against the threshold
        is_kf = True
        if cfg.keyframe_new_fraction > 0:  # first keyframe, or the map would keep enough of the scan; the pose test is not evaluated
            pv = backend.preview_map(R, t)
            new_fraction.append(pv["n_added"] / pv["n_points"] if pv["n_points"] else 0.0)
            is_kf = not kf_poses or pv["n_added"] >= cfg.keyframe_new_fraction * pv["n_points"]
        elif kf_poses:
            dists = [np.linalg.norm(t - tk) for _, tk in kf_poses]
            j = int(np.argmin(dists))
            d = kf_poses[j][0].T @ R
            ypr = (np.arctan2(d[1, 0], d[0, 0]), np.arctan2(-d[2, 0], np.hypot(d[2, 1], d[2, 2])), np.arctan2(d[2, 1], d[2, 2]))
            is_kf = dists[j] > cfg.keyframe_trans_thresh or max(abs(a) for a in ypr) > cfg.keyframe_rot_thresh_deg * 0.017453293
        if is_kf:
            if cfg.carve_keyframes:
                carved.append(backend.update_map_carved(R, t, carve_cfg))
            else:
                backend.update_map(R, t)
            if hasattr(backend, "map_points"):
                map_points.append(backend.map_points())
            kf_poses.append((R, t))
            kf_scans.append(k)
            n_kf += 1
        if cfg.photometric:
            if pf is not None:
                n_photo_valid.append(int(pf.linearize(R, t)["status_hist"][8]))
            backend.photo_update_map(pf, R, t)
            if pf is not None and not cfg.photo_window:
                backend.release(pf)
        a6 = time.perf_counter()
        stage["front_end"] += (a1 - a0) + (a3 - a2)
        stage["imu"] += a2 - a1
        stage["factor_create"] += a4 - a3
        stage["optimise"] += a5 - a4
        stage["update_map"] += a6 - a5
        est.append((R, t))
        # velocity: the propagated one, carried into the corrected attitude
        R_prev, t_prev, vel_prev = R, t, R @ (R_pred.T @ vel_pred)
    for w in win:
        backend.release(w["f"])
        if w["pf"] is not None:
            backend.release(w["pf"])
    total = time.perf_counter() - t0
    terr = [float(np.linalg.norm(te - s["t_gt"])) for (_, te), s in zip(est, scans)]
    rerr = [float(np.rad2deg(np.linalg.norm(_so3_log(Re.T @ s["R_gt"])))) for (Re, _), s in zip(est, scans)]
    return {"poses_est": est, "trans_err": terr, "rot_err_deg": rerr, "n_keyframes": n_kf, "seconds": total,
            "scans_per_s": len(scans) / total, "stage_s": stage, "costs": costs, "photo_valid": n_photo_valid,
            "photo_in_window": n_photo_window, "marginal_valid": marginal_valid, "separator_sizes": separator_sizes, "relocalised": relocalised,
            "new_fraction": new_fraction, "keyframe_scans": kf_scans, "carve": carved, "map_points": map_points}
