"""The photometric factor zoo: PhotometricFactor::linearize (photometric_factor.hpp:136-355, photometric_utils.cpp:80-388) with
every branch reached by design, and every row held to a multi-precision reference.

Two parts, both importable without a GPU (the builder needs the C++ oracle for the image chain and the base features):

BUILDER.  64 x 512 frames of synth_photo.make_frame (seed SEED), 5 x 5 and 8 x 8 patches, base features detected on frame 0.
Every zoo feature is a base feature edited in Le_ps / psi (or re-centred on another pixel of frame 0: Le_ps = the deskewed
points of the patch pixels, psi = getPsi of the image there), or the frame is preprocessed from edited inputs (ranges of a
column's points zeroed, pose-table entries removed).  Two settings: identity motion in the binary form on frame 0 (T_a = T_b =
identity: residuals ~ 0, the statuses are the point) and frame 1 at its true pose plus a small step (the rows are the point),
unary and binary.  A Scene holds the bytes both the device and the oracle receive.  Designed tags, all asserted present
(DESIGNED_TAGS): valid / valid_low_contrast, range_far / range_near, range_at_0 / _mid / _last, seam_low / seam_high, theta_above /
theta_below, throw_first (counter 1) / throw_after_fail (counter 0: only the first failing point is evaluated), first_fail_range /
first_fail_mask (two different failures in one patch, the lower index decides), empty_search (pj[0] == 0, the column has
projections in another row) / empty_column (none: false), dup_vote / dup_tie (two candidates at equal f32 distance, the first
wins), pose_missing (some features Valid, others throw, n_exceptions = their number), mask, margin / margin_pass, occlusion /
occlusion_pass, maxerr_negated / maxerr_permuted, footprint (margin_size 1), second_project_false, robust scenes (huber_below / huber_above / cauchy,
error_scale 2: the reference reads error_scale into its config and never uses it, so do the oracle and the device), factors of
0, 1, 3, 4 and 5 features (kFeatPerBlock = 4; the device refuses the empty one at creation, as the reference's constructor
throws), unary with a non-trivial VSVt.  At identity motion an unedited deskewed point projects ONTO the tables (every decision a
tie), so every patch of those scenes is first turned by JIG_U columns and lowered by JIG_V rows.  Branch tags the reference itself records while
it evaluates (REFERENCE_TAGS) are asserted present too.  second_project_false (the second projection, of Li_p, failing where the
first passed) exists: early columns are undistorted by about three columns, so a point just inside the seam bound loses it.
The guess-miss fallback of the device's timestamp search is not the reference's business (it has a map lookup); the pose_missing
table has holes, so the interpolation guess misses there and the Valid features of that scene went through the binary search.

REFERENCE.  mpmath at DPS digits of project, projectUndistorted and the per-feature part of linearize (the formulas of
oracle/numpy_photo.py:70-101, 188-303), evaluated on the downloaded images themselves (yaw, proj_idx, mask, range, intensity,
dx, dy: f32 / integers, exact inputs), the deskewed cloud and the pose table.  Per feature: status, which exception, branch
tags, the residual row and the J_b / J_a rows (double-double: hi + lo), kappa = |Ib| / sigma.  Every discrete decision records
its distance to the tie in its own unit (pixel: the two rounds, floor in bilinear, the seam / field-of-view bounds and the
footprint exit; rad: the beam bounds and every probe of the yaw search; deg: the altitude search; m: range gate and occlusion;
ulp of f32: the rounding of the duplicate vote's squared distances; 1: max_error and Huber's threshold); both test modules
assert the smallest over the whole zoo is >= MARGIN = 1e-9 with no feature left out (measured: 6.1e-6, a yaw probe).  The one designed tie is the (-r, 0, 0) point of
throw_first / throw_after_fail (phi = pi, u = fx * pi + cx against 0): its expected outcome is fixed by hand (Scene.expect) to
what the reference source yields in fp64 (u < 0: "Invalid x coordinate" thrown) and what the oracle yields.

PS_PROJECT (3): declared by the reference (RejectStatus::PointProject, photometric_factor.hpp:40) and never assigned there; no
input can produce it, here or there.

The footprint exit (photo_kernels.hip, after the occlusion check): the reference's getSubPixelValue reads pixel (y0 + 1, x0 + 1);
that is inside the image for every u < cols - 1, v < rows - 1.  The config accepts margin_size 0 and 1, where a point between
the last two beams passes the margin test (round(v) = rows - 2 at margin 1) with rows - 2 < v < rows - 1: the reference samples
it (footprint rows rows - 2, rows - 1).  The device used to end such a feature as PS_PROJECT_UNDISTORTED (uy > rows - 2); it now
exits only where the footprint really leaves the image (uy >= rows - 1 or ux >= cols - 1, where the reference reads out of
bounds).  Case `footprint`.

THE ROW BOUND.  |row - reference| <= K * 2^-53 * kappa_f * scale, scale = wgt * max(|psi_b|, |psi_a|) for the residual entry and
wgt / sigma_b * max_i |D_ik| for column k of J (the size of the terms that cancel in the normalisation; never below |row|).
K is measured on the CPU from the C++ oracle against this reference over the whole zoo (test_photo_zoo_cpu prints it): worst
ratio 70.9, so the oracle is held to K_ORACLE = 128; the device measured 67.0 on the MI355X (MEASURED below); the device gets that worst ratio times 8 rounded up to a power of two (64-lane tree sums, a second libm for
atan2 / asin whose ulp on phi is amplified by 1 / (yl - yr)).
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import mpmath as mp
import numpy as np
from mpmath import mpf

DPS = 50
U = 2.0 ** -53
MARGIN = 1e-9
SEED = 1000
ROWS, COLS = 64, 512
JIG_U, JIG_V = 0.137, 0.061    # columns, rows
DEG2RAD, RAD2DEG = 0.017453293, 57.29578

# MEASURED: worst |row - reference| / (2^-53 * kappa * scale) over the whole zoo
#   oracle (CPU, sequential sums, glibc):  70.9  (rows5_binary; identity5 42.2, rows5_unary 51.7, rows8_unary 34.1)   -> K_ORACLE = 128
#   device (MI355X, tree sums, ocml):      67.0  (rows5_binary; identity5 57.6, rows5_unary 54.5, rows8_unary 31.9)   -> K_DEVICE = 1024
K_ORACLE_MEASURED = 70.9
K_ORACLE = 128.0                 # the measurement rounded up to a power of two
K_DEVICE = 1024.0                # 8 * 70.9 = 567 rounded up to a power of two
K_DEVICE_MEASURED = 67.0

SCENES = ("identity5", "footprint5", "empty_column5", "pose_missing5", "identity8", "rows5_binary", "rows5_huber", "rows5_cauchy", "rows5_unary",
          "rows5_unary_vsvt", "rows8_unary")
DESIGNED_TAGS = ("valid", "valid_low_contrast", "range_far", "range_near", "range_at_0", "range_at_mid", "range_at_last", "seam_low",
                 "seam_high", "theta_above", "theta_below", "throw_first", "throw_after_fail", "first_fail_range", "first_fail_mask",
                 "empty_search", "empty_column", "dup_vote", "dup_tie", "pose_missing", "mask", "margin", "margin_pass", "occlusion",
                 "occlusion_pass", "maxerr_negated", "maxerr_permuted", "footprint", "second_project_false")
REFERENCE_TAGS = ("ref_seam", "ref_theta", "ref_throw_project", "ref_throw_pose", "ref_empty_search", "ref_empty_column", "ref_dup_vote",
                  "ref_dup_tie", "ref_range", "ref_mask", "ref_margin", "ref_occlusion", "ref_maxerr", "ref_footprint", "ref_huber_below",
                  "ref_huber_above", "ref_cauchy", "second_project_false")


# ------------------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------------------
class Margins(dict):
    """smallest distance to a tie per unit, with the decision that set it"""

    def rec(self, unit, dist, what):
        d = float(abs(dist))
        if unit not in self or d < self[unit][0]:
            self[unit] = (d, what)

    def merge(self, other, label=""):
        for k, (d, w) in other.items():
            if k not in self or d < self[k][0]:
                self[k] = (d, f"{label} {w}")

    def smallest(self):
        return min((d for d, _ in self.values()), default=float("inf"))


def _m(x):
    return mpf(float(x))


class Model:
    """the constants of src/lidar/photometric_config.cpp:98-110 as the fp64 / f32 values every implementation holds, read as exact"""

    def __init__(self, cfg):
        from oracle import numpy_photo as npo

        self.cfg = cfg
        self.rows, self.cols = cfg["rows"], cfg["cols"]
        fx, fy, cx, bo = npo.derived(cfg)
        self.fx, self.fy, self.cx, self.bo = _m(fx), _m(fy), _m(cx), _m(bo)
        self.alt32 = np.asarray(cfg["beam_altitude_angles"], np.float32)
        self.alt = [_m(a) for a in self.alt32]
        self.rmin, self.rmax = _m(np.float32(cfg["range_min"])), _m(np.float32(cfg["range_max"]))
        self.occ = _m(np.float32(cfg["occlusion_range_diff_threshold"]))
        self.margin = int(cfg["margin_size"])
        self.TBL_R = [[_m(v) for v in r] for r in np.asarray(cfg["T_B_L_R"], float).reshape(3, 3)]
        self.TBL_t = [_m(v) for v in np.asarray(cfg["T_B_L_t"], float)]


def _round_half_away(x, mg, what):
    mg.rec("pixel", abs(x - mp.floor(x)) - mpf("0.5"), what)
    return int(mp.floor(abs(x) + mpf("0.5"))) * (1 if x >= 0 else -1)


def project(M, p, yaw, mg):
    """photometric_utils.cpp:80-198.  -> ("ok", u, v) | ("false", why) | ("throw",)"""
    L = mp.sqrt(p[0] * p[0] + p[1] * p[1]) - M.bo
    R = mp.sqrt(L * L + p[2] * p[2])
    phi, theta = mp.atan2(p[1], p[0]), mp.asin(p[2] / R)
    u = M.fx * phi + M.cx
    mg.rec("pixel", min(abs(u), abs(u - M.cols)), "u against 0 / cols")
    if u < 0 or u >= M.cols:
        return ("throw",)
    mg.rec("pixel", min(abs(u - 5), abs(u - (M.cols - 5))), "u against the seam bounds")
    if u < 5 or u > M.cols - 5:
        return ("false", "seam")
    hi, lo = M.alt[0] * _m(DEG2RAD), M.alt[-1] * _m(DEG2RAD)
    mg.rec("rad", min(abs(theta - hi), abs(theta - lo)), "theta against the beam bounds")
    if theta > hi or theta < lo:
        return ("false", "theta")
    th = theta * _m(RAD2DEG)
    mg.rec("deg", min(abs(a - th) for a in M.alt), "altitude search")
    above = [k for k, a in enumerate(M.alt) if a > th]
    g = min(above[-1] if above else 0, M.rows - 2)
    v = g + (M.alt[g] - th) / _m(np.float32(M.alt32[g] - M.alt32[g + 1]))
    vr = _round_half_away(v, mg, "round(v) for the yaw row")
    if vr < 0 or vr >= M.rows:
        return ("false", "row")
    row = yaw[vr]
    il, ir = int(mp.floor(u)) - 5, int(mp.floor(u)) + 5     # u >= 5: truncation = floor; the bracket found does not depend on the window
    il, ir = max(il, 0), min(ir, M.cols - 1)
    exact = None
    while ir - il > 1:
        mid = il + (ir - il) // 2
        ym = _m(row[mid])
        mg.rec("rad", abs(ym - phi), "yaw search probe")
        if ym == phi:
            exact = mid
            break
        if ym < phi:
            ir = mid
        else:
            il = mid
    if exact is not None:
        u = mpf(exact)
    else:
        u = il + (_m(row[il]) - phi) / _m(np.float32(row[il] - row[ir]))
    mg.rec("pixel", min(abs(u), abs(u - (M.cols - 1)), abs(v), abs(v - (M.rows - 1))), "in_fov")
    if not (0 <= u <= M.cols - 1 and 0 <= v <= M.rows - 1):
        return ("false", "fov")
    return ("ok", u, v)


def _f32_round(x, mg, what):
    """an mpf (>= 0) rounded to f32 as a double-computed value would be; the distance to the rounding boundary in ulps"""
    f = np.float32(float(x))
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    ulp = _m(hi) - _m(f)
    for nb in (lo, hi):
        mid = (_m(f) + _m(nb)) / 2
        if ulp > 0:
            mg.rec("ulp_f32", abs(x - mid) / ulp, what)
    return f


def project_undistorted(M, fr, p, mg, tags):
    """photometric_utils.cpp:287-366.  -> ("ok", Li, u, v, R) | ("false",) | ("throw", which)"""
    r = project(M, p, fr["yaw"], mg)
    if r[0] == "throw":
        tags.add("ref_throw_project")
        return ("throw", "project")
    if r[0] == "false":
        tags.add("ref_" + r[1])
        return ("false",)
    col, row = _round_half_away(r[1], mg, "round(u) of the first projection"), _round_half_away(r[2], mg, "round(v) of the first projection")
    pj = fr["proj_idx"]
    if pj[row, col, 0] == 0:
        rr = np.nonzero(pj[:, col, 0] > 0)[0]
        if len(rr) == 0:
            tags.add("ref_empty_column")
            return ("false",)
        tags.add("ref_empty_search")
        row = int(rr[0])
    n = int(pj[row, col, 0])
    cand = [int(j) for j in pj[row, col, 1:1 + n]]
    pts = fr["points"]
    if n > 1:
        tags.add("ref_dup_vote")
        d = []
        for j in cand:
            sq = sum((p[k] - _m(pts[ax][j])) ** 2 for k, ax in enumerate("xyz"))
            d.append(_f32_round(sq, mg, "f32 squared distance of the duplicate vote"))
        best = min(d)
        if sum(1 for x in d if x == best) > 1:
            tags.add("ref_dup_tie")
        j = cand[d.index(best)]                  # the first minimum: strict "<" in the reference
    else:
        j = cand[0]
    ns = fr["pose_ns"]
    k = int(np.searchsorted(ns, pts["t"][j]))
    if k >= len(ns) or ns[k] != pts["t"][j]:
        tags.add("ref_throw_pose")
        return ("throw", "pose")
    T = fr["pose_T"][k]
    Rm = [[_m(T[3 * a + b]) for b in range(3)] for a in range(3)]
    t = [_m(T[9 + a]) for a in range(3)]
    # gtsam Pose3::inverse then act: R^T p + (-(R^T t))
    Li = [sum(Rm[a][b] * p[a] for a in range(3)) - sum(Rm[a][b] * t[a] for a in range(3)) for b in range(3)]
    r = project(M, Li, fr["yaw"], mg)
    if r[0] == "throw":
        tags.add("ref_throw_project")
        tags.add("second_project_throw")
        return ("throw", "project")
    if r[0] == "false":
        tags.add("ref_" + r[1])
        tags.add("second_project_false")
        return ("false",)
    return ("ok", Li, r[1], r[2], Rm)


def bilinear(img, x, y, mg=None):
    x0, y0 = int(mp.floor(x)), int(mp.floor(y))
    if mg is not None:
        mg.rec("pixel", min(x - x0, x0 + 1 - x, y - y0, y0 + 1 - y), "floor in bilinear")
    dx, dy = x - x0, y - y0
    return ((1 - dx) * (1 - dy) * _m(img[y0, x0]) + dx * (1 - dy) * _m(img[y0, x0 + 1]) + (1 - dx) * dy * _m(img[y0 + 1, x0]) +
            dx * dy * _m(img[y0 + 1, x0 + 1]))


def _mat(a):
    return [[_m(v) for v in r] for r in np.asarray(a, float).reshape(3, 3)]


def _mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [sum(A[i][k] * v[k] for k in range(3)) for i in range(3)]


def _tr(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def _inv(R, t):
    Rt = _tr(R)
    return Rt, [-x for x in _mv(Rt, t)]


def _compose(Ra, ta, Rb, tb):
    return _mm(Ra, Rb), [x + y for x, y in zip(_mv(Ra, tb), ta)]


def _dd(x):
    hi = float(x)
    return hi, float(x - _m(hi))


def feature_reference(M, fr, ft, pose):
    """One feature of PhotometricFactor::linearize.  pose = (R_b, t_b, R_a, t_a) with R_a None for the unary form."""
    with mp.workdps(DPS):
        cfg = M.cfg
        mg, tags = Margins(), set()
        binary = pose[2] is not None
        Rb, tb = _mat(pose[0]), [_m(v) for v in pose[1]]
        Ra, ta = (_mat(pose[2]), [_m(v) for v in pose[3]]) if binary else (_mat(np.eye(3)), [mpf(0)] * 3)
        dBe = _compose(*_inv(Rb, tb), Ra, ta)
        dLe = _compose(*_compose(*_inv(M.TBL_R, M.TBL_t), *dBe), M.TBL_R, M.TBL_t)
        m = len(ft["Le_ps"])
        out = SimpleNamespace(status=0, exception=None, tags=tags, margins=mg, m=m, center=None, kappa=None, e=None, Jb=None, Ja=None,
                              e_scale=None, J_scale=None, whitened=None, n_eval=0)
        uv, pl, Rl, Ib = [], [], [], []
        for i in range(m):
            out.n_eval = i + 1
            a = [_m(v) for v in ft["Le_ps"][i]]
            p = [x + y for x, y in zip(_mv(dLe[0], a), dLe[1])]
            r = project_undistorted(M, fr, p, mg, tags)
            if r[0] != "ok":
                out.status = 1
                out.exception = r[1] if r[0] == "throw" else None
                break
            _, Li, u, v, Rm = r
            rng = mp.sqrt(sum(x * x for x in Li))
            mg.rec("m", min(abs(rng - M.rmin), abs(rng - M.rmax)), "range gate")
            if rng < M.rmin or rng > M.rmax:
                out.status = 2
                tags.add("ref_range")
                break
            ux, uy = _round_half_away(u, mg, "round(u) of the second projection"), _round_half_away(v, mg, "round(v) of the second projection")
            if not fr["mask"][uy, ux]:
                out.status = 4
                tags.add("ref_mask")
                break
            if ux < M.margin or ux >= M.cols - M.margin or uy < M.margin or uy >= M.rows - M.margin:
                out.status = 5
                tags.add("ref_margin")
                break
            diff = abs(_m(fr["range"][uy, ux]) - rng)
            mg.rec("m", abs(diff - M.occ), "occlusion threshold")
            if diff > M.occ:
                out.status = 6
                tags.add("ref_occlusion")
                break
            mg.rec("pixel", min(abs(u - (M.cols - 1)), abs(v - (M.rows - 1))), "bilinear footprint")
            if u >= M.cols - 1 or v >= M.rows - 1:   # the footprint leaves the image: the reference reads out of bounds there
                out.status = 1
                tags.add("ref_footprint_exit")
                break
            if v > M.rows - 2 or u > M.cols - 2:
                tags.add("ref_footprint")
            uv.append((u, v)), pl.append(Li), Rl.append(Rm), Ib.append(bilinear(fr["intensity"], u, v, mg))
        if out.status:
            return out
        mean = sum(Ib) / m
        cen = [x - mean for x in Ib]
        sigma = mp.sqrt(sum(c * c for c in cen))
        assert sigma > 0, "constant patch: not a zoo case"
        out.kappa = float(mp.sqrt(sum(x * x for x in Ib)) / sigma)
        psi = [c / sigma for c in cen]
        psi_a = [_m(v) for v in ft["psi"]]
        e = [x - y for x, y in zip(psi, psi_a)]
        e2 = sum(x * x for x in e)
        ncc = (2 - e2) / 2
        mg.rec("1", abs(ncc - _m(cfg["max_error"])), "max_error")
        if ncc < _m(cfg["max_error"]):
            out.status = 7
            tags.add("ref_maxerr")
            return out
        out.status = 8
        out.center = (float(uv[m // 2][0]), float(uv[m // 2][1]))
        Db, Da = [], []
        for i in range(m):
            u, v = uv[i]
            gx, gy = bilinear(fr["dx"], u, v), bilinear(fr["dy"], u, v)
            p = pl[i]
            rxy2 = p[0] * p[0] + p[1] * p[1]
            rxy = mp.sqrt(rxy2)
            L = rxy - M.bo
            R2 = L * L + p[2] * p[2]
            den = (L + M.bo) * R2
            P = [[-M.fx * p[1] / rxy2, M.fx * p[0] / rxy2, mpf(0)], [-M.fy * p[0] * p[2] / den, -M.fy * p[1] * p[2] / den, M.fy * L / R2]]
            g = [gx * P[0][k] + gy * P[1][k] for k in range(3)]
            a = [_m(x) for x in ft["Le_ps"][i]]
            p_a = [x + y for x, y in zip(_mv(M.TBL_R, a), M.TBL_t)]
            p_b = [x + y for x, y in zip(_mv(dBe[0], p_a), dBe[1])]
            Rk = _mm(_tr(Rl[i]), _tr(M.TBL_R))
            w = [sum(g[a_] * Rk[a_][k] for a_ in range(3)) for k in range(3)]
            # w^T Hat(p): (w1 p_z - w2 p_y, w2 p_x - w0 p_z, w0 p_y - w1 p_x)
            Db.append([w[1] * p_b[2] - w[2] * p_b[1], w[2] * p_b[0] - w[0] * p_b[2], w[0] * p_b[1] - w[1] * p_b[0], -w[0], -w[1], -w[2]])
            if binary:
                wa = [sum(w[a_] * dBe[0][a_][k] for a_ in range(3)) for k in range(3)]
                Da.append([-(wa[1] * p_a[2] - wa[2] * p_a[1]), -(wa[2] * p_a[0] - wa[0] * p_a[2]), -(wa[0] * p_a[1] - wa[1] * p_a[0]),
                           wa[0], wa[1], wa[2]])
        wh = mp.sqrt(e2) / _m(cfg["sigma"])
        out.whitened = float(wh)
        sw = mpf(1)
        if cfg["use_robust_cost_function"]:
            c = _m(cfg["robust_cost_function_parameter"])
            if cfg["robust_cost_function"] == 0:
                mg.rec("1", abs(wh - c), "Huber threshold")
                tags.add("ref_huber_below" if wh <= c else "ref_huber_above")
                sw = mpf(1) if wh <= c else mp.sqrt(c / wh)
            else:
                tags.add("ref_cauchy")
                sw = c * c / (c * c + wh * wh)
        wgt = sw / _m(cfg["sigma"])

        def jpsi(D):
            J = [[None] * 6 for _ in range(m)]
            scale = []
            for k in range(6):
                cm = sum(D[i][k] for i in range(m)) / m
                dc = [D[i][k] - cm for i in range(m)]
                pd = sum(psi[i] * dc[i] for i in range(m))
                for i in range(m):
                    J[i][k] = (dc[i] - psi[i] * pd) / sigma * wgt
                scale.append(float(max(abs(D[i][k]) for i in range(m)) / sigma * wgt))
            return J, scale

        Jb, sb = jpsi(Db)
        out.Jb = np.array([[_dd(x) for x in r] for r in Jb])        # (m, 6, 2)
        out.J_scale = np.array(sb)
        if binary:
            Ja, sa = jpsi(Da)
            out.Ja = np.array([[_dd(x) for x in r] for r in Ja])
            out.Ja_scale = np.array(sa)
        out.e = np.array([_dd(x * wgt) for x in e])                   # (m, 2)
        out.e_scale = float(max(max(abs(x) for x in psi), max(abs(x) for x in psi_a)) * wgt)
        return out


# ------------------------------------------------------------------------------------------------------------------------
# builder
# ------------------------------------------------------------------------------------------------------------------------
class Scene(SimpleNamespace):
    """name, cfg, inputs (raw, desk, unique_ns, T_Le_Lt), features, designed (tag per feature), expect ({index: (status, exception)}
    for the designed tie), pose (R_b, t_b, R_a | None, t_a | None), VSVt | None, binary, subsets (index lists: the factor sizes)"""


def frame_images(P):
    return {k: P.image(k) for k in ("yaw", "proj_idx", "mask", "range", "intensity", "dx", "dy", "idx")}


def frame_view(images, inputs):
    _, desk, ns, T = inputs
    fr = dict(images)
    fr["points"] = desk
    fr["pose_ns"] = np.asarray(ns, np.uint32)
    fr["pose_T"] = np.asarray(T, np.float64).reshape(-1, 12)
    return fr


def _copy(ft, **over):
    f = dict(ft)
    f["Le_ps"], f["psi"], f["intensities"] = np.array(ft["Le_ps"], float), np.array(ft["psi"], float), np.array(ft["intensities"], float)
    f.update(over)
    return f


def _xyz(desk, j):
    return np.array([desk["x"][j], desk["y"][j], desk["z"][j]], np.float64)


def feature_at(cfg, images, desk, base, u0, v0):
    """base re-centred on pixel (u0, v0) of the frame: Le_ps = the deskewed points of the patch pixels, psi = getPsi of the image.
    None when a patch pixel holds no point."""
    offs = np.asarray(cfg["patch_offsets"]).reshape(-1, 2)
    js = [int(images["idx"][v0 + dv, u0 + du]) if 0 <= v0 + dv < cfg["rows"] and 0 <= u0 + du < cfg["cols"] else -1 for du, dv in offs]
    if min(js) < 0:
        return None
    I = np.array([float(images["intensity"][v0 + dv, u0 + du]) for du, dv in offs])
    c = I - I.mean()
    s = np.linalg.norm(c)
    if s == 0:
        return None
    return _copy(base, Le_ps=np.stack([_xyz(desk, j) for j in js]), psi=c / s, intensities=I, center=np.array([float(u0), float(v0)]),
                 mean_intensity=float(I.mean()), sigma_intensity=float(s))


def _rot_z(P, a):
    c, s = math.cos(a), math.sin(a)
    return np.stack([c * P[:, 0] - s * P[:, 1], s * P[:, 0] + c * P[:, 1], P[:, 2]], 1)


def _lift(P, bo, d):
    """every point's beam elevation raised by d (rad) at constant beam range"""
    rxy = np.hypot(P[:, 0], P[:, 1])
    L = rxy - bo
    R = np.hypot(L, P[:, 2])
    th = np.arcsin(P[:, 2] / R) + d
    k = (R * np.cos(th) + bo) / rxy
    return np.stack([P[:, 0] * k, P[:, 1] * k, R * np.sin(th)], 1)


def _fproject(cfg, p, yaw):
    from oracle import numpy_photo as npo

    try:
        return npo.project(cfg, np.asarray(p, float), yaw)
    except ValueError:
        return False, -1.0, -1.0


_ZOO = {}


def build():
    """-> list of Scene.  Deterministic; asserts nothing about outcomes (reference() and the tests do)."""
    if "scenes" in _ZOO:
        return _ZOO["scenes"]
    from mimosa_amd import synth, synth_photo as sp
    from oracle import numpy_photo as npo, photo_ref

    scenes = []
    I3, z3 = np.eye(3), np.zeros(3)
    cfg5 = sp.photo_config(rows=ROWS, cols=COLS, patch=5)
    cfg8 = sp.photo_config(rows=ROWS, cols=COLS, patch=8)
    fr5 = [sp.make_frame(cfg5, k, seed=SEED) for k in range(2)]
    inputs = [(f["raw"], f["deskewed"], f["unique_ns"], f["T_Le_Lt"]) for f in fr5]
    bo = npo.derived(cfg5)[3]

    def oracle_features(cfg, n, unary):
        P = photo_ref.Photo(cfg)
        P.preprocess(*inputs[0])
        if unary:
            P.detect(n, fr5[0]["R_W_Be"], fr5[0]["t_W_Be"], sp.BIAS_DIRECTIONS)
        else:
            P.detect(n, I3, z3, np.eye(3))
        return P, P.features()

    # ---- identity motion, binary, frame 0: the statuses ----
    # At identity motion an unedited deskewed point projects ONTO the tables (phi equals a yaw entry, u and v are integers or sit at
    # x.5): every such decision would be a tie.  Every patch is therefore turned by JIG_U columns and lowered by JIG_V rows first.
    fx = npo.derived(cfg5)[0]
    alt = np.asarray(cfg5["beam_altitude_angles"], np.float64)
    pitch = math.radians(abs(alt[0] - alt[-1]) / (ROWS - 1))

    def jig(P):
        P = np.asarray(P, float).reshape(-1, 3)
        return _lift(_rot_z(P, JIG_U / fx), bo, -JIG_V * pitch)

    P0, base_raw = oracle_features(cfg5, 12, unary=False)
    base = [_copy(f, Le_ps=jig(f["Le_ps"])) for f in base_raw]
    im0 = frame_images(P0)
    desk0 = inputs[0][1]
    yaw0, pj0, mask0, idx0 = im0["yaw"], im0["proj_idx"], im0["mask"], im0["idx"]
    fv0 = frame_view(im0, inputs[0])
    feats, tags, expect = [], [], {}

    def add(ft, tag):
        feats.append(ft), tags.append(tag)
        return len(feats) - 1

    def fpu(p):
        """fp64 projectUndistorted on frame 0 -> (ok, u, v) of the second projection"""
        try:
            ok, _, q, _ = npo.project_undistorted(cfg5, fv0, np.asarray(p, float))
        except (ValueError, KeyError):
            return False, -1.0, -1.0
        return (True, q[0], q[1]) if ok else (False, -1.0, -1.0)

    def clear(x):
        return abs(x - round(x)) < 0.4999 and abs(x - round(x)) > 1e-4       # neither a rounding nor a floor tie

    def landed(ft, empty_ok=(), need=True):
        """per patch point (first-projection pixel, second-projection pixel), or None when a point fails, sits near a tie, or on a
        pixel the mask rejects or (first projection) without a candidate"""
        px = []
        for p in ft["Le_ps"]:
            ok, pu, pv = _fproject(cfg5, p, yaw0)
            if not ok or not clear(pu) or not clear(pv):
                return None
            a = (int(npo.round_half_away(pu)), int(npo.round_half_away(pv)))
            if pj0[a[1], a[0], 0] == 0 and len(px) not in empty_ok:
                return None
            ok, qu, qv = fpu(p)
            if not ok or not clear(qu) or not clear(qv):
                return None
            b = (int(npo.round_half_away(qu)), int(npo.round_half_away(qv)))
            if need and not mask0[b[1], b[0]]:
                return None
            px.append((a, b))
        return px

    order = sorted(range(len(base)), key=lambda i: base[i]["sigma_intensity"])
    add(_copy(base[order[0]]), "valid_low_contrast")
    for i in order[len(order) // 2:len(order) // 2 + 2] + [order[-1]]:
        add(_copy(base[i]), "valid")
    b0, b1, b2 = base[order[-1]], base[order[-2]], base[order[1]]
    norms = lambda f: np.linalg.norm(f["Le_ps"], axis=1)  # noqa: E731
    add(_copy(b0, Le_ps=b0["Le_ps"] * (31.0 / norms(b0).min())), "range_far")
    add(_copy(b0, Le_ps=b0["Le_ps"] * (0.3 / norms(b0).max())), "range_near")
    for k, tag in ((0, "range_at_0"), (12, "range_at_mid"), (24, "range_at_last")):
        Q = b1["Le_ps"].copy()
        Q[k] *= 31.0 / np.linalg.norm(Q[k])
        add(_copy(b1, Le_ps=Q), tag)
    r1 = np.linalg.norm(b1["Le_ps"][12])
    add(_copy(b1, Le_ps=b1["Le_ps"] * (1 - 0.27 / r1)), "occlusion")
    add(_copy(b1, Le_ps=b1["Le_ps"] * (1 - 0.12 / r1)), "occlusion_pass")
    phi0 = math.atan2(b0["Le_ps"][0][1], b0["Le_ps"][0][0])
    add(_copy(b0, Le_ps=_rot_z(b0["Le_ps"], (3.3 - COLS / 2) / fx - phi0)), "seam_low")             # point 0 at u = 3.3 (< 5)
    add(_copy(b0, Le_ps=_rot_z(b0["Le_ps"], (COLS - 3.3 - COLS / 2) / fx - phi0)), "seam_high")     # point 0 at u = cols - 3.3
    # the second projection failing where the first passed: early columns are undistorted by about three columns, so a point
    # whose first projection clears the seam bound by less than that can lose it in the second
    for u_t in (5.3, 5.8, 6.3, 6.8, 7.3, 7.8):
        Q = _rot_z(b0["Le_ps"], (u_t - COLS / 2) / fx - phi0)
        ok1, pu, pv = _fproject(cfg5, Q[0], yaw0)
        if ok1 and pj0[:, int(npo.round_half_away(pu)), 0].any() and not fpu(Q[0])[0]:
            add(_copy(b0, Le_ps=Q), "second_project_false")
            break
    c = b0["Le_ps"][0]
    th0 = math.asin(c[2] / math.hypot(math.hypot(c[0], c[1]) - bo, c[2]))
    c = b0["Le_ps"][24]
    th24 = math.asin(c[2] / math.hypot(math.hypot(c[0], c[1]) - bo, c[2]))
    add(_copy(b0, Le_ps=_lift(b0["Le_ps"], bo, math.radians(alt[0] + 0.7) - th0)), "theta_above")   # point 0 above the first beam
    lowered = _lift(b0["Le_ps"], bo, math.radians(alt[-1] - 0.7) - th24)
    add(_copy(b0, Le_ps=lowered[::-1].copy(), psi=b0["psi"][::-1].copy()), "theta_below")           # point 0 below the last beam
    Q = b2["Le_ps"].copy()
    Q[0] = [-np.linalg.norm(Q[0]), 0.0, 0.0]
    expect[add(_copy(b2, Le_ps=Q), "throw_first")] = (1, "project")
    Q = b2["Le_ps"].copy()
    Q[3] *= 31.0 / np.linalg.norm(Q[3])
    Q[7] = [-np.linalg.norm(Q[7]), 0.0, 0.0]
    expect[add(_copy(b2, Le_ps=Q), "throw_after_fail")] = (2, None)
    # a point that projects (twice) onto a pixel inside the margin that the eroded mask rejects
    mg_ = cfg5["margin_size"]
    vv, uu = np.nonzero((mask0 == 0) & (idx0 >= 0))
    masked = None
    for v_, u_ in zip(vv, uu):
        if mg_ + 2 <= v_ < ROWS - mg_ - 2 and 20 <= u_ < COLS - 20:
            p = jig(_xyz(desk0, int(idx0[v_, u_])))[0]
            ok, pu, pv = _fproject(cfg5, p, yaw0)
            ok2, qu, qv = fpu(p)
            if ok and ok2 and clear(pu) and clear(pv) and clear(qu) and clear(qv) and not mask0[int(npo.round_half_away(qv)), int(npo.round_half_away(qu))] \
                    and abs(float(im0["range"][int(npo.round_half_away(qv)), int(npo.round_half_away(qu))]) - np.linalg.norm(p)) < 0.1:
                masked = p
                break
    assert masked is not None
    Q = b2["Le_ps"].copy()
    Q[0] = masked
    add(_copy(b2, Le_ps=Q), "mask")
    Q = b2["Le_ps"].copy()
    Q[3] *= 31.0 / np.linalg.norm(Q[3])
    Q[7] = masked
    add(_copy(b2, Le_ps=Q), "first_fail_range")
    Q = b2["Le_ps"].copy()
    Q[3] = masked
    Q[7] *= 31.0 / np.linalg.norm(Q[7])
    add(_copy(b2, Le_ps=Q), "first_fail_mask")
    add(_copy(b0, psi=-b0["psi"]), "maxerr_negated")
    add(_copy(b0, psi=b0["psi"][::-1].copy()), "maxerr_permuted")

    # re-centred patches: margin on both sides, duplicates, the empty pixel
    def at(u_, v_):
        ft = feature_at(cfg5, im0, desk0, b0, u_, v_)
        return None if ft is None else _copy(ft, Le_ps=jig(ft["Le_ps"]))

    def first_at(pred, vs, us):
        for v_ in vs:
            for u_ in us:
                ft = at(u_, v_)
                if ft is not None and pred(ft):
                    return ft
        raise AssertionError("no pixel for a designed case")

    us = range(40, COLS - 40, 7)

    def margin_case(fails):
        def pred(ft):
            px = landed(ft, need=False)
            return px is not None and all(mask0[b[1], b[0]] for _, b in px) and (px[0][1][1] < mg_) == fails and all(b[1] >= mg_ for _, b in px[5:])
        return pred

    add(first_at(margin_case(True), [mg_ + 1], us), "margin")          # point 0 (top row of the patch) in row margin - 1
    add(first_at(margin_case(False), [mg_ + 2], us), "margin_pass")    # ... in row margin

    def has_dup(ft):
        px = landed(ft)
        return px is not None and any(pj0[a[1], a[0], 0] > 1 for a, _ in px)

    vs = range(mg_ + 3, ROWS - mg_ - 3)
    add(first_at(has_dup, vs, us), "dup_vote")
    add(first_at(has_dup, reversed(vs), reversed(us)), "dup_vote")
    # two candidates at equal f32 distance: the point midway between the two deskewed points of a two-candidate pixel
    done = False
    for v_ in vs:
        for u_ in range(40, COLS - 40):
            if pj0[v_, u_, 0] != 2 or done:
                continue
            j1, j2 = int(pj0[v_, u_, 1]), int(pj0[v_, u_, 2])
            if desk0["t"][j1] == desk0["t"][j2]:
                continue
            mid = (_xyz(desk0, j1) + _xyz(desk0, j2)) / 2
            ok, pu, pv = _fproject(cfg5, mid, yaw0)
            ft = at(u_, v_)
            if not ok or ft is None or int(npo.round_half_away(pu)) != u_ or int(npo.round_half_away(pv)) != v_:
                continue
            ft["Le_ps"][12] = mid
            d = [np.float32(np.sum((mid - _xyz(desk0, j)) ** 2)) for j in (j1, j2)]
            if d[0] != d[1] or landed(ft) is None:
                continue
            add(ft, "dup_tie")
            done = True
    assert done, "no pixel for the duplicate tie"
    # the empty pixel: the turn by JIG_U takes a point from its own pixel's projection into the next one, which may hold none
    def hits_empty(ft):
        px = landed(ft, empty_ok=range(25))
        return px is not None and any(pj0[a[1], a[0], 0] == 0 and (pj0[:, a[0], 0] > 0).any() for a, _ in px)

    add(first_at(hits_empty, vs, us), "empty_search")
    scenes.append(Scene(name="identity5", cfg=cfg5, inputs=inputs[0], features=feats, designed=tags, expect=expect, pose=(I3, z3, I3, z3),
                        VSVt=None, binary=True, subsets=[]))

    # ---- margin_size 1: a point between the last two beams is sampled (its footprint is rows - 2, rows - 1) ----
    def in_last_gap(ft):
        px = landed(ft)
        if px is None or any(b[1] > ROWS - 2 for _, b in px):
            return False
        return any(fpu(p)[2] > ROWS - 2 for p in ft["Le_ps"])

    scenes.append(Scene(name="footprint5", cfg=dict(cfg5, margin_size=1), inputs=inputs[0], features=[first_at(in_last_gap, [ROWS - 4], us), _copy(b0)],
                        designed=["footprint", "valid"], expect={}, pose=(I3, z3, I3, z3), VSVt=None, binary=True, subsets=[]))

    # ---- the wholly empty column: every point that projects into the column of point 0 of a base feature leaves the range gate ----
    ft = b1
    ok, pu, pv = _fproject(cfg5, ft["Le_ps"][0], yaw0)
    col = int(npo.round_half_away(pu))
    drop = np.unique(np.concatenate([pj0[r, col, 1:1 + pj0[r, col, 0]] for r in range(ROWS)]).astype(np.int64))
    far = max(base, key=lambda f: min(abs(f["center"][0] - col), COLS - abs(f["center"][0] - col)))
    desk_e = desk0.copy()
    desk_e["range"][drop] = 0.0
    scenes.append(Scene(name="empty_column5", cfg=cfg5, inputs=(inputs[0][0], desk_e, inputs[0][2], inputs[0][3]),
                        features=[_copy(ft), _copy(far)], designed=["empty_column", "valid"], expect={}, pose=(I3, z3, I3, z3), VSVt=None,
                        binary=True, subsets=[]))

    # ---- pose table lacking a run of timestamps ----
    ns, T = np.asarray(inputs[0][2]), np.asarray(inputs[0][3]).reshape(-1, 12)
    keep = np.ones(len(ns), bool)
    keep[len(ns) // 3:2 * len(ns) // 3] = False
    keep[::37] = False
    scenes.append(Scene(name="pose_missing5", cfg=cfg5, inputs=(inputs[0][0], desk0, ns[keep], T[keep]), features=[_copy(f) for f in base],
                        designed=["pose_missing"] * len(base), expect={}, pose=(I3, z3, I3, z3), VSVt=None, binary=True, subsets=[]))

    # ---- 8 x 8 at identity ----
    _, base8 = oracle_features(cfg8, 8, unary=False)
    base8 = [_copy(f, Le_ps=jig(f["Le_ps"])) for f in base8]
    o8 = sorted(range(len(base8)), key=lambda i: base8[i]["sigma_intensity"])
    f8 = [_copy(base8[o8[0]]), _copy(base8[o8[-1]])]
    t8 = ["valid_low_contrast", "valid"]
    Q = base8[o8[-1]]["Le_ps"].copy()
    Q[63] *= 31.0 / np.linalg.norm(Q[63])
    f8.append(_copy(base8[o8[-1]], Le_ps=Q)), t8.append("range_at_last")
    f8.append(_copy(base8[o8[1]], psi=-base8[o8[1]]["psi"])), t8.append("maxerr_negated")
    scenes.append(Scene(name="identity8", cfg=cfg8, inputs=inputs[0], features=f8, designed=t8, expect={}, pose=(I3, z3, I3, z3), VSVt=None,
                        binary=True, subsets=[]))

    # ---- frame 1 at its true pose and a small step: the rows ----
    Rb = fr5[1]["R_W_Be"] @ synth.so3_exp(np.array([0.001, 0.002, -0.002]))
    tb = fr5[1]["t_W_Be"] + np.array([0.01, 0.015, -0.005])
    sizes = [[], [0], [0, 1, 2], [0, 1, 2, 3], [0, 1, 2, 3, 4]]
    nb = [_copy(f) for f in base[:8]]
    scenes.append(Scene(name="rows5_binary", cfg=cfg5, inputs=inputs[1], features=nb, designed=["valid"] * len(nb), expect={},
                        pose=(Rb, tb, fr5[0]["R_W_Be"], fr5[0]["t_W_Be"]), VSVt=None, binary=True, subsets=sizes))
    for name, over in (("rows5_huber", dict(use_robust_cost_function=1, robust_cost_function=0, robust_cost_function_parameter=1.345, error_scale=2.0)),
                       ("rows5_cauchy", dict(use_robust_cost_function=1, robust_cost_function=1, robust_cost_function_parameter=0.8, error_scale=2.0))):
        scenes.append(Scene(name=name, cfg=dict(cfg5, **over), inputs=inputs[1], features=nb[:6], designed=["valid"] * 6, expect={},
                            pose=(Rb, tb, fr5[0]["R_W_Be"], fr5[0]["t_W_Be"]), VSVt=None, binary=True, subsets=[]))
    _, base_u = oracle_features(cfg5, 10, unary=True)
    V = synth.so3_exp(np.array([0.3, -0.2, 0.5]))
    V6 = np.block([[V, np.zeros((3, 3))], [np.zeros((3, 3)), V.T]])
    VSVt = V6 @ np.diag([1.0, 0, 1, 0, 1, 1]) @ V6.T
    Ru = fr5[1]["R_W_Be"] @ synth.so3_exp(np.array([0.002, -0.001, 0.003]))
    tu = fr5[1]["t_W_Be"] + np.array([0.02, -0.01, 0.01])
    fu = [_copy(f) for f in base_u]
    scenes.append(Scene(name="rows5_unary", cfg=cfg5, inputs=inputs[1], features=fu, designed=["valid"] * len(fu), expect={}, pose=(Ru, tu, None, None),
                        VSVt=None, binary=False, subsets=sizes))
    scenes.append(Scene(name="rows5_unary_vsvt", cfg=cfg5, inputs=inputs[1], features=fu, designed=["valid"] * len(fu), expect={}, pose=(Ru, tu, None, None),
                        VSVt=VSVt, binary=False, subsets=[]))
    _, base8u = oracle_features(cfg8, 5, unary=True)
    f8u = [_copy(f) for f in base8u]
    scenes.append(Scene(name="rows8_unary", cfg=cfg8, inputs=inputs[1], features=f8u, designed=["valid"] * len(f8u), expect={}, pose=(Ru, tu, None, None),
                        VSVt=None, binary=False, subsets=[]))
    assert tuple(sc.name for sc in scenes) == SCENES
    _ZOO["scenes"] = scenes
    return scenes


_REF = {}


def reference(sc, images):
    """-> list of per-feature references of scene sc on the given downloaded images (cached per scene and image bytes)"""
    key = (sc.name, hash(images["yaw"].tobytes()), hash(images["proj_idx"].tobytes()))
    if key not in _REF:
        M = Model(sc.cfg)
        fr = frame_view(images, sc.inputs)
        _REF[key] = [feature_reference(M, fr, ft, sc.pose) for ft in sc.features]
    return _REF[key]


def expected(sc, refs):
    """(status, exception) per feature: the reference's, except the designed tie"""
    return [sc.expect.get(i, (r.status, r.exception)) for i, r in enumerate(refs)]


def zoo_margins(sc, refs):
    mg = Margins()
    for i, r in enumerate(refs):
        if i in sc.expect:                       # the designed tie
            continue
        mg.merge(r.margins, f"{sc.name}[{i}]")
    return mg


def row_ratios(refs, rows, K=None, label=""):
    """Every row of every Valid feature against the reference: -> worst |row - ref| / (2^-53 kappa scale); asserts <= K if given.
    rows: (n, 64, 8) = [e, J_b (6), flag] as state() returns them."""
    worst = 0.0
    for i, r in enumerate(refs):
        if r.status != 8:
            assert not np.any(rows[i] != 0), (label, i, "rows of a feature that is not Valid")
            continue
        assert np.all(rows[i, :r.m, 7] == 1.0) and not np.any(rows[i, r.m:] != 0), (label, i)
        unit = U * r.kappa
        err_e = np.abs((rows[i, :r.m, 0] - r.e[:, 0]) - r.e[:, 1]) / (unit * np.maximum(np.abs(r.e[:, 0]), r.e_scale))
        err_J = np.abs((rows[i, :r.m, 1:7] - r.Jb[:, :, 0]) - r.Jb[:, :, 1]) / (unit * np.maximum(np.abs(r.Jb[:, :, 0]), r.J_scale[None, :]))
        w = float(max(err_e.max(), err_J.max()))
        if K is not None:
            assert w <= K, (label, i, "row", int(np.argmax(np.maximum(err_e, err_J.max(1)))), w, K)
        worst = max(worst, w)
    return worst


def sums_from_rows(rows, statuses):
    """H_bb, b_b, f as math.fsum sums of reported rows, and the sums of the absolute terms"""
    v = [i for i, s in enumerate(statuses) if s == 8]
    R = rows[v].reshape(-1, 8)
    R = R[R[:, 7] == 1.0]
    H, Ha = np.zeros((6, 6)), np.zeros((6, 6))
    b, ba = np.zeros(6), np.zeros(6)
    for a in range(6):
        for c in range(6):
            t = R[:, 1 + a] * R[:, 1 + c]       # each product rounded once: inside the bound of n_rows * 2^-53 * sum |terms|
            H[a, c], Ha[a, c] = math.fsum(t), math.fsum(np.abs(t))
        t = R[:, 1 + a] * R[:, 0]
        b[a], ba[a] = math.fsum(t), math.fsum(np.abs(t))
    t = R[:, 0] * R[:, 0]
    return H, b, math.fsum(t), Ha, ba, math.fsum(np.abs(t)), len(R)


# ------------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU and the GPU module
# ------------------------------------------------------------------------------------------------------------------------
CENTER_TOL = 64 * U * COLS   # sub-pixel centre: a few ulps of phi (|phi| <= pi) amplified by 1 / (yl - yr) = cols / 2 pi, and of v likewise


def subset(sc, idx):
    return Scene(**{**sc.__dict__, "name": f"{sc.name}{list(idx)}", "features": [sc.features[i] for i in idx],
                    "designed": [sc.designed[i] for i in idx], "expect": {k: sc.expect[i] for k, i in enumerate(idx) if i in sc.expect}, "subsets": []})


def run(P, sc, factory=None):
    """preprocess, set_features, make_factor, linearize on a Photo-like object -> (images, factor, result, state)"""
    P.preprocess(*sc.inputs)
    images = frame_images(P)
    P.set_features(sc.features)
    F = P.make_factor(sc.VSVt, sc.binary)
    res = F.linearize(*sc.pose)
    return images, F, res, F.state()


def check_discrete(sc, refs, res, state, label=""):
    """statuses, the centres' pixel, n_exceptions and status_hist: exact"""
    exp = expected(sc, refs)
    st, ce, _ = state
    assert st.tolist() == [e[0] for e in exp], (label, st.tolist(), [e[0] for e in exp], sc.designed)
    assert int(res["n_exceptions"]) == sum(1 for e in exp if e[1] is not None), (label, res["n_exceptions"], exp)
    assert np.asarray(res["status_hist"]).tolist() == np.bincount([e[0] for e in exp], minlength=9).tolist(), label
    for i, r in enumerate(refs):
        if r.status == 8:
            assert [math.floor(c + 0.5) for c in ce[i]] == [math.floor(c + 0.5) for c in r.center], (label, i, ce[i], r.center)
            assert max(abs(ce[i][0] - r.center[0]), abs(ce[i][1] - r.center[1])) <= CENTER_TOL, (label, i, ce[i], r.center)


def check_sums(sc, refs, res, state, K, label=""):
    """H_bb, b_b, f against math.fsum sums of the rows the result's own state reports (n_rows * 2^-53 * sum |terms|); the binary
    blocks against sums of the reference's rows with the row bound propagated; the unary V H V, b and localizabilities"""
    st, _, rows = state
    H, b, f, Ha, ba, fa, n = sums_from_rows(rows, st)
    tolH, tolb, tolf = n * U * Ha, n * U * ba, n * U * fa
    Hr, br = np.asarray(res["H_bb"], float).reshape(6, 6), np.asarray(res["b_b"], float)
    assert abs(res["f"] - f) <= tolf, (label, "f", res["f"], f, tolf)
    if sc.binary:
        assert np.all(np.abs(Hr - H) <= tolH), (label, "H_bb", float(np.abs(Hr - H).max()))
        assert np.all(np.abs(br - b) <= tolb), (label, "b_b", np.abs(br - b).tolist(), tolb.tolist())
        v = [r for r in refs if r.status == 8]
        if not v:
            for k in ("H_ba", "H_aa", "b_a"):
                assert not np.any(np.asarray(res[k])), (label, k)
            return
        Jb, Ja, e = (np.concatenate([r.Jb[:, :, 0] for r in v]), np.concatenate([r.Ja[:, :, 0] for r in v]), np.concatenate([r.e[:, 0] for r in v]))
        dJb = np.concatenate([K * U * r.kappa * np.maximum(np.abs(r.Jb[:, :, 0]), r.J_scale[None]) for r in v])
        dJa = np.concatenate([K * U * r.kappa * np.maximum(np.abs(r.Ja[:, :, 0]), r.Ja_scale[None]) for r in v])
        de = np.concatenate([K * U * r.kappa * np.maximum(np.abs(r.e[:, 0]), r.e_scale) for r in v])
        m = len(e)

        def hold(name, got, A, dA, B, dB):
            got = np.asarray(got, float)
            for a in range(A.shape[1]):
                for c in range(B.shape[1]):
                    t = A[:, a] * B[:, c]
                    tol = float(np.sum(np.abs(A[:, a]) * dB[:, c] + dA[:, a] * np.abs(B[:, c]) + dA[:, a] * dB[:, c])) + (m + 2) * U * float(np.abs(t).sum())
                    g = got[a, c] if got.ndim == 2 else got[a]
                    assert abs(g - math.fsum(t)) <= tol, (label, name, a, c, g, math.fsum(t), tol)

        hold("H_ba", res["H_ba"], Jb, dJb, Ja, dJa)
        hold("H_aa", res["H_aa"], Ja, dJa, Ja, dJa)
        hold("b_a", res["b_a"], Ja, dJa, e[:, None], de[:, None])
        return
    V = np.eye(6) if sc.VSVt is None else np.asarray(sc.VSVt, float)
    aV = np.abs(V)
    want = V @ H @ V
    tol = aV @ tolH @ aV + 14 * U * (aV @ np.abs(H) @ aV)          # two products of length six: gamma_12, and the sums' own bound
    assert np.all(np.abs(Hr - want) <= tol), (label, "V H V", float(np.abs(Hr - want).max()), float(tol.max()))
    if n and np.all(np.isfinite(H)) and np.linalg.cond(H) < 1e9:     # b = V H V H^-1 b is arbitrary where H is singular (test_gpu_photo_fuzz)
        x = np.linalg.solve(H, b)
        cond = np.linalg.cond(H)
        relH, relb = np.linalg.norm(tolH) / np.linalg.norm(H), np.linalg.norm(tolb) / max(np.linalg.norm(b), 1e-300)
        tb = (64 * U + relH + relb) * cond * np.linalg.norm(want, 2) * np.linalg.norm(x)   # explicit inverse in fp64: c n u cond(H), n = 6
        assert np.linalg.norm(br - want @ x) <= tb, (label, "b_b", br.tolist(), (want @ x).tolist(), tb)
    if n and np.all(np.isfinite(Hr)):
        import degeneracy_zoo as DZ

        for name, blk in (("rot", Hr[:3, :3]), ("trans", Hr[3:, 3:])):
            DZ.check_block((blk + blk.T) / 2, res[f"loc_{name}_final"], res[f"eigvec_{name}"], f"{label} {name}")
