"""tracking_module::search_local_landmarks, restated sequentially: DESIGN.md 3.17's rules V1 - V7 with one landmark per iteration, as upstream's loop
over local_landmarks_ runs them. Python floats are IEEE doubles and every operation below is rounded on its own, which is what the kernel does
(the library is built with -ffp-contract=off). V2 comes from the oracle's reproject_to_image, logf from its detmath_eval, float narrowing from
sim3_ref.f32, the matcher stage from the oracle's projection_match_frame_and_landmarks. Nothing of the product is imported here."""
import math

import numpy as np

from sim3_ref import f32

SKIPPED, DEPTH, BOUNDS, RANGE, ANGLE, OBSERVABLE = range(6)
OUTCOME_NAMES = ("skipped", "V2 depth", "V2 bounds", "V3 range", "V4 angle", "observable")


def pose12(pose_cw):
    T = np.asarray(pose_cw, np.float64)
    return [float(v) for v in T[:3, :3].reshape(-1)] + [float(v) for v in T[:3, 3]]


def camera_centre(P):
    """-R^T t of P = [R | t] as 12 doubles, in camera_centre()'s operation order."""
    return [-((P[i] * P[9] + P[3 + i] * P[10]) + P[6 + i] * P[11]) for i in range(3)]


def depth_in_camera(P, X):
    return (P[6] * X[0] + P[7] * X[1]) + P[8] * X[2] + P[11]


def range_limits(dmin, dmax):
    """landmark::get_min_valid_distance / get_max_valid_distance: a double product returned as float."""
    return f32(0.7 * f32(dmin)), f32(1.3 * f32(dmax))


def predict_level(oracle, dmax, dist, num_levels, log_scale_factor):
    """V5: (int)ceilf(logf(dmax / (float)dist) / log_scale_factor) in float arithmetic, clamped."""
    ratio = f32(f32(dmax) / f32(dist))
    lg = float(oracle.detmath_eval(oracle.DETMATH_LOGF, [ratio])[0])
    q = f32(f32(lg) / f32(log_scale_factor))
    if math.isinf(q):   # (a ratio of 0 or inf: beyond either clamp)
        return 0 if q < 0 else num_levels - 1
    return min(max(int(math.ceil(q)), 0), num_levels - 1)


def gates(oracle, X, cc, dmin, dmax, nrm, num_levels, log_scale_factor):
    """V3 - V5 on a landmark that projects into the image: (outcome, level)."""
    dx, dy, dz = X[0] - cc[0], X[1] - cc[1], X[2] - cc[2]
    dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
    lo, hi = range_limits(dmin, dmax)
    if dist < lo or hi < dist:
        return RANGE, 0
    dot = (dx * nrm[0] + dy * nrm[1]) + dz * nrm[2]
    if dot < 0.5 * dist:
        return ANGLE, 0
    return OBSERVABLE, predict_level(oracle, dmax, dist, num_levels, log_scale_factor)


def can_observe(oracle, cam, gp, pose_cw, X, dmin, dmax, nrm, num_levels, log_scale_factor):
    """frame::can_observe(lm, 0.5, ...): (outcome, (u, v), x_right, level) with V6's values unless observable."""
    P = pose12(pose_cw)
    X = [float(v) for v in X]
    none = ((0.0, 0.0), -1.0, 0)
    if cam.model == 0 and depth_in_camera(P, X) <= 0.0:
        return (DEPTH,) + none
    ok, uv, xr = oracle.reproject_to_image(cam, gp, pose_cw, X)
    if not ok:
        return (BOUNDS,) + none
    out, lvl = gates(oracle, X, camera_centre(P), float(dmin), float(dmax), [float(v) for v in nrm], num_levels, log_scale_factor)
    if out != OBSERVABLE:
        return (out,) + none
    return OBSERVABLE, (float(uv[0]), float(uv[1])), float(xr), lvl


def search_local_landmarks(oracle, cam, gp, kps, desc, pose_cw, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc, scale_factors, log_scale_factor,
                           margin, lowe_ratio, stereo_x_right=None, occupied=None, lm_search=None):
    """The whole call: {"outcome", "observable", "reproj", "x_right", "level", "assigned", "num_observable", "num_matches"}."""
    m = len(lm_pos_w)
    num_levels = len(scale_factors)
    outcome = np.zeros(m, np.int32)
    reproj = np.zeros((m, 2), np.float64)
    x_right = np.full(m, -1.0, np.float32)
    level = np.zeros(m, np.int32)
    for l in range(m):
        if lm_search is not None and not lm_search[l]:   # V1
            outcome[l] = SKIPPED
            continue
        outcome[l], reproj[l], x_right[l], level[l] = can_observe(oracle, cam, gp, pose_cw, lm_pos_w[l], lm_dist_min_max[l][0], lm_dist_min_max[l][1],
                                                                  lm_normal[l], num_levels, log_scale_factor)
    observable = (outcome == OBSERVABLE).astype(np.uint8)
    assigned, num = np.full(m, -1, np.int32), 0
    if len(kps) and observable.any():   # V7 (upstream: `if (!found_proj_candidate) return;`)
        assigned, num = oracle.projection_match_frame_and_landmarks(gp, kps, desc, scale_factors, reproj.astype(np.float32), level, lm_desc, margin,
                                                                    lowe_ratio, frm_stereo_x_right=stereo_x_right, frm_occupied=occupied,
                                                                    lm_x_right=x_right if stereo_x_right is not None else None, lm_valid=observable)
    return {"outcome": outcome, "observable": observable, "reproj": reproj, "x_right": x_right, "level": level, "assigned": assigned,
            "num_observable": int(observable.sum()), "num_matches": int(num)}


def gates_vectorised(oracle, pose_cw, lm_pos_w, lm_dist_min_max, lm_normal, num_levels, log_scale_factor):
    """V3 - V5 for every landmark at once in numpy (no V1, no V2): (outcome in {RANGE, ANGLE, OBSERVABLE}, level). A second form of the same
    algebra: tests/test_observe_ref.py holds it to the sequential one."""
    P = pose12(pose_cw)
    cc = np.array(camera_centre(P))
    X = np.asarray(lm_pos_w, np.float64)
    nrm = np.asarray(lm_normal, np.float64)
    dmm = np.asarray(lm_dist_min_max, np.float32)
    dx, dy, dz = X[:, 0] - cc[0], X[:, 1] - cc[1], X[:, 2] - cc[2]
    dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
    lo = (0.7 * dmm[:, 0].astype(np.float64)).astype(np.float32).astype(np.float64)
    hi = (1.3 * dmm[:, 1].astype(np.float64)).astype(np.float32).astype(np.float64)
    out_of_range = (dist < lo) | (hi < dist)
    dot = (dx * nrm[:, 0] + dy * nrm[:, 1]) + dz * nrm[:, 2]
    oblique = dot < 0.5 * dist
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = dmm[:, 1] / dist.astype(np.float32)
        lg = oracle.detmath_eval(oracle.DETMATH_LOGF, ratio.astype(np.float64)).astype(np.float32)
        q = np.ceil(lg / np.float32(log_scale_factor))
    lvl = np.clip(np.nan_to_num(q, nan=0.0, posinf=num_levels, neginf=0.0), 0, num_levels - 1).astype(np.int32)
    outcome = np.where(out_of_range, RANGE, np.where(oblique, ANGLE, OBSERVABLE)).astype(np.int32)
    return outcome, np.where(outcome == OBSERVABLE, lvl, 0).astype(np.int32)
