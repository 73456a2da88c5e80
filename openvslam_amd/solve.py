"""solve/ and its neighbours on the MI355X, every one a batch call over packed problems (_pack): the Sim3, EPnP, homography / fundamental and
essential RANSACs, the Sim3 transform optimiser, the two-view triangulator and the monocular initialiser's pose recovery.

solve::sim3_solver (expected: src/openvslam/solve/sim3_solver.{h,cc}) on the MI355X: the RANSAC the loop detector runs on every loop
candidate between bow_tree::match_keyframes and projection::match_by_Sim3_transform. All candidates of a keyframe go to the device in ONE
call (ovs_sim3_solve_batch, csrc/sim3_solve.hip): two launches whatever their number. DESIGN.md 3.9 has the rules; the results are
bit-exact functions of (inputs, seed, position in the batch).

solve::pnp_solver (expected: src/openvslam/solve/pnp_solver.{h,cc}): the EPnP RANSAC the relocaliser runs on every candidate keyframe between
bow_tree::match_frame_and_keyframe and the pose optimiser. All candidates go to the device in ONE call (ovs_pnp_solve_batch,
csrc/pnp_solve.hip): two launches whatever their number. DESIGN.md 3.10 has the rules; bit-exact in the same sense.

optimize::transform_optimizer (expected: src/openvslam/optimize/transform_optimizer.{h,cc}): the Sim3 refinement the loop detector runs on
every candidate after projection::match_by_Sim3_transform. It lives here, beside the handle and packing code it shares with the solvers.
All candidates go to the device in ONE call and ONE launch (ovs_sim3opt_optimize_batch, csrc/sim3_opt.hip). DESIGN.md 3.11 has the rules;
the results are bit-exact functions of the inputs.

module::two_view_triangulator (expected: src/openvslam/module/two_view_triangulator.{h,cc}): the triangulation local mapping runs on every
pair robust::match_for_triangulation returns. All pairs of all neighbours of a new keyframe go to the device in ONE call and ONE launch
(ovs_triangulate_batch, csrc/triangulate.hip). DESIGN.md 3.12 has the rules; bit-exact in the same sense.

solve::homography_solver and solve::fundamental_solver (expected: src/openvslam/solve/{homography,fundamental}_solver.{h,cc}): the two RANSACs
initialize::perspective::initialize runs on two threads for every frame until the map exists. Both models of all problems go to the device in
ONE call (ovs_twoview_solve_batch, csrc/two_view_solve.hip): two launches, with upstream's choice between the models. DESIGN.md 3.13 has
the rules; bit-exact in the same sense.

initialize::perspective's reconstruct_with_H / reconstruct_with_F (expected: src/openvslam/initialize/{base,perspective}.{h,cc}): the pose
hypotheses of the chosen model, check_pose over every inlier match and find_most_plausible_pose. All problems go to the device in ONE call
(ovs_reconstruct_batch, csrc/two_view_reconstruct.hip): two launches. DESIGN.md 3.15 has the rules; bit-exact in the same sense.

solve::essential_solver (expected: src/openvslam/solve/essential_solver.{h,cc}): the bearing-vector eight-point RANSAC
robust::match_frame_and_keyframe runs after its brute-force match. All problems go to the device in ONE call (ovs_essential_solve_batch,
csrc/essential_solve.hip): two launches. DESIGN.md 3.16 has the rules; bit-exact in the same sense."""
import ctypes as C
import math

import numpy as np

from . import _lib

DEFAULT_SEED = 0x53696D33   # upstream draws from random_device; here a run is reproducible
_G = 0x9E3779B97F4A7C15
_MASK = (1 << 64) - 1


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def problem_seed(seed, p):
    """The seed under which problem p of a batch, solved ALONE (as problem 0), draws the samples it draws in the batch (rule 1)."""
    return (seed + _G * (p << 22)) & _MASK


def camera(model=0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, cols=0, rows=0):
    """ovs_camera for one side: model 0 (perspective: fx fy cx cy) or 1 (equirectangular: cols rows)."""
    return _lib.Camera(int(model), 0, float(fx), float(fy), float(cx), float(cy), 0.0, 0.0, int(cols), int(rows))


def _transform(pose_cw, pos_w):
    """rot_cw * pos_w + trans_cw, per point, in upstream's order of operations (Eigen: the row's products added left to right, then the translation)."""
    T = np.asarray(pose_cw, np.float64)
    P = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    out = np.empty_like(P)
    for r in range(3):
        out[:, r] = ((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3]
    return out


def problem_from_keyframes(pose_cw_1, pose_cw_2, pos_w_1, pos_w_2, octaves_1, octaves_2, level_sigma_sq_1, level_sigma_sq_2, cam_1, cam_2):
    """What sim3_solver's constructor collects for the matched landmark pairs (lm_1[i], lm_2[i]): common_pts_in_keyfrm_1_ / _2_ (each
    landmark in its own keyframe's camera) and chi_sq_x_sigma_sq_1_ / _2_ = 9.21 * level_sigma_sq[octave of the landmark's keypoint], narrowed
    to float. pose_cw_*: 4 x 4 (or 3 x 4) world -> camera; pos_w_*: (n, 3); octaves_*: (n,); level_sigma_sq_*: per level."""
    s1 = np.asarray(level_sigma_sq_1, np.float32)[np.asarray(octaves_1, np.int64)]
    s2 = np.asarray(level_sigma_sq_2, np.float32)[np.asarray(octaves_2, np.int64)]
    return dict(p1=_transform(pose_cw_1, pos_w_1), p2=_transform(pose_cw_2, pos_w_2), thr1=(9.21 * s1.astype(np.float64)).astype(np.float32),
                thr2=(9.21 * s2.astype(np.float64)).astype(np.float32), cam_1=cam_1, cam_2=cam_2)


class _ransac_handle:
    """A solver's device handle (ovs_sim3, ovs_pnp, ...: `_abi` is the prefix of its create / destroy / solve_batch) with its capacity."""
    _abi = None

    def __init__(self, max_problems, max_total_matches, device=0):
        self._L = _lib.lib()
        _lib.require_device()
        self.max_problems, self.max_total_matches = int(max_problems), int(max_total_matches)
        h = C.c_void_p()
        _lib.check(getattr(self._L, self._abi + "_create")(device, self.max_problems, self.max_total_matches, C.byref(h)), self._abi + "_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            getattr(self._L, self._abi + "_destroy")(h)


class _handle(_ransac_handle):
    """ovs_sim3 with its capacity."""
    _abi = "ovs_sim3"


class _pnp_handle(_ransac_handle):
    """ovs_pnp with its capacity."""
    _abi = "ovs_pnp"


def _pack(problems, arrays, count_key, error):
    """What every batch call stages: (P, offsets, T, packed). arrays: (key, dtype, width) of the per-match arrays in the ABI's order;
    count_key names the one whose rows are a problem's matches: offsets (int32, P + 1) are their running sum and T the total. packed: every
    array of all problems in one contiguous (T, width) array of its dtype; error is the ValueError's text when one has another length."""
    P = len(problems)
    width = {key: w for key, _, w in arrays}[count_key]
    offsets = np.zeros(P + 1, np.int32)
    offsets[1:] = np.cumsum([len(np.asarray(q[count_key]).reshape(-1, width)) for q in problems])
    T = int(offsets[-1])
    cat = lambda key, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(q[key], dt).reshape(-1, w) for q in problems]) if T else np.zeros((0, w), dt))
    packed = [cat(*a) for a in arrays]
    if any(len(a) != T for a in packed):
        raise ValueError(error)
    return P, offsets, T, packed


def _solve_batch(handle_type, problems, arrays, count_key, error, middle, suffix, with_scale, handle, device):
    """One solve_batch call of handle_type's ABI over `problems`. arrays, count_key, error: as _pack takes them; middle: the ABI's
    arguments between the arrays and the outputs; the returned dicts name the pose rot_<suffix>, trans_<suffix> (and scale_<suffix>)."""
    P, offsets, T, packed = _pack(problems, arrays, count_key, error)
    if P == 0:
        return []
    if handle is None:
        handle = handle_type(P, max(T, 1), device)
    valid, best_iter, num = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    rot, trans, flags = np.zeros((P, 3, 3)), np.zeros((P, 3)), np.zeros(max(T, 1), np.uint8)
    scale = [np.zeros(P)] if with_scale else []
    name = handle_type._abi + "_solve_batch"
    _lib.check(getattr(handle._L, name)(handle._h, P, _p(offsets), *map(_p, packed), *middle, _p(valid), _p(best_iter), _p(num), _p(rot), _p(trans), *map(_p, scale),
                                        _p(flags)), name)
    rot_key, trans_key, scale_key = "rot_" + suffix, "trans_" + suffix, "scale_" + suffix
    out = []
    for i in range(P):
        r = {"valid": bool(valid[i]), "best_iter": int(best_iter[i]), "num_inliers": int(num[i]), rot_key: rot[i].copy(), trans_key: trans[i].copy()}
        if with_scale:
            r[scale_key] = float(scale[0][i])
        r["inlier_flags"] = flags[offsets[i]:offsets[i + 1]].astype(bool)
        out.append(r)
    return out


_SIM3_ARRAYS = (("p1", np.float64, 3), ("p2", np.float64, 3), ("thr1", np.float32, 1), ("thr2", np.float32, 1))
_PNP_ARRAYS = (("bearings", np.float64, 3), ("pos_w", np.float64, 3), ("max_cos_error", np.float64, 1))


def solve_sim3_batch(problems, fix_scale, min_num_inliers=20, max_num_iter=200, seed=DEFAULT_SEED, handle=None, device=0):
    """find_via_ransac for every problem (dicts as problem_from_keyframes returns them) in one call: a list of dicts valid, best_iter,
    num_inliers, rot_12 (3 x 3), trans_12 (3), scale_12, inlier_flags (n, bool). `handle`: a _handle to reuse (the loop detector keeps one)."""
    cams_1 = (_lib.Camera * len(problems))(*[q["cam_1"] for q in problems])
    cams_2 = (_lib.Camera * len(problems))(*[q["cam_2"] for q in problems])
    return _solve_batch(_handle, problems, _SIM3_ARRAYS, "thr1", "p1, p2, thr1 and thr2 of a problem must have one entry per match",
                        [cams_1, cams_2, 1 if fix_scale else 0, int(min_num_inliers), int(max_num_iter), int(seed) & _MASK], "12", True, handle, device)


class _ransac_solver:
    """What the two solver classes share: the result of find_via_ransac and upstream's getters that both have."""
    _result = None

    def _get(self, key):
        if self._result is None:
            raise RuntimeError("find_via_ransac has not run")
        return self._result[key]

    def solution_is_valid(self):
        return self._result is not None and self._result["valid"]

    def get_inlier_flags(self):
        return self._get("inlier_flags")

    def get_best_iter(self):
        return self._get("best_iter")

    def get_num_inliers(self):
        return self._get("num_inliers")


class sim3_solver(_ransac_solver):
    """solve::sim3_solver over one problem: the constructor takes what upstream's collects from the two keyframes (see
    problem_from_keyframes), find_via_ransac runs the device RANSAC, the getters are upstream's."""

    def __init__(self, p1, p2, thr1, thr2, cam_1, cam_2, fix_scale, min_num_inliers=20, device=0):
        self._problem = dict(p1=p1, p2=p2, thr1=thr1, thr2=thr2, cam_1=cam_1, cam_2=cam_2)
        self._fix_scale, self._min_num_inliers, self._device = bool(fix_scale), int(min_num_inliers), device

    def find_via_ransac(self, max_num_iter, seed=DEFAULT_SEED):
        self._result = solve_sim3_batch([self._problem], self._fix_scale, self._min_num_inliers, max_num_iter, seed, device=self._device)[0]

    def get_best_rotation_12(self):
        return self._get("rot_12")

    def get_best_translation_12(self):
        return self._get("trans_12")

    def get_best_scale_12(self):
        return self._get("scale_12")


# ---- solve::pnp_solver
PNP_DEFAULT_SEED = 0x45506E50   # upstream draws from random_device; here a run is reproducible


def pnp_problem_seed(seed, p):
    """The seed under which problem p of a batch, solved ALONE (as problem 0), draws the samples it draws in the batch (3.10 rule 1)."""
    return (seed + _G * (p << 23)) & _MASK


def pnp_problem(bearings, octaves, pos_w, scale_factors):
    """What pnp_solver's constructor keeps for the matched (keypoint, landmark) pairs: the bearings, the landmarks in the world and
    max_cos_errors_ = cos(scale_factors[octave] * 1 degree) (math.cos: the C library's, as the C++ class calls it). bearings, pos_w: (n, 3);
    octaves: (n,); scale_factors: per level, floats."""
    sf = np.asarray(scale_factors, np.float32)
    deg = math.pi / 180.0
    return dict(bearings=np.ascontiguousarray(bearings, np.float64).reshape(-1, 3), pos_w=np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3),
                max_cos_error=np.array([math.cos(float(sf[int(o)]) * deg) for o in np.asarray(octaves).ravel()], np.float64))


def solve_pnp_batch(problems, min_num_inliers=10, max_num_iter=30, recompute=True, seed=PNP_DEFAULT_SEED, handle=None, device=0):
    """find_via_ransac for every problem (dicts as pnp_problem returns them) in one call: a list of dicts valid, best_iter, num_inliers,
    rot_cw (3 x 3), trans_cw (3), inlier_flags (n, bool). `handle`: a _pnp_handle to reuse (the relocaliser keeps one)."""
    return _solve_batch(_pnp_handle, problems, _PNP_ARRAYS, "max_cos_error", "bearings, pos_w and max_cos_error of a problem must have one entry per match",
                        [int(min_num_inliers), int(max_num_iter), 1 if recompute else 0, int(seed) & _MASK], "cw", False, handle, device)


class pnp_solver(_ransac_solver):
    """solve::pnp_solver over one problem: the constructor takes what upstream's does (the valid bearings, their keypoints' octaves, the
    landmarks and the scale factors), find_via_ransac runs the device RANSAC, the getters are upstream's."""

    def __init__(self, valid_bearings, valid_octaves, valid_landmarks, scale_factors, min_num_inliers=10, device=0):
        self._problem = pnp_problem(valid_bearings, valid_octaves, valid_landmarks, scale_factors)
        self._min_num_inliers, self._device = int(min_num_inliers), device

    def find_via_ransac(self, max_num_iter, recompute=True, seed=PNP_DEFAULT_SEED):
        self._result = solve_pnp_batch([self._problem], self._min_num_inliers, max_num_iter, recompute, seed, device=self._device)[0]

    def get_best_rotation(self):
        return self._get("rot_cw")

    def get_best_translation(self):
        return self._get("trans_cw")

    def get_best_cam_pose(self):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = self._get("rot_cw"), self._get("trans_cw")
        return T


# ---- optimize::transform_optimizer
def transform_problem_from_keyframes(pose_cw_1, pose_cw_2, pos_w_1, pos_w_2, keypts_1, keypts_2, octaves_1, octaves_2, inv_level_sigma_sq_1,
                                     inv_level_sigma_sq_2, cam_1, cam_2, rot_12, trans_12, scale_12):
    """What transform_optimizer collects for the matched landmark pairs (lm_1[i], lm_2[i]): each landmark in its own keyframe's camera (as
    problem_from_keyframes does), the two undistorted keypoints widened to double and inv_level_sigma_sq[octave] of each, with the initial
    Sim3_12. keypts_*: (n, 2) float32; the other arguments as problem_from_keyframes takes them."""
    w1 = np.asarray(inv_level_sigma_sq_1, np.float32)[np.asarray(octaves_1, np.int64)]
    w2 = np.asarray(inv_level_sigma_sq_2, np.float32)[np.asarray(octaves_2, np.int64)]
    return dict(p1=_transform(pose_cw_1, pos_w_1), p2=_transform(pose_cw_2, pos_w_2), obs1=np.asarray(keypts_1, np.float32).reshape(-1, 2).astype(np.float64),
                obs2=np.asarray(keypts_2, np.float32).reshape(-1, 2).astype(np.float64), w1=w1, w2=w2, cam_1=cam_1, cam_2=cam_2,
                R=np.asarray(rot_12, np.float64).reshape(3, 3), t=np.asarray(trans_12, np.float64).reshape(3), s=float(scale_12))


class _transform_handle(_ransac_handle):
    """ovs_sim3opt with its capacity."""
    _abi = "ovs_sim3opt"


_OPT_ARRAYS = (("p1", np.float64, 3), ("p2", np.float64, 3), ("obs1", np.float64, 2), ("obs2", np.float64, 2), ("w1", np.float32, 1), ("w2", np.float32, 1))


def optimize_transform_batch(problems, fix_scale, chi_sq=10.0, num_iter=10, handle=None, device=0, with_info=True):
    """transform_optimizer::optimize for every problem (dicts as transform_problem_from_keyframes returns them) in one call: a list of dicts
    num_inliers, rot_12 (3 x 3), trans_12 (3), scale_12, outlier_flags (n, bool) and info (8 doubles: iterations and trials of round 1, its
    robust chi-square, its outliers, the same three of round 2, the last lambda). `handle`: a _transform_handle to reuse."""
    P, offsets, T, packed = _pack(problems, _OPT_ARRAYS, "w1", "p1, p2, obs1, obs2, w1 and w2 of a problem must have one entry per match")
    if P == 0:
        return []
    cams_1 = (_lib.Camera * P)(*[q["cam_1"] for q in problems])
    cams_2 = (_lib.Camera * P)(*[q["cam_2"] for q in problems])
    rot_in = np.ascontiguousarray([np.asarray(q["R"], np.float64).reshape(3, 3) for q in problems])
    trans_in = np.ascontiguousarray([np.asarray(q["t"], np.float64).reshape(3) for q in problems])
    scale_in = np.ascontiguousarray([float(q["s"]) for q in problems])
    if handle is None:
        handle = _transform_handle(P, max(T, 1), device)
    num, rot, trans, scale = np.zeros(P, np.int32), np.zeros((P, 3, 3)), np.zeros((P, 3)), np.zeros(P)
    flags, info = np.zeros(max(T, 1), np.uint8), np.zeros((P, 8)) if with_info else None
    _lib.check(handle._L.ovs_sim3opt_optimize_batch(handle._h, P, _p(offsets), *map(_p, packed), cams_1, cams_2, _p(rot_in), _p(trans_in), _p(scale_in),
                                                    1 if fix_scale else 0, float(chi_sq), int(num_iter), _p(num), _p(rot), _p(trans), _p(scale), _p(flags),
                                                    _p(info)), "ovs_sim3opt_optimize_batch")
    return [dict(num_inliers=int(num[i]), rot_12=rot[i].copy(), trans_12=trans[i].copy(), scale_12=float(scale[i]),
                 outlier_flags=flags[offsets[i]:offsets[i + 1]].astype(bool), info=None if info is None else info[i].copy()) for i in range(P)]


class transform_optimizer:
    """optimize::transform_optimizer: the constructor is upstream's (fix_scale, num_iter); optimize takes what the C++ class collects from the
    two keyframes (see transform_problem_from_keyframes) and returns (num_inliers, rot_12, trans_12, scale_12, outlier_flags)."""

    def __init__(self, fix_scale, num_iter=10, device=0):
        self._fix_scale, self._num_iter, self._device = bool(fix_scale), int(num_iter), device

    def optimize(self, problem, chi_sq=10.0):
        r = optimize_transform_batch([problem], self._fix_scale, chi_sq, self._num_iter, device=self._device)[0]
        return r["num_inliers"], r["rot_12"], r["trans_12"], r["scale_12"], r["outlier_flags"]


# ---- module::two_view_triangulator
def _det_cos(x):
    """ovs_det_cos of include/ovs_detmath.h (DESIGN.md 3.11 rule 3), operation for operation: a Python float is an IEEE f64 and every
    operation rounds once. The class shims of both languages turn rays_parallax_deg_thr into cos_rays_parallax_thr with it."""
    if not abs(x) <= 1048576.0:
        return float("nan")
    m = 0
    while abs(x) > _PI_O_4:
        x = x * 0.5
        m += 1
    z = x * x
    p = _SIN_K[0]
    for k in _SIN_K[1:]:
        p = k + z * p
    s = x + x * (z * p)
    p = _COS_K[0]
    for k in _COS_K[1:]:
        p = k + z * p
    c = (1.0 - 0.5 * z) + z * (z * p)
    for _ in range(m):
        s, c = 2.0 * (s * c), 1.0 - 2.0 * (s * s)
    return c


_PI_O_4 = float.fromhex("0x1.921fb54442d18p-1")
_SIN_K = [float.fromhex(h) for h in ("0x1.952c77030ad4ap-49", "-0x1.ae7f3e733b81fp-41", "0x1.6124613a86d09p-33", "-0x1.ae64567f544e4p-26",
                                     "0x1.71de3a556c734p-19", "-0x1.a01a01a01a01ap-13", "0x1.1111111111111p-7", "-0x1.5555555555555p-3")]
_COS_K = [float.fromhex(h) for h in ("0x1.ae7f3e733b81fp-45", "-0x1.93974a8c07c9dp-37", "0x1.1eed8eff8d898p-29", "-0x1.27e4fb7789f5cp-22",
                                     "0x1.a01a01a01a01ap-16", "-0x1.6c16c16c16c17p-10", "0x1.5555555555555p-5")]


def cos_rays_parallax_thr(rays_parallax_deg_thr=1.0):
    """two_view_triangulator's cos_rays_parallax_thr_ for the constructor's rays_parallax_deg_thr."""
    return _det_cos(float(rays_parallax_deg_thr) * math.pi / 180.0)


_TRI_ARRAYS = (("bearings_1", np.float64, 3), ("bearings_2", np.float64, 3), ("keypts_1", np.float32, 2), ("keypts_2", np.float32, 2),
               ("x_right_1", np.float32, 1), ("x_right_2", np.float32, 1), ("depths_1", np.float32, 1), ("depths_2", np.float32, 1),
               ("sigma_sq_1", np.float32, 1), ("sigma_sq_2", np.float32, 1), ("scale_factors_1", np.float32, 1), ("scale_factors_2", np.float32, 1))


def _pose12(pose_cw):
    """rotation row-major, then translation, of a 4 x 4 or 3 x 4 world -> camera pose (12 doubles pass through)."""
    T = np.asarray(pose_cw, np.float64)
    if T.size == 12 and T.ndim == 1:
        return T.copy()
    return np.concatenate([T[:3, :3].ravel(), T[:3, 3]])


def triangulation_problem_from_keyframes(matches, keypts_1, keypts_2, stereo_x_right_1, stereo_x_right_2, depths_1, depths_2, bearings_1, bearings_2,
                                         octaves_1, octaves_2, scale_factors, level_sigma_sq, pose_cw_1, pose_cw_2, cam_1, cam_2):
    """What two_view_triangulator reads of two keyframes for the matched pairs. matches: (m, 2) pairs (idx_1, idx_2), or a 1-D matched_2_in_1
    array exactly as match_for_triangulation returns it (entry idx_1 holds idx_2, or -1). keypts_*: (n, 2) undistorted keypoints;
    stereo_x_right_* / depths_*: (n,), or None for a keyframe without stereo observations; bearings_*: (n, 3); octaves_*: (n,);
    scale_factors / level_sigma_sq: per level; pose_cw_*: 4 x 4 (or 3 x 4) world -> camera. The problem keeps the pairs as idx_1 / idx_2."""
    m = np.asarray(matches)
    if m.ndim == 1:
        idx_1 = np.nonzero(m >= 0)[0].astype(np.int64)
        idx_2 = m[idx_1].astype(np.int64)
    else:
        m = m.reshape(-1, 2).astype(np.int64)
        idx_1, idx_2 = m[:, 0], m[:, 1]
    sf, sig = np.asarray(scale_factors, np.float32), np.asarray(level_sigma_sq, np.float32)
    take = lambda a, idx, n: np.full(len(idx), -1.0, np.float32) if a is None else np.asarray(a, np.float32).reshape(n)[idx]
    q = dict(idx_1=idx_1, idx_2=idx_2, cam_1=cam_1, cam_2=cam_2, pose_cw_1=_pose12(pose_cw_1), pose_cw_2=_pose12(pose_cw_2))
    for side, idx, kp, xr, dep, b, octv in (("1", idx_1, keypts_1, stereo_x_right_1, depths_1, bearings_1, octaves_1),
                                             ("2", idx_2, keypts_2, stereo_x_right_2, depths_2, bearings_2, octaves_2)):
        n = len(np.asarray(octv).ravel())
        o = np.asarray(octv, np.int64).ravel()[idx]
        q["bearings_" + side] = np.asarray(b, np.float64).reshape(n, 3)[idx]
        q["keypts_" + side] = np.asarray(kp, np.float32).reshape(n, 2)[idx]
        q["x_right_" + side] = take(xr, idx, n)
        q["depths_" + side] = take(dep, idx, n)
        q["sigma_sq_" + side] = sig[o]
        q["scale_factors_" + side] = sf[o]
    return q


class _triangulate_handle(_ransac_handle):
    """ovs_triangulate with its capacity."""
    _abi = "ovs_triangulate"


def triangulate_batch(problems, ratio_factor, cos_rays_parallax_thr=cos_rays_parallax_thr(1.0), handle=None, device=0):
    """two_view_triangulator::triangulate for every match of every problem (dicts as triangulation_problem_from_keyframes returns them) in one
    call: a list of dicts pos_w (n, 3), status (n, uint8: 0 accepted, else the gate that rejected, DESIGN.md 3.12 rule T9), method (n, uint8),
    accepted (n, bool) and num_accepted. ratio_factor: the caller's 1.5f * scale_factor. `handle`: a _triangulate_handle to reuse (the mapping
    thread keeps one)."""
    P, offsets, T, packed = _pack(problems, _TRI_ARRAYS, "x_right_1", "every per-match array of a problem must have one entry per match")
    if P == 0:
        return []
    cams_1 = (_lib.Camera * P)(*[q["cam_1"] for q in problems])
    cams_2 = (_lib.Camera * P)(*[q["cam_2"] for q in problems])
    poses_1 = np.ascontiguousarray([_pose12(q["pose_cw_1"]) for q in problems])
    poses_2 = np.ascontiguousarray([_pose12(q["pose_cw_2"]) for q in problems])
    if handle is None:
        handle = _triangulate_handle(P, max(T, 1), device)
    pos, status, method, num = np.zeros((max(T, 1), 3)), np.zeros(max(T, 1), np.uint8), np.zeros(max(T, 1), np.uint8), np.zeros(P, np.int32)
    _lib.check(handle._L.ovs_triangulate_batch(handle._h, P, _p(offsets), *map(_p, packed), cams_1, cams_2, _p(poses_1), _p(poses_2),
                                               float(cos_rays_parallax_thr), float(ratio_factor), _p(pos), _p(status), _p(method), _p(num)),
               "ovs_triangulate_batch")
    return [dict(pos_w=pos[offsets[i]:offsets[i + 1]].copy(), status=status[offsets[i]:offsets[i + 1]].copy(), method=method[offsets[i]:offsets[i + 1]].copy(),
                 accepted=status[offsets[i]:offsets[i + 1]] == 0, num_accepted=int(num[i])) for i in range(P)]


class two_view_triangulator:
    """module::two_view_triangulator: upstream's constructor (keyfrm_1, keyfrm_2, rays_parallax_deg_thr) and triangulate(idx_1, idx_2), which
    returns (accepted, pos_w); triangulate_matches(pairs) hands every pair of the two keyframes to one device call. A keyframe is a dict:
    undist_keypts (n, 2), stereo_x_right and depths ((n,) or None), bearings (n, 3), octaves (n,), scale_factors and level_sigma_sq (per
    level), scale_factor, pose_cw (4 x 4) and camera (solve.camera)."""

    def __init__(self, keyfrm_1, keyfrm_2, rays_parallax_deg_thr=1.0, device=0):
        self._k1, self._k2, self._device = keyfrm_1, keyfrm_2, device
        self._cos_thr = cos_rays_parallax_thr(rays_parallax_deg_thr)
        self._ratio_factor = np.float32(1.5) * np.float32(max(keyfrm_1["scale_factor"], keyfrm_2["scale_factor"]))

    def problem(self, pairs):
        a, b = self._k1, self._k2
        if np.asarray(a["scale_factors"], np.float32).tolist() != np.asarray(b["scale_factors"], np.float32).tolist():
            raise ValueError("both keyframes must share their scale pyramid")
        return triangulation_problem_from_keyframes(np.asarray(pairs, np.int64).reshape(-1, 2), a["undist_keypts"], b["undist_keypts"], a.get("stereo_x_right"),
                                                    b.get("stereo_x_right"), a.get("depths"), b.get("depths"), a["bearings"], b["bearings"], a["octaves"],
                                                    b["octaves"], a["scale_factors"], a["level_sigma_sq"], a["pose_cw"], b["pose_cw"], a["camera"], b["camera"])

    def triangulate_matches(self, pairs, handle=None):
        """(accepted (m, bool), pos_w (m, 3)) for the pairs (idx_1, idx_2)."""
        r = triangulate_batch([self.problem(pairs)], float(self._ratio_factor), self._cos_thr, handle=handle, device=self._device)[0]
        return r["accepted"], r["pos_w"]

    def triangulate(self, idx_1, idx_2):
        accepted, pos_w = self.triangulate_matches([(idx_1, idx_2)])
        return bool(accepted[0]), pos_w[0]


# ---- solve::homography_solver and solve::fundamental_solver
TWO_VIEW_DEFAULT_SEED = 0x48462D32   # upstream draws from random_device; here a run is reproducible
MODEL_H, MODEL_F = 1, 2              # the bits of `models`, and the values of `selected`


def two_view_problem_seed(seed, p):
    """The seed under which problem p of a batch, solved ALONE (as problem 0), draws the samples it draws in the batch (3.13 rule 2)."""
    return (seed + _G * (p << 24)) & _MASK


def two_view_problem(undist_keypts_1, undist_keypts_2, matches_12):
    """What the two solvers' constructors keep: the undistorted keypoints of the matched pairs (idx_1, idx_2), widened to double. keypts:
    (n, 2); matches_12: (m, 2) pairs."""
    m = np.asarray(matches_12, np.int64).reshape(-1, 2)
    return dict(x1=np.asarray(undist_keypts_1, np.float64).reshape(-1, 2)[m[:, 0]], x2=np.asarray(undist_keypts_2, np.float64).reshape(-1, 2)[m[:, 1]])


class _two_view_handle(_ransac_handle):
    """ovs_twoview with its capacity."""
    _abi = "ovs_twoview"


_TWO_VIEW_ARRAYS = (("x1", np.float64, 2), ("x2", np.float64, 2))


def solve_two_view_batch(problems, sigma=1.0, max_num_iter=100, recompute=True, seed=TWO_VIEW_DEFAULT_SEED, models=3, handle=None, device=0):
    """Both find_via_ransac of the monocular initialiser for every problem (dicts with x1, x2: (n, 2)) in one call: a list of dicts H and F
    (each valid, best_iter, num_inliers, score, the matrix H_21 / F_21 (3 x 3) and inlier_flags (n, bool); the invalid form for a model
    `models` leaves out) and selected (1: H, 2: F, 0: neither). `handle`: a _two_view_handle to reuse (the initialiser keeps one)."""
    P, offsets, T, (x1, x2) = _pack(problems, _TWO_VIEW_ARRAYS, "x1", "x1 and x2 of a problem must have one entry per match")
    if P == 0:
        return []
    if handle is None:
        handle = _two_view_handle(P, max(T, 1), device)
    mats = [np.zeros((P, 3, 3)), np.zeros((P, 3, 3))]
    scores, valid, best_iter, num = np.zeros((P, 2)), np.zeros((P, 2), np.int32), np.zeros((P, 2), np.int32), np.zeros((P, 2), np.int32)
    selected, flags = np.zeros(P, np.int32), [np.zeros(max(T, 1), np.uint8), np.zeros(max(T, 1), np.uint8)]
    _lib.check(handle._L.ovs_twoview_solve_batch(handle._h, P, _p(offsets), _p(x1), _p(x2), float(sigma), int(max_num_iter), 1 if recompute else 0,
                                                 int(seed) & _MASK, int(models), _p(mats[0]), _p(mats[1]), _p(scores), _p(valid), _p(best_iter), _p(num),
                                                 _p(selected), _p(flags[0]), _p(flags[1])), "ovs_twoview_solve_batch")
    out = []
    for i in range(P):
        r = {"selected": int(selected[i])}
        for m, (name, key) in enumerate((("H", "H_21"), ("F", "F_21"))):
            r[name] = {"valid": bool(valid[i, m]), "best_iter": int(best_iter[i, m]), "num_inliers": int(num[i, m]), "score": float(scores[i, m]),
                       key: mats[m][i].copy(), "inlier_flags": flags[m][offsets[i]:offsets[i + 1]].astype(bool)}
        out.append(r)
    return out


class _two_view_solver(_ransac_solver):
    """What homography_solver and fundamental_solver share: upstream's constructor (undist_keypts_1, undist_keypts_2, matches_12, sigma),
    find_via_ransac and the getters both have."""
    _model, _name = None, None

    def __init__(self, undist_keypts_1, undist_keypts_2, matches_12, sigma, device=0):
        self._matches = [tuple(int(v) for v in m) for m in np.asarray(matches_12, np.int64).reshape(-1, 2)]
        self._problem, self._sigma, self._device = two_view_problem(undist_keypts_1, undist_keypts_2, matches_12), float(sigma), device

    def find_via_ransac(self, max_num_iter, recompute=True, seed=TWO_VIEW_DEFAULT_SEED):
        self._result = solve_two_view_batch([self._problem], self._sigma, max_num_iter, recompute, seed, self._model, device=self._device)[0][self._name]

    def get_best_score(self):
        return self._get("score")

    def get_inlier_matches(self):
        return self._get("inlier_flags")


class homography_solver(_two_view_solver):
    """solve::homography_solver over one problem."""
    _model, _name = MODEL_H, "H"

    def get_best_H_21(self):
        return self._get("H_21")


class fundamental_solver(_two_view_solver):
    """solve::fundamental_solver over one problem."""
    _model, _name = MODEL_F, "F"

    def get_best_F_21(self):
        return self._get("F_21")


# ---- solve::essential_solver
ESSENTIAL_DEFAULT_SEED = 0x45737365   # upstream draws from random_device; here a run is reproducible
# upstream's residual_cos_thr as recalled: the float 0.01745240643f (one degree), widened to double
ESSENTIAL_RESIDUAL_COS_THR = float(np.float32(0.01745240643))


def essential_problem_seed(seed, p):
    """The seed under which problem p of a batch, solved ALONE (as problem 0), draws the samples it draws in the batch (3.16 rule E1)."""
    return (seed + _G * (p << 24)) & _MASK


def essential_problem(bearings_1, bearings_2, matches_12):
    """What the solver's constructor is given: the bearings of the matched pairs (idx_1, idx_2). bearings: (n, 3); matches_12: (m, 2)."""
    m = np.asarray(matches_12, np.int64).reshape(-1, 2)
    return dict(b1=np.asarray(bearings_1, np.float64).reshape(-1, 3)[m[:, 0]], b2=np.asarray(bearings_2, np.float64).reshape(-1, 3)[m[:, 1]])


class _essential_handle(_ransac_handle):
    """ovs_essential with its capacity."""
    _abi = "ovs_essential"


_ESSENTIAL_ARRAYS = (("b1", np.float64, 3), ("b2", np.float64, 3))


def solve_essential_batch(problems, residual_cos_thr=ESSENTIAL_RESIDUAL_COS_THR, max_num_iter=50, recompute=False, seed=ESSENTIAL_DEFAULT_SEED,
                          handle=None, device=0):
    """find_via_ransac of solve::essential_solver for every problem (dicts with b1, b2: (n, 3)) in one call: a list of dicts valid,
    best_iter, num_inliers, score, E_21 (3 x 3) and inlier_flags (n, bool). The defaults are robust::match_frame_and_keyframe's: 50
    iterations, no recompute. `handle`: an _essential_handle to reuse."""
    P, offsets, T, (b1, b2) = _pack(problems, _ESSENTIAL_ARRAYS, "b1", "b1 and b2 of a problem must have one entry per match")
    if P == 0:
        return []
    if handle is None:
        handle = _essential_handle(P, max(T, 1), device)
    E, scores = np.zeros((P, 3, 3)), np.zeros(P)
    valid, best_iter, num, flags = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(max(T, 1), np.uint8)
    _lib.check(handle._L.ovs_essential_solve_batch(handle._h, P, _p(offsets), _p(b1), _p(b2), float(residual_cos_thr), int(max_num_iter),
                                                   1 if recompute else 0, int(seed) & _MASK, _p(E), _p(scores), _p(valid), _p(best_iter), _p(num),
                                                   _p(flags)), "ovs_essential_solve_batch")
    return [{"valid": bool(valid[i]), "best_iter": int(best_iter[i]), "num_inliers": int(num[i]), "score": float(scores[i]), "E_21": E[i].copy(),
             "inlier_flags": flags[offsets[i]:offsets[i + 1]].astype(bool)} for i in range(P)]


class essential_solver(_ransac_solver):
    """solve::essential_solver over one problem: upstream's constructor (bearings_1, bearings_2, matches_12), find_via_ransac and getters."""

    def __init__(self, bearings_1, bearings_2, matches_12, device=0):
        self._problem, self._device = essential_problem(bearings_1, bearings_2, matches_12), device

    def find_via_ransac(self, max_num_iter, recompute=True, seed=ESSENTIAL_DEFAULT_SEED, residual_cos_thr=ESSENTIAL_RESIDUAL_COS_THR):
        self._result = solve_essential_batch([self._problem], residual_cos_thr, max_num_iter, recompute, seed, device=self._device)[0]

    def get_best_score(self):
        return self._get("score")

    def get_best_E_21(self):
        return self._get("E_21")

    def get_inlier_matches(self):
        return self._get("inlier_flags")


# ---- initialize::perspective's reconstruct_with_H / reconstruct_with_F, check_pose and find_most_plausible_pose
def bearings_of(undist_keypts, cam):
    """camera::perspective::convert_keypoints_to_bearings: ((u - cx) / fx, (v - cy) / fy, 1) normalised, per undistorted keypoint, in f64."""
    kp = np.asarray(undist_keypts, np.float64).reshape(-1, 2)
    x, y = (kp[:, 0] - cam.cx) / cam.fx, (kp[:, 1] - cam.cy) / cam.fy
    l = np.sqrt((x * x + y * y) + 1.0)
    return np.stack([x / l, y / l, 1.0 / l], axis=1)


def reconstruct_problem(model, mat, cam, inlier_flags, keypts_ref, keypts_cur, bearings_ref, bearings_cur):
    """One (reference frame, current frame) problem of the pose recovery: model (MODEL_H or MODEL_F) with its matrix H_21 / F_21 (3 x 3),
    the perspective camera (solve.camera), and per match the model's inlier flag, the two undistorted keypoints (n, 2) and the two bearings
    (n, 3)."""
    return dict(model=int(model), mat=np.ascontiguousarray(mat, np.float64).reshape(3, 3), cam=cam, inlier=np.ascontiguousarray(inlier_flags, np.uint8).ravel(),
                kp_ref=np.ascontiguousarray(keypts_ref, np.float64).reshape(-1, 2), kp_cur=np.ascontiguousarray(keypts_cur, np.float64).reshape(-1, 2),
                b_ref=np.ascontiguousarray(bearings_ref, np.float64).reshape(-1, 3), b_cur=np.ascontiguousarray(bearings_cur, np.float64).reshape(-1, 3))


def reconstruct_problem_from_solution(solution, two_view, cam, bearings_ref=None, bearings_cur=None):
    """The problem of the model one result of solve_two_view_batch selected (None where it selected neither). two_view: the problem that
    call solved (x1, x2: the matched undistorted keypoints); the bearings default to bearings_of the keypoints."""
    if solution["selected"] not in (MODEL_H, MODEL_F):
        return None
    name, key = ("H", "H_21") if solution["selected"] == MODEL_H else ("F", "F_21")
    x1, x2 = np.asarray(two_view["x1"], np.float64).reshape(-1, 2), np.asarray(two_view["x2"], np.float64).reshape(-1, 2)
    return reconstruct_problem(solution["selected"], solution[name][key], cam, solution[name]["inlier_flags"], x1, x2,
                               bearings_of(x1, cam) if bearings_ref is None else bearings_ref, bearings_of(x2, cam) if bearings_cur is None else bearings_cur)


class _reconstruct_handle(_ransac_handle):
    """ovs_reconstruct with its capacity."""
    _abi = "ovs_reconstruct"


_REC_ARRAYS = (("inlier", np.uint8, 1), ("kp_ref", np.float64, 2), ("kp_cur", np.float64, 2), ("b_ref", np.float64, 3), ("b_cur", np.float64, 3))


def reconstruct_two_view_batch(problems, reproj_err_thr=4.0, parallax_deg_thr=1.0, min_num_triangulated=50, handle=None, device=0):
    """reconstruct_with_H / reconstruct_with_F for every problem (dicts as reconstruct_problem returns them) in one call: a list of dicts
    success, best (the winning hypothesis, -1), rot_ref_to_cur (3 x 3), trans_ref_to_cur (3), triangulated_pts (n, 3), is_triangulated
    (n, bool), counts (8) and parallax_deg (8, float32) per hypothesis. `handle`: a _reconstruct_handle to reuse (the initialiser keeps one)."""
    P, offsets, T, packed = _pack(problems, _REC_ARRAYS, "inlier", "every per-match array of a problem must have one entry per match")
    if P == 0:
        return []
    models = np.ascontiguousarray([q["model"] for q in problems], np.int32)
    mats = np.ascontiguousarray([np.asarray(q["mat"], np.float64).reshape(3, 3) for q in problems])
    cams = (_lib.Camera * P)(*[q["cam"] for q in problems])
    if handle is None:
        handle = _reconstruct_handle(P, max(T, 1), device)
    success, best, rot, trans = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros((P, 3, 3)), np.zeros((P, 3))
    counts, parallax, pts, flags = np.zeros((P, 8), np.int32), np.zeros((P, 8), np.float32), np.zeros((max(T, 1), 3)), np.zeros(max(T, 1), np.uint8)
    _lib.check(handle._L.ovs_reconstruct_batch(handle._h, P, _p(offsets), _p(models), _p(mats), cams, *map(_p, packed), float(reproj_err_thr),
                                               float(parallax_deg_thr), int(min_num_triangulated), _p(success), _p(best), _p(rot), _p(trans), _p(counts),
                                               _p(parallax), _p(pts), _p(flags)), "ovs_reconstruct_batch")
    return [dict(success=bool(success[i]), best=int(best[i]), rot_ref_to_cur=rot[i].copy(), trans_ref_to_cur=trans[i].copy(),
                 triangulated_pts=pts[offsets[i]:offsets[i + 1]].copy(), is_triangulated=flags[offsets[i]:offsets[i + 1]].astype(bool),
                 counts=counts[i].copy(), parallax_deg=parallax[i].copy()) for i in range(P)]
