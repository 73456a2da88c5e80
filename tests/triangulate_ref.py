"""Sequential restatement of module::two_view_triangulator::triangulate as DESIGN.md 3.12 fixes it (rules T1 to T9): one match after the other.
Pure Python on purpose: a Python float is an IEEE f64 and every operation below rounds once, so the results are the bits the rules ask for.
No numpy in the arithmetic; imports nothing of the product. det_cos is tests/transform_ref.py's, the Jacobi sweeps, the equirectangular
projection and atan2 (include/ovs_detmath.h through the oracle library) are tests/sim3_ref.py's.

A problem is a dict: cam_1, cam_2 (dicts: model 0 with fx fy cx cy focal_x_baseline true_baseline, or model 1 with cols rows), pose_1, pose_2
(12 floats: the rotation row-major, then the translation) and per match b1, b2 (3-tuples), kp1, kp2 (2-tuples), xr1, xr2, depth1, depth2, sig1,
sig2, sf1, sf2 (floats that hold f32 values).

Below the rules: a scene builder with named cases (CASES) for the CPU and the device tests."""
import functools
import math
import random

from sim3_ref import _detmath, _div, _sqrt, bits, dot3, f32, jacobi, project  # noqa: F401
from transform_ref import det_cos

CHI_SQ_MONO, CHI_SQ_STEREO = f32(5.99146), f32(7.81473)
COS_THR = det_cos(1.0 * math.pi / 180.0)      # the class shims' cos_rays_parallax_thr
SCALE_FACTOR = f32(1.2)
RATIO_FACTOR = f32(f32(1.5) * SCALE_FACTOR)   # the caller's 1.5f * scale_factor, a float product
NUM_LEVELS = 8


def det_atan2(y, x):
    return _detmath(3, y, x)


# ---- T4
def dlt_rows(P1, P2, b1, b2):
    """The four rows of A; P[r] = (R[r][0], R[r][1], R[r][2], t[r])."""
    row = lambda P, r: [P[3 * r], P[3 * r + 1], P[3 * r + 2], P[9 + r]]
    out = []
    for P, b in ((P1, b1), (P2, b2)):
        p0, p1, p2 = row(P, 0), row(P, 1), row(P, 2)
        out.append([b[0] * p2[k] - b[2] * p0[k] for k in range(4)])
        out.append([b[1] * p2[k] - b[2] * p1[k] for k in range(4)])
    return out


def two_view(P1, P2, b1, b2):
    A = dlt_rows(P1, P2, b1, b2)
    M = [[((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j] for j in range(4)] for i in range(4)]
    for r in range(4):
        for c in range(r):
            M[r][c] = M[c][r]
    D, V = jacobi(M)
    best = 0
    for i in range(1, 4):
        if D[i][i] < D[best][best]:
            best = i
    return [_div(V[k][best], V[3][best]) for k in range(3)]


# ---- T5
def back_project(cam, P, kp, depth):
    x = _div((kp[0] - cam["cx"]) * depth, cam["fx"]) - P[9]
    y = _div((kp[1] - cam["cy"]) * depth, cam["fy"]) - P[10]
    z = depth - P[11]
    return [dot3(P[c], P[3 + c], P[6 + c], x, y, z) for c in range(3)]


# ---- T6, T7
def depth_is_positive(cam, P, X):
    return cam["model"] != 0 or dot3(P[6], P[7], P[8], *X) + P[11] > 0.0


def reprojection_is_good(cam, P, X, kp, stereo, x_right, sigma_sq):
    x = dot3(P[0], P[1], P[2], *X) + P[9]
    y = dot3(P[3], P[4], P[5], *X) + P[10]
    z = dot3(P[6], P[7], P[8], *X) + P[11]
    u, v = project(cam, x, y, z)
    ex, ey = u - kp[0], v - kp[1]
    if stereo:
        ex_r = (u - _div(cam["focal_x_baseline"], z)) - x_right
        return ((ex * ex + ey * ey) + ex_r * ex_r) <= CHI_SQ_STEREO * sigma_sq
    return (ex * ex + ey * ey) <= CHI_SQ_MONO * sigma_sq


def centre_of(P):
    return [-dot3(P[c], P[3 + c], P[6 + c], P[9], P[10], P[11]) for c in range(3)]


def triangulate(prob, i, cos_thr=COS_THR, ratio_factor=RATIO_FACTOR):
    """Rules T1 to T9 for match i: dict status, method, pos_w."""
    cam1, cam2, P1, P2 = prob["cam_1"], prob["cam_2"], prob["pose_1"], prob["pose_2"]
    b1, b2 = prob["b1"][i], prob["b2"][i]
    ray1 = [dot3(P1[c], P1[3 + c], P1[6 + c], *b1) for c in range(3)]
    ray2 = [dot3(P2[c], P2[3 + c], P2[6 + c], *b2) for c in range(3)]
    cos_rays = dot3(*ray1, *ray2)
    stereo1 = cam1["model"] == 0 and prob["xr1"][i] >= 0.0
    stereo2 = cam2["model"] == 0 and prob["xr2"][i] >= 0.0
    cs1 = det_cos(2.0 * det_atan2(cam1["true_baseline"] / 2.0, prob["depth1"][i])) if stereo1 else 2.0
    cs2 = det_cos(2.0 * det_atan2(cam2["true_baseline"] / 2.0, prob["depth2"][i])) if stereo2 else 2.0
    cos_stereo = cs2 if cs2 < cs1 else cs1
    any_stereo = stereo1 or stereo2
    if 0.0 < cos_rays and ((not any_stereo and cos_rays < cos_thr) or (any_stereo and cos_rays < cos_stereo)):
        method, X = 1, two_view(P1, P2, b1, b2)
    elif stereo1 and cs1 < cs2:
        method, X = 2, back_project(cam1, P1, prob["kp1"][i], prob["depth1"][i])
    elif stereo2 and cs2 < cs1:
        method, X = 3, back_project(cam2, P2, prob["kp2"][i], prob["depth2"][i])
    else:
        return dict(status=1, method=0, pos_w=[0.0, 0.0, 0.0])
    status = 0
    if not depth_is_positive(cam1, P1, X):
        status = 2
    elif not depth_is_positive(cam2, P2, X):
        status = 3
    elif not reprojection_is_good(cam1, P1, X, prob["kp1"][i], stereo1, prob["xr1"][i], prob["sig1"][i]):
        status = 4
    elif not reprojection_is_good(cam2, P2, X, prob["kp2"][i], stereo2, prob["xr2"][i], prob["sig2"][i]):
        status = 5
    else:
        c1, c2 = centre_of(P1), centre_of(P2)
        d1v, d2v = [X[k] - c1[k] for k in range(3)], [X[k] - c2[k] for k in range(3)]
        d1, d2 = _sqrt(dot3(*d1v, *d1v)), _sqrt(dot3(*d2v, *d2v))
        ratio_dists, ratio_octave = _div(d2, d1), _div(prob["sf1"][i], prob["sf2"][i])
        if not (d1 > 0.0 and d2 > 0.0 and ratio_octave <= ratio_dists * ratio_factor and ratio_dists <= ratio_octave * ratio_factor):
            status = 6
    return dict(status=status, method=method, pos_w=X)


def solve(prob, cos_thr=COS_THR, ratio_factor=RATIO_FACTOR):
    return [triangulate(prob, i, cos_thr, ratio_factor) for i in range(len(prob["b1"]))]


def result_bits(results):
    """[(status, method, [3 bit patterns])] of solve()'s list."""
    return [(r["status"], r["method"], [bits(v) for v in r["pos_w"]]) for r in results]


# ---- the scene builder
SCALE_FACTORS = [f32(1.2 ** l) for l in range(NUM_LEVELS)]
LEVEL_SIGMA_SQ = [f32(s * s) for s in SCALE_FACTORS]
MONO = dict(model=0, fx=458.0, fy=457.0, cx=367.0, cy=248.0, focal_x_baseline=0.0, true_baseline=0.0, cols=752, rows=480)
STEREO = dict(MONO, focal_x_baseline=f32(458.0 * 0.11), true_baseline=f32(0.11))   # (camera::base holds the two as floats)
EQUIRECT = dict(model=1, fx=0.0, fy=0.0, cx=0.0, cy=0.0, focal_x_baseline=0.0, true_baseline=0.0, cols=1920, rows=960)
PAIRS = {"mono_mono": (MONO, MONO, False, False), "stereo_mono": (STEREO, MONO, True, False), "stereo_stereo": (STEREO, STEREO, True, True),
         "equirect": (EQUIRECT, EQUIRECT, False, False), "persp_equirect": (MONO, EQUIRECT, False, False)}


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return [c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c]


def pose_of(R, C):
    """12 doubles of the world -> camera pose with rotation R (9, row-major) and camera centre C."""
    return list(R) + [-dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], *C) for r in range(3)]


def in_camera(P, X):
    return [dot3(P[3 * r], P[3 * r + 1], P[3 * r + 2], *X) + P[9 + r] for r in range(3)]


def pixel_of(cam, pc):
    """Data generation only (libm): the pixel of a point in camera coordinates."""
    if cam["model"] == 0:
        return cam["fx"] * pc[0] / pc[2] + cam["cx"], cam["fy"] * pc[1] / pc[2] + cam["cy"]
    L = math.sqrt(pc[0] ** 2 + pc[1] ** 2 + pc[2] ** 2)
    return cam["cols"] * (0.5 + math.atan2(pc[0], pc[2]) / (2.0 * math.pi)), cam["rows"] * (0.5 + math.asin(pc[1] / L) / math.pi)


def bearing_of(cam, kp):
    """camera::base::convert_keypoint_to_bearing on an undistorted keypoint (data generation: libm)."""
    if cam["model"] == 0:
        x, y = (kp[0] - cam["cx"]) / cam["fx"], (kp[1] - cam["cy"]) / cam["fy"]
        n = math.sqrt(x * x + y * y + 1.0)
        return (x / n, y / n, 1.0 / n)
    lon, lat = (kp[0] / cam["cols"] - 0.5) * 2.0 * math.pi, -(kp[1] / cam["rows"] - 0.5) * math.pi
    return (math.cos(lat) * math.sin(lon), -math.sin(lat), math.cos(lat) * math.cos(lon))


def observe(cam, P, X, stereo, rng, noise_px):
    """(bearing, keypoint, x_right, depth) of the world point X in one keyframe, the keypoint rounded to float as a frame holds it."""
    pc = in_camera(P, X)
    u, v = pixel_of(cam, pc)
    kp = (f32(u + rng.gauss(0.0, noise_px)), f32(v + rng.gauss(0.0, noise_px)))
    if stereo:
        return bearing_of(cam, kp), kp, f32(kp[0] - cam["focal_x_baseline"] / pc[2]), f32(pc[2])
    return bearing_of(cam, kp), kp, -1.0, -1.0


def empty(cam_1, cam_2, pose_1, pose_2):
    q = dict(cam_1=cam_1, cam_2=cam_2, pose_1=pose_1, pose_2=pose_2, truth=[], kinds=[])
    for k in ("b1", "b2", "kp1", "kp2", "xr1", "xr2", "depth1", "depth2", "sig1", "sig2", "sf1", "sf2"):
        q[k] = []
    return q


def add_match(q, o1, o2, oct1=0, oct2=0, truth=None, kind="good"):
    for side, o, octave in (("1", o1, oct1), ("2", o2, oct2)):
        q.setdefault("oct" + side, []).append(octave)
        q["b" + side].append(tuple(o[0]))
        q["kp" + side].append(tuple(o[1]))
        q["xr" + side].append(o[2])
        q["depth" + side].append(o[3])
        q["sig" + side].append(LEVEL_SIGMA_SQ[octave])
        q["sf" + side].append(SCALE_FACTORS[octave])
    q["truth"].append(truth)
    q["kinds"].append(kind)


def scene(n, pair="mono_mono", seed=0, baseline=0.6, depth=(3.0, 9.0), noise_px=0.3, mix=True):
    """n matches between two keyframes `baseline` apart that look nearly the same way. With `mix`, about a third of the matches are spoiled so
    that each gate rejects some: a point too far for its parallax, a keypoint moved by 25 pixels on either side, octaves that contradict the
    distances."""
    cam_1, cam_2, st1, st2 = PAIRS[pair]
    rng = random.Random(1000 * n + seed)
    P1 = pose_of(rot_y(0.02), (0.0, 0.0, 0.0))
    P2 = pose_of(rot_y(-0.04), (baseline, 0.02, -0.03))
    q = empty(cam_1, cam_2, P1, P2)
    for _ in range(n):
        kind = rng.choice(["good"] * 10 + ["far", "kp1", "kp2", "octave"]) if mix else "good"
        d = rng.uniform(*depth) * (400.0 if kind == "far" else 1.0)
        X = [rng.uniform(-0.4, 0.4) * d, rng.uniform(-0.25, 0.25) * d, d]
        o1, o2 = observe(cam_1, P1, X, st1, rng, noise_px), observe(cam_2, P2, X, st2, rng, noise_px)
        if kind == "kp1":
            o1 = (o1[0], (f32(o1[1][0] + 25.0), o1[1][1]), o1[2], o1[3])
        if kind == "kp2":
            o2 = (o2[0], (o2[1][0], f32(o2[1][1] - 25.0)), o2[2], o2[3])
        octave = rng.randrange(0, 3)
        add_match(q, o1, o2, octave, octave + (5 if kind == "octave" else 0), X, kind)
    return q


def _single(pair, P1, P2, X, kind, edit=None, oct2=0):
    cam_1, cam_2, st1, st2 = PAIRS[pair]
    rng = random.Random(7)
    q = empty(cam_1, cam_2, P1, P2)
    for Xi in X:
        o1, o2 = observe(cam_1, P1, Xi, st1, rng, 0.0), observe(cam_2, P2, Xi, st2, rng, 0.0)
        if edit:
            o1, o2 = edit(o1, o2)
        add_match(q, o1, o2, 0, oct2, Xi, kind)
    return q


def _reject_scene(name):
    """One small problem per gate, built so that exactly this gate decides."""
    P1, P2 = pose_of(rot_y(0.0), (0.0, 0.0, 0.0)), pose_of(rot_y(0.0), (1.0, 0.0, 0.0))
    pts = [[0.3, -0.2, 5.0], [-0.5, 0.1, 4.0], [0.8, 0.3, 6.5]]
    if name == "low_parallax":   # T3: a mono pair under one degree of parallax
        return _single("mono_mono", P1, P2, [[3.0, 1.0, 400.0], [-20.0, 5.0, 900.0]], name)
    if name == "behind_1":       # T6 side 1: the rays meet behind both cameras (a keypoint's bearing points forward: away from such a point)
        return _single("mono_mono", P1, P2, [[0.5, 0.0, -2.0], [0.4, 0.1, -3.0]], name)
    if name == "behind_2":       # T6 side 2: camera 2 looks the other way; camera 1's stereo observation decides the point
        return _single("stereo_mono", P1, pose_of(rot_y(math.pi), (1.0, 0.0, 0.0)), pts, name, lambda o1, o2: (o1, ((0.0, 0.0, 1.0), (367.0, 248.0), -1.0, -1.0)))
    if name == "reproj_1":       # T7 side 1: the keypoint is 25 pixels from where its bearing points
        return _single("mono_mono", P1, P2, pts, name, lambda o1, o2: ((o1[0], (f32(o1[1][0] + 25.0), o1[1][1]), o1[2], o1[3]), o2))
    if name == "reproj_2":
        return _single("mono_mono", P1, P2, pts, name, lambda o1, o2: (o1, (o2[0], (o2[1][0], f32(o2[1][1] + 25.0)), o2[2], o2[3])))
    if name == "stereo_xr_bad":  # T7 side 1 through its third term alone: x_right is 10 pixels off
        return _single("stereo_mono", P1, P2, pts, name, lambda o1, o2: ((o1[0], o1[1], f32(o1[2] + 10.0), o1[3]), o2))
    if name == "scale":          # T8: octave 0 against octave 7 at equal distances
        return _single("mono_mono", P1, P2, pts, name, oct2=7)
    if name == "equal_stereo":   # T3: two equal stereo parallaxes and too little parallax between the keyframes
        near = pose_of(rot_y(0.0), (0.01, 0.0, 0.0))
        same_depth = lambda o1, o2: (o1, (o2[0], o2[1], o2[2], o1[3]))
        return _single("stereo_stereo", P1, near, pts, name, same_depth)
    if name == "stereo_close":   # methods 2 and 3: keyframes 1 cm apart, the nearer stereo observation wins
        near = pose_of(rot_y(0.0), (0.01, 0.0, 0.4))
        back = pose_of(rot_y(0.0), (0.01, 0.0, -0.4))
        q, q2 = _single("stereo_stereo", P1, near, pts, name), _single("stereo_stereo", P1, back, pts, name)
        return q, q2
    raise KeyError(name)


def _nan_inf():
    q = scene(65, "stereo_mono", seed=3)
    q["b1"][17] = (float("nan"), q["b1"][17][1], q["b1"][17][2])
    q["depth1"][17] = float("inf")
    return q


REJECTS = ["low_parallax", "behind_1", "behind_2", "reproj_1", "reproj_2", "stereo_xr_bad", "scale", "equal_stereo"]
SIZES = {"n0": 0, "n1": 1, "n63": 63, "n64": 64, "n65": 65, "n129": 129, "n257": 257}
CASES = sorted(list(SIZES) + list(PAIRS) + REJECTS + ["n130", "stereo_close_2", "stereo_close_3", "nan_inf", "nan_inf_clean"])
# which status codes and methods a case has to reach (tests/test_triangulate_ref.py holds the scenes to this)
REACHES = {
    "low_parallax": ({1}, {0}), "behind_1": ({2}, {1}), "behind_2": ({3}, {2}), "reproj_1": ({4}, {1}), "reproj_2": ({5}, {1}),
    "stereo_xr_bad": ({4}, {1}), "scale": ({6}, {1}), "equal_stereo": ({1}, {0}), "stereo_close_2": ({0}, {2}), "stereo_close_3": ({0}, {3}),
    "mono_mono": ({0, 1, 4, 5, 6}, {0, 1}), "stereo_mono": ({0, 4, 5, 6}, {1}), "stereo_stereo": ({0, 4, 5, 6}, {1}),
    "equirect": ({0, 1, 4, 5, 6}, {0, 1}), "persp_equirect": ({0, 1, 4, 5, 6}, {0, 1}), "n1": ({0}, {1}), "n257": ({0, 1, 4, 5, 6}, {0, 1}),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    if name in SIZES:
        return scene(SIZES[name], "mono_mono", seed=1, mix=SIZES[name] > 1)
    if name == "n130":
        return scene(130, "stereo_mono", seed=2)
    if name in PAIRS:
        return scene(65, name, seed=5)
    if name == "stereo_close_2":
        return _reject_scene("stereo_close")[1]
    if name == "stereo_close_3":
        return _reject_scene("stereo_close")[0]
    if name == "nan_inf":
        return _nan_inf()
    if name == "nan_inf_clean":
        return scene(65, "stereo_mono", seed=3)
    return _reject_scene(name)


@functools.lru_cache(maxsize=None)
def solved(name):
    """The reference's results on a case, computed once and shared."""
    return solve(problem(name))


def parallax_scene(parallax_deg, depth, k, exact=True):
    """One noise-free mono match at the given parallax and depth: (problem, true point). With `exact` the bearings are the exact doubles,
    not those of the float keypoint."""
    base = 2.0 * depth * math.tan(math.radians(parallax_deg) / 2.0)
    P1, P2 = pose_of(rot_y(0.01), (0.0, 0.0, 0.0)), pose_of(rot_y(-0.015), (base, 0.0, 0.0))
    X = [base / 2.0 + 0.02 * depth * math.cos(k), 0.03 * depth * math.sin(k), depth]
    q = _single("mono_mono", P1, P2, [X], "good")
    if exact:
        for side, P in (("1", P1), ("2", P2)):
            pc = in_camera(P, X)
            n = math.sqrt(pc[0] ** 2 + pc[1] ** 2 + pc[2] ** 2)
            q["b" + side] = [(pc[0] / n, pc[1] / n, pc[2] / n)]
            q["kp" + side] = [pixel_of(MONO, pc)]
    return q, X
