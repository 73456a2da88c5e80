"""The scenes of the pose-recovery tests (tests/test_reconstruct_ref.py asserts their distance from every decision, tests/test_gpu_reconstruct.py
runs them on the device): two views of a plane with the planted homography, or of a cloud with the planted fundamental matrix. Pure Python
and seeded, so that every machine builds the same bits."""
import functools
import math
import random

import reconstruct_ref as ref
from sim3_ref import dot3, f32

CAM = (458.654, 457.296, 367.215, 248.375)
ANGLE, AXIS, TRANS = 0.12, (0.2, 1.0, 0.1), (0.45, -0.05, 0.1)
PLANE_N, PLANE_D = (0.1, -0.15, 1.0), 6.0    # the plane n . X = d in the reference camera's coordinates
NAN = float("nan")


def rotation(angle=ANGLE, axis=AXIS):
    nrm = math.sqrt(sum(v * v for v in axis))
    x, y, z = (v / nrm for v in axis)
    c, s = math.cos(angle), math.sin(angle)
    k = 1.0 - c
    return [c + x * x * k, x * y * k - z * s, x * z * k + y * s, y * x * k + z * s, c + y * y * k, y * z * k - x * s, z * x * k - y * s, z * y * k + x * s,
            c + z * z * k]


def planted(model, R, t, cam=CAM, plane_n=PLANE_N, plane_d=PLANE_D):
    """H_21 = K (R + t n^T / d) K^-1 for the plane, F_21 = K^-T [t]x R K^-1."""
    fx, fy, cx, cy = cam
    K = [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0]
    Kinv = [1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0]
    if model == ref.MODEL_H:
        M = [R[3 * r + c] + t[r] * plane_n[c] / plane_d for r in range(3) for c in range(3)]
        return ref.mul3(K, ref.mul3(M, Kinv))
    tx = [0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0]
    return ref.mul3(ref.transpose3(Kinv), ref.mul3(ref.mul3(tx, R), Kinv))


def bearing(kp, cam=CAM):
    x, y = (kp[0] - cam[2]) / cam[0], (kp[1] - cam[3]) / cam[1]
    l = math.sqrt((x * x + y * y) + 1.0)
    return (x / l, y / l, 1.0 / l)


def scene(model, n_good, n_bad=None, n_gross=0, noise_px=0.3, trans_scale=1.0, angle=ANGLE, rng_seed=0, plane_n=PLANE_N, half_fov=(0.7, 0.45), cam=CAM,
          mat=None):
    """n_good matches that obey the planted model up to Gaussian keypoint noise and carry the inlier flag, n_bad (a fifth of them and three)
    with a random keypoint in the current image and no flag, n_gross flagged ones 30 pixels off, all shuffled. Every keypoint is narrowed to
    f32, as a cv::KeyPoint holds it, and the bearings come from the narrowed keypoints, as a frame's do."""
    plane = model == ref.MODEL_H
    rng = random.Random(7919 * n_good + rng_seed + (500000 if plane else 0))
    n_bad = n_good // 5 + 3 if n_bad is None else n_bad
    kinds = ["good"] * n_good + ["bad"] * n_bad + ["gross"] * n_gross
    rng.shuffle(kinds)
    R, t = rotation(angle), [v * trans_scale for v in TRANS]
    fx, fy, cx, cy = cam
    q = dict(model=model, mat=planted(model, R, t, cam, plane_n) if mat is None else mat, cam=cam, inlier=[], kp1=[], kp2=[], b1=[], b2=[], truth=(R, t), kinds=kinds)
    for kind in kinds:
        u, v = rng.uniform(-half_fov[0], half_fov[0]), rng.uniform(-half_fov[1], half_fov[1])
        z = PLANE_D / (plane_n[0] * u + plane_n[1] * v + plane_n[2]) if plane else rng.uniform(4.0, 9.0)
        X = (u * z, v * z, z)
        Y = [dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], *X) + t[r] for r in range(3)]
        a = (fx * u + cx + rng.gauss(0.0, noise_px), fy * v + cy + rng.gauss(0.0, noise_px))
        b = (fx * Y[0] / Y[2] + cx + rng.gauss(0.0, noise_px), fy * Y[1] / Y[2] + cy + rng.gauss(0.0, noise_px))
        if kind == "bad":
            b = (rng.uniform(0.0, 752.0), rng.uniform(0.0, 480.0))
        if kind == "gross":
            b = (b[0] + 30.0, b[1] - 30.0)
        a, b = (f32(a[0]), f32(a[1])), (f32(b[0]), f32(b[1]))
        q["inlier"].append(0 if kind == "bad" else 1)
        q["kp1"].append(a)
        q["kp2"].append(b)
        q["b1"].append(bearing(a, cam))
        q["b2"].append(bearing(b, cam))
    return q


def with_nan(q, which):
    """The scene with the reference keypoint of its `which`-th flagged match not a number."""
    q = dict(q, kp1=list(q["kp1"]))
    i = [k for k, f in enumerate(q["inlier"]) if f][which]
    q["kp1"][i] = (NAN, q["kp1"][i][1])
    return q


def chained_problem(name):
    """What follows tests/test_twoview_ref.py's case `name` in the initialiser: the model the two RANSACs selected there, its matrix and its
    inlier flags (the two-view reference's), over that case's keypoints and their bearings."""
    import test_twoview_ref as tv
    want, q = tv.expected(name), tv.problem(name)
    model = want["selected"]
    cam = (tv.FOCAL, tv.FOCAL, tv.CX, tv.CY)
    return dict(model=model, mat=list(want[model - 1]["M"]), cam=cam, inlier=list(want[model - 1]["flags"]), kp1=list(q["x1"]), kp2=list(q["x2"]),
                b1=[bearing(a, cam) for a in q["x1"]], b2=[bearing(b, cam) for b in q["x2"]])


H, F = ref.MODEL_H, ref.MODEL_F
COUNTS = (0, 1, 50, 51, 52, 63, 64, 65, 129, 200)
# every scene the device tests use
CASES = {}
for _n in COUNTS:
    CASES["h%d" % _n] = functools.partial(scene, H, _n, rng_seed=1 if _n == 200 else 0)
    CASES["f%d" % _n] = functools.partial(scene, F, _n)
CASES.update({
    "empty": functools.partial(scene, F, 0, 0),
    "h_rotation": functools.partial(scene, H, 65, mat=planted(H, rotation(), [0.0, 0.0, 0.0])),   # K R K^-1: three equal singular values
    "h_two_similar": functools.partial(scene, H, 65, half_fov=(0.12, 0.1), plane_n=(0.0, 0.0, 1.0)),
    "h_success": functools.partial(scene, H, 65, plane_n=(1.5, 0.2, 1.0)),   # a plane tilted enough for the mirror solution to lose a fifth of its points
    "f_low_parallax": functools.partial(scene, F, 65, trans_scale=0.25, noise_px=0.05),
    "f_gross": functools.partial(scene, F, 65, n_gross=4),
    "f_nan": lambda: with_nan(scene(F, 50), 7),   # "f50" with one keypoint not a number: 49 triangulated, one short
    "h_noisy": functools.partial(scene, H, 129, noise_px=1.2),
    "f_noisy": functools.partial(scene, F, 129, noise_px=1.2),
})
CHAINED = ["p65", "c129"]                        # cases of tests/test_twoview_ref.py: a plane and a cloud
CASES.update({name: functools.partial(chained_problem, name) for name in CHAINED})
SIZES = ["%s%d" % (m, n) for m in "hf" for n in COUNTS]
FAILING = ["h_rotation", "h_two_similar", "f_low_parallax", "f_nan"]   # (the fifth failing exit is "f65" under min_num_triangulated = 66)
BATCH = ["h65", "empty", "f129", "f0", "h52", "f_gross", "h_rotation", "f63"]
GROW = (["f63"], ["h200", "f129"], ["f63"])      # past the 256 matches' keys a handle is created with, and back
SHIM_CASES = ["h65", "f129"]


@functools.lru_cache(maxsize=None)
def problem(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def solved(name, reproj_err_thr=4.0, parallax_deg_thr=1.0, min_num_triangulated=50):
    """(result, margins, stats, info) of a case: computed once, shared by the CPU and the device tests."""
    margin, stats, info = {}, {}, {}
    r = ref.reconstruct(problem(name), reproj_err_thr, parallax_deg_thr, min_num_triangulated, margin, stats, info)
    return r, margin, stats, info


def expected(name, **params):
    return solved(name, **params)[0]
