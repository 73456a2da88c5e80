"""Two-view scenes for solve::essential_solver and their files: what tests/essential_host.cc and the C++ class's program
(openvslam_amd/cpp/test_essential_shim.cc) read, and what they write.

A problem is a dict: b1, b2 (lists of 3-tuples: the bearing of the match's keypoint in frame 1 and in frame 2)."""
import math
import random
import struct

import numpy as np

# the second camera's pose: a rotation about (0.2, 1, 0.1) and a sideways step
ANGLE, AXIS, TRANS = 0.12, (0.2, 1.0, 0.1), (0.45, -0.05, 0.1)


def rotation(angle=ANGLE, axis=AXIS):
    nrm = math.sqrt(sum(v * v for v in axis))
    x, y, z = (v / nrm for v in axis)
    c, s = math.cos(angle), math.sin(angle)
    k = 1.0 - c
    return [c + x * x * k, x * y * k - z * s, x * z * k + y * s, y * x * k + z * s, c + y * y * k, y * z * k - x * s, z * x * k - y * s, z * y * k + x * s,
            c + z * z * k]


def planted():
    """E_21 = [t]x R: b2^T E_21 b1 = 0 for the exact scenes."""
    R, t = np.array(rotation()).reshape(3, 3), np.array(TRANS)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return tx @ R


def _unit(v):
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / n, v[1] / n, v[2] / n)


def scene(n, noise_deg=0.1, outlier_fraction=0.3, rng_seed=0, zero_baseline=False, all_equal=None):
    """n matches of two views of a cloud 4 to 9 m in front of camera 1 (a wide field of view: bearings, not pixels): each bearing with
    Gaussian noise of `noise_deg` degrees, `outlier_fraction` of the matches with a random bearing in frame 2. zero_baseline: the second
    camera only rotates; all_equal: that one bearing everywhere."""
    rng = random.Random(7000 * n + rng_seed)
    R = rotation()
    t = (0.0, 0.0, 0.0) if zero_baseline else TRANS
    sigma = noise_deg * math.pi / 180.0
    outliers = set(rng.sample(range(n), int(outlier_fraction * n)))
    noisy = lambda b: _unit(tuple(v + rng.gauss(0.0, sigma) for v in b)) if sigma > 0.0 else b
    b1, b2 = [], []
    for i in range(n):
        z = rng.uniform(4.0, 9.0)
        X = (rng.uniform(-1.2, 1.2) * z, rng.uniform(-0.8, 0.8) * z, z)
        Y = tuple((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2] + t[r] for r in range(3))
        a, b = noisy(_unit(X)), noisy(_unit(Y))
        if i in outliers:
            b = _unit((rng.uniform(-1.2, 1.2), rng.uniform(-0.8, 0.8), 1.0))
        b1.append(a)
        b2.append(b)
    if all_equal is not None:
        b1 = [tuple(all_equal)] * n
        b2 = [tuple(all_equal)] * n
    return dict(b1=b1, b2=b2)


def write_scene(path, problems, residual_cos_thr, max_num_iter, recompute, seed):
    """scene.bin (little endian): f64 residual_cos_thr, i32 max_num_iter, recompute, u64 seed, i32 n_problems; per problem i32 n, 3 n f64
    bearings of frame 1, 3 n f64 bearings of frame 2 (match i pairs bearing i of both; the C++ program stores frame 2's in reverse and
    matches across)."""
    blob = struct.pack("<diiQi", residual_cos_thr, max_num_iter, int(recompute), seed, len(problems))
    for q in problems:
        n = len(q["b1"])
        blob += struct.pack("<i", n) + np.asarray(q["b1"], "<f8").reshape(n, 3).tobytes() + np.asarray(q["b2"], "<f8").reshape(n, 3).tobytes()
    path.write_bytes(blob)


def read_results(path, sizes):
    """out.bin of test_essential_shim: every problem through the class on its own ("single"), then all of them through one
    find_via_ransac_batch ("batch"). Per problem: i32 valid, best_iter, num_inliers, f64 score, 9 f64 E_21, i32 n, n u8 flags. Returns
    {"single": [...], "batch": [...]}, the doubles as bit patterns."""
    raw = path.read_bytes()
    at = 0
    out = {}
    for run in ("single", "batch"):
        out[run] = []
        for size in sizes:
            valid, best_iter, num = struct.unpack_from("<iii", raw, at)
            score, = struct.unpack_from("<Q", raw, at + 12)
            E = list(struct.unpack_from("<9Q", raw, at + 20))
            (n,) = struct.unpack_from("<i", raw, at + 92)
            assert n == size
            at += 96
            out[run].append(dict(valid=valid, best_iter=best_iter, num_inliers=num, score=score, E=E, flags=list(raw[at:at + n])))
            at += n
    assert at == len(raw)
    return out


def read_host(text):
    """What essential_host prints, per problem, the doubles as bit patterns."""
    out = []
    lines = text.splitlines()
    for head, flags in zip(lines[0::2], lines[1::2]):
        h, f = head.split(), flags.split()
        assert h[0] == "P" and f[0] == "F"
        out.append(dict(valid=int(h[1]), best_iter=int(h[2]), num_inliers=int(h[3]), score=int(h[4], 16), E=[int(v, 16) for v in h[5:14]],
                        flags=[int(v) for v in f[1:]]))
    return out
