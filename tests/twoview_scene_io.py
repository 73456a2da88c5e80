"""Scene files for the C++ classes solve::homography_solver and solve::fundamental_solver (openvslam_amd/cpp/test_twoview_shim.cc): what the
monocular initialiser hands their constructors -- the undistorted keypoints of both frames and the matches -- and the result file.

A problem is a dict: x1, x2 (lists of 2-tuples whose values are exact in f32, as a cv::KeyPoint holds them)."""
import struct

import numpy as np

H, F = 0, 1


def write_scene(path, problems, sigma, max_num_iter, recompute, seed):
    """scene.bin (little endian): f32 sigma, i32 max_num_iter, recompute, u64 seed, i32 n_problems; per problem i32 n, 2 n f32 keypoints of
    frame 1, 2 n f32 keypoints of frame 2 (match i pairs keypoint i of both; the program stores frame 2's in reverse and matches across)."""
    blob = struct.pack("<fiiQi", sigma, max_num_iter, int(recompute), seed, len(problems))
    for q in problems:
        n = len(q["x1"])
        a, b = np.asarray(q["x1"], np.float64).reshape(n, 2), np.asarray(q["x2"], np.float64).reshape(n, 2)
        assert np.array_equal(a.astype("<f4").astype(np.float64), a) and np.array_equal(b.astype("<f4").astype(np.float64), b)
        blob += struct.pack("<i", n) + a.astype("<f4").tobytes() + b.astype("<f4").tobytes()
    path.write_bytes(blob)


def read_results(path, sizes):
    """out.bin: every problem through the two classes one by one ("single"), then all of them through one both-models call ("both"). Per
    problem: for H, then F: i32 valid, best_iter, num_inliers, f64 score, 9 f64 matrix, i32 n, n u8 flags; then i32 selected (0 in the
    single runs, whose classes make no choice). Returns {"single": [...], "both": [...]} of {H:, F:, "selected":}, the doubles as bit
    patterns."""
    raw = path.read_bytes()
    at = 0
    out = {}
    for run in ("single", "both"):
        out[run] = []
        for size in sizes:
            r = {}
            for m in (H, F):
                valid, best_iter, num = struct.unpack_from("<iii", raw, at)
                score, = struct.unpack_from("<Q", raw, at + 12)
                M = list(struct.unpack_from("<9Q", raw, at + 20))
                (n,) = struct.unpack_from("<i", raw, at + 92)
                assert n == size
                at += 96
                r[m] = dict(valid=valid, best_iter=best_iter, num_inliers=num, score=score, M=M, flags=list(raw[at:at + n]))
                at += n
            (r["selected"],) = struct.unpack_from("<i", raw, at)
            at += 4
            out[run].append(r)
    assert at == len(raw)
    return out


def as_bits(result):
    """A reference result ({H:, F:, "selected":}) in read_results' shape."""
    bits = lambda x: struct.unpack("<Q", struct.pack("<d", x))[0]
    out = {"selected": result["selected"]}
    for m in (H, F):
        r = result[m]
        out[m] = dict(valid=r["valid"], best_iter=r["best_iter"], num_inliers=r["num_inliers"], score=bits(r["score"]), M=[bits(v) for v in r["M"]],
                      flags=list(r["flags"]))
    return out
