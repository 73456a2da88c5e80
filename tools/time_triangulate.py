"""Time ovs_triangulate_batch (csrc/triangulate.hip) on what local mapping hands over for one new keyframe -- 1 neighbour of 150 matches, 20 of
150 and 20 of 1000 -- against the only baseline there is: the same algebra as a host loop (openvslam_amd/cpp/triangulate_host, a plain g++
build of csrc/triangulate_math.inc, one core). Per batch: 5 runs of 200 calls each, the first 20 of every run dropped; prints the median, the
minimum and the 90th percentile of the WHOLE ABI call over all kept calls (host clock around the call, which ends in a stream synchronise),
the spread of the five runs' medians, and the host program's median, minimum and 90th percentile of a pass over the same matches.
Usage (GPU box): python tools/time_triangulate.py [--host-only]"""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = ((1, 150), (20, 150), (20, 1000))
RUNS, CALLS, DROP, HOST_PASSES = 5, 200, 20, 200
FX, FY, CX, CY, TRUE_BASELINE = 458.0, 457.0, 367.0, 248.0, 0.11
SCALE_FACTORS = (1.2 ** np.arange(8)).astype(np.float32)
RATIO_FACTOR = float(np.float32(1.5) * np.float32(1.2))
COS_THR = 0.9998476951563913   # cos(1 degree)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def problem(rng, n, stereo):
    """n matches between a stereo (or mono) keyframe and a neighbour 0.3 to 0.9 m away: 0.3 pixels of keypoint noise, a tenth of the matches
    wrong (a keypoint 25 pixels off), points 3 to 12 m away."""
    R1, R2 = rot_y(0.02), rot_y(rng.uniform(-0.08, 0.08))
    C2 = np.array([rng.uniform(0.3, 0.9), rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1)])
    t1, t2 = np.zeros(3), -R2 @ C2
    d = rng.uniform(3.0, 12.0, n)
    X = np.stack([rng.uniform(-0.4, 0.4, n) * d, rng.uniform(-0.25, 0.25, n) * d, d], 1)
    out = dict(pose_cw_1=np.concatenate([R1.ravel(), t1]), pose_cw_2=np.concatenate([R2.ravel(), t2]))
    octave = rng.integers(0, 4, n)
    for side, R, t, st in (("1", R1, t1, stereo), ("2", R2, t2, False)):
        pc = X @ R.T + t
        kp = np.stack([FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY], 1) + rng.normal(0, 0.3, (n, 2))
        wrong = rng.random(n) < 0.05
        kp[wrong, 0] += 25.0
        kp = kp.astype(np.float32)
        b = np.stack([(kp[:, 0].astype(np.float64) - CX) / FX, (kp[:, 1].astype(np.float64) - CY) / FY, np.ones(n)], 1)
        out["bearings_" + side] = b / np.linalg.norm(b, axis=1, keepdims=True)
        out["keypts_" + side] = kp
        out["x_right_" + side] = (kp[:, 0] - FX * TRUE_BASELINE / pc[:, 2]).astype(np.float32) if st else np.full(n, -1.0, np.float32)
        out["depths_" + side] = pc[:, 2].astype(np.float32) if st else np.full(n, -1.0, np.float32)
        out["sigma_sq_" + side] = (SCALE_FACTORS[octave] * SCALE_FACTORS[octave]).astype(np.float32)
        out["scale_factors_" + side] = SCALE_FACTORS[octave]
    out["stereo"] = stereo
    return out


def batch(n_problems, n_matches, seed=0):
    rng = np.random.default_rng(seed)
    return [problem(rng, n_matches, stereo=(p % 2 == 0)) for p in range(n_problems)]


def host_case(problems):
    """The batch as tests/triangulate_host.cc reads it."""
    out = [struct.pack("<dfi", COS_THR, RATIO_FACTOR, len(problems))]
    for q in problems:
        fxb, tb = (float(np.float32(FX * TRUE_BASELINE)), float(np.float32(TRUE_BASELINE))) if q["stereo"] else (0.0, 0.0)
        out.append(struct.pack("<i6d2i", 0, FX, FY, CX, CY, fxb, tb, 752, 480) + struct.pack("<i6d2i", 0, FX, FY, CX, CY, 0.0, 0.0, 752, 480))
        out.append(q["pose_cw_1"].astype("<f8").tobytes() + q["pose_cw_2"].astype("<f8").tobytes() + struct.pack("<i", len(q["x_right_1"])))
        rec = np.zeros(len(q["x_right_1"]), np.dtype([("b", "<f8", 6), ("f", "<f4", 12)]))
        rec["b"][:, :3], rec["b"][:, 3:] = q["bearings_1"], q["bearings_2"]
        rec["f"][:, 0:2], rec["f"][:, 2:4] = q["keypts_1"], q["keypts_2"]
        for k, key in enumerate(("x_right_1", "x_right_2", "depths_1", "depths_2", "sigma_sq_1", "sigma_sq_2", "scale_factors_1", "scale_factors_2")):
            rec["f"][:, 4 + k] = q[key]
        out.append(rec.tobytes())
    return b"".join(out)


def time_host(problems):
    exe = os.path.join(ROOT, "openvslam_amd", "cpp", "triangulate_host")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "triangulate_host"])
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "case.bin")
        with open(path, "wb") as f:
            f.write(host_case(problems))
        return json.loads(subprocess.run([exe, path, "--time", str(HOST_PASSES)], capture_output=True, text=True, check=True).stdout)


def time_device(problems):
    from openvslam_amd import _lib, solve
    _lib.require_device()
    L = _lib.lib()
    P = len(problems)
    offsets = np.zeros(P + 1, np.int32)
    offsets[1:] = np.cumsum([len(q["x_right_1"]) for q in problems])
    T = int(offsets[-1])
    arrays = [np.ascontiguousarray(np.concatenate([q[key] for q in problems]).astype(dt)) for key, dt, _ in solve._TRI_ARRAYS]
    cam = lambda st: solve._lib.Camera(0, 1 if st else 0, FX, FY, CX, CY, float(np.float32(FX * TRUE_BASELINE)) if st else 0.0,
                                       float(np.float32(TRUE_BASELINE)) if st else 0.0, 752, 480)
    cams_1 = (_lib.Camera * P)(*[cam(q["stereo"]) for q in problems])
    cams_2 = (_lib.Camera * P)(*[cam(False) for q in problems])
    poses_1 = np.ascontiguousarray([q["pose_cw_1"] for q in problems])
    poses_2 = np.ascontiguousarray([q["pose_cw_2"] for q in problems])
    pos, status, method, num = np.zeros((T, 3)), np.zeros(T, np.uint8), np.zeros(T, np.uint8), np.zeros(P, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    handle = solve._triangulate_handle(P, T)
    kept, medians = [], []
    for _ in range(RUNS):
        times = []
        for _ in range(CALLS):
            t = time.perf_counter()
            _lib.check(L.ovs_triangulate_batch(handle._h, P, p(offsets), *map(p, arrays), cams_1, cams_2, p(poses_1), p(poses_2), COS_THR, RATIO_FACTOR, p(pos),
                                               p(status), p(method), p(num)), "ovs_triangulate_batch")
            times.append(time.perf_counter() - t)
        kept += times[DROP:]
        medians.append(float(np.median(times[DROP:])))
    ms = lambda v: round(v * 1e3, 4)
    return {"abi_call_median_ms": ms(np.median(kept)), "abi_call_min_ms": ms(min(kept)), "abi_call_p90_ms": ms(np.percentile(kept, 90)),
            "run_medians_ms": [ms(m) for m in medians], "accepted": int(num.sum()), "methods": np.bincount(method, minlength=4).tolist()}


if __name__ == "__main__":
    for n_problems, n_matches in BATCHES:
        problems = batch(n_problems, n_matches)
        row = {"n_problems": n_problems, "matches_per_problem": n_matches, "host_loop": time_host(problems)}
        if "--host-only" not in sys.argv:
            row["device"] = time_device(problems)
        print(json.dumps(row), flush=True)
