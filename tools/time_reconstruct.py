"""Time ovs_reconstruct_batch (csrc/two_view_reconstruct.hip) on 1 and 16 problems of 300 matches each, 30 % of them not inliers, for a plane
with its planted homography (eight hypotheses) and for a cloud with its planted fundamental matrix (four) -- what the monocular initialiser
hands over after its two RANSACs for one frame (one problem) or for several frame pairs. 50 calls per size, the first 5 dropped; prints the
median and the minimum of the WHOLE call (host clock around the ABI call, which ends in a stream synchronise) on arrays packed once, and
the same algebra as a host loop: cpp/reconstruct_host (tests/reconstruct_host.cc, built from csrc/reconstruct_math.inc) over the same
problems. The two kernels alone: run one size under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_reconstruct.py <model> <n_problems>` in a run of its own,
then `python tools/time_reconstruct.py --summarise <dir>` prints the median and minimum of k_reconstruct_hypotheses and k_reconstruct_finish
over the same 45 dispatches.
Usage (GPU box): python tools/time_reconstruct.py [H|F n_problems]"""
import csv
import ctypes as C
import glob
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
from openvslam_amd import _lib, solve

MATCHES, CALLS, DROP = 300, 50, 5
CAM = (458.654, 457.296, 367.215, 248.375)
HOST = os.path.join(ROOT, "openvslam_amd", "cpp", "reconstruct_host")


def problem(rng, model):
    """300 matches of a plane 6 m away, or of a cloud 4 to 9 m away, seen from two poses 0.45 m and 0.12 rad apart, 0.3 pixels of noise;
    30 % of the matches are wrong and carry no inlier flag. The matrix is the planted one."""
    fx, fy, cx, cy = CAM
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    uv = np.stack([rng.uniform(-0.7, 0.7, MATCHES), rng.uniform(-0.45, 0.45, MATCHES)], 1)
    c, s = np.cos(0.12), np.sin(0.12)
    R, t, n, d = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.array([0.45, -0.05, 0.1]), np.array([1.5, 0.2, 1.0]), 6.0
    z = d / (uv @ n[:2] + n[2]) if model == solve.MODEL_H else rng.uniform(4, 9, MATCHES)
    X = np.concatenate([uv * z[:, None], z[:, None]], 1)
    Y = X @ R.T + t
    x1 = uv * (fx, fy) + (cx, cy) + rng.normal(0, 0.3, (MATCHES, 2))
    x2 = Y[:, :2] / Y[:, 2:] * (fx, fy) + (cx, cy) + rng.normal(0, 0.3, (MATCHES, 2))
    wrong = rng.random(MATCHES) < 0.3
    x2[wrong] = np.stack([rng.uniform(0, 752, wrong.sum()), rng.uniform(0, 480, wrong.sum())], 1)
    x1, x2 = x1.astype(np.float32).astype(np.float64), x2.astype(np.float32).astype(np.float64)
    Kinv = np.linalg.inv(K)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    mat = K @ (R + np.outer(t, n) / d) @ Kinv if model == solve.MODEL_H else Kinv.T @ tx @ R @ Kinv
    cam = solve.camera(0, *CAM)
    return solve.reconstruct_problem(model, mat, cam, (~wrong).astype(np.uint8), x1, x2, solve.bearings_of(x1, cam), solve.bearings_of(x2, cam))


def host_loop(problems):
    """The same problems through the stand-alone host program: the median and the minimum of a pass over them, in microseconds."""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(HOST), "reconstruct_host"])
    blob = [struct.pack("<ffii", 4.0, 1.0, 50, len(problems))]
    for q in problems:
        blob.append(struct.pack("<i9d4di", q["model"], *q["mat"].ravel(), *CAM, len(q["inlier"])))
        for i in range(len(q["inlier"])):
            blob.append(struct.pack("<B10d", int(q["inlier"][i]), *q["kp_ref"][i], *q["kp_cur"][i], *q["b_ref"][i], *q["b_cur"][i]))
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(b"".join(blob))
        f.flush()
        r = json.loads(subprocess.run([HOST, f.name, "--time", str(CALLS - DROP)], capture_output=True, text=True, check=True).stdout)
    return {"host_loop_median_us": round(r["median_ms"] * 1e3, 1), "host_loop_min_us": round(r["min_ms"] * 1e3, 1), "host_succeeded": r["succeeded_per_pass"]}


def run(model, n_problems, seed=0):
    _lib.require_device()
    rng = np.random.default_rng(seed)
    problems = [problem(rng, model) for _ in range(n_problems)]
    handle = solve._reconstruct_handle(n_problems, n_problems * MATCHES)
    out = solve.reconstruct_two_view_batch(problems, handle=handle)
    L = _lib.lib()
    P, T = n_problems, n_problems * MATCHES
    offsets = (np.arange(P + 1) * MATCHES).astype(np.int32)
    cat = lambda key: np.ascontiguousarray(np.concatenate([q[key] for q in problems]))
    arrays = [cat(k) for k in ("inlier", "kp_ref", "kp_cur", "b_ref", "b_cur")]
    models, mats = np.full(P, model, np.int32), np.ascontiguousarray([q["mat"] for q in problems])
    cams = (_lib.Camera * P)(*[q["cam"] for q in problems])
    success, best, rot, trans = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros((P, 9)), np.zeros((P, 3))
    counts, parallax, pts, flags = np.zeros((P, 8), np.int32), np.zeros((P, 8), np.float32), np.zeros((T, 3)), np.zeros(T, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    abi = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        _lib.check(L.ovs_reconstruct_batch(handle._h, P, p(offsets), p(models), p(mats), cams, *map(p, arrays), 4.0, 1.0, 50, p(success), p(best), p(rot),
                                           p(trans), p(counts), p(parallax), p(pts), p(flags)), "ovs_reconstruct_batch")
        abi.append(time.perf_counter() - t0)
    us = lambda v: round(v * 1e6, 1)
    res = {"model": "H" if model == solve.MODEL_H else "F", "n_problems": P, "matches_per_problem": MATCHES, "abi_call_median_us": us(np.median(abi[DROP:])),
           "abi_call_min_us": us(min(abi[DROP:])), "succeeded": int(success.sum()), "succeeded_python": sum(r["success"] for r in out),
           "triangulated_first": int(counts[0].max())}
    res.update(host_loop(problems))
    return res


def summarise(directory):
    """Median / minimum of the two kernels over a rocprofv3 kernel trace of ONE size: run() dispatches each kernel once through the Python
    mirror and then CALLS times; the first 1 + DROP are warm-up."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for kernel in ("k_reconstruct_hypotheses", "k_reconstruct_finish"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        kept = d[1 + DROP:]
        out[kernel] = {"dispatches": len(d), "kept": len(kept), "median_us": round(float(np.median(kept)), 2), "min_us": round(min(kept), 2)}
    return out


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        print(json.dumps(summarise(sys.argv[2])), flush=True)
    elif len(sys.argv) == 3:
        print(json.dumps(run(solve.MODEL_H if sys.argv[1] == "H" else solve.MODEL_F, int(sys.argv[2]))), flush=True)
    else:
        for model in (solve.MODEL_H, solve.MODEL_F):
            for size in (1, 16):
                print(json.dumps(run(model, size)), flush=True)
