"""Time ovs_sim3opt_optimize_batch (csrc/sim3_opt.hip) on 1, 4 and 16 loop candidates of 150 matches each -- what a loop detector hands over for
one keyframe. 50 calls per size, the first 5 dropped; prints the median and the minimum of the WHOLE call (host clock around the call,
which ends in a stream synchronise). The kernel alone: run one size under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_transform.py <n_problems>` in a run of its own, then
`python tools/time_transform.py --summarise <dir>` prints the median and minimum of k_sim3_optimize over the same 45 + 45 dispatches.
Usage (GPU box): python tools/time_transform.py [n_problems ...]"""
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openvslam_amd import _lib, solve

MATCHES, NUM_ITER, CHI_SQ, CALLS, DROP = 150, 10, 10.0, 50, 5
FX, FY, CX, CY = 458.0, 457.0, 367.0, 248.0


def problem(rng):
    """150 matches, 20 % of them wrong, 0.7 pixels of keypoint noise, a Sim3 of 0.4 rad and scale 1.7 between the sides; the start is 1.5
    degrees, a few centimetres and 3 % of scale off."""
    p2 = np.stack([rng.uniform(-3, 3, MATCHES), rng.uniform(-2, 2, MATCHES), rng.uniform(4, 9, MATCHES)], 1)
    c, s = np.cos(0.4), np.sin(0.4)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = np.array([0.3, -0.2, 0.5])
    p1 = 1.7 * p2 @ R.T + t
    wrong = rng.random(MATCHES) < 0.2
    p1[wrong] = 1.7 * np.stack([rng.uniform(-3, 3, wrong.sum()), rng.uniform(-2, 2, wrong.sum()), rng.uniform(4, 9, wrong.sum())], 1)
    proj = lambda p: np.stack([FX * p[:, 0] / p[:, 2] + CX, FY * p[:, 1] / p[:, 2] + CY], 1)
    inv_sigma_sq = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)
    w = lambda: inv_sigma_sq[rng.integers(0, 8, MATCHES)]
    cam = solve.camera(0, FX, FY, CX, CY)
    a = 0.027
    dR = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return dict(p1=p1, p2=p2, obs1=(proj(p1) + rng.normal(0, 0.7, (MATCHES, 2))).astype(np.float32).astype(np.float64),
                obs2=(proj(p2) + rng.normal(0, 0.7, (MATCHES, 2))).astype(np.float32).astype(np.float64), w1=w(), w2=w(), cam_1=cam, cam_2=cam,
                R=dR @ R, t=t + np.array([0.05, -0.03, 0.04]), s=1.75)


def run(n_problems, seed=0):
    _lib.require_device()
    rng = np.random.default_rng(seed)
    problems = [problem(rng) for _ in range(n_problems)]
    handle = solve._transform_handle(n_problems, n_problems * MATCHES)
    times, inliers, info = [], [], []
    for k in range(CALLS):
        t = time.perf_counter()
        out = solve.optimize_transform_batch(problems, False, CHI_SQ, NUM_ITER, handle=handle)
        times.append(time.perf_counter() - t)
        inliers = [r["num_inliers"] for r in out]
        info = [[int(r["info"][0] + r["info"][4]), int(r["info"][1] + r["info"][5])] for r in out]
    # the Python mirror's own packing is inside these times; the ABI call alone, on arrays packed once:
    L = _lib.lib()
    offsets = (np.arange(n_problems + 1) * MATCHES).astype(np.int32)
    cat = lambda key, dt: np.ascontiguousarray(np.concatenate([q[key] for q in problems]).astype(dt))
    arrays = [cat(k, np.float64) for k in ("p1", "p2", "obs1", "obs2")] + [cat(k, np.float32) for k in ("w1", "w2")]
    cams = (_lib.Camera * n_problems)(*[q["cam_1"] for q in problems])
    rot, trans = np.ascontiguousarray([q["R"] for q in problems]), np.ascontiguousarray([q["t"] for q in problems])
    scale = np.array([q["s"] for q in problems])
    num, od = np.zeros(n_problems, np.int32), [np.zeros(9 * n_problems) for _ in range(4)]
    fl = np.zeros(n_problems * MATCHES, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    abi = []
    for k in range(CALLS):
        t = time.perf_counter()
        _lib.check(L.ovs_sim3opt_optimize_batch(handle._h, n_problems, p(offsets), *map(p, arrays), cams, cams, p(rot), p(trans), p(scale), 0, CHI_SQ, NUM_ITER,
                                                p(num), p(od[0]), p(od[1]), p(od[2]), p(fl), p(od[3])), "ovs_sim3opt_optimize_batch")
        abi.append(time.perf_counter() - t)
    us = lambda v: round(v * 1e6, 1)
    return {"n_problems": n_problems, "matches_per_problem": MATCHES, "num_iter": NUM_ITER, "abi_call_median_us": us(np.median(abi[DROP:])),
            "abi_call_min_us": us(min(abi[DROP:])), "python_call_median_us": us(np.median(times[DROP:])), "python_call_min_us": us(min(times[DROP:])),
            "inliers_last": inliers[:4], "iterations_trials_last": info[:4]}


def summarise(directory):
    """Median / minimum of the kernel over a rocprofv3 kernel trace of ONE size: both loops of run() dispatch it CALLS times; the first DROP of
    each loop are warm-up."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_sim3_optimize" in r["Kernel_Name"]]
    kept = [v for i, v in enumerate(d) if i % CALLS >= DROP]
    return {"k_sim3_optimize": {"dispatches": len(d), "kept": len(kept), "median_us": round(float(np.median(kept)), 2), "min_us": round(min(kept), 2)}}


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        print(json.dumps(summarise(sys.argv[2])), flush=True)
    else:
        for size in [int(a) for a in sys.argv[1:]] or [1, 4, 16]:
            print(json.dumps(run(size)), flush=True)
