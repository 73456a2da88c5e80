"""Time ovs_essential_solve_batch (csrc/essential_solve.hip). Two settings: "product" -- what robust::match_frame_and_keyframe hands over:
1, 4 and 16 problems of 500 matches each, 30 % of them wrong, 50 iterations, no refit -- and "refit" -- 300 matches, 100 iterations, with the
refit, beside ovs_twoview_solve_batch with models = 2 (F alone: the same eight-point problem swept in the sequential ordering) on the same
number of matches in the same process. 50 calls per size, the first 5 dropped; prints the median and the minimum of the WHOLE call (host
clock around the call, which ends in a stream synchronise), on arrays packed once and through the Python mirror. The two kernels alone: run
one size under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_essential.py <setting> <n_problems>` in a
run of its own, then `python tools/time_essential.py --summarise <dir>` prints the median and minimum of every solver kernel in the trace
over the kept dispatches. The host loop: `essential_host scene.bin --time N` on the file `--write-scene <setting> <n_problems> <path>` writes.
Usage (GPU box): python tools/time_essential.py [product | refit] [n_problems ...]"""
import csv
import ctypes as C
import glob
import json
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, DROP = 50, 5
SETTINGS = {"product": dict(matches=500, iters=50, recompute=0), "refit": dict(matches=300, iters=100, recompute=1)}
FOCAL, CX, CY = 458.0, 376.0, 240.0
THR = float(np.float32(0.01745240643))


def problem(rng, matches):
    """A cloud 4 to 9 m away seen from two poses 0.45 m and 0.12 rad apart, half a pixel of noise, 30 % of the matches wrong: the keypoints
    (for the F solver) and their bearings (for the essential solver)."""
    uv = np.stack([rng.uniform(-0.7, 0.7, matches), rng.uniform(-0.45, 0.45, matches)], 1)
    z = rng.uniform(4, 9, matches)
    X = np.concatenate([uv * z[:, None], z[:, None]], 1)
    c, s = np.cos(0.12), np.sin(0.12)
    Y = X @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T + np.array([0.45, -0.05, 0.1])
    x1 = FOCAL * uv + (CX, CY) + rng.normal(0, 0.5, (matches, 2))
    x2 = FOCAL * Y[:, :2] / Y[:, 2:] + (CX, CY) + rng.normal(0, 0.5, (matches, 2))
    wrong = rng.random(matches) < 0.3
    x2[wrong] = np.stack([rng.uniform(0, 752, wrong.sum()), rng.uniform(0, 480, wrong.sum())], 1)
    x1, x2 = x1.astype(np.float32).astype(np.float64), x2.astype(np.float32).astype(np.float64)

    def bearings(x):
        b = np.concatenate([(x - (CX, CY)) / FOCAL, np.ones((matches, 1))], 1)
        return b / np.linalg.norm(b, axis=1, keepdims=True)
    return dict(x1=x1, x2=x2, b1=bearings(x1), b2=bearings(x2))


def problems_of(setting, n_problems, seed=0):
    rng = np.random.default_rng(seed)
    return [problem(rng, SETTINGS[setting]["matches"]) for _ in range(n_problems)]


def write_scene(setting, n_problems, path):
    """The file tests/essential_host.cc reads: the same problems, the same settings, seed 1000."""
    cfg = SETTINGS[setting]
    blob = struct.pack("<diiQi", THR, cfg["iters"], cfg["recompute"], 1000, n_problems)
    for q in problems_of(setting, n_problems):
        blob += struct.pack("<i", len(q["b1"])) + q["b1"].astype("<f8").tobytes() + q["b2"].astype("<f8").tobytes()
    with open(path, "wb") as f:
        f.write(blob)


def run(setting, n_problems):
    from openvslam_amd import _lib, solve
    _lib.require_device()
    cfg = SETTINGS[setting]
    matches, iters, recompute = cfg["matches"], cfg["iters"], cfg["recompute"]
    problems = problems_of(setting, n_problems)
    handle = solve._essential_handle(n_problems, n_problems * matches)
    times, out = [], []
    for k in range(CALLS):
        t = time.perf_counter()
        out = solve.solve_essential_batch(problems, THR, iters, bool(recompute), seed=1000 + k, handle=handle)
        times.append(time.perf_counter() - t)
    # the Python mirror's own packing is inside these times; the ABI call alone, on arrays packed once:
    L = _lib.lib()
    offsets = (np.arange(n_problems + 1) * matches).astype(np.int32)
    cat = lambda key: np.ascontiguousarray(np.concatenate([q[key] for q in problems]))
    b1, b2 = cat("b1"), cat("b2")
    od = [np.zeros(9 * n_problems), np.zeros(n_problems)]
    oi = [np.zeros(n_problems, np.int32) for _ in range(3)]
    fl = np.zeros(n_problems * matches, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    abi = []
    for k in range(CALLS):
        t = time.perf_counter()
        _lib.check(L.ovs_essential_solve_batch(handle._h, n_problems, p(offsets), p(b1), p(b2), THR, iters, recompute, 1000 + k, p(od[0]), p(od[1]),
                                               p(oi[0]), p(oi[1]), p(oi[2]), p(fl)), "ovs_essential_solve_batch")
        abi.append(time.perf_counter() - t)
    us = lambda v: round(v * 1e6, 1)
    row = {"setting": setting, "n_problems": n_problems, "matches_per_problem": matches, "max_num_iter": iters, "recompute": recompute,
           "abi_call_median_us": us(np.median(abi[DROP:])), "abi_call_min_us": us(min(abi[DROP:])), "python_call_median_us": us(np.median(times[DROP:])),
           "python_call_min_us": us(min(times[DROP:])), "valid_last": [int(r["valid"]) for r in out][:4], "inliers_last": [r["num_inliers"] for r in out][:4]}
    if setting == "refit":   # beside it: F alone through ovs_twoview_solve_batch, the sequential ordering on the same number of matches
        h2 = solve._two_view_handle(n_problems, n_problems * matches)
        x1, x2 = cat("x1"), cat("x2")
        d2 = [np.zeros(9 * n_problems), np.zeros(9 * n_problems), np.zeros(2 * n_problems)]
        i2 = [np.zeros(2 * n_problems, np.int32) for _ in range(3)] + [np.zeros(n_problems, np.int32)]
        f2 = [np.zeros(n_problems * matches, np.uint8) for _ in range(2)]
        tv = []
        for k in range(CALLS):
            t = time.perf_counter()
            _lib.check(L.ovs_twoview_solve_batch(h2._h, n_problems, p(offsets), p(x1), p(x2), 1.0, iters, recompute, 1000 + k, 2, p(d2[0]), p(d2[1]),
                                                 p(d2[2]), p(i2[0]), p(i2[1]), p(i2[2]), p(i2[3]), p(f2[0]), p(f2[1])), "ovs_twoview_solve_batch")
            tv.append(time.perf_counter() - t)
        row.update(twoview_F_call_median_us=us(np.median(tv[DROP:])), twoview_F_call_min_us=us(min(tv[DROP:])),
                   twoview_F_inliers_last=[int(v) for v in i2[2][1::2]][:4])
    return row


def summarise(directory):
    """Median / minimum of the solver kernels over a rocprofv3 kernel trace of ONE size: every loop of run() dispatches each of its kernels CALLS
    times; the first DROP of each loop are warm-up."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for kernel in ("k_essential_hypotheses", "k_essential_finish", "k_twoview_hypotheses", "k_twoview_finish"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        kept = [v for i, v in enumerate(d) if i % CALLS >= DROP]
        if kept:
            out[kernel] = {"dispatches": len(d), "kept": len(kept), "median_us": round(float(np.median(kept)), 2), "min_us": round(min(kept), 2)}
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) == 2 and args[0] == "--summarise":
        print(json.dumps(summarise(args[1])), flush=True)
    elif len(args) == 4 and args[0] == "--write-scene":
        write_scene(args[1], int(args[2]), args[3])
    else:
        settings = [a for a in args if a in SETTINGS] or ["product", "refit"]
        sizes = [int(a) for a in args if a not in SETTINGS] or [1, 4, 16]
        for setting in settings:
            for size in sizes:
                print(json.dumps(run(setting, size)), flush=True)
