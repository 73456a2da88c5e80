"""Time ovs_pnp_solve_batch (csrc/pnp_solve.hip) on 1, 4 and 16 relocalisation candidates of 100 matches each at 30 iterations with the refit -- what
the relocaliser hands over for one lost frame. 50 calls per size, the first 5 dropped; prints the median and the minimum of the WHOLE call
(host clock around the call, which ends in a stream synchronise), on arrays packed once and through the Python mirror. The two kernels alone:
run one size under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_pnp.py <n_problems>` in a run of its own, then
`python tools/time_pnp.py --summarise <dir>` prints the median and minimum of k_pnp_hypotheses and k_pnp_finish over the same 45 + 45 dispatches.
Usage (GPU box): python tools/time_pnp.py [n_problems ...]"""
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

MATCHES, ITERS, CALLS, DROP = 100, 30, 50, 5


def problem(rng):
    """100 matches, 30 % of them wrong, half a pixel of noise at f = 458, a pose of 0.4 rad."""
    pc = np.stack([rng.uniform(-3, 3, MATCHES), rng.uniform(-2, 2, MATCHES), rng.uniform(4, 9, MATCHES)], 1)
    c, s = np.cos(0.4), np.sin(0.4)
    R, t = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.array([0.3, -0.2, 0.5])
    pos_w = (pc - t) @ R
    seen = pc.copy()
    wrong = rng.random(MATCHES) < 0.3
    seen[wrong] = np.stack([rng.uniform(-3, 3, wrong.sum()), rng.uniform(-2, 2, wrong.sum()), rng.uniform(4, 9, wrong.sum())], 1)
    uv = seen[:, :2] / seen[:, 2:] + rng.normal(0, 0.5 / 458.0, (MATCHES, 2))
    bearings = np.concatenate([uv, np.ones((MATCHES, 1))], 1)
    bearings /= np.linalg.norm(bearings, axis=1, keepdims=True)
    scale_factors = (1.2 ** np.arange(8)).astype(np.float32)
    return solve.pnp_problem(bearings, rng.integers(0, 8, MATCHES), pos_w, scale_factors)


def run(n_problems, seed=0):
    _lib.require_device()
    rng = np.random.default_rng(seed)
    problems = [problem(rng) for _ in range(n_problems)]
    handle = solve._pnp_handle(n_problems, n_problems * MATCHES)
    times, valid, inliers = [], 0, []
    for k in range(CALLS):
        t = time.perf_counter()
        out = solve.solve_pnp_batch(problems, 10, ITERS, True, seed=1000 + k, handle=handle)
        times.append(time.perf_counter() - t)
        valid = sum(r["valid"] for r in out)
        inliers = [r["num_inliers"] for r in out]
    # the Python mirror's own packing is inside these times; the ABI call alone, on arrays packed once:
    L = _lib.lib()
    offsets = (np.arange(n_problems + 1) * MATCHES).astype(np.int32)
    cat = lambda key: np.ascontiguousarray(np.concatenate([q[key] for q in problems]).astype(np.float64))
    bearings, pos_w, max_cos = cat("bearings"), cat("pos_w"), cat("max_cos_error")
    oi = [np.zeros(n_problems, np.int32) for _ in range(3)]
    od = [np.zeros(9 * n_problems) for _ in range(2)]
    fl = np.zeros(n_problems * MATCHES, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    abi = []
    for k in range(CALLS):
        t = time.perf_counter()
        _lib.check(L.ovs_pnp_solve_batch(handle._h, n_problems, p(offsets), p(bearings), p(pos_w), p(max_cos), 10, ITERS, 1, 1000 + k, p(oi[0]), p(oi[1]),
                                         p(oi[2]), p(od[0]), p(od[1]), p(fl)), "ovs_pnp_solve_batch")
        abi.append(time.perf_counter() - t)
    us = lambda v: round(v * 1e6, 1)
    return {"n_problems": n_problems, "matches_per_problem": MATCHES, "max_num_iter": ITERS, "abi_call_median_us": us(np.median(abi[DROP:])),
            "abi_call_min_us": us(min(abi[DROP:])), "python_call_median_us": us(np.median(times[DROP:])), "python_call_min_us": us(min(times[DROP:])),
            "valid_last": valid, "inliers_last": inliers[:4]}


def summarise(directory):
    """Median / minimum of the two kernels over a rocprofv3 kernel trace of ONE size: both loops of run() dispatch each kernel CALLS times; the
    first DROP of each loop are warm-up."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for kernel in ("k_pnp_hypotheses", "k_pnp_finish"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        kept = [v for i, v in enumerate(d) if i % CALLS >= DROP]
        out[kernel] = {"dispatches": len(d), "kept": len(kept), "median_us": round(float(np.median(kept)), 2), "min_us": round(min(kept), 2)}
    return out


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        print(json.dumps(summarise(sys.argv[2])), flush=True)
    else:
        for size in [int(a) for a in sys.argv[1:]] or [1, 4, 16]:
            print(json.dumps(run(size)), flush=True)
