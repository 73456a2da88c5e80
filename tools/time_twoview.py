"""Time ovs_twoview_solve_batch (csrc/two_view_solve.hip) on 1, 4 and 16 problems of 300 matches each, 30 % of them wrong, at 100 iterations, both
models, with the refit -- what the monocular initialiser hands over for one frame (one problem) or for several frame pairs. 50 calls per
size, the first 5 dropped; prints the median and the minimum of the WHOLE call (host clock around the call, which ends in a stream
synchronise), on arrays packed once and through the Python mirror. The two kernels alone: run one size under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_twoview.py <n_problems>` in a run of its own, then
`python tools/time_twoview.py --summarise <dir>` prints the median and minimum of k_twoview_hypotheses and k_twoview_finish over the same
45 + 45 dispatches. The host's two threads (upstream's H + F) are not timed here: this tree holds no host form of the two solvers.
Usage (GPU box): python tools/time_twoview.py [n_problems ...]"""
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

MATCHES, ITERS, CALLS, DROP = 300, 100, 50, 5
FOCAL, CX, CY = 458.0, 376.0, 240.0


def problem(rng):
    """300 matches of a cloud 4 to 9 m away seen from two poses 0.45 m and 0.12 rad apart, half a pixel of noise, 30 % of them wrong."""
    uv = np.stack([rng.uniform(-0.7, 0.7, MATCHES), rng.uniform(-0.45, 0.45, MATCHES)], 1)
    z = rng.uniform(4, 9, MATCHES)
    X = np.concatenate([uv * z[:, None], z[:, None]], 1)
    c, s = np.cos(0.12), np.sin(0.12)
    Y = X @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T + np.array([0.45, -0.05, 0.1])
    x1 = FOCAL * uv + (CX, CY) + rng.normal(0, 0.5, (MATCHES, 2))
    x2 = FOCAL * Y[:, :2] / Y[:, 2:] + (CX, CY) + rng.normal(0, 0.5, (MATCHES, 2))
    wrong = rng.random(MATCHES) < 0.3
    x2[wrong] = np.stack([rng.uniform(0, 752, wrong.sum()), rng.uniform(0, 480, wrong.sum())], 1)
    return dict(x1=x1.astype(np.float32).astype(np.float64), x2=x2.astype(np.float32).astype(np.float64))


def run(n_problems, seed=0):
    _lib.require_device()
    rng = np.random.default_rng(seed)
    problems = [problem(rng) for _ in range(n_problems)]
    handle = solve._two_view_handle(n_problems, n_problems * MATCHES)
    times, out = [], []
    for k in range(CALLS):
        t = time.perf_counter()
        out = solve.solve_two_view_batch(problems, 1.0, ITERS, True, seed=1000 + k, handle=handle)
        times.append(time.perf_counter() - t)
    # the Python mirror's own packing is inside these times; the ABI call alone, on arrays packed once:
    L = _lib.lib()
    offsets = (np.arange(n_problems + 1) * MATCHES).astype(np.int32)
    cat = lambda key: np.ascontiguousarray(np.concatenate([q[key] for q in problems]))
    x1, x2 = cat("x1"), cat("x2")
    od = [np.zeros(9 * n_problems), np.zeros(9 * n_problems), np.zeros(2 * n_problems)]
    oi = [np.zeros(2 * n_problems, np.int32) for _ in range(3)] + [np.zeros(n_problems, np.int32)]
    fl = [np.zeros(n_problems * MATCHES, np.uint8) for _ in range(2)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    abi = []
    for k in range(CALLS):
        t = time.perf_counter()
        _lib.check(L.ovs_twoview_solve_batch(handle._h, n_problems, p(offsets), p(x1), p(x2), 1.0, ITERS, 1, 1000 + k, 3, p(od[0]), p(od[1]), p(od[2]),
                                             p(oi[0]), p(oi[1]), p(oi[2]), p(oi[3]), p(fl[0]), p(fl[1])), "ovs_twoview_solve_batch")
        abi.append(time.perf_counter() - t)
    us = lambda v: round(v * 1e6, 1)
    return {"n_problems": n_problems, "matches_per_problem": MATCHES, "max_num_iter": ITERS, "abi_call_median_us": us(np.median(abi[DROP:])),
            "abi_call_min_us": us(min(abi[DROP:])), "python_call_median_us": us(np.median(times[DROP:])), "python_call_min_us": us(min(times[DROP:])),
            "selected_last": [r["selected"] for r in out][:4], "inliers_F_last": [r["F"]["num_inliers"] for r in out][:4]}


def summarise(directory):
    """Median / minimum of the two kernels over a rocprofv3 kernel trace of ONE size: both loops of run() dispatch each kernel CALLS times; the
    first DROP of each loop are warm-up."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for kernel in ("k_twoview_hypotheses", "k_twoview_finish"):
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
