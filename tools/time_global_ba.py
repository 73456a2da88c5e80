"""Time ovs_global_ba_optimize (csrc/ba_optimize.hip with the conjugate gradient of csrc/ba_pcg.hip) on rings of 100, 170, 256 and 512 free
keyframes plus one fixed (and, asked for by size, of 1024: the capacity; pass --no-host there): synth_local_ba with seed 5, noise 0.02, 25 landmarks and 100 observations per keyframe, num_iter = 10. Per size:
the WHOLE call (host clock around the ABI call; the arrays are packed once) with solver 0 (by size), 2 (conjugate gradient) and 1 (Cholesky,
where it fits), the LM iterations and trials, the solver's iterations per solve, and what the parent offers for the same input:
ovs_local_ba_optimize(10, 0), which takes the device Cholesky up to 170 free keyframes and its host path beyond. The first call of every
form is dropped, except where a call runs for many seconds (the host path beyond 170: one call, kept). Nothing is gated: the figures go to
profiles/global_ba_times.json (or --out PATH) as found.
The kernels alone: run one size under `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/time_global_ba.py --pcg-only N`
in a run of its own, then `python tools/time_global_ba.py --summarise <dir> N` merges, per k_pcg_* kernel, the dispatch count and the median
and minimum duration, and the median start-to-start distance of consecutive k_pcg_product dispatches (one iteration with its two kernel
boundaries) into the JSON.
Usage (GPU box): python tools/time_global_ba.py [--out PATH] [--no-host] [N ...]"""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "global_ba_times.json")
NUM_ITER = 10
CHOLESKY_MAX_FREE = 170


def scene(n_free):
    from openvslam_amd.synth import synth_local_ba
    n = n_free + 1
    return synth_local_ba(n_pose=n, n_pt=25 * n, obs_per_pose=100, seed=5, pose_noise=0.02, point_noise=0.02, n_fixed=1)


def timed(fn, calls, drop_first=True):
    times, res = [], None
    for _ in range(calls):
        t0 = time.perf_counter()
        res = fn()
        times.append(time.perf_counter() - t0)
    kept = times[1:] if drop_first and len(times) > 1 else times
    return res, {"calls_kept": len(kept), "median_ms": round(float(np.median(kept)) * 1e3, 3), "min_ms": round(min(kept) * 1e3, 3)}


def run(n_free, with_host=True, pcg_only=False):
    from openvslam_amd import _lib, ba
    _lib.require_device()
    d = scene(n_free)
    hm, hs = ba.huber_deltas(0)
    args = (d["poses"], d["pose_fixed"], d["points"], d["edges"], d["cam"], None, 0.0)
    row = {"free_keyframes": n_free, "landmarks": len(d["points"]), "edges": len(d["edges"]), "num_iter": NUM_ITER}
    res, row["pcg"] = timed(lambda: ba.global_ba_optimize(*args, hm, hs, NUM_ITER, ba.SOLVER_PCG), 3 if pcg_only else 5)
    info = res["info"]
    row.update(lm_iterations=int(info[2]), trials=int(info[3]), pcg_iterations=int(info[5]), pcg_iterations_per_solve=round(info[5] / max(info[3], 1), 1),
               pcg_capped=int(info[6]), failed_solves=int(info[7]), chi_initial=float(info[0]), chi_final=float(info[1]))
    if pcg_only:
        return row
    by_size, row["by_size"] = timed(lambda: ba.global_ba_optimize(*args, hm, hs, NUM_ITER, ba.SOLVER_BY_SIZE), 5)
    row["by_size"]["solver"] = int(by_size["info"][4])
    if n_free <= CHOLESKY_MAX_FREE:
        chol, row["cholesky"] = timed(lambda: ba.global_ba_optimize(*args, hm, hs, NUM_ITER, ba.SOLVER_CHOLESKY), 5)
        row["pcg_vs_cholesky_max_abs"] = float(max(np.abs(chol["poses"] - res["poses"]).max(), np.abs(chol["points"] - res["points"]).max()))
        row["cholesky_trials"] = int(chol["info"][3])
    if n_free <= CHOLESKY_MAX_FREE or with_host:
        device = n_free <= CHOLESKY_MAX_FREE
        loc, row["local_ba_10_0"] = timed(lambda: ba.local_ba_optimize(*args, NUM_ITER, 0), 5 if device else 1, drop_first=device)
        row["local_ba_10_0"]["path"] = "device Cholesky" if device else "host"
        row["pcg_vs_local_ba_max_abs"] = float(max(np.abs(loc["poses"] - res["poses"]).max(), np.abs(loc["points"] - res["points"]).max()))
    return row


def summarise(directory, n_free):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for name in ("k_pcg_init", "k_pcg_product", "k_pcg_update", "k_pcg_finish"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if d:
            out[name] = {"dispatches": len(d), "median_us": round(float(np.median(d)), 2), "min_us": round(min(d), 2)}
    starts = [int(r["Start_Timestamp"]) for r in rows if "k_pcg_product" in r["Kernel_Name"]]
    gaps = np.diff(starts) / 1e3 if len(starts) > 1 else np.zeros(0)
    if len(gaps):
        out["product_start_to_start_median_us"] = round(float(np.median(gaps)), 2)
    return {"free_keyframes": n_free, "kernels": out}


def merge(row, out):
    data = json.load(open(out)) if os.path.exists(out) else {"sizes": {}}
    data["sizes"].setdefault(str(row["free_keyframes"]), {}).update(row)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out = OUT
    if "--out" in args:
        i = args.index("--out")
        out = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    if args[:1] == ["--summarise"]:
        row = summarise(args[1], int(args[2]))
        print(json.dumps(row), flush=True)
        merge(row, out)
    else:
        pcg_only = "--pcg-only" in args
        sizes = [int(a) for a in args if a.isdigit()] or [100, 170, 256, 512]
        for size in sizes:
            row = run(size, "--no-host" not in args, pcg_only)
            print(json.dumps(row), flush=True)
            if not pcg_only:
                merge(row, out)
