"""Time ovs_posegraph_optimize (csrc/pose_graph.hip) on rings of 50, 200, 1000 and 4000 keyframes: every keyframe joined to the next three, one
closing edge, ten landmarks per keyframe, consistent measurements, a start that drifts along the ring, num_iter = 20. Per size: the WHOLE
call (host clock around the ABI call, which ends in a stream synchronise; the arrays are packed once), the Levenberg-Marquardt iterations, the
trials and the PCG iterations it ran, and the same algebra as a host loop on one core (openvslam_amd/cpp/posegraph_host, the stand-alone program
the tests hold to the reference; its time includes reading and writing its files, microseconds against its seconds). The first call of a
size is dropped. Nothing is gated: the figures go to profiles/posegraph_times.json as found.
The kernel alone: run one size under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/time_posegraph.py --sizes N`
in a run of its own, then `python tools/time_posegraph.py --summarise <dir> N` prints the median and minimum of k_posegraph_optimize and
k_posegraph_correct over the kept dispatches and merges them into the JSON.
Usage (GPU box): python tools/time_posegraph.py [--sizes N ...] [--no-host]"""
import csv
import ctypes as C
import glob
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "posegraph_times.json")
NUM_ITER, LM_PER_KF = 20, 10
CALLS = {50: 12, 200: 8, 1000: 4, 4000: 3}   # the first is dropped; a call at 4000 keyframes runs for seconds


def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)


def ring(n, seed=0):
    """The arrays of the C ABI for a ring of n keyframes on a circle whose radius grows with n (neighbours stay about a unit apart)."""
    rng = np.random.default_rng(seed)
    radius = max(4.0, n / (2 * math.pi))
    R, t = [], []
    for v in range(n):
        a = 2 * math.pi * v / n
        Rv = rodrigues(np.array([0.1 * math.sin(3 * a), a, 0.05 * math.cos(2 * a)]))
        c = np.array([radius * math.cos(a), 0.3 * math.sin(2 * a), radius * math.sin(a)])
        R.append(Rv)
        t.append(-Rv @ c)
    edges = [(v, v + k) for v in range(n) for k in (1, 2, 3) if v + k < n] + [(n - 1, 0)]
    e_rot = np.array([R[j] @ R[i].T for i, j in edges])
    e_trans = np.array([t[j] - R[j] @ R[i].T @ t[i] for i, j in edges])
    rot, trans, scale = np.array(R), np.array(t), np.ones(n)
    for v in range(1, n):   # the drift: up to 0.03 rad, 0.15 units and 5 % of scale at the far end
        f = v / (n - 1)
        dR, s = rodrigues(np.array([0.02, -0.01, 0.015]) * f), math.exp(0.05 * f)
        rot[v], trans[v], scale[v] = dR @ R[v], s * (dR @ t[v]) + np.array([0.10, -0.05, 0.08]) * f, s
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    n_l = LM_PER_KF * n
    return dict(rot=np.ascontiguousarray(rot.reshape(n, 9)), trans=np.ascontiguousarray(trans), scale=scale, fixed=fixed,
                edge_ij=np.array(edges, np.int32), edge_rot=np.ascontiguousarray(e_rot.reshape(len(edges), 9)), edge_trans=np.ascontiguousarray(e_trans),
                edge_scale=np.ones(len(edges)), lm_ref=(np.arange(n_l) // LM_PER_KF).astype(np.int32), lm_pos=rng.uniform(-2, 2, (n_l, 3)))


def host_loop_seconds(q):
    """The same optimisation by the stand-alone host program on one core."""
    exe = os.path.join(ROOT, "openvslam_amd", "cpp", "posegraph_host")
    if not os.path.exists(exe):
        return None
    n, e, l = len(q["scale"]), len(q["edge_scale"]), len(q["lm_ref"])
    states = lambda r, t, s: np.concatenate([r.reshape(-1, 9), t.reshape(-1, 3), s.reshape(-1, 1)], 1).ravel()
    start = states(q["rot"], q["trans"], q["scale"])
    flat = np.concatenate([[0.0, 0.0, 1.0, n, e, l, 0, NUM_ITER, 0], start, start, q["fixed"].astype(np.float64), q["edge_ij"].ravel().astype(np.float64),
                           states(q["edge_rot"], q["edge_trans"], q["edge_scale"]), q["lm_ref"].astype(np.float64), q["lm_pos"].ravel()])
    with tempfile.TemporaryDirectory() as tmp:
        flat.astype(np.float64).tofile(os.path.join(tmp, "in.bin"))
        t0 = time.perf_counter()
        subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
        dt = time.perf_counter() - t0
        out = np.fromfile(os.path.join(tmp, "out.bin"), np.float64)
    return dt, out[-8:].tolist()


def run(n, with_host=True):
    from openvslam_amd import _lib
    _lib.require_device()
    L = _lib.lib()
    q = ring(n)
    e, l = len(q["edge_scale"]), len(q["lm_ref"])
    h = C.c_void_p()
    _lib.check(L.ovs_posegraph_create(0, n, e, l, C.byref(h)), "ovs_posegraph_create")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    o_rot, o_trans, o_scale, o_lm, info = np.zeros((n, 9)), np.zeros((n, 3)), np.zeros(n), np.zeros((l, 3)), np.zeros(8)
    times = []
    for _ in range(CALLS.get(n, 4)):
        t0 = time.perf_counter()
        _lib.check(L.ovs_posegraph_optimize(h, n, p(q["rot"]), p(q["trans"]), p(q["scale"]), p(q["fixed"]), p(q["rot"]), p(q["trans"]), p(q["scale"]), e,
                                            p(q["edge_ij"]), p(q["edge_rot"]), p(q["edge_trans"]), p(q["edge_scale"]), 0, NUM_ITER, 0, l, p(q["lm_ref"]),
                                            p(q["lm_pos"]), p(o_rot), p(o_trans), p(o_scale), p(o_lm), p(info)), "ovs_posegraph_optimize")
        times.append(time.perf_counter() - t0)
    L.ovs_posegraph_destroy(h)
    kept = times[1:]
    row = {"keyframes": n, "edges": e, "landmarks": l, "num_iter": NUM_ITER, "calls_kept": len(kept), "call_median_ms": round(float(np.median(kept)) * 1e3, 3),
           "call_min_ms": round(min(kept) * 1e3, 3), "lm_iterations": int(info[0]), "trials": int(info[1]), "pcg_iterations": int(info[5]),
           "pcg_iterations_last_solve": int(info[6]), "chi_initial": float(info[2]), "chi_final": float(info[3])}
    if with_host:
        host = host_loop_seconds(q)
        if host is not None:
            row["host_one_core_ms"] = round(host[0] * 1e3, 3)
            row["host_same_bits"] = [float(x) for x in host[1]] == [float(x) for x in info]
    return row


def summarise(directory, n):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for name in ("k_posegraph_optimize", "k_posegraph_correct"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if name in r["Kernel_Name"]][1:]
        if d:
            out[name] = {"dispatches_kept": len(d), "median_ms": round(float(np.median(d)), 4), "min_ms": round(min(d), 4)}
    return {"keyframes": n, "kernels": out}


def merge(row):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {"sizes": {}}
    data["sizes"].setdefault(str(row["keyframes"]), {}).update(row)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--summarise"]:
        row = summarise(args[1], int(args[2]))
        print(json.dumps(row), flush=True)
        merge(row)
    else:
        with_host = "--no-host" not in args
        sizes = [int(a) for a in args if a.isdigit()] or [50, 200, 1000, 4000]
        for size in sizes:
            row = run(size, with_host)
            print(json.dumps(row), flush=True)
            merge(row)
