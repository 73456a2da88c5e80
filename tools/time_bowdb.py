"""Time ovs_bowdb_query (csrc/bow_db.hip) on databases of 1 000 and 10 000 keyframes of 1 500 words each out of 10^6 possible words -- the real
vocabulary's order of magnitude. 50 queries per size, the first 5 dropped; prints the median of the WHOLE call (host clock around the call,
which ends in a stream synchronise) with the bytes the algorithm has to read, sum(length) x 12 + nq x 12, and that rate as a fraction of
8.0 TB/s (HBM3E peak) and of 6.29 TB/s (the microarchitecture guide's copy figure). The kernel alone: run this under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_bowdb.py [sizes]` in a run of its own and read k_bowdb_score there.
Usage (GPU box): python tools/time_bowdb.py [n_keyframes ...]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openvslam_amd import _lib

N_WORDS, LENGTH, QUERIES, DROP = 10 ** 6, 1500, 50, 5


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def vector(rng):
    u = np.unique(rng.integers(0, N_WORDS, LENGTH + 64))            # (a permutation of 10^6 per vector would dominate the fill)
    ids = np.sort(rng.choice(u, LENGTH, replace=False)).astype(np.int32)
    w = rng.uniform(0.5, 9.0, LENGTH)
    return ids, w / w.sum()


def run(n_keyframes, seed=0):
    L = _lib.lib()
    _lib.require_device()
    rng = np.random.default_rng(seed)
    h = C.c_void_p()
    _lib.check(L.ovs_bowdb_create(0, n_keyframes, 1536, C.byref(h)), "ovs_bowdb_create")
    t = time.perf_counter()
    for k in range(n_keyframes):
        ids, vals = vector(rng)
        _lib.check(L.ovs_bowdb_add(h, k, p(ids), p(vals), LENGTH), "ovs_bowdb_add")
    fill_s = time.perf_counter() - t
    out_i, out_n, out_s = np.zeros(n_keyframes, np.int32), np.zeros(n_keyframes, np.int32), np.zeros(n_keyframes)
    n, mc = C.c_int32(), C.c_int32()
    times, survivors = [], []
    for _ in range(QUERIES):
        ids, vals = vector(rng)
        t = time.perf_counter()
        _lib.check(L.ovs_bowdb_query(h, p(ids), p(vals), LENGTH, None, 0, p(out_i), p(out_n), p(out_s), n_keyframes, C.byref(n), C.byref(mc)),
                   "ovs_bowdb_query")
        times.append(time.perf_counter() - t)
        survivors.append(n.value)
    L.ovs_bowdb_destroy(h)
    med = float(np.median(times[DROP:]))
    nbytes = n_keyframes * LENGTH * 12 + LENGTH * 12
    return {"n_keyframes": n_keyframes, "words_per_keyframe": LENGTH, "fill_s": round(fill_s, 3), "query_call_median_us": round(med * 1e6, 1),
            "query_call_min_us": round(min(times[DROP:]) * 1e6, 1), "query_call_max_us": round(max(times[DROP:]) * 1e6, 1),
            "algorithmic_bytes": nbytes, "call_TB_per_s": round(nbytes / med / 1e12, 3), "call_fraction_of_8.0_TBps": round(nbytes / med / 8.0e12, 4),
            "call_fraction_of_6.29_TBps": round(nbytes / med / 6.29e12, 4), "max_common_last": mc.value, "survivors_median": int(np.median(survivors))}


if __name__ == "__main__":
    for size in [int(a) for a in sys.argv[1:]] or [1000, 10000]:
        print(json.dumps(run(size)), flush=True)
