"""Time ovs_landmarks_update_batch (csrc/landmark_update.hip) on the three places the landmark upkeep runs at: (a) a new keyframe -- 1 500
landmarks of about 6 observations, both parts; (b) local BA's write-back -- 20 000 landmarks of about 6 observations, the geometry only; (c) a map
load -- the same 20 000 with both parts. Against the only baseline there is: the same algebra as a host loop (openvslam_amd/cpp/landmark_host, a
plain g++ -O2 build of csrc/landmark_math.inc, one core). The plain form (descriptors in the call) and the _f form (descriptors gathered on the
device from resident keyframes) side by side. Per case and form: 5 runs of 100 calls each, the first 10 of every run dropped; prints the median,
the minimum and the 90th percentile of the WHOLE ABI call over all kept calls (host clock around the call, which ends in a stream synchronise),
the five runs' medians, and the host program's median, minimum and 90th percentile of a pass over the same landmarks. The clock state is noted
once, as the driver reports it, if it does.
Usage (GPU box): python tools/time_landmarks.py [--host-only] [--case a|b|c] [--calls N] [--runs N]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"a": ("new keyframe", 1500, 3), "b": ("local BA write-back", 20000, 1), "c": ("map load", 20000, 3)}
KEYFRAMES, KEYPOINTS, NUM_LEVELS, HOST_PASSES = 50, 4000, 8, 30
DROP = 10


def scene(n_landmarks, seed=0):
    """n landmarks seen from 50 keyframes of 4000 keypoints: 2 to 10 observations each (6 on average) in distinct keyframes, every observation a
    keypoint of its own, a landmark's descriptors a few bits apart. Returns the ABI's arrays plus obs_keypoint and the keyframes' descriptors."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(2, 11, n_landmarks)
    offsets = np.zeros(n_landmarks + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    T = int(offsets[-1])
    assert T <= KEYFRAMES * KEYPOINTS
    obs_kf = np.concatenate([rng.choice(KEYFRAMES, c, replace=False) for c in counts]).astype(np.int32)
    taken = np.zeros(KEYFRAMES, np.int64)
    obs_kp = np.zeros(T, np.int32)
    for t, k in enumerate(obs_kf):
        obs_kp[t] = taken[k]
        taken[k] += 1
    assert taken.max() <= KEYPOINTS
    base = rng.integers(0, 256, (n_landmarks, 32), dtype=np.uint8)
    obs_desc = np.repeat(base, counts, axis=0)
    flips = rng.integers(0, 256, (T, 12))
    for j in range(12):
        obs_desc[np.arange(T), flips[:, j] >> 3] ^= (1 << (flips[:, j] & 7)).astype(np.uint8)
    kf_desc = rng.integers(0, 256, (KEYFRAMES, KEYPOINTS, 32), dtype=np.uint8)
    kf_desc[obs_kf, obs_kp] = obs_desc
    ref_kf = obs_kf[offsets[:-1]].copy()
    sf = np.cumprod(np.concatenate([[np.float32(1.0)], np.full(NUM_LEVELS - 1, np.float32(1.2), np.float32)])).astype(np.float32)
    return dict(offsets=offsets, pos_w=rng.uniform(-5, 5, (n_landmarks, 3)) + [0, 0, 8], ref_keyfrm=ref_kf, ref_level=rng.integers(0, NUM_LEVELS, n_landmarks).astype(np.int32),
                obs_keyfrm=obs_kf, obs_desc=obs_desc, obs_use=None, cam_centers=rng.uniform(-2, 2, (KEYFRAMES, 3)), scale_factors=sf, obs_keypoint=obs_kp, kf_desc=kf_desc)


def time_host(s, what):
    import landmark_io
    exe = os.path.join(ROOT, "openvslam_amd", "cpp", "landmark_host")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "landmark_host"])
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "case.bin")
        with open(path, "wb") as f:
            f.write(landmark_io.host_input(s))
        return json.loads(subprocess.run([exe, path, "--time", str(HOST_PASSES), str(what)], capture_output=True, text=True, check=True).stdout)


def time_device(s, what, resident, runs, calls):
    from openvslam_amd import _lib, landmarks, match
    _lib.require_device()
    n, T = len(s["offsets"]) - 1, len(s["obs_keyfrm"])
    u = landmarks.landmark_updater(0, max_landmarks=n, max_total_observations=T, max_keyframes=KEYFRAMES)
    out = dict(mean_normal=np.zeros((n, 3)), min_max_dist=np.zeros((n, 2), np.float32), best_obs=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8),
               status=np.zeros(n, np.uint8))
    kw = dict(obs_use=None, cam_centers=s["cam_centers"], scale_factors=s["scale_factors"], out=out)
    if resident:
        gp = match.grid_params(752, 480)
        kp = np.zeros(KEYPOINTS, match.KP_DTYPE)
        kp["x"], kp["y"] = np.linspace(1, 750, KEYPOINTS), np.linspace(1, 478, KEYPOINTS)
        kw.update(frame_devs=[match.frame_dev(gp, kp, s["kf_desc"][k]) for k in range(KEYFRAMES)], obs_keypoint=s["obs_keypoint"])
    else:
        kw.update(obs_desc=s["obs_desc"])
    call = lambda: u.update(what, s["offsets"], s["pos_w"], s["ref_keyfrm"], s["ref_level"], s["obs_keyfrm"], **kw)
    kept, medians = [], []
    for _ in range(runs):
        times = []
        for _ in range(calls):
            t = time.perf_counter()
            call()
            times.append(time.perf_counter() - t)
        kept += times[DROP:]
        medians.append(float(np.median(times[DROP:])))
    ms = lambda v: round(v * 1e3, 4)
    digest = int(out["best_obs"].astype(np.int64).sum()) if what & 2 else None
    return {"abi_call_median_ms": ms(np.median(kept)), "abi_call_min_ms": ms(min(kept)), "abi_call_p90_ms": ms(np.percentile(kept, 90)),
            "run_medians_ms": [ms(m) for m in medians], "best_obs_sum": digest}


def clock_state():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=30)
        lines = [w.strip() for w in r.stdout.split("\n") if "GPU[0]" in w and ("sclk" in w or "mclk" in w or "Performance" in w)]
        return lines or "not reported"
    except (OSError, subprocess.SubprocessError):
        return "not reported"


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    runs, calls = int(arg("--runs", 5)), int(arg("--calls", 100))
    if "--host-only" not in sys.argv:
        print(json.dumps({"clock_state": clock_state()}), flush=True)
    for key in ([arg("--case", None)] if "--case" in sys.argv else list(CASES)):
        name, n, what = CASES[key]
        s = scene(n)
        row = {"case": key, "name": name, "landmarks": n, "observations": int(s["offsets"][-1]), "what": what, "host_loop": time_host(s, what)}
        if "--host-only" not in sys.argv:
            row["device_plain"] = time_device(s, what, False, runs, calls)
            row["device_resident"] = time_device(s, what, True, runs, calls)
            if what & 2:
                assert row["device_plain"]["best_obs_sum"] == row["device_resident"]["best_obs_sum"]
        print(json.dumps(row), flush=True)
