"""Files between the landmark upkeep's tests and its two C++ programs: the case file of tests/landmark_host.cc (the shared algebra under a plain
host compiler) with its printed lines, and the scene of openvslam_amd/cpp/test_landmark_shim.cc (data::update_landmarks on stub keyframes) with
its results."""
import struct

import numpy as np

import landmark_ref as lr


# ---- tests/landmark_host.cc
def host_input(case):
    n, T, K, L = len(case["offsets"]) - 1, len(case["obs_keyfrm"]), len(case["cam_centers"]), len(case["scale_factors"])
    use = case["obs_use"]
    c = lambda a, t: np.ascontiguousarray(a, t).tobytes()
    return b"".join([struct.pack("<5i", n, T, K, L, 0 if use is None else 1), c(case["offsets"], np.int32), c(case["pos_w"], np.float64), c(case["ref_keyfrm"], np.int32),
                     c(case["ref_level"], np.int32), c(case["obs_keyfrm"], np.int32), c(case["obs_desc"], np.uint8), b"" if use is None else c(use, np.uint8),
                     c(case["cam_centers"], np.float64), c(case["scale_factors"], np.float32)])


def host_output(text):
    """The host program's lines as the five output arrays after a call on sentinel-filled arrays."""
    lines = [w.split() for w in text.split("\n") if w.strip()]
    out = lr.sentinel_outputs(len(lines))
    for p, w in enumerate(lines):
        out["status"][p] = int(w[0])
        if w[0] != "0":
            continue
        out["mean_normal"][p] = np.array([int(x, 16) for x in w[1:4]], np.uint64).view(np.float64)
        out["min_max_dist"][p] = np.array([int(x, 16) for x in w[4:6]], np.uint32).view(np.float32)
        out["best_obs"][p] = int(w[6])
        if w[7] != "-":
            out["desc"][p] = np.frombuffer(bytes.fromhex(w[7]), np.uint8)
    return out


# ---- openvslam_amd/cpp/test_landmark_shim.cc
def shim_scene(case, keypoints_per_keyframe, seed=3, erased=()):
    """The case as stub keyframes: keyframe k has keypoints_per_keyframe[k] keypoints, each observation a keypoint of its own (descriptor, octave),
    the others filler. A landmark's observations have to be in distinct keyframes (a std::map holds them). Returns (bytes, order): order[p] the
    case's observation indices of landmark p in the order the stub iterates them (ascending keyframe address = ascending slot: the program
    allocates the keyframes in one array)."""
    import random
    rng = random.Random(seed)
    K, n = len(case["cam_centers"]), len(case["offsets"]) - 1
    kp_desc = [[bytes(rng.randrange(256) for _ in range(32)) for _ in range(keypoints_per_keyframe[k])] for k in range(K)]
    kp_oct = [[rng.randrange(lr.NUM_LEVELS) for _ in range(keypoints_per_keyframe[k])] for k in range(K)]
    free = [list(range(keypoints_per_keyframe[k])) for k in range(K)]
    for f in free:
        rng.shuffle(f)
    obs_kp, order = [], []
    for p in range(n):
        a, b = int(case["offsets"][p]), int(case["offsets"][p + 1])
        slots = [int(s) for s in case["obs_keyfrm"][a:b]]
        assert len(set(slots)) == len(slots)
        for t in range(a, b):
            k = int(case["obs_keyfrm"][t])
            idx = free[k].pop()
            kp_desc[k][idx] = case["obs_desc"][t].tobytes()
            if k == int(case["ref_keyfrm"][p]):
                kp_oct[k][idx] = int(case["ref_level"][p])
            obs_kp.append(idx)
        order.append(sorted(range(a, b), key=lambda t: int(case["obs_keyfrm"][t])))
    out = [struct.pack("<3i", K, n, lr.NUM_LEVELS), np.ascontiguousarray(case["scale_factors"], np.float32).tobytes()]
    for k in range(K):
        out += [struct.pack("<ii3d", keypoints_per_keyframe[k], 1 if k in erased else 0, *case["cam_centers"][k]), struct.pack("<%di" % len(kp_oct[k]), *kp_oct[k]),
                b"".join(kp_desc[k])]
    for p in range(n):
        a, b = int(case["offsets"][p]), int(case["offsets"][p + 1])
        out.append(struct.pack("<3d2i", *case["pos_w"][p], int(case["ref_keyfrm"][p]), b - a))
        out += [struct.pack("<ii", int(case["obs_keyfrm"][t]), obs_kp[t]) for t in range(a, b)]
    return b"".join(out), order


def reordered(case, order, erased=()):
    """The case with every landmark's observations in the given order, and obs_use cleared for the erased keyframes: what the stub hands over."""
    perm = [t for o in order for t in o]
    kf = case["obs_keyfrm"][perm]
    return dict(case, obs_keyfrm=kf, obs_desc=case["obs_desc"][perm], obs_use=np.array([0 if int(k) in erased else 1 for k in kf], np.uint8))


def shim_results(data, n):
    """Per landmark: normal [3 u64], min / max valid [2 u32], descriptor bytes (empty: none), num_normal_updates."""
    at, out = 0, []
    for _ in range(n):
        normal = list(struct.unpack_from("<3Q", data, at))
        rng = list(struct.unpack_from("<2I", data, at + 24))
        updates, has = struct.unpack_from("<ii", data, at + 32)
        at += 40
        out.append(dict(normal=normal, range=rng, updates=updates, desc=data[at:at + 32] if has else b""))
        at += 32 if has else 0
    assert at == len(data)
    return out
