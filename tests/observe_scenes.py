"""Scenes for tracking_module::search_local_landmarks, built like _last_and_current / _sim3_scene of tests/test_gpu_window.py and
restated here in numpy alone: a frame of n keypoints under a pose, and m local landmarks that are those keypoints back-projected at random
depths (so they reproject near them), with valid ranges from the true distance and about 15 % random normals -- plus landmarks behind the
camera, outside the image, outside their range, entries that are not searched, and duplicates that contend for one keypoint.
tests/test_observe_ref.py checks on the CPU that every gate is met; tests/test_gpu_search_local.py asserts it again where it uses them."""
import struct
from types import SimpleNamespace

import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])   # cv::KeyPoint
NUM_LEVELS = 8
SCALE_FACTORS = np.cumprod(np.concatenate([[1.0], np.full(NUM_LEVELS - 1, 1.2)]).astype(np.float32)).astype(np.float32)
LOG_SCALE_FACTOR = float(np.log(np.float32(1.2)))
BASELINE = 0.12


def _rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    x, y, z = axis
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def _keypoints(rng, n, rows, cols):
    k = np.zeros(n, KP_DTYPE)
    octs = np.sort(rng.integers(0, NUM_LEVELS, n))
    sf = np.float32(1.2) ** octs.astype(np.float32)
    k["octave"] = octs
    k["x"] = (np.floor(rng.uniform(22, cols / sf - 22)) * sf).astype(np.float32)
    k["y"] = (np.floor(rng.uniform(22, rows / sf - 22)) * sf).astype(np.float32)
    k["size"] = 31 * sf
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.integers(7, 120, n)
    k["class_id"] = -1
    return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip_bits(rng, desc, max_flip):
    bits = np.unpackbits(desc)
    bits[rng.permutation(256)[:int(rng.integers(0, max_flip + 1))]] ^= 1
    return np.packbits(bits)


def _back_project(model, u, v, depth, intr, rows, cols):
    fx, fy, cx, cy = intr
    if model == 0:
        return np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], 1)
    lon = (u / cols - 0.5) * 2 * np.pi
    lat = -(v / rows - 0.5) * np.pi
    return np.stack([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)], 1) * depth[:, None]


def scene(model, n, m, seed, stereo=False):
    """model 0 perspective / 1 equirectangular. Returns a namespace: rows, cols, intr (fx, fy, cx, cy), focal_x_baseline, kps, desc, x_right
    (None unless stereo), occupied, pose (3 x 4), pos, dmm, nrm, lm_desc, search, dup_of (index of the landmark a duplicate copies, else -1)."""
    rng = np.random.default_rng(seed)
    rows, cols = (960, 1920) if model == 1 else (720, 1280)
    kps, desc = _keypoints(rng, n, rows, cols)
    R = _rot((0, 1, 0), 2.0) @ _rot((1, 0, 0), -1.0)
    t = np.array([0.05, -0.02, 0.3])
    fx = fy = 0.6 * cols
    intr = (fx, fy, cols / 2.0, rows / 2.0)
    fxb = BASELINE * fx
    kp_depth = rng.uniform(2.0, 20.0, max(n, 1))
    if n:
        src = np.concatenate([rng.permutation(n), rng.integers(0, n, max(m - n, 0))])[:m]
        u = kps["x"][src].astype(np.float64) + rng.normal(0, 1.5, m)
        v = kps["y"][src].astype(np.float64) + rng.normal(0, 1.5, m)
        depth = kp_depth[src]
        octave = kps["octave"][src]
        lm_desc = np.stack([_flip_bits(rng, desc[i], 60) for i in src]) if m else np.zeros((0, 32), np.uint8)
    else:
        u, v, depth = rng.uniform(30, cols - 30, m), rng.uniform(30, rows - 30, m), rng.uniform(2.0, 20.0, m)
        octave = rng.integers(0, NUM_LEVELS, m)
        lm_desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    kind = rng.random(m)
    behind = kind < 0.06                       # V2 depth (perspective)
    outside = (kind >= 0.06) & (kind < 0.12)   # V2 bounds (perspective)
    u = np.where(outside, np.where(rng.random(m) < 0.5, cols + rng.uniform(20, 200, m), u), u)
    v = np.where(outside & (u <= cols), -rng.uniform(20, 200, m), v)
    pc = _back_project(model, u, v, depth, intr, rows, cols)
    pc[behind] *= -1.0
    pos = (pc - t) @ R + rng.normal(0, 0.002, (m, 3))
    vec = pos - (-R.T @ t)
    dist = np.linalg.norm(vec, axis=1)
    lvl = np.clip(octave + rng.integers(0, 2, m), 0, NUM_LEVELS - 1)
    dmax = dist * SCALE_FACTORS[lvl] * rng.uniform(0.85, 1.0, m)
    dmin = dmax / SCALE_FACTORS[NUM_LEVELS - 1] * rng.uniform(0.5, 1.3, m)
    too_far = (kind >= 0.12) & (kind < 0.15)     # V3: beyond 1.3 x max
    too_near = (kind >= 0.15) & (kind < 0.18)    # V3: inside 0.7 x min
    dmax = np.where(too_far, dist * 0.5, dmax)
    dmin = np.where(too_far, dist * 0.05, dmin)
    dmin = np.where(too_near, dist * 2.0, dmin)
    dmax = np.where(too_near, dist * 8.0, dmax)
    dmm = np.ascontiguousarray(np.stack([dmin, dmax], 1).astype(np.float32))
    nrm = vec / dist[:, None]
    flip = rng.random(m) < 0.15                  # V4: random normals
    nrm[flip] = rng.normal(0, 1, (int(flip.sum()), 3))
    search = (rng.random(m) >= 0.08).astype(np.uint8)   # V1
    # duplicates contending for a keypoint: a later landmark copies an earlier one (position up to noise, descriptor up to 6 bits)
    dup_of = np.full(m, -1, np.int32)
    for l in range(m // 2, m):
        if m >= 2 and rng.random() < 0.2:
            o = int(rng.integers(0, m // 2))
            dup_of[l] = o
            pos[l] = pos[o] + rng.normal(0, 0.002, 3)
            dmm[l], nrm[l], lm_desc[l] = dmm[o], nrm[o], _flip_bits(rng, lm_desc[o], 6)
    x_right = None
    if stereo and n:   # most keypoints carry the right-image x their landmark's depth gives
        x_right = np.where(rng.random(n) < 0.7, kps["x"] - fxb / kp_depth[:n] + rng.normal(0, 0.5, n), -1.0)
        wrong = (rng.random(n) < 0.15) & (x_right >= 0)   # ... and some a disparity that disagrees: the stereo test rejects their landmark
        x_right = np.where(wrong, x_right - rng.uniform(30, 80, n), x_right).astype(np.float32)
    occupied = (rng.random(n) < 0.05).astype(np.uint8)
    return SimpleNamespace(model=model, rows=rows, cols=cols, intr=intr, focal_x_baseline=fxb, kps=kps, desc=desc, x_right=x_right, occupied=occupied,
                           pose=np.concatenate([R, t[:, None]], 1), pos=np.ascontiguousarray(pos), dmm=dmm, nrm=np.ascontiguousarray(nrm),
                           lm_desc=np.ascontiguousarray(lm_desc), search=search, dup_of=dup_of, n=n, m=m)


def cameras(sc, camera_type, grid_type):
    """(camera, grid parameters) of a scene as the given ctypes structures (the oracle's or the library's)."""
    fx, fy, cx, cy = sc.intr
    return (camera_type(sc.model, 1 if sc.x_right is not None else 0, fx, fy, cx, cy, sc.focal_x_baseline, BASELINE, sc.cols, sc.rows),
            grid_type(0.0, 0.0, float(sc.cols), float(sc.rows), 64, 48))


def reference(oracle, observe_ref, sc, margin, ratio):
    cam, gp = cameras(sc, oracle.Camera, oracle.GridParams)
    return observe_ref.search_local_landmarks(oracle, cam, gp, sc.kps, sc.desc, sc.pose, sc.pos, sc.dmm, sc.nrm, sc.lm_desc, SCALE_FACTORS,
                                              LOG_SCALE_FACTOR, margin, ratio, stereo_x_right=sc.x_right, occupied=sc.occupied, lm_search=sc.search)


def contended_keypoints(oracle, sc, ref, margin, ratio):
    """Keypoints that two landmarks wanted: an observable duplicate that, matched ALONE, takes the keypoint its original holds in the full run, and
    does not hold it there."""
    _, gp = cameras(sc, oracle.Camera, oracle.GridParams)
    hit = set()
    for l in np.nonzero((sc.dup_of >= 0) & (ref["observable"] != 0))[0]:
        o = int(sc.dup_of[l])
        if ref["assigned"][o] < 0:
            continue
        alone = np.zeros(sc.m, np.uint8)
        alone[l] = 1
        got, _ = oracle.projection_match_frame_and_landmarks(gp, sc.kps, sc.desc, SCALE_FACTORS, ref["reproj"].astype(np.float32), ref["level"], sc.lm_desc,
                                                             margin, ratio, frm_stereo_x_right=sc.x_right, frm_occupied=sc.occupied,
                                                             lm_x_right=ref["x_right"] if sc.x_right is not None else None, lm_valid=alone)
        if got[l] == ref["assigned"][o] and ref["assigned"][l] != got[l]:
            hit.add(int(got[l]))
    return hit


# ---- the scene as openvslam_amd/cpp/test_search_shim.cc reads it, and what that program writes (little endian) ----
def write_scene(path, sc, margin, ratio, frame_id, held, erased):
    """held: keypoint index -> landmark index the frame already holds (curr_frm.landmarks_); erased: landmark indices with will_be_erased()."""
    fx, fy, cx, cy = sc.intr
    with open(path, "wb") as f:
        f.write(struct.pack("<i4d2f2i", sc.model, fx, fy, cx, cy, sc.focal_x_baseline, BASELINE, sc.cols, sc.rows))
        f.write(struct.pack("<2fIi", margin, ratio, frame_id, NUM_LEVELS))
        f.write(SCALE_FACTORS.tobytes())
        f.write(struct.pack("<f", LOG_SCALE_FACTOR))
        T = np.eye(4)
        T[:3] = sc.pose
        f.write(T.astype("<f8").tobytes())
        f.write(struct.pack("<2i", sc.n, 1 if sc.x_right is not None else 0))
        f.write(np.ascontiguousarray(sc.kps).tobytes())
        f.write(np.ascontiguousarray(sc.desc).tobytes())
        if sc.x_right is not None:
            f.write(sc.x_right.astype("<f4").tobytes())
        f.write(struct.pack("<i", sc.m))
        f.write(sc.pos.astype("<f8").tobytes())
        f.write(sc.nrm.astype("<f8").tobytes())
        f.write(sc.dmm.astype("<f4").tobytes())
        f.write(sc.lm_desc.tobytes())
        er = np.zeros(sc.m, np.uint8)
        er[list(erased)] = 1
        f.write(er.tobytes())
        hl = np.full(sc.n, -1, np.int32)
        for k, l in held.items():
            hl[k] = l
        f.write(hl.astype("<i4").tobytes())


def read_results(path, n, m):
    """Two runs (write_tracking_fields off, then on, each on a fresh copy of the scene): per run u32 num_matches, n i32 frm.landmarks_ (landmark
    index or -1), then per landmark u8 is_observable_in_tracking_, u32 num_observable_, 2 f64 reproj, f32 x_right, i32 level."""
    rec = np.dtype([("observable", "u1"), ("num_observable", "<u4"), ("reproj", "<f8", 2), ("x_right", "<f4"), ("level", "<i4")])
    buf = open(path, "rb").read()
    runs, off = [], 0
    for _ in range(2):
        num = struct.unpack_from("<I", buf, off)[0]
        off += 4
        held = np.frombuffer(buf, "<i4", n, off).copy()
        off += 4 * n
        lms = np.frombuffer(buf, rec, m, off).copy()
        off += rec.itemsize * m
        runs.append({"num_matches": num, "landmarks": held, "lms": lms})
    assert off == len(buf)
    return runs
