"""Files between the triangulator's tests and its two C++ programs: the case file of tests/triangulate_host.cc (the shared algebra under a
plain host compiler) with its printed lines, and the keyframe scene of openvslam_amd/cpp/test_triangulate_shim.cc (the C++ class) with its
results. Plus the keyframe form of tests/triangulate_ref.py's problems: a current keyframe and its neighbours as arrays per keypoint, the
matches as index pairs."""
import random
import struct

import triangulate_ref as tri

DEG_THR = 1.0


# ---- tests/triangulate_host.cc
def _cam_bytes(c):
    return struct.pack("<i6d2i", c["model"], c["fx"], c["fy"], c["cx"], c["cy"], c["focal_x_baseline"], c["true_baseline"], c["cols"], c["rows"])


def host_input(problems, cos_thr=tri.COS_THR, ratio_factor=tri.RATIO_FACTOR):
    out = [struct.pack("<dfi", cos_thr, ratio_factor, len(problems))]
    for q in problems:
        out += [_cam_bytes(q["cam_1"]), _cam_bytes(q["cam_2"]), struct.pack("<24d", *(q["pose_1"] + q["pose_2"])), struct.pack("<i", len(q["b1"]))]
        for i in range(len(q["b1"])):
            out.append(struct.pack("<6d12f", *q["b1"][i], *q["b2"][i], *q["kp1"][i], *q["kp2"][i], q["xr1"][i], q["xr2"][i], q["depth1"][i], q["depth2"][i],
                                   q["sig1"][i], q["sig2"][i], q["sf1"][i], q["sf2"][i]))
    return b"".join(out)


def host_output(text):
    """[(status, method, [3 bit patterns])] of the host program's lines."""
    rows = []
    for line in text.split("\n"):
        if line.strip():
            w = line.split()
            rows.append((int(w[0]), int(w[1]), [int(x, 16) for x in w[2:5]]))
    return rows


# ---- keyframes
def _pose44(P):
    return [P[0], P[1], P[2], P[9], P[3], P[4], P[5], P[10], P[6], P[7], P[8], P[11], 0.0, 0.0, 0.0, 1.0]


def _keyframe(cam, pose):
    return dict(cam=cam, pose=_pose44(pose), octaves=[], keypts=[], bearings=[], x_right=[], depths=[])


def keyframes_of(problems, seed=0):
    """The problems (which share camera 1 and pose 1) as one current keyframe and a neighbour per problem: (curr, neighbours, matches), matches[k]
    the (idx_1, idx_2) pairs of neighbour k in the problem's match order. The keypoints of every keyframe are shuffled, and every keyframe
    holds a few keypoints no match uses."""
    rng = random.Random(seed)
    assert all(q["cam_1"] == problems[0]["cam_1"] and q["pose_1"] == problems[0]["pose_1"] for q in problems)
    curr, neighbours, matches = _keyframe(problems[0]["cam_1"], problems[0]["pose_1"]), [], []

    def fill(kf, entries):
        """entries: (octave, kp, bearing, x_right, depth); returns where each went."""
        extra = [(0, (10.0 + k, 20.0), (0.0, 0.0, 1.0), -1.0, -1.0) for k in range(3)]
        order = list(range(len(entries) + len(extra)))
        rng.shuffle(order)
        where = {src: dst for dst, src in enumerate(order)}
        for src in order:
            o, kp, b, xr, d = (entries + extra)[src]
            kf["octaves"].append(o), kf["keypts"].append(kp), kf["bearings"].append(b), kf["x_right"].append(xr), kf["depths"].append(d)
        return [where[i] for i in range(len(entries))]

    side = lambda q, s: [(q["oct" + s][i], q["kp" + s][i], q["b" + s][i], q["xr" + s][i], q["depth" + s][i]) for i in range(len(q["b1"]))]
    all_1 = [e for q in problems for e in side(q, "1")]
    idx_1 = fill(curr, all_1)
    at = 0
    for q in problems:
        kf = _keyframe(q["cam_2"], q["pose_2"])
        idx_2 = fill(kf, side(q, "2"))
        neighbours.append(kf)
        matches.append(list(zip(idx_1[at:at + len(idx_2)], idx_2)))
        at += len(idx_2)
    return curr, neighbours, matches


def _keyframe_bytes(kf):
    c, n = kf["cam"], len(kf["octaves"])
    out = [struct.pack("<i4d2f2i", c["model"], c["fx"], c["fy"], c["cx"], c["cy"], c["focal_x_baseline"], c["true_baseline"], c["cols"], c["rows"]),
           struct.pack("<16d", *kf["pose"]), struct.pack("<i", n), struct.pack("<%di" % n, *kf["octaves"]),
           struct.pack("<%df" % (2 * n), *[v for kp in kf["keypts"] for v in kp]), struct.pack("<%dd" % (3 * n), *[v for b in kf["bearings"] for v in b]),
           struct.pack("<%df" % n, *kf["x_right"]), struct.pack("<%df" % n, *kf["depths"])]
    return b"".join(out)


def write_scene(path, curr, neighbours, matches, deg_thr=DEG_THR):
    out = [struct.pack("<ffi", deg_thr, tri.SCALE_FACTOR, tri.NUM_LEVELS), struct.pack("<%df" % tri.NUM_LEVELS, *tri.SCALE_FACTORS),
           struct.pack("<%df" % tri.NUM_LEVELS, *tri.LEVEL_SIGMA_SQ), struct.pack("<i", len(neighbours)), _keyframe_bytes(curr)]
    for kf, m in zip(neighbours, matches):
        out += [_keyframe_bytes(kf), struct.pack("<i", len(m))] + [struct.pack("<ii", a, b) for a, b in m]
    with open(path, "wb") as f:
        f.write(b"".join(out))


def read_results(path, n_neighbours):
    """{"single" | "neighbour" | "all": [per neighbour dict num_accepted, accepted [0 / 1], pos [[3 bit patterns]]]}"""
    data = open(path, "rb").read()
    at, out = 0, {}
    for section in ("single", "neighbour", "all"):
        out[section] = []
        for _ in range(n_neighbours):
            n, num = struct.unpack_from("<ii", data, at)
            at += 8
            acc, pos = [], []
            for _ in range(n):
                acc.append(data[at])
                pos.append(list(struct.unpack_from("<3Q", data, at + 1)))
                at += 25
            out[section].append(dict(num_accepted=num, accepted=acc, pos=pos))
    assert at == len(data)
    return out


def class_scene():
    """Three neighbours of one stereo keyframe: stereo-mono, stereo-stereo and a short stereo-mono baseline."""
    return [tri.scene(20, "stereo_mono", seed=11), tri.scene(33, "stereo_stereo", seed=12), tri.scene(7, "stereo_mono", seed=13, baseline=0.3)]
