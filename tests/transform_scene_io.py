"""Scenes for optimize::transform_optimizer and their files: the problems of tests/test_sim3_ref.py's generator with keypoints (Gaussian noise,
random octaves) and a start moved off the planted transform; the input of the stand-alone host program (tests/transform_host.cc); keyframe
pairs, the scene file and the result file of the C++ class's driver (openvslam_amd/cpp/test_transform_shim.cc).

A problem is tests/transform_ref.py's dict. The keypoints are float32 values, as a keyframe's undist_keypts_ are."""
import functools
import random
import struct

import numpy as np

import sim3_ref
import test_sim3_ref as ts
import transform_ref as tr

START_STEP = (0.01, -0.02, 0.015, 0.05, -0.03, 0.04, 0.03)
CHI_SQ, NUM_ITER = 10.0, 10


def inv_level_sigma_sq():
    """orb_params' table as upstream fills it, in float: 1.0f / level_sigma_sq[l]."""
    return [float(np.float32(1.0) / np.float32(s)) for s in ts.level_sigma_sq()]


def scene(n, fix_scale=False, rng_seed=0, cam_1=ts.CAM, cam_2=ts.CAM, noise_px=0.7, wrong=0.2, nan_at=None):
    """n matches of a loop candidate with their keypoints: the generator's points (no noise in space), each projected into its own camera with
    `noise_px` of Gaussian noise and a random octave; `wrong` of the matches are wrong (their indices: the key "wrong"). The start is the planted
    transform moved by START_STEP."""
    scale = 1.0 if fix_scale else ts.TRUE_S
    q = ts.scene(n, noise=0.0, outlier_fraction=wrong, rng_seed=rng_seed, scale=scale, cam_1=cam_1, cam_2=cam_2)
    rng = random.Random(7000 * n + rng_seed)
    inv = inv_level_sigma_sq()
    obs1, obs2, w1, w2 = [], [], [], []
    for i in range(n):
        for cam, p, obs, w in ((cam_1, q["p1"][i], obs1, w1), (cam_2, q["p2"][i], obs2, w2)):
            u, v = sim3_ref.project(cam, *p)
            obs.append((sim3_ref.f32(u + rng.gauss(0.0, noise_px)), sim3_ref.f32(v + rng.gauss(0.0, noise_px))) if noise_px else
                       (sim3_ref.f32(u), sim3_ref.f32(v)))
            w.append(inv[rng.randrange(8)])
    p1 = list(q["p1"])
    if nan_at is not None:
        p1[nan_at] = (float("nan"), p1[nan_at][1], p1[nan_at][2])
    planted = tr.with_inverse(ts.true_rotation(), ts.TRUE_T, scale)
    start = tr.exp_apply(list(START_STEP[:6]) + [0.0 if fix_scale else START_STEP[6]], fix_scale, planted)
    planted_wrong = sorted(random.Random(1000 * n + rng_seed).sample(range(n), int(wrong * n)))   # the generator's first draw
    return dict(p1=p1, p2=list(q["p2"]), obs1=obs1, obs2=obs2, w1=w1, w2=w2, cam_1=cam_1, cam_2=cam_2, R=start["R"], t=start["t"], s=start["s"],
                wrong=planted_wrong)


# Every scene the device tests use. name -> (problem builder, fix_scale)
CASES = {
    "n0": (lambda: scene(0), False),
    "n9": (lambda: scene(9, wrong=0.0), False),
    "n10": (lambda: scene(10, wrong=0.0), False),
    "n12": (lambda: scene(12, wrong=0.0), False),
    "n63": (lambda: scene(63), False),
    "n64": (lambda: scene(64), False),
    "n65": (lambda: scene(65), False),
    "n129": (lambda: scene(129), False),
    "n65_fixed": (lambda: scene(65, fix_scale=True), True),
    "equirect": (lambda: scene(40, cam_1=ts.EQUIRECT, cam_2=ts.EQUIRECT), False),
    "mixed": (lambda: scene(40, rng_seed=5, cam_1=ts.CAM, cam_2=ts.EQUIRECT), False),
    "clean": (lambda: scene(30, noise_px=0.0, wrong=0.0), False),
    "too_few": (lambda: scene(14, wrong=0.5, rng_seed=3), False),
    "r1_rejected": (lambda: scene(33, fix_scale=True, rng_seed=5), True),   # round 1 ends on a rejected trial of a solved system
    "nan_point": (lambda: scene(40, rng_seed=2, nan_at=17), False),
    # what the C++ class collects from two keyframes
    "kf20": (lambda: problem_of(keyframe_pair("kf20"))[0], False),
    "kf64": (lambda: problem_of(keyframe_pair("kf64"))[0], False),
}
BATCH = ["n65", "n0", "n9", "n12", "n64"]


@functools.lru_cache(maxsize=None)
def problem(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def solved(name):
    """The reference's Optimizer after its run (computed once, shared by the CPU and the device tests) and its result."""
    opt = tr.Optimizer(problem(name), CASES[name][1], CHI_SQ, NUM_ITER)
    return opt, opt.run()


def result_bits(r):
    """A reference result as the bit patterns the device tests compare."""
    return dict(num_inliers=r["num_inliers"], R=[sim3_ref.bits(v) for v in r["R"]], t=[sim3_ref.bits(v) for v in r["t"]], s=sim3_ref.bits(r["s"]),
                info=[sim3_ref.bits(v) for v in r["info"]], flags=list(r["flags"]))


# ---- the stand-alone host program
def _cam_blob(cam):
    if cam["model"] == 0:
        return struct.pack("<idddd", 0, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    return struct.pack("<idddd", 1, float(cam["cols"]), float(cam["rows"]), 0.0, 0.0)


def host_input(det, exps, problems):
    """in.bin of tests/transform_host.cc. det: (fn, x); exps: (u, fix_scale, state dict); problems: (problem, fix_scale, num_iter, chi_sq)."""
    blob = struct.pack("<i", len(det)) + b"".join(struct.pack("<id", fn, x) for fn, x in det)
    blob += struct.pack("<i", len(exps))
    for u, fix, S in exps:
        blob += struct.pack("<7di13d", *u, int(fix), *S["R"], *S["t"], S["s"])
    blob += struct.pack("<i", len(problems))
    for q, fix, num_iter, chi_sq in problems:
        n = len(q["p1"])
        blob += struct.pack("<iiif", n, int(fix), num_iter, chi_sq) + _cam_blob(q["cam_1"]) + _cam_blob(q["cam_2"])
        blob += struct.pack("<13d", *q["R"], *q["t"], q["s"])
        for i in range(n):
            blob += struct.pack("<12d", *q["p1"][i], *q["p2"][i], *q["obs1"][i], *q["obs2"][i], q["w1"][i], q["w2"][i])
    return blob


def host_output(raw, n_det, n_exp, sizes):
    """out.bin: (det bit patterns, per exp 17 bit patterns, per problem a result_bits dict)."""
    det = list(struct.unpack_from("<%dQ" % n_det, raw, 0))
    at = 8 * n_det
    exps = []
    for _ in range(n_exp):
        exps.append(list(struct.unpack_from("<17Q", raw, at)))
        at += 136
    out = []
    for n in sizes:
        (num,) = struct.unpack_from("<i", raw, at)
        v = struct.unpack_from("<21Q", raw, at + 4)
        at += 4 + 168
        out.append(dict(num_inliers=num, R=list(v[:9]), t=list(v[9:12]), s=v[12], info=list(v[13:21]), flags=list(raw[at:at + n])))
        at += n
    assert at == len(raw)
    return det, exps, out


# ---- keyframe pairs for the C++ class
def _project_f32(cam, p, rng, noise_px):
    u, v = sim3_ref.project(cam, *map(float, p))
    return sim3_ref.f32(u + rng.gauss(0.0, noise_px)), sim3_ref.f32(v + rng.gauss(0.0, noise_px))


@functools.lru_cache(maxsize=None)
def keyframe_pair(name):
    """tests/sim3_scene_io.py's pair (poses, landmarks in the world, octaves, one unmatched keypoint, one match to an erased landmark) with
    keypoints: every landmark projected into its keyframe with noise, 20 % of keyframe 2's moved away (wrong matches), and the start."""
    import sim3_scene_io
    n = {"kf20": 20, "kf64": 64}[name]
    pair = dict(sim3_scene_io.pair_of(ts.scene(n, noise=0.0, outlier_fraction=0.0, rng_seed=9), ts.level_sigma_sq()))
    rng = random.Random(n)
    for side in ("1", "2"):
        pose, cam = pair["pose_" + side], pair["cam_" + side]
        pts = in_camera(pose, pair["pos_w_" + side])
        pair["kp_" + side] = [_project_f32(cam, p, rng, 0.7) for p in pts]
    for j in rng.sample(range(n), n // 5):
        u, v = pair["kp_2"][j]
        pair["kp_2"][j] = (sim3_ref.f32(u + 40.0), sim3_ref.f32(v - 25.0))
    planted = tr.with_inverse(ts.true_rotation(), ts.TRUE_T, ts.TRUE_S)
    start = tr.exp_apply(list(START_STEP), False, planted)
    pair["R"], pair["t"], pair["s"] = start["R"], start["t"], start["s"]
    return pair


def in_camera(pose, pos_w):
    """rot_cw * pos_w + trans_cw per point in pure floats, in the C++ class's order of operations (the row's products added left to right, then
    the translation): a restatement of its own, not the product's helper."""
    T = [[float(v) for v in row] for row in np.asarray(pose)]
    return [tuple(((T[r][0] * float(p[0]) + T[r][1] * float(p[1])) + T[r][2] * float(p[2])) + T[r][3] for r in range(3)) for p in np.asarray(pos_w)]


def problem_of(pair):
    """(the reference problem the class collects from a pair, the keypoint indices in keyframe 1 of its matches), restated here: the usable
    matches by sim3_solver's skip rules, both landmarks in their own camera, the float keypoints widened, inv_level_sigma_sq of their octaves.
    tests/test_transform_ref.py holds openvslam_amd.solve.transform_problem_from_keyframes to it."""
    idx1 = [i for i, j in enumerate(pair["matched"]) if j >= 0 and not pair["erased_2"][j]]
    idx2 = [pair["matched"][i] for i in idx1]
    inv = inv_level_sigma_sq()
    return dict(p1=in_camera(pair["pose_1"], [pair["pos_w_1"][i] for i in idx1]), p2=in_camera(pair["pose_2"], [pair["pos_w_2"][j] for j in idx2]),
                obs1=[tuple(sim3_ref.f32(v) for v in pair["kp_1"][i]) for i in idx1], obs2=[tuple(sim3_ref.f32(v) for v in pair["kp_2"][j]) for j in idx2],
                w1=[inv[pair["oct_1"][i]] for i in idx1], w2=[inv[pair["oct_2"][j]] for j in idx2],
                cam_1=pair["cam_1"], cam_2=pair["cam_2"], R=list(pair["R"]), t=list(pair["t"]), s=pair["s"]), idx1


def write_scene(path, pairs, fix_scale, num_iter, chi_sq):
    """scene.bin (little endian): i32 fix_scale, num_iter, f32 chi_sq, i32 n_levels, f32 inv_level_sigma_sq[n_levels], i32 n_pairs; per pair two
    keyframes (i32 model, f64 fx fy cx cy, i32 cols rows, 16 f64 pose row-major, i32 n, n i32 octaves, 2 n f32 keypoints, 3 n f64 positions,
    n u8 erased), i32 n_1 and n_1 i32 matched, then the start: 9 f64 rotation, 3 f64 translation, f64 scale."""
    inv = inv_level_sigma_sq()
    blob = struct.pack("<iifi", int(fix_scale), num_iter, chi_sq, len(inv)) + np.asarray(inv, "<f4").tobytes() + struct.pack("<i", len(pairs))

    def keyframe(cam, pose, pos_w, octaves, kps, erased):
        return (struct.pack("<iddddii", cam["model"], cam.get("fx", 0.0), cam.get("fy", 0.0), cam.get("cx", 0.0), cam.get("cy", 0.0), cam.get("cols", 0),
                            cam.get("rows", 0)) + np.asarray(pose, "<f8").tobytes() + struct.pack("<i", len(octaves)) + np.asarray(octaves, "<i4").tobytes() +
                np.asarray(kps, "<f4").tobytes() + np.ascontiguousarray(pos_w, "<f8").tobytes() + np.asarray(erased, np.uint8).tobytes())

    for q in pairs:
        blob += keyframe(q["cam_1"], q["pose_1"], q["pos_w_1"], q["oct_1"], q["kp_1"], [0] * len(q["oct_1"]))
        blob += keyframe(q["cam_2"], q["pose_2"], q["pos_w_2"], q["oct_2"], q["kp_2"], q["erased_2"])
        blob += struct.pack("<i", len(q["matched"])) + np.asarray(q["matched"], "<i4").tobytes()
        blob += struct.pack("<13d", *q["R"], *q["t"], q["s"])
    path.write_bytes(blob)


def read_results(path, n_pairs):
    """out.bin: the pairs optimised one by one, then as one batch; per pair i32 num_inliers, 9 f64 rotation, 3 f64 translation, f64 scale, i32 n_1,
    n_1 u8 (1 where matched_lms_in_keyfrm_2 holds a landmark after the call). {"single": [...], "batch": [...]}, the doubles as bit patterns."""
    raw = path.read_bytes()
    at = 0
    out = {}
    for run in ("single", "batch"):
        out[run] = []
        for _ in range(n_pairs):
            (num,) = struct.unpack_from("<i", raw, at)
            v = struct.unpack_from("<13Q", raw, at + 4)
            (n1,) = struct.unpack_from("<i", raw, at + 108)
            at += 112
            out[run].append(dict(num_inliers=num, R=list(v[:9]), t=list(v[9:12]), s=v[12], kept=list(raw[at:at + n1])))
            at += n1
    assert at == len(raw)
    return out
