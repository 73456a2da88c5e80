"""The landmark upkeep on the device (csrc/landmark_update.hip, openvslam_amd.landmarks, cpp/openvslam/data/landmark_batch.h) against the
sequential reference tests/landmark_ref.py through the C ABI: every output byte for byte (a NaN as a NaN), on sentinel-filled arrays, so that
what a rule leaves untouched is seen untouched. Every scene is one of tests/landmark_ref.py's CASES, which tests/test_landmark_ref.py holds
to the sizes and contents they have to reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import landmark_io as io
import landmark_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def updater():
    from openvslam_amd import landmarks
    return landmarks.landmark_updater(0, max_landmarks=1024, max_total_observations=4096, max_keyframes=512)


def run(updater, case, what=3, **kw):
    out = kw.pop("out", None)
    out = lr.sentinel_outputs(len(case["offsets"]) - 1) if out is None else out
    args = dict(obs_desc=case["obs_desc"], obs_use=case["obs_use"], cam_centers=case["cam_centers"], scale_factors=case["scale_factors"])
    args.update(kw)
    return updater.update(what, case["offsets"], case["pos_w"], case["ref_keyfrm"], case["ref_level"], case["obs_keyfrm"], out=out, **args)


def same(got, want):
    names = ("mean_normal", "min_max_dist", "best_obs", "desc", "status")
    return [k for k, g, w in zip(names, lr.canon_bytes(got), lr.canon_bytes(want)) if g != w]


# ---- every size alone, the mixed batch, the batch sizes, the use patterns, the descriptor contents, the keyframe tables, L5, the levels
@pytest.mark.parametrize("name", lr.CASES)
def test_outputs_equal_the_reference_byte_for_byte(updater, name):
    assert same(run(updater, lr.case(name)), lr.expected(name)) == []


def test_mixed_batch_reaches_both_descriptor_kernels_and_equals_its_landmarks_alone(updater):
    c = lr.case("mixed")
    counts = np.diff(c["offsets"])
    assert set(lr.COUNTS) <= set(counts.tolist()) and (counts > 8).any() and ((counts > 0) & (counts <= 8)).any()
    got = run(updater, c)
    assert same(got, lr.expected("mixed")) == []
    for p in (0, 5, len(counts) - 1):   # a landmark's result does not depend on its place in the batch
        a, b = int(c["offsets"][p]), int(c["offsets"][p + 1])
        one = dict(c, offsets=np.array([0, b - a], np.int32), pos_w=c["pos_w"][p:p + 1], ref_keyfrm=c["ref_keyfrm"][p:p + 1], ref_level=c["ref_level"][p:p + 1],
                   obs_keyfrm=c["obs_keyfrm"][a:b], obs_desc=c["obs_desc"][a:b])
        alone = run(updater, one)
        assert same(alone, {k: v[p:p + 1] for k, v in got.items()}) == []


def test_unused_observations_leave_the_descriptor_untouched(updater):
    got = run(updater, lr.case("use_none"))
    assert got["best_obs"].tolist() == [lr.BEST_SENTINEL, -1, -1, -1] and (got["desc"] == lr.BYTE_SENTINEL).all()
    assert got["status"].tolist() == [1, 0, 0, 0] and (got["mean_normal"][1:] != lr.GEO_SENTINEL).all()   # the geometry does not read the flag
    assert run(updater, lr.case("use_first"))["best_obs"].tolist() == [0, 0, 0, 0]
    assert run(updater, lr.case("use_last"))["best_obs"].tolist() == [0, 4, 8, 69]


def test_tie_goes_to_the_earlier_row_and_a_landmark_at_a_centre_gives_nans(updater):
    assert run(updater, lr.case("tie"))["best_obs"].tolist() == [1, 1, 1]
    got = run(updater, lr.case("at_centre"))
    assert np.isnan(got["mean_normal"][:3]).all() and not np.isnan(got["mean_normal"][3]).any()


@pytest.mark.parametrize("name", ["mixed", "k300", "use_alt"])
def test_each_part_alone_gives_its_bytes_and_leaves_the_other_untouched(updater, name):
    c, both = lr.case(name), run(updater, lr.case(name))
    for what in (1, 2):
        assert same(run(updater, c, what), lr.expected(name, what)) == []
    geo = run(updater, c, 1, obs_desc=None)   # the arrays of the part not asked for may be NULL
    assert same(geo, lr.expected(name, 1)) == [] and geo["mean_normal"].tobytes() == both["mean_normal"].tobytes()
    dsc = updater.update(2, c["offsets"], None, None, None, None, obs_desc=c["obs_desc"], obs_use=c["obs_use"], out=lr.sentinel_outputs(len(c["offsets"]) - 1))
    assert same(dsc, lr.expected(name, 2)) == [] and dsc["desc"].tobytes() == both["desc"].tobytes()


# ---- the descriptors gathered on the device from resident keyframes
@pytest.fixture(scope="module")
def resident_scene():
    """The mixed case's observations as keypoints of twelve keyframes of different keypoint counts; each observation a keypoint of its own."""
    from openvslam_amd import match
    c = lr.make_case([0, 1, 2, 3, 7, 8, 9, 12, 5, 4, 11, 10], K=12, seed=31, use="alt")
    rng = np.random.default_rng(5)
    K = 12
    counts = [40 + 37 * k for k in range(K)]
    descs = [rng.integers(0, 256, (counts[k], 32), dtype=np.uint8) for k in range(K)]
    taken = [0] * K
    obs_kp = np.zeros(len(c["obs_keyfrm"]), np.int32)
    for t, k in enumerate(c["obs_keyfrm"]):
        idx = counts[k] - 1 - 3 * taken[k]
        taken[k] += 1
        descs[k][idx] = c["obs_desc"][t]
        obs_kp[t] = idx
    gp = match.grid_params(752, 480)
    devs = []
    for k in range(K):
        kp = np.zeros(counts[k], match.KP_DTYPE)
        kp["x"], kp["y"] = rng.uniform(1, 750, counts[k]), rng.uniform(1, 478, counts[k])
        devs.append(match.frame_dev(gp, kp, descs[k]))
    return c, devs, obs_kp, counts


def test_resident_form_equals_the_plain_form(updater, resident_scene):
    c, devs, obs_kp, _ = resident_scene
    plain = run(updater, c)
    assert same(plain, lr.expected_outputs(c)) == []
    for what in (3, 2, 1):
        got = run(updater, c, what, obs_desc=None, frame_devs=devs, obs_keypoint=obs_kp)
        assert same(got, lr.expected_outputs(c, what)) == []


def test_resident_form_refuses_a_keypoint_outside_its_handle_and_a_null_handle(updater, resident_scene):
    from openvslam_amd import _lib
    c, devs, obs_kp, counts = resident_scene
    out = lr.sentinel_outputs(len(c["offsets"]) - 1)
    for t in (0, len(obs_kp) - 1):
        for bad in (-1, counts[int(c["obs_keyfrm"][t])]):
            kp = obs_kp.copy()
            kp[t] = bad
            with pytest.raises(_lib.OvsError) as e:
                run(updater, c, 3, obs_desc=None, frame_devs=devs, obs_keypoint=kp, out=out)
            assert e.value.status == INVALID
    L, vp = _lib.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    handles = (C.c_void_p * len(devs))(*[f._h.value for f in devs])
    handles[3] = None
    st = L.ovs_landmarks_update_batch_f(updater._h, 3, len(c["offsets"]) - 1, vp(c["offsets"]), vp(c["pos_w"]), vp(c["ref_keyfrm"]), vp(c["ref_level"]),
                                        vp(c["obs_keyfrm"]), handles, vp(obs_kp), vp(c["obs_use"]), vp(c["cam_centers"]), len(devs), vp(c["scale_factors"]),
                                        lr.NUM_LEVELS, vp(out["mean_normal"]), vp(out["min_max_dist"]), vp(out["best_obs"]), vp(out["desc"]), vp(out["status"]))
    assert st == INVALID
    assert same(out, lr.sentinel_outputs(len(c["offsets"]) - 1)) == []
    if L.ovs_device_count() > 1:   # a handle from another device
        from openvslam_amd import match
        kp = np.zeros(counts[0], match.KP_DTYPE)
        other = match.frame_dev(match.grid_params(752, 480), kp, np.zeros((counts[0], 32), np.uint8), device=1)
        with pytest.raises(_lib.OvsError) as e:
            run(updater, c, 3, obs_desc=None, frame_devs=[other] + devs[1:], obs_keypoint=obs_kp, out=out)
        assert e.value.status == INVALID and same(out, lr.sentinel_outputs(len(c["offsets"]) - 1)) == []


# ---- capacity and argument errors return before anything is written and leave the handle usable
def test_error_contract_handle_reuse_and_no_leak():
    from openvslam_amd import _lib, landmarks
    L = _lib.lib()
    live = L.ovs_debug_live_resources()
    u = landmarks.landmark_updater(0, max_landmarks=8, max_total_observations=140, max_keyframes=6)
    small, large = lr.case("use_first"), lr.case("n130")
    ok = lambda: same(run(u, large), lr.expected("n130")) == [] and same(run(u, small), lr.expected("use_first")) == [] and \
        same(run(u, large), lr.expected("n130")) == []   # a large call leaves nothing behind for a small one
    assert ok()
    c = lr.case("n9")
    out = lr.sentinel_outputs(4)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(what=3, n=1, K=len(c["cam_centers"]), levels=lr.NUM_LEVELS, **over):
        a = dict(c, **out)
        a.update(over)
        return L.ovs_landmarks_update_batch(u._h, what, n, vp(a["offsets"]), vp(a["pos_w"]), vp(a["ref_keyfrm"]), vp(a["ref_level"]), vp(a["obs_keyfrm"]),
                                            vp(a["obs_desc"]), vp(a["obs_use"]), vp(a["cam_centers"]), K, vp(a["scale_factors"]), levels, vp(a["mean_normal"]),
                                            vp(a["min_max_dist"]), vp(a["best_obs"]), vp(a["desc"]), vp(a["status"]))

    i32 = lambda *v: np.array(v, np.int32)
    for key in ("offsets", "pos_w", "ref_keyfrm", "ref_level", "obs_keyfrm", "obs_desc", "cam_centers", "scale_factors", "mean_normal", "min_max_dist", "best_obs",
                "desc", "status"):
        assert call(**{key: None}) == INVALID, key
    assert call(what=0) == INVALID and call(what=4) == INVALID and call(n=-1) == INVALID
    assert call(offsets=i32(1, 9)) == INVALID and call(n=2, offsets=i32(0, 9, 5)) == INVALID
    assert call(levels=0) == INVALID and call(levels=17) == INVALID
    bad_slot = c["obs_keyfrm"].copy()
    bad_slot[8] = len(c["cam_centers"])
    assert call(obs_keyfrm=bad_slot) == INVALID and call(obs_keyfrm=-1 - c["obs_keyfrm"]) == INVALID
    assert call(ref_keyfrm=i32(6)) == INVALID and call(ref_keyfrm=i32(-1)) == INVALID and call(K=int(c["obs_keyfrm"].max())) == INVALID
    assert call(ref_level=i32(lr.NUM_LEVELS)) == INVALID and call(ref_level=i32(-1)) == INVALID and call(ref_level=i32(3), levels=3) == INVALID
    assert same(out, lr.sentinel_outputs(4)) == []
    nine = np.arange(10, dtype=np.int32)
    assert call(n=9, offsets=nine) == CAPACITY                          # more landmarks than the handle was created for
    assert call(offsets=i32(0, 141)) == CAPACITY                        # more observations (refused before anything is read)
    assert call(K=7, cam_centers=np.zeros((7, 3))) == CAPACITY          # more keyframes
    assert same(out, lr.sentinel_outputs(4)) == []                      # nothing truncated, nothing written
    assert call(n=0) == 0 and same(out, lr.sentinel_outputs(4)) == []   # no landmarks: nothing to do
    assert call(n=2, offsets=i32(0, 0, 0)) == 0                         # no observations is not an error
    assert out["status"].tolist() == [1, 1, lr.BYTE_SENTINEL, lr.BYTE_SENTINEL] and (out["best_obs"] == lr.BEST_SENTINEL).all()
    assert call(what=2, pos_w=None, ref_keyfrm=None, ref_level=None, obs_keyfrm=None, cam_centers=None, scale_factors=None, mean_normal=None, min_max_dist=None,
                K=0, levels=0) == 0                                     # the descriptor alone reads none of the geometry's arguments
    assert ok()
    del u
    assert L.ovs_debug_live_resources() == live


# ---- a loaded map: update_map is the step after load_map_database
@pytest.fixture(scope="module")
def small_map():
    from openvslam_amd import synth
    db, scene = synth.synth_map(n_pose=6, n_pt=200, obs_per_pose=120, seed=3, pose_noise=0.0, point_noise=0.0)
    rng = np.random.default_rng(9)
    base = {lid: rng.integers(0, 256, 32, dtype=np.uint8) for lid in db.landmarks}
    for kf in db.keyframes.values():   # a landmark's observations look alike, as an extractor's would
        for i, lid in enumerate(kf.lm_ids):
            kf.descs[i] = synth.flip_bits(rng, base[int(lid)], 12)
    return db, scene


def test_update_map_equals_the_reference_per_landmark_and_feeds_a_matcher(small_map):
    from openvslam_amd import _lib, ba, landmarks, match
    db, scene = small_map
    assert all(lm.descriptor is None and lm.mean_normal is None and lm.min_valid_dist is None and lm.max_valid_dist is None for lm in db.landmarks.values())
    u = landmarks.landmark_updater(0, max_landmarks=64, max_total_observations=1024, max_keyframes=8)   # 64 per call: the map takes several chunks
    assert len(db.landmarks) > 64 and u.update_map(db) == len(db.landmarks)
    obs, kf_ids = db.observations(), sorted(db.keyframes)
    centres = {k: landmarks.cam_center_of(db.keyframes[k].rot_cw, db.keyframes[k].trans_cw) for k in kf_ids}
    sf = landmarks.scale_factors_of(1.2, 8)
    for lid, lm in db.landmarks.items():
        mine = obs[lid]
        level = int(db.keyframes[lm.ref_keyfrm].keypts["octave"][[i for k, i in mine if k == lm.ref_keyfrm][0]])
        normal, mn, mx = lr.geometry(lm.pos_w, [centres[k] for k, _ in mine], centres[lm.ref_keyfrm], sf[level], sf[-1])
        descs = [db.keyframes[k].descs[i].tobytes() for k, i in mine]
        assert np.array(normal).tobytes() == lm.mean_normal.tobytes() and (np.float32(lm.min_valid_dist), np.float32(lm.max_valid_dist)) == (mn, mx)
        assert lm.descriptor.tobytes() == descs[lr.descriptor(descs, [1] * len(descs))]
    # keyframe 1's landmarks searched in keyframe 0 taken as the current frame: the stored ranges and descriptors are what the matcher reads
    cam = db.cameras["cam"]
    cur, kf = db.keyframes[0], db.keyframes[1]
    Tc = np.concatenate([ba.quat_to_rot(cur.rot_cw), np.asarray(cur.trans_cw).reshape(3, 1)], 1)
    lms = [db.landmarks[int(l)] for l in kf.lm_ids]
    dmm = np.array([[l.min_valid_dist, l.max_valid_dist] for l in lms], np.float32)
    w = match.projection(0.9, False, max_targets=512, max_queries=512)
    assigned, n = w.match_frame_and_keyframe(_lib.Camera(0, 0, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.0, 0.0, cam["cols"], cam["rows"]),
                                             match.grid_params(cam["cols"], cam["rows"]), cur.keypts, cur.descs, Tc, kf.keypts,
                                             np.array([l.pos_w for l in lms]), dmm, np.array([l.descriptor for l in lms]), sf, float(np.log(np.float32(1.2))), 20.0, 80)
    shared = set(int(l) for l in cur.lm_ids) & set(int(l) for l in kf.lm_ids)
    hits = [(int(kf.lm_ids[i]), int(cur.lm_ids[j])) for i, j in enumerate(assigned) if j >= 0]
    print("shared landmarks", len(shared), "matches", n)
    assert n == len(hits) and n >= len(shared) // 2 > 5 and sum(1 for a, b in hits if a == b) >= len(hits) * 9 // 10


# ---- the C++ batch form on stub keyframes
def test_cpp_update_landmarks_equals_the_reference(tmp_path):
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_landmark_shim"]))
    case = lr.make_case([0, 1, 2, 3, 7, 8, 9, 12, 5, 4], K=12, seed=41)
    erased = (2, 7)
    scene, order = io.shim_scene(case, [30 + 11 * k for k in range(12)], erased=erased)
    (tmp_path / "scene.bin").write_bytes(scene)
    r = subprocess.run([os.path.join(cpp, "test_landmark_shim" + SUFFIX), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "update_landmarks ok" in r.stdout and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    assert "caller errors thrown 2" in r.stdout
    handed = io.reordered(case, order, erased)
    want = lr.solve(handed)
    assert any(u == 0 for u in handed["obs_use"])
    got = io.shim_results((tmp_path / "out.bin").read_bytes(), len(want))
    bits = lambda v, t, u: np.array(v, t).view(u).tolist()
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["updates"] == 1, p
        if w["status"] == 1:   # left as it was
            assert g["normal"][0] == bits([-7.0], np.float64, np.uint64)[0] and g["range"] == bits([-3.0, -3.0], np.float32, np.uint32) and g["desc"] == b""
            continue
        assert g["normal"] == bits(w["normal"], np.float64, np.uint64) and g["range"] == bits([w["min_valid"], w["max_valid"]], np.float32, np.uint32), p
        assert g["desc"] == (w["desc"] or b""), p   # (none where every observing keyframe is being erased)
    # an erased keyframe is left out of the descriptor but not of the normal: the reference with every observation taking part differs somewhere
    everyone = lr.solve(dict(handed, obs_use=None))
    assert [w["normal"] for w in want] == [w["normal"] for w in everyone] and [w["best_obs"] for w in want] != [w["best_obs"] for w in everyone]
