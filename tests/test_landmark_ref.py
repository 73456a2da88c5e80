"""The sequential reference of the landmark upkeep (tests/landmark_ref.py; DESIGN.md 3.14, rules L1 to L9) checked on its own, and the algebra
the device shares (openvslam_amd/csrc/landmark_math.inc) held to it without a device: hand-computed descriptor sets pin rules L6 to L9, a value
where the two orders of rounding differ pins rule L4, and a stand-alone host program built from the shared file by the plain host compiler
gives the reference's bits on every case -- and runs clean under AddressSanitizer and UndefinedBehaviorSanitizer. Plus the C ABI's argument
errors, which are decided before the device is touched, and the Python layer's tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import landmark_io as io
import landmark_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
A = bytes((37 * k + 11) & 0xFF for k in range(32))


# ---- rules L6 to L9 by hand
def test_one_and_two_descriptors_have_median_zero_and_the_first_wins():
    b = lr.flip(A, 0, 9, 100)
    assert lr.medians([A]) == [0] and lr.descriptor([A], [1]) == 0
    assert lr.hamming(A, b) == 3 and lr.medians([A, b]) == [0, 0] and lr.descriptor([A, b], [1, 1]) == 0 and lr.descriptor([b, A], [1, 1]) == 0


def test_three_descriptors_the_middle_one_wins_and_a_tie_goes_to_the_earlier_row():
    # d(a, b) = 3, d(b, c) = 1, d(a, c) = 4: rows sorted [0 3 4] [0 1 3] [0 1 4], medians 3 1 1: b and c tie, b is earlier
    a, b = A, lr.flip(A, 1, 2, 3)
    c = lr.flip(b, 200)
    assert (lr.hamming(a, b), lr.hamming(b, c), lr.hamming(a, c)) == (3, 1, 4)
    assert lr.medians([a, b, c]) == [3, 1, 1] and lr.descriptor([a, b, c], [1, 1, 1]) == 1
    assert lr.descriptor([a, c, b], [1, 1, 1]) == 1 and lr.descriptor([c, b, a], [1, 1, 1]) == 0   # always the earlier of the tied two
    # four: the median is element floor(0.5 * 3) = 1 of the sorted row, the nearest other descriptor
    d = lr.flip(A, 1)
    assert lr.medians([a, b, c, d]) == [1, 1, 1, 1] and lr.descriptor([a, b, c, d], [1] * 4) == 0


def test_all_identical_descriptors_give_the_first():
    assert lr.medians([A] * 5) == [0] * 5 and lr.descriptor([A] * 5, [1] * 5) == 0


def test_a_complement_pair_and_a_third():
    na = lr.complement(A)
    c = lr.flip(A, *range(200))
    assert lr.hamming(A, na) == 256 and lr.hamming(A, c) == 200 and lr.hamming(na, c) == 56
    assert lr.medians([A, na, c]) == [200, 56, 56] and lr.descriptor([A, na, c], [1, 1, 1]) == 1
    assert lr.medians([A, na, na]) == [256, 0, 0] and lr.descriptor([A, na, na], [1, 1, 1]) == 1
    assert lr.medians([A, A, na]) == [0, 0, 256] and lr.descriptor([A, A, na], [1, 1, 1]) == 0


def test_the_tie_scene_ties_and_row_one_wins():
    import random
    descs = lr.tie_descriptors(random.Random(4))
    assert lr.medians(descs) == [4, 2, 2, 4, 2, 4] and lr.descriptor(descs, [1] * 6) == 1
    for r in lr.solved("tie"):
        assert r["best_obs"] == 1


def test_only_flagged_observations_take_part_and_the_position_is_the_full_lists():
    a, b = A, lr.flip(A, 1, 2, 3)
    c = lr.flip(b, 200)
    assert lr.descriptor([a, b, c], [0, 0, 0]) == -1
    assert lr.descriptor([a, b, c], [0, 0, 1]) == 2 and lr.descriptor([a, b, c], [0, 1, 1]) == 1 and lr.descriptor([a, a, b, c], [1, 0, 1, 1]) == 2
    assert [r["best_obs"] for r in lr.solved("use_none")] == [None, -1, -1, -1] and [r["status"] for r in lr.solved("use_none")] == [1, 0, 0, 0]
    use = lr.case("use_alt")["obs_use"]
    off = lr.case("use_alt")["offsets"]
    assert [int(use[off[p]:off[p + 1]].sum()) for p in range(6)] == [8, 8, 9, 9, 1, 1]


# ---- rules L2 to L5
def test_range_rounds_the_double_product_once():
    sf = lr.SCALE_FACTORS
    found = None
    for i in range(1, 400):
        dist = 1.0 + i / 397.0
        once, twice = np.float32(np.float64(dist) * np.float64(sf[1])), np.float32(np.float32(dist) * sf[1])
        if once != twice:
            found = dist
            break
    assert found is not None
    _, mn, mx = lr.geometry([found, 0.0, 0.0], [[0.0, 0.0, 0.0]], [0.0, 0.0, 0.0], sf[1], sf[-1])
    assert mx == once and mx != twice and mx.dtype == np.float32
    assert mn == np.float32(once / sf[-1]) and mn.dtype == np.float32   # a float division of the rounded maximum


def test_normal_is_the_sequential_mean_of_unit_rays():
    n, mn, mx = lr.geometry([0.0, 0.0, 2.0], [[0.0, 0.0, 0.0], [2.0, 0.0, 2.0]], [0.0, 0.0, 0.0], np.float32(1.0), np.float32(2.0))
    assert [float(v) for v in n] == [-0.5, 0.0, 0.5] and (float(mn), float(mx)) == (1.0, 2.0)
    # the order of the list is part of the bits and of nothing else: the reversed list gives the same mean to the last few ulps
    c = [[0.1, 0.2, 0.3], [-4.0, 1.0, 0.5], [3.0, -2.0, 0.7], [0.3, 0.3, -9.0], [1e-3, 5.0, 2.0]]
    fwd = lr.geometry([0.7, -0.3, 5.0], c, c[0], np.float32(1.0), np.float32(2.0))[0]
    rev = lr.geometry([0.7, -0.3, 5.0], c[::-1], c[0], np.float32(1.0), np.float32(2.0))[0]
    assert max(abs(float(a) - float(b)) for a, b in zip(fwd, rev)) < 1e-15
    assert abs(sum(float(v) ** 2 for v in fwd) ** 0.5 - 1.0) < 0.5   # a mean of unit vectors


def test_a_landmark_at_a_camera_centre_gives_nans_and_an_empty_list_nothing():
    got = lr.solved("at_centre")
    for r in got[:3]:
        assert all(np.isnan(v) for v in r["normal"]) and r["status"] == 0 and r["best_obs"] >= 0
    assert not any(np.isnan(v) for v in got[3]["normal"])
    r = lr.solved("n0")[0]
    assert r == dict(status=1, normal=None, min_valid=None, max_valid=None, best_obs=None, desc=None)
    out = lr.expected("n0")
    assert out["status"].tolist() == [1] and (out["mean_normal"] == lr.GEO_SENTINEL).all() and (out["desc"] == lr.BYTE_SENTINEL).all()


def test_cases_cover_the_sizes_the_kernels_switch_at():
    assert [int(lr.case("n%d" % c)["offsets"][1]) for c in lr.COUNTS] == list(lr.COUNTS)
    assert [len(lr.case("batch%d" % n)["offsets"]) - 1 for n in lr.BATCHES] == list(lr.BATCHES)
    k300 = lr.case("k300")
    assert len(k300["cam_centers"]) == 300 > lr.LDS_CENTRES and (k300["obs_keyfrm"] >= lr.LDS_CENTRES).any() and (k300["obs_keyfrm"] < lr.LDS_CENTRES).any()
    assert len(lr.case("k1")["cam_centers"]) == 1
    assert set(lr.case("ref_levels")["ref_level"].tolist()) == {0, lr.NUM_LEVELS - 1}
    second = lr.case("extremes")["obs_desc"][2:5]   # the landmark of three observations: a descriptor, itself and its complement
    dists = {lr.hamming(a, b) for a in second for b in second}
    assert dists == {0, 256}


# ---- the shared algebra through a plain host compiler
@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("landmark_host")
    for name in lr.CASES:
        (d / (name + ".bin")).write_bytes(io.host_input(lr.case(name)))
    return d


def _held_to_the_reference(exe, case_files, timeout):
    for name in lr.CASES:
        r = subprocess.run([exe, str(case_files / (name + ".bin"))], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr)
        assert lr.canon_bytes(io.host_output(r.stdout)) == lr.canon_bytes(lr.expected(name)), name


def test_host_program_gives_the_reference_bits_on_every_case(case_files):
    subprocess.check_call(["make", "-s", "-C", CPP, "landmark_host"])
    _held_to_the_reference(os.path.join(CPP, "landmark_host"), case_files, 120)


def test_host_program_runs_clean_under_the_sanitizers(case_files, tmp_path):
    exe = str(tmp_path / "landmark_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I",   # (the runtimes inside the program: it stands alone)
                           os.path.join(ROOT, "openvslam_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "landmark_host.cc")])
    _held_to_the_reference(exe, case_files, 300)


# ---- the Python layer's tables
def test_python_tables():
    from openvslam_amd import io as map_io, landmarks
    assert landmarks.scale_factors_of(1.2, lr.NUM_LEVELS).tobytes() == lr.SCALE_FACTORS.tobytes()
    assert landmarks.cam_center_of([0, 0, 0, 1], [1.0, -2.0, 3.0]).tolist() == [-1.0, 2.0, -3.0]
    s = 0.5 ** 0.5   # a quarter turn about z: R = [[0 -1 0] [1 0 0] [0 0 1]], -R^T t
    assert np.allclose(landmarks.cam_center_of([0, 0, s, s], [1.0, 2.0, 3.0]), [-2.0, 1.0, -3.0], atol=1e-15)
    lm = map_io.landmark(id=1, first_keyfrm=0, pos_w=np.zeros(3), ref_keyfrm=0)
    assert lm.descriptor is None and lm.mean_normal is None and lm.min_valid_dist is None and lm.max_valid_dist is None


# ---- the C ABI without a device in the way: every argument error is decided before the device is touched
def test_abi_argument_errors_come_before_the_device():
    from openvslam_amd import _lib, landmarks
    L = _lib.lib()
    INVALID, NO_DEVICE = -1, -2
    h = C.c_void_p()
    for args in ((0, 100, 4), (4, 0, 4), (4, 100, 0), (65536, 100, 4)):
        assert L.ovs_landmarks_create(0, *args, C.byref(h)) == INVALID and not h
    assert L.ovs_landmarks_create(0, 4, 100, 4, None) == INVALID
    assert L.ovs_landmarks_create(99, 4, 100, 4, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_landmarks_create(-1, 4, 100, 4, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_landmarks_destroy(None) == INVALID
    c = lr.case("n3")
    out = lr.sentinel_outputs(1)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(handle=C.c_void_p(1), what=3, n=1, offsets=c["offsets"], levels=lr.NUM_LEVELS, K=len(c["cam_centers"]), **drop):
        a = {k: (None if k in drop else v) for k, v in dict(c, **out).items()}
        return L.ovs_landmarks_update_batch(handle, what, n, vp(offsets), vp(a["pos_w"]), vp(a["ref_keyfrm"]), vp(a["ref_level"]), vp(a["obs_keyfrm"]), vp(a["obs_desc"]),
                                            None, vp(a["cam_centers"]), K, vp(a["scale_factors"]), levels, vp(a["mean_normal"]), vp(a["min_max_dist"]),
                                            vp(a["best_obs"]), vp(a["desc"]), vp(a["status"]))

    # (the handle 1 is never dereferenced: these are refused before it is read)
    assert call(handle=None) == INVALID
    assert call(what=0) == INVALID and call(what=4) == INVALID and call(what=-1) == INVALID and call(n=-1) == INVALID
    assert call(n=0) == 0
    assert call(levels=0) == INVALID and call(levels=17) == INVALID and call(K=-1) == INVALID
    assert call(offsets=None) == INVALID and call(offsets=np.array([1, 3], np.int32)) == INVALID and call(n=2, offsets=np.array([0, 3, 2], np.int32)) == INVALID
    for key in ("pos_w", "ref_keyfrm", "ref_level", "obs_keyfrm", "obs_desc", "cam_centers", "scale_factors", "mean_normal", "min_max_dist", "best_obs", "desc", "status"):
        assert call(**{key: True}) == INVALID, key
    assert lr.canon_bytes(out) == lr.canon_bytes(lr.sentinel_outputs(1))
    with pytest.raises(_lib.OvsError):   # the Python mirror raises: no device 99 anywhere
        landmarks.landmark_updater(device=99, max_landmarks=4, max_total_observations=16, max_keyframes=4)


def test_cpp_batch_form_degrades_without_its_device_and_throws_on_caller_errors(tmp_path):
    """The wrapper alone: on a device that does not exist the landmarks are left as they were and nothing is thrown; the two caller errors are
    decided before the device is touched."""
    subprocess.check_call(["make", "-s", "-C", CPP, "test_landmark_shim"])
    case = lr.make_case([0, 1, 2, 3, 7, 5], K=8, seed=41)
    scene, _ = io.shim_scene(case, [20 + 5 * k for k in range(8)])
    (tmp_path / "scene.bin").write_bytes(scene)
    r = subprocess.run([os.path.join(CPP, "test_landmark_shim"), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "99"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "update_landmarks degraded" in r.stdout and "caller errors thrown 2" in r.stdout and "ABI calls failed 1, degraded 1" in r.stdout
    for g in io.shim_results((tmp_path / "out.bin").read_bytes(), 6):
        assert g["updates"] == 0 and g["desc"] == b"" and g["range"] == np.array([-3.0, -3.0], np.float32).view(np.uint32).tolist()
