"""The sequential triangulation reference (tests/triangulate_ref.py; DESIGN.md 3.12, rules T1 to T9) checked on its own, and the algebra the
device shares (openvslam_amd/csrc/triangulate_math.inc) held to it without a device: on noise-free scenes the reference returns the true point
and agrees with numpy's SVD of the same system, the named cases reach every status code and every method, and a stand-alone host program
built from the shared file by the plain host compiler gives the reference's bits on every case -- and runs clean under AddressSanitizer and
UndefinedBehaviorSanitizer. Plus the Python helper's gathering, the C ABI's argument errors, which are decided before the device is touched,
and the C++ class's empty result when its device is absent."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import transform_ref as tr
import triangulate_io as io
import triangulate_ref as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
PARALLAX_DEG, DEPTHS = (1.2, 2.0, 5.0, 10.0, 20.0, 40.0, 60.0), (0.5, 2.0, 10.0, 50.0)
# Measured: the largest relative distance between the reference's point (the eigenvector of A^T A by eight Jacobi sweeps) and numpy's SVD of the
# same A over the 168 scenes below (at 1.2 degrees of parallax and depth 2). The factor ten covers other hosts' LAPACK.
SVD_GAP = 1.6e-14
# The true point: every entry of A carries a few roundings of 1.1e-16, and the null vector of A^T A moves by them times the square of A's
# condition number, 1 / sin^2(1.2 degrees) = 2280 at the narrowest scene: 2.5e-13, with a factor four for the number of roundings.
TRUE_POINT_BOUND = 1e-12


# ---- T4 against the planted point and against another decomposition
def test_noise_free_scenes_return_the_true_point_and_agree_with_the_svd():
    worst_gap, worst_true = 0.0, 0.0
    for parallax in PARALLAX_DEG:
        for depth in DEPTHS:
            for k in range(6):
                q, X = tri.parallax_scene(parallax, depth, k)
                r = tri.triangulate(q, 0)
                assert (r["status"], r["method"]) == (0, 1), (parallax, depth, k, r)
                A = np.array(tri.dlt_rows(q["pose_1"], q["pose_2"], q["b1"][0], q["b2"][0]))
                v = np.linalg.svd(A)[2][3]
                svd = v[:3] / v[3]
                got = np.array(r["pos_w"])
                worst_gap = max(worst_gap, float(np.linalg.norm(got - svd) / np.linalg.norm(svd)))
                worst_true = max(worst_true, float(np.linalg.norm(got - np.array(X)) / np.linalg.norm(X)))
    print("largest relative distance from the SVD's point:", worst_gap, "from the true point:", worst_true)
    assert worst_gap <= 10 * SVD_GAP
    assert worst_true <= TRUE_POINT_BOUND


def test_float_keypoints_still_give_the_point_to_a_millimetre_per_metre_of_depth():
    """The scenes the device tests use derive the bearing from the float keypoint, as a frame does: a 3e-5 pixel rounding at 5 degrees."""
    q, X = tri.parallax_scene(5.0, 4.0, 1, exact=False)
    r = tri.triangulate(q, 0)
    assert r["status"] == 0 and max(abs(a - b) for a, b in zip(r["pos_w"], X)) < 4e-3


# ---- the scenes
def test_every_case_reaches_the_codes_and_methods_the_table_names():
    for name, (statuses, methods) in tri.REACHES.items():
        got = tri.solved(name)
        assert {r["status"] for r in got} >= statuses, (name, sorted({r["status"] for r in got}))
        assert {r["method"] for r in got} >= methods, (name, sorted({r["method"] for r in got}))
    assert set().union(*(s for s, _ in tri.REACHES.values())) == set(range(7))
    assert set().union(*(m for _, m in tri.REACHES.values())) == set(range(4))
    for name in tri.REJECTS:   # a reject scene holds nothing but its gate
        assert len({(r["status"], r["method"]) for r in tri.solved(name)}) == 1, name


def test_spoiled_matches_end_at_their_gate():
    q, got = tri.problem("n257"), tri.solved("n257")
    want = {"good": 0, "far": 1, "kp1": 4, "kp2": 5, "octave": 6}
    assert [r["status"] for r in got] == [want[k] for k in q["kinds"]]
    for r, X in zip(got, q["truth"]):
        if r["status"] == 0:   # depth error z^2 * (0.3 * sqrt(2) px) / (458 px * 0.6 m): 1.4 % of the depth at 9 m, less nearer; 5 % is over three of them
            assert max(abs(a - b) for a, b in zip(r["pos_w"], X)) < 0.05 * X[2]


def test_status_one_returns_zeros_and_a_non_finite_match_is_rejected():
    assert all(r["pos_w"] == [0.0, 0.0, 0.0] and r["method"] == 0 for r in tri.solved("low_parallax"))
    bad, clean = tri.solved("nan_inf"), tri.solved("nan_inf_clean")
    assert bad[17]["status"] == 2 and bad[17]["method"] == 2 and clean[17]["status"] == 0
    assert tri.result_bits(bad[:17] + bad[18:]) == tri.result_bits(clean[:17] + clean[18:])


def test_ratio_factor_and_threshold_are_the_callers():
    assert tri.RATIO_FACTOR == float(np.float32(1.5) * np.float32(1.2)) and tri.COS_THR == tr.det_cos(1.0 * math.pi / 180.0)
    assert abs(tri.COS_THR - math.cos(math.radians(1.0))) < 1e-15


# ---- the shared algebra through a plain host compiler
@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("triangulate_host") / "cases.bin"
    path.write_bytes(io.host_input([tri.problem(k) for k in tri.CASES]))
    return str(path)


def expected_rows():
    return [row for k in tri.CASES for row in tri.result_bits(tri.solved(k))]


def test_host_program_gives_the_reference_bits_on_every_case(case_file):
    subprocess.check_call(["make", "-s", "-C", CPP, "triangulate_host"])
    r = subprocess.run([os.path.join(CPP, "triangulate_host"), case_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got, want = io.host_output(r.stdout), expected_rows()
    assert len(got) == len(want) == sum(len(tri.problem(k)["b1"]) for k in tri.CASES)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


def test_host_program_runs_clean_under_the_sanitizers(case_file, tmp_path):
    exe = str(tmp_path / "triangulate_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-I",   # (the runtimes inside the program: it stands alone)
                           os.path.join(ROOT, "openvslam_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "triangulate_host.cc")])
    r = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert io.host_output(r.stdout) == expected_rows()


# ---- the Python mirror's gathering
def _python_keyframe(solve, kf):
    cam = {k: v for k, v in kf["cam"].items() if k not in ("focal_x_baseline", "true_baseline")}
    camera = solve.camera(**cam)
    camera.focal_x_baseline, camera.true_baseline = kf["cam"]["focal_x_baseline"], kf["cam"]["true_baseline"]
    return dict(undist_keypts=np.array(kf["keypts"], np.float32), stereo_x_right=np.array(kf["x_right"], np.float32), depths=np.array(kf["depths"], np.float32),
                bearings=np.array(kf["bearings"]), octaves=np.array(kf["octaves"]), scale_factors=tri.SCALE_FACTORS, level_sigma_sq=tri.LEVEL_SIGMA_SQ,
                scale_factor=tri.SCALE_FACTOR, pose_cw=np.array(kf["pose"]).reshape(4, 4), camera=camera)


def test_python_helper_gathers_what_the_problem_holds():
    from openvslam_amd import solve
    problems = io.class_scene()
    curr, neighbours, matches = io.keyframes_of(problems)
    k1 = _python_keyframe(solve, curr)
    for q, kf, m in zip(problems, neighbours, matches):
        k2 = _python_keyframe(solve, kf)
        t = solve.two_view_triangulator(k1, k2)
        got = t.problem(m)
        assert float(t._ratio_factor) == tri.RATIO_FACTOR and t._cos_thr == tri.COS_THR
        assert got["bearings_1"].tolist() == [list(b) for b in q["b1"]] and got["bearings_2"].tolist() == [list(b) for b in q["b2"]]
        for key, ref in (("keypts_1", "kp1"), ("keypts_2", "kp2")):
            assert got[key].tolist() == [list(v) for v in q[ref]]
        for key, ref in (("x_right_1", "xr1"), ("x_right_2", "xr2"), ("depths_1", "depth1"), ("depths_2", "depth2"), ("sigma_sq_1", "sig1"),
                         ("sigma_sq_2", "sig2"), ("scale_factors_1", "sf1"), ("scale_factors_2", "sf2")):
            assert got[key].dtype == np.float32 and got[key].tolist() == q[ref], key
        assert got["pose_cw_1"].tolist() == q["pose_1"] and got["pose_cw_2"].tolist() == q["pose_2"]
        # the matcher's own form: entry idx_1 holds idx_2
        matched = np.full(len(curr["octaves"]), -1, np.int32)
        for a, b in m:
            matched[a] = b
        again = solve.triangulation_problem_from_keyframes(matched, k1["undist_keypts"], k2["undist_keypts"], k1["stereo_x_right"], None, k1["depths"], None,
                                                           k1["bearings"], k2["bearings"], k1["octaves"], k2["octaves"], tri.SCALE_FACTORS, tri.LEVEL_SIGMA_SQ,
                                                           k1["pose_cw"], k2["pose_cw"], k1["camera"], k2["camera"])
        assert sorted(zip(again["idx_1"].tolist(), again["idx_2"].tolist())) == sorted(m) and (again["x_right_2"] == -1.0).all()


def test_python_cosine_is_the_headers():
    from openvslam_amd import solve
    xs = [k / 997.0 for k in range(-7000, 7000)] + [1e-9, 100.0, 1048576.0, 2e6, float("inf")]
    for x in xs:
        a, b = solve._det_cos(x), tr.det_cos(x)
        assert (a != a and b != b) or a == b, x


# ---- the C ABI without a device in the way: every argument error is decided before the device is touched
def test_abi_argument_errors_come_before_the_device():
    from openvslam_amd import _lib, solve
    L = _lib.lib()
    INVALID, NO_DEVICE = -1, -2
    h = C.c_void_p()
    assert L.ovs_triangulate_create(0, 0, 100, C.byref(h)) == INVALID and L.ovs_triangulate_create(0, 4, 0, C.byref(h)) == INVALID
    assert L.ovs_triangulate_create(0, 4, 100, None) == INVALID
    assert L.ovs_triangulate_create(99, 4, 100, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_triangulate_create(-1, 4, 100, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_triangulate_destroy(None) == INVALID
    off = np.array([0, 2], np.int32)
    d, f = np.zeros((2, 3)), np.zeros((2, 2), np.float32)
    cams = (_lib.Camera * 1)(solve.camera(0, 458, 457, 367, 248))
    pose, out_d, out_b, out_i = np.zeros(12), np.full(6, -7.0), np.full(4, 9, np.uint8), np.full(2, -7, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda handle, thr, ratio: L.ovs_triangulate_batch(handle, 1, vp(off), vp(d), vp(d), *([vp(f)] * 10), cams, cams, vp(pose), vp(pose), thr, ratio,
                                                              vp(out_d), vp(out_b), vp(out_b), vp(out_i))
    assert call(None, 0.99, 1.8) == INVALID
    fake = C.c_void_p(1)   # never dereferenced: these are refused before the handle is read
    for thr, ratio in ((float("nan"), 1.8), (float("inf"), 1.8), (0.99, float("nan")), (0.99, float("inf")), (0.99, float("-inf"))):
        assert call(fake, thr, ratio) == INVALID
    assert (out_d == -7.0).all() and (out_b == 9).all() and (out_i == -7).all()
    with pytest.raises(_lib.OvsError):   # the Python mirror raises: no device 99 anywhere
        solve._triangulate_handle(4, 16, device=99)


def test_cpp_class_degrades_without_its_device(tmp_path):
    """The wrapper alone: on a device that does not exist the class accepts nothing and throws nothing."""
    subprocess.check_call(["make", "-s", "-C", CPP, "test_triangulate_shim"])
    problems = io.class_scene()
    curr, neighbours, matches = io.keyframes_of(problems)
    io.write_scene(tmp_path / "scene.bin", curr, neighbours, matches)
    r = subprocess.run([os.path.join(CPP, "test_triangulate_shim"), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "99"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = io.read_results(tmp_path / "out.bin", len(problems))
    for section in got.values():
        for g, q in zip(section, problems):
            assert g["num_accepted"] == 0 and g["accepted"] == [0] * len(q["b1"]) and all(p == [0, 0, 0] for p in g["pos"])
    calls = sum(len(q["b1"]) for q in problems) + len(problems) + 1
    assert "ABI calls failed %d, degraded %d" % (calls, calls) in r.stdout
