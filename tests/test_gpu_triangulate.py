"""The triangulator on the device (csrc/triangulate.hip, openvslam_amd.solve, cpp/openvslam/module/two_view_triangulator.h) against the
sequential reference tests/triangulate_ref.py through the C ABI: status and method for equality, pos_w as uint64 bit patterns. Every scene is
one of tests/triangulate_ref.py's CASES, which tests/test_triangulate_ref.py holds to the codes and methods they have to reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import triangulate_io as io
import triangulate_ref as tri

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def solve():
    from openvslam_amd import solve
    return solve


def camera_of(solve, c):
    cam = solve.camera(c["model"], c["fx"], c["fy"], c["cx"], c["cy"], c["cols"], c["rows"])
    cam.focal_x_baseline, cam.true_baseline = c["focal_x_baseline"], c["true_baseline"]
    return cam


def device_problem(solve, q):
    d = lambda key, w: np.array(q[key], np.float64).reshape(-1, w)
    f = lambda key, w=1: np.array(q[key], np.float32).reshape(-1, w)
    return dict(bearings_1=d("b1", 3), bearings_2=d("b2", 3), keypts_1=f("kp1", 2), keypts_2=f("kp2", 2), x_right_1=f("xr1"), x_right_2=f("xr2"),
                depths_1=f("depth1"), depths_2=f("depth2"), sigma_sq_1=f("sig1"), sigma_sq_2=f("sig2"), scale_factors_1=f("sf1"), scale_factors_2=f("sf2"),
                cam_1=camera_of(solve, q["cam_1"]), cam_2=camera_of(solve, q["cam_2"]), pose_cw_1=np.array(q["pose_1"]), pose_cw_2=np.array(q["pose_2"]))


def canon(u):
    """A bit pattern as it is compared: a NaN is a NaN whatever its sign and payload (the host's and the device's default NaNs differ); every
    other value, the infinities and the signed zeros included, is its own bits."""
    return 0x7ff8000000000000 if (u & 0x7ff0000000000000) == 0x7ff0000000000000 and (u & 0xfffffffffffff) else u


def of_device(r):
    pos = np.ascontiguousarray(r["pos_w"], np.float64).view(np.uint64).reshape(-1, 3)
    return [(int(s), int(m), [canon(int(v)) for v in p]) for s, m, p in zip(r["status"], r["method"], pos)]


def run(solve, names, handle=None):
    out = solve.triangulate_batch([device_problem(solve, tri.problem(k)) for k in names], tri.RATIO_FACTOR, tri.COS_THR, handle=handle)
    for k, r in zip(names, out):
        assert r["num_accepted"] == sum(1 for x in tri.solved(k) if x["status"] == 0) == int(r["accepted"].sum())
    return [of_device(r) for r in out]


def expected(name):
    return [(s, m, [canon(v) for v in p]) for s, m, p in tri.result_bits(tri.solved(name))]


# ---- the wavefront's edges and more than one workgroup; every camera pair; every reject code and method
@pytest.mark.parametrize("name", list(tri.SIZES) + list(tri.PAIRS) + tri.REJECTS + ["stereo_close_2", "stereo_close_3"])
def test_result_equals_the_reference_bit_for_bit(solve, name):
    got, want = run(solve, [name])[0], expected(name)
    assert len(got) == len(want) == len(tri.problem(name)["b1"])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    if name in tri.REACHES:
        assert {g[0] for g in got} >= tri.REACHES[name][0] and {g[1] for g in got} >= tri.REACHES[name][1]


# ---- a batch against its problems one by one; a problem's position does not matter
def test_batch_equals_its_problems_solved_alone(solve):
    names = ["n0", "n1", "n65", "n0", "n130"]
    probs = [device_problem(solve, tri.problem(k)) for k in names]
    assert np.cumsum([0] + [len(q["x_right_1"]) for q in probs]).tolist() == [0, 0, 1, 66, 66, 196]
    got = run(solve, names)
    for k, g in zip(names, got):
        assert g == run(solve, [k])[0] == expected(k)


def test_same_problem_at_two_positions_gives_the_same_bits(solve):
    got = run(solve, ["stereo_mono", "n63", "stereo_mono", "n1"])
    assert got[0] == got[2] == expected("stereo_mono") and got[1] == expected("n63") and got[3] == expected("n1")


# ---- a non-finite match is rejected and touches nothing else
def test_nan_bearing_and_inf_depth_reject_their_match_alone(solve):
    bad, clean = run(solve, ["nan_inf"])[0], run(solve, ["nan_inf_clean"])[0]
    assert bad == expected("nan_inf") and clean == expected("nan_inf_clean")
    assert bad[17][0] != 0 and clean[17][0] == 0
    assert bad[:17] + bad[18:] == clean[:17] + clean[18:] and len(bad) == 65


# ---- one handle, many calls: a large call leaves nothing behind for a small one
def test_handle_reuse_leaves_no_stale_results(solve):
    h = solve._triangulate_handle(4, 300)
    a, b, c = run(solve, ["n257"], handle=h)[0], run(solve, ["reproj_1"], handle=h)[0], run(solve, ["n257"], handle=h)[0]
    assert a == c == expected("n257") and b == expected("reproj_1")
    assert run(solve, ["n0", "low_parallax"], handle=h) == [[], expected("low_parallax")]


# ---- capacity and argument errors return before anything is written and leave the handle usable
def test_error_contract(solve):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = solve._triangulate_handle(2, 70)
    ok = lambda: run(solve, ["n65"], handle=h)[0] == expected("n65")
    assert ok()
    q = device_problem(solve, tri.problem("n65"))
    n = 65
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cams = (_lib.Camera * 3)(q["cam_1"], q["cam_1"], q["cam_1"])
    poses = np.tile(q["pose_cw_1"], (3, 1))
    out_pos, out_status, out_method, out_num = np.full((256, 3), -7.0), np.full(256, 9, np.uint8), np.full(256, 9, np.uint8), np.full(4, -7, np.int32)
    keys = ["bearings_1", "bearings_2", "keypts_1", "keypts_2", "x_right_1", "x_right_2", "depths_1", "depths_2", "sigma_sq_1", "sigma_sq_2",
            "scale_factors_1", "scale_factors_2"]

    def call(P=1, offsets=(0, n), drop=None, cams_1=cams, cams_2=cams, poses_1=poses, poses_2=poses, thr=tri.COS_THR, ratio=tri.RATIO_FACTOR, pos=out_pos,
             status=out_status, method=out_method, num=out_num, handle=h._h):
        opt = lambda a: None if a is None else vp(a)
        off = None if offsets is None else np.array(offsets, np.int32)
        arrays = [None if k == drop else vp(q[k]) for k in keys]
        return L.ovs_triangulate_batch(handle, P, opt(off), *arrays, cams_1, cams_2, opt(poses_1), opt(poses_2), thr, ratio, opt(pos), opt(status), opt(method),
                                       opt(num))

    untouched = lambda: (out_pos == -7.0).all() and (out_status == 9).all() and (out_method == 9).all() and (out_num == -7).all()
    assert call(handle=None) == INVALID
    for kw in [dict(offsets=None), dict(cams_1=None), dict(cams_2=None), dict(poses_1=None), dict(poses_2=None), dict(pos=None), dict(status=None),
               dict(method=None), dict(num=None)] + [dict(drop=k) for k in keys]:
        assert call(**kw) == INVALID, kw
    assert call(P=-1) == INVALID
    assert call(offsets=(1, n)) == INVALID and call(P=2, offsets=(0, 40, 30)) == INVALID
    for thr, ratio in ((float("nan"), 1.8), (float("inf"), 1.8), (0.99, float("nan")), (0.99, float("inf"))):
        assert call(thr=thr, ratio=ratio) == INVALID
    one = lambda cam: (_lib.Camera * 1)(cam)
    for bad in (solve.camera(2, 458, 457, 367, 248), solve.camera(0, float("nan"), 457, 367, 248), solve.camera(0, 458, float("inf"), 367, 248),
                solve.camera(0, 458, 457, float("nan"), 248), solve.camera(0, 0.0, 457, 367, 248), solve.camera(0, 458, 0.0, 367, 248),
                solve.camera(1, cols=1920, rows=0), solve.camera(1, cols=0, rows=960)):
        assert call(cams_1=one(bad)) == INVALID and call(cams_2=one(bad)) == INVALID
    assert untouched()
    assert call(P=3, offsets=(0, 20, 40, 60)) == CAPACITY           # more problems than the handle was created for
    assert call(offsets=(0, 71)) == CAPACITY                        # more matches (refused before anything is read)
    assert untouched()                                              # nothing truncated, nothing written
    assert call(P=0) == 0 and untouched()                           # no problems: nothing to do
    assert call(P=2, offsets=(0, 0, 0)) == 0                        # no matches is not an error
    assert out_num[:2].tolist() == [0, 0] and (out_num[2:] == -7).all() and (out_pos == -7.0).all() and (out_status == 9).all()
    assert ok()
    with pytest.raises(_lib.OvsError):
        solve.triangulate_batch([q, q, q], tri.RATIO_FACTOR, handle=h)


# ---- the Python class
def test_python_class(solve):
    from test_triangulate_ref import _python_keyframe
    problems = io.class_scene()
    curr, neighbours, matches = io.keyframes_of(problems)
    k1 = _python_keyframe(solve, curr)
    for q, kf, m in list(zip(problems, neighbours, matches))[:2]:
        t = solve.two_view_triangulator(k1, _python_keyframe(solve, kf), rays_parallax_deg_thr=1.0)
        want = tri.solve(q)
        accepted, pos = t.triangulate_matches(m)
        assert accepted.tolist() == [r["status"] == 0 for r in want]
        assert np.ascontiguousarray(pos).view(np.uint64).tolist() == [[tri.bits(v) for v in r["pos_w"]] for r in want]
        ok, one = t.triangulate(*m[3])
        assert ok == (want[3]["status"] == 0) and [tri.bits(float(v)) for v in one] == [tri.bits(v) for v in want[3]["pos_w"]]


# ---- the C++ class: pair by pair, neighbour by neighbour and all neighbours at once
def test_cpp_class_returns_the_reference_results(tmp_path):
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_triangulate_shim"]))
    problems = io.class_scene()
    curr, neighbours, matches = io.keyframes_of(problems)
    io.write_scene(tmp_path / "scene.bin", curr, neighbours, matches)
    r = subprocess.run([os.path.join(cpp, "test_triangulate_shim" + SUFFIX), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    got = io.read_results(tmp_path / "out.bin", len(problems))
    assert got["all"] == got["neighbour"] == got["single"]           # three neighbours in one call equal three calls equal sixty
    for g, q in zip(got["all"], problems):
        want = tri.solve(q)
        assert g["accepted"] == [1 if w["status"] == 0 else 0 for w in want] and g["num_accepted"] == sum(g["accepted"]) > 0
        assert g["pos"] == [[tri.bits(v) for v in w["pos_w"]] for w in want]
