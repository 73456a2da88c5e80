"""The monocular initialiser's pose recovery on the device (csrc/two_view_reconstruct.hip, openvslam_amd.solve.reconstruct_two_view_batch,
openvslam_amd.initialize) against the sequential reference tests/reconstruct_ref.py: success, best, the counts and the flags for equality, the
pose, the parallaxes and the points as bit patterns. Every scene is one of tests/reconstruct_scenes.py's CASES, whose distance from every
decision tests/test_reconstruct_ref.py asserts."""
import ctypes as C

import numpy as np
import pytest

import reconstruct_io as io
import reconstruct_ref as ref
import reconstruct_scenes as sc
from test_reconstruct_ref import MIN_ABOVE, NOISY_THR

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def solve():
    from openvslam_amd import solve
    return solve


def run(solve, names, handle=None, **params):
    return [io.of_device(r) for r in solve.reconstruct_two_view_batch([io.device_problem(sc.problem(k)) for k in names], handle=handle, **params)]


def want(name, **params):
    return ref.as_bits(sc.expected(name, **params))


# ---- 0 and 1, both sides of min(50, n - 1) and of min_num_triangulated (50, 51, 52), the wave's round edge (63, 64, 65), three and four
# rounds (129, 200); a plane with its eight hypotheses and a cloud with its four; non-inlier matches in every scene
@pytest.mark.parametrize("name", sc.SIZES + ["h_success", "f_gross"])
def test_result_equals_the_reference_bit_for_bit(solve, name):
    got = run(solve, [name])[0]
    assert got == want(name)
    n = int(name[1:]) if name[1:].isdigit() else 65
    assert max(got["counts"]) == n
    if name[0] == "f" or name == "h_success":
        assert got["success"] == (1 if n >= 50 else 0)


@pytest.mark.parametrize("name", sc.FAILING)
def test_failing_exits(solve, name):
    got = run(solve, [name])[0]
    assert got == want(name) and got["success"] == 0 and got["best"] == -1
    assert not any(got["flags"]) and all(p == [0, 0, 0] for p in got["pts"]) and got["R"] == [0] * 9 and got["t"] == [0] * 3


def test_min_num_triangulated_one_above_the_winner(solve):
    name, above = MIN_ABOVE
    ok, fail = run(solve, [name])[0], run(solve, [name], min_num_triangulated=above)[0]
    assert ok == want(name) and ok["success"] == 1 and max(ok["counts"]) == above - 1
    assert fail == want(name, min_num_triangulated=above) and fail["success"] == 0 and fail["counts"] == ok["counts"]


def test_a_nan_keypoint_costs_its_match_and_nothing_else(solve):
    bad, clean = run(solve, ["f_nan"])[0], run(solve, ["f50"])[0]
    assert clean["success"] == 1 and bad["success"] == 0 and bad["counts"][2] == clean["counts"][2] - 1


@pytest.mark.parametrize("name", ["h_noisy", "f_noisy"])
def test_reproj_err_thr(solve, name):
    tight, loose = (run(solve, [name], reproj_err_thr=thr)[0] for thr in NOISY_THR)
    assert tight == want(name, reproj_err_thr=NOISY_THR[0]) and loose == want(name, reproj_err_thr=NOISY_THR[1]) and tight != loose
    assert max(tight["counts"]) < max(loose["counts"])


def test_batch_equals_its_problems_solved_alone(solve):
    got = run(solve, sc.BATCH)
    assert [len(g["flags"]) for g in got] == [81, 0, 157, 3, 65, 85, 81, 78]
    for name, g in zip(sc.BATCH, got):
        assert g == run(solve, [name])[0] == want(name), name
    assert [g["success"] for g in got] == [0, 0, 1, 0, 0, 1, 0, 1]


def test_key_buffer_grows_on_a_live_handle(solve):
    """A handle holds the keys of 256 matches when it is created: the second call has 400. The calls before and after it are unchanged."""
    h = solve._reconstruct_handle(2, 400)
    got = [run(solve, names, handle=h) for names in sc.GROW]
    assert got == [[want(k) for k in names] for names in sc.GROW] and got[0] == got[2]
    assert sum(len(sc.problem(k)["inlier"]) for k in sc.GROW[1]) == 400 and got[1][1]["success"] == 1


@pytest.mark.parametrize("name", sc.CHAINED)
def test_chained_with_the_two_view_solver(solve, name):
    """solve_two_view_batch -> reconstruct_problem_from_solution -> reconstruct_two_view_batch against the references chained the same way."""
    import test_twoview_ref as tv
    q = tv.problem(name)
    two_view = dict(x1=np.array(q["x1"], np.float64).reshape(-1, 2), x2=np.array(q["x2"], np.float64).reshape(-1, 2))
    solution = solve.solve_two_view_batch([two_view], 1.0, tv.CASE_ITERS.get(name, tv.ITERS), True, tv.SEED)[0]
    assert solution["selected"] == sc.problem(name)["model"]
    problem = solve.reconstruct_problem_from_solution(solution, two_view, solve.camera(0, tv.FOCAL, tv.FOCAL, tv.CX, tv.CY))
    got = io.of_device(solve.reconstruct_two_view_batch([problem])[0])
    assert got == want(name)
    if name.startswith("c"):
        assert got["success"] == 1


def test_initialize_class(solve):
    """openvslam_amd.initialize.perspective strings the two calls together: upstream's constructor, initialize() and the four getters."""
    import test_twoview_ref as tv
    from openvslam_amd import initialize
    name = "c129"
    q = tv.problem(name)
    n = len(q["x1"])
    cam = solve.camera(0, tv.FOCAL, tv.FOCAL, tv.CX, tv.CY)
    kp_ref, kp_cur = np.array(q["x1"], np.float32), np.array(q["x2"], np.float32)[::-1].copy()
    matches = np.full(n + 5, -1, np.int32)          # ref_matches_with_cur: five unmatched reference keypoints at the end
    matches[:n] = np.arange(n)[::-1]
    ref_frm = dict(undist_keypts=np.concatenate([kp_ref, np.zeros((5, 2), np.float32)]), camera=cam)
    ref_frm["bearings"] = solve.bearings_of(ref_frm["undist_keypts"], cam)
    init = initialize.perspective(ref_frm, num_ransac_iters=tv.ITERS, min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0, seed=tv.SEED)
    assert init.initialize(kp_cur, solve.bearings_of(kp_cur, cam), matches)
    w = want(name)
    bits = lambda a: [int(v) for v in np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)]
    assert bits(init.get_rotation_ref_to_cur()) == w["R"] and bits(init.get_translation_ref_to_cur()) == w["t"]
    pts, flags = init.get_triangulated_pts(), init.get_triangulated_flags()
    assert len(pts) == len(flags) == n + 5 and [bits(p) for p in pts[:n]] == w["pts"] and [int(f) for f in flags[:n]] == w["flags"]
    assert not flags[n:].any() and not pts[n:].any()


def test_cpp_class_returns_the_reference_results(tmp_path):
    """cpp/openvslam/initialize/perspective.h through its test program: upstream's getters equal the Python mirror's reference, by the
    reference frame's keypoints; a caller error throws."""
    import os
    import subprocess
    from test_reconstruct_ref import CPP, write_shim_scene
    suffix = os.environ.get("OVS_SHIM_SUFFIX", "")
    subprocess.check_call(["make", "-s", "-C", CPP] + (["asan"] if suffix else ["test_reconstruct_shim"]))
    sizes = write_shim_scene(tmp_path / "scene.bin")
    r = subprocess.run([os.path.join(CPP, "test_reconstruct_shim" + suffix), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout and "caller error thrown 1" in r.stdout, r.stdout + r.stderr
    for name, n, g in zip(sc.CHAINED, sizes, io.read_shim_results(tmp_path / "out.bin", sizes)):
        w = want(name)
        assert g["initialised"] == w["success"] and g["R"] == w["R"] and g["t"] == w["t"], name
        assert g["pts"][:n] == w["pts"] and g["flags"][:n] == w["flags"] and g["pts"][n:] == [[0, 0, 0]] * 5 and g["flags"][n:] == [0] * 5
    assert want("c129")["success"] == 1


def test_error_contract(solve):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = solve._reconstruct_handle(2, 100)
    ok = lambda: run(solve, ["f65"], handle=h)[0] == want("f65")
    assert ok()
    q = io.device_problem(sc.problem("f65"))
    n = 81
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out_i = [np.full(20, -7, np.int32) for _ in range(3)]      # success, best, counts
    out_d = [np.full(400, -7.0) for _ in range(3)]              # rot, trans, pts
    out_f, flags = np.full(20, -7.0, np.float32), np.full(256, 9, np.uint8)
    good_cam = q["cam"]

    def call(P=1, offsets=(0, n), models=(2,), mats=q["mat"], cams=(good_cam,), inlier=q["inlier"], kp_ref=q["kp_ref"], b_cur=q["b_cur"], thr=4.0, par=1.0,
             success=out_i[0], rot=out_d[0], pts=out_d[2], out_flags=flags, handle=h._h):
        opt = lambda a: None if a is None else vp(np.ascontiguousarray(a))
        off = None if offsets is None else np.array(offsets, np.int32)
        mod = None if models is None else np.array(models, np.int32)
        cam_arr = None if cams is None else (_lib.Camera * len(cams))(*cams)
        mat_arr = None if mats is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mats, np.float64).reshape(-1, 3, 3)[:1], (max(P, 1), 3, 3)))
        return L.ovs_reconstruct_batch(handle, P, opt(off), opt(mod), opt(mat_arr), cam_arr, opt(inlier), opt(kp_ref), vp(q["kp_cur"]), vp(q["b_ref"]), opt(b_cur),
                                       thr, par, 50, opt(success), vp(out_i[1]), opt(rot), vp(out_d[1]), vp(out_i[2]), vp(out_f), opt(pts), opt(out_flags))

    assert call(handle=None) == INVALID
    for kw in (dict(offsets=None), dict(models=None), dict(mats=None), dict(cams=None), dict(inlier=None), dict(kp_ref=None), dict(b_cur=None), dict(success=None),
               dict(rot=None), dict(pts=None), dict(out_flags=None)):
        assert call(**kw) == INVALID, kw
    assert call(P=-1) == INVALID
    assert call(offsets=(1, n)) == INVALID and call(P=2, offsets=(0, 40, 30), models=(2, 2), cams=(good_cam, good_cam)) == INVALID
    assert call(models=(0,)) == INVALID and call(models=(3,)) == INVALID
    for thr, par in ((0.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (4.0, 0.0), (4.0, -1.0), (4.0, float("nan"))):
        assert call(thr=thr, par=par) == INVALID
    for bad in (dict(fx=0.0), dict(fy=0.0), dict(fx=float("nan")), dict(fy=float("inf")), dict(cx=float("nan")), dict(model=1)):
        kw = dict(model=0, fx=458.0, fy=457.0, cx=367.0, cy=248.0)
        kw.update(bad)
        assert call(cams=(solve.camera(**kw),)) == INVALID, bad
    three = (good_cam,) * 3
    assert call(P=3, offsets=(0, 20, 40, 60), models=(2, 2, 2), cams=three) == CAPACITY      # more problems than the handle was created for
    big = np.ones((120, 3))
    assert call(offsets=(0, 101), inlier=np.ones(120, np.uint8), kp_ref=big[:, :2], b_cur=big) == CAPACITY   # more matches
    assert all((a == -7).all() for a in out_i) and all((a == -7.0).all() for a in out_d) and (out_f == -7.0).all() and (flags == 9).all()   # nothing written
    assert call(P=0) == 0 and (out_i[0] == -7).all()                                          # no problems: nothing to do
    assert call(P=2, offsets=(0, 0, 0), models=(1, 2), cams=(good_cam, good_cam)) == 0      # no matches is not an error: both fail
    assert out_i[0][:2].tolist() == [0, 0] and out_i[1][:2].tolist() == [-1, -1] and (out_d[0][:18] == 0.0).all()
    assert ok()
    with pytest.raises(_lib.OvsError):
        run(solve, ["f0", "f0", "f0"], handle=h)
