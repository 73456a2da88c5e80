"""The Sim3 RANSAC on the device (csrc/sim3_solve.hip, openvslam_amd.solve, cpp/openvslam/solve/sim3_solver.h) against the sequential
reference tests/sim3_ref.py: valid, best_iter, num_inliers and the flags for equality, R12, t12 and s12 as uint64 bit patterns. Every scene
is one of tests/test_sim3_ref.py's CASES, whose distance from the thresholds is asserted there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_ref
import sim3_scene_io
from test_sim3_ref import (BATCH, BATCH_MIN_INLIERS, CASE_ITERS, CASES, EDGE_ITERS, GROW_ITERS, ITERS, SEED, SEED_2, edge_seed, expected,
                           keyframe_pair, level_sigma_sq, problem)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def solve():
    from openvslam_amd import solve
    return solve


def device_problem(solve, prob):
    cam = lambda c: solve.camera(**c)
    return dict(p1=np.array(prob["p1"], np.float64).reshape(-1, 3), p2=np.array(prob["p2"], np.float64).reshape(-1, 3),
                thr1=np.array(prob["thr1"], np.float32), thr2=np.array(prob["thr2"], np.float32), cam_1=cam(prob["cam_1"]), cam_2=cam(prob["cam_2"]))


def canon(valid, best_iter, num_inliers, R, t, s, flags):
    return dict(valid=int(valid), best_iter=int(best_iter), num_inliers=int(num_inliers), R=[sim3_ref.bits(float(v)) for v in np.ravel(R)],
                t=[sim3_ref.bits(float(v)) for v in t], s=sim3_ref.bits(float(s)), flags=[int(f) for f in flags])


def of_device(r):
    return canon(r["valid"], r["best_iter"], r["num_inliers"], r["rot_12"], r["trans_12"], r["scale_12"], r["inlier_flags"])


def of_reference(r):
    return canon(r["valid"], r["best_iter"], r["num_inliers"], r["R"], r["t"], r["s"], r["flags"])


def run(solve, name, max_num_iter=None, seed=SEED, handle=None):
    return solve.solve_sim3_batch([device_problem(solve, problem(name))], CASES[name][1], CASES[name][2],
                                  CASE_ITERS.get(name, ITERS) if max_num_iter is None else max_num_iter, seed, handle=handle)[0]


# ---- the match loop's lane / wave edges, both values of fix_scale, both camera models, ties, too few inliers
@pytest.mark.parametrize("name", ["n3", "n20", "n63", "n64", "n65", "n257", "n65_noisy", "n65_fixed", "equirect", "mixed", "clean", "too_few_inliers"])
def test_result_equals_the_reference_bit_for_bit(solve, name):
    got, want = of_device(run(solve, name)), of_reference(expected(name))
    assert got == want
    if name == "clean":             # many hypotheses tie at the full count: the lowest one wins
        assert got["best_iter"] == 0 and got["num_inliers"] == 30
    elif name == "too_few_inliers":
        assert got == of_reference(dict(sim3_ref.INVALID, flags=[0] * 24))
    else:
        assert got["valid"] == 1


# ---- the edges of the hypothesis blocks
@pytest.mark.parametrize("max_num_iter", EDGE_ITERS)
def test_hypothesis_block_edges(solve, max_num_iter):
    """Under edge_seed the last hypothesis asked for is the winner: one hypothesis too few, or a block's last lane dropped, changes the result."""
    seed = edge_seed(max_num_iter)
    got = of_device(run(solve, "n65_noisy", max_num_iter, seed))
    assert got == of_reference(expected("n65_noisy", max_num_iter, seed)) and got["best_iter"] == max_num_iter - 1


# ---- a batch against its problems one by one
def test_batch_equals_its_problems_solved_alone(solve):
    probs = [device_problem(solve, problem(name)) for name, _ in BATCH]
    assert [len(q["thr1"]) for q in probs] == [65, 0, 3, 2, 64]
    got = solve.solve_sim3_batch(probs, False, BATCH_MIN_INLIERS, ITERS, SEED)
    for (name, p), q, g in zip(BATCH, probs, got):
        alone = solve.solve_sim3_batch([q], False, BATCH_MIN_INLIERS, ITERS, solve.problem_seed(SEED, p))[0]
        assert of_device(g) == of_device(alone)
        assert of_device(g) == of_reference(expected(name, p=p, min_num_inliers=BATCH_MIN_INLIERS))
    for i in (1, 2, 3):   # n = 0, n < min_num_inliers, n = 2: the invalid-output convention
        assert of_device(got[i]) == of_reference(dict(sim3_ref.INVALID, flags=[0] * len(probs[i]["thr1"])))
    assert got[0]["valid"] and got[4]["valid"]


# ---- rule 3's NaN path
def test_identical_points_are_invalid_not_an_error(solve):
    got = of_device(run(solve, "identical"))
    assert got == of_reference(dict(sim3_ref.INVALID, flags=[0] * 12)) == of_reference(expected("identical"))


# ---- seeds
def test_same_seed_same_bytes_other_seed_other_winner(solve):
    h = solve._handle(2, 128)
    a, b = of_device(run(solve, "n65", handle=h)), of_device(run(solve, "n65", handle=h))
    assert a == b
    c = of_device(run(solve, "n65", seed=SEED_2, handle=h))
    assert c == of_reference(expected("n65", seed=SEED_2)) and c["best_iter"] != a["best_iter"]


# ---- the models' buffer grows on a live handle
def test_models_grow_on_a_live_handle(solve):
    """A handle for one problem holds 64 records of four hypotheses: GROW_ITERS needs 65. The calls before and after it are unchanged."""
    h = solve._handle(1, 70)
    got = [of_device(run(solve, "n65_noisy", k, handle=h)) for k in (ITERS, GROW_ITERS, ITERS)]
    assert got == [of_reference(expected("n65_noisy", k)) for k in (ITERS, GROW_ITERS, ITERS)]
    assert got[0] == got[2] and got[1]["valid"] == 1


# ---- capacity and argument errors leave the handle usable
def test_error_contract(solve):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = solve._handle(2, 70)
    ok = lambda: of_device(run(solve, "n65", handle=h)) == of_reference(expected("n65"))
    assert ok()
    q = device_problem(solve, problem("n65"))
    n = 65
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cams = (_lib.Camera * 3)(q["cam_1"], q["cam_1"], q["cam_1"])
    out_i = [np.full(4, -7, np.int32) for _ in range(3)]
    out_d = [np.full(36, -7.0) for _ in range(3)]
    flags = np.full(256, 9, np.uint8)

    def call(P=1, offsets=(0, n), p1=q["p1"], thr1=q["thr1"], cams_1=cams, min_inl=20, iters=ITERS, valid=out_i[0], flags=flags, handle=h._h):
        off = None if offsets is None else np.array(offsets, np.int32)
        return L.ovs_sim3_solve_batch(handle, P, None if off is None else vp(off), None if p1 is None else vp(p1), vp(q["p2"]),
                                      None if thr1 is None else vp(thr1), vp(q["thr2"]), cams_1, cams, 0, min_inl, iters, SEED,
                                      None if valid is None else vp(valid), vp(out_i[1]), vp(out_i[2]), vp(out_d[0]), vp(out_d[1]), vp(out_d[2]),
                                      None if flags is None else vp(flags))

    assert call(handle=None) == INVALID
    for kw in (dict(offsets=None), dict(p1=None), dict(thr1=None), dict(cams_1=None), dict(valid=None), dict(flags=None)):
        assert call(**kw) == INVALID, kw
    assert call(P=-1) == INVALID
    assert call(offsets=(1, n)) == INVALID and call(P=2, offsets=(0, 40, 30)) == INVALID
    assert call(iters=0) == INVALID and call(iters=(1 << 20) + 1) == INVALID and call(min_inl=-1) == INVALID
    bad_model = (_lib.Camera * 1)(solve.camera(2, 458, 457, 367, 248))
    nan_fx = (_lib.Camera * 1)(solve.camera(0, float("nan"), 457, 367, 248))
    inf_cy = (_lib.Camera * 1)(solve.camera(0, 458, 457, 367, float("inf")))
    no_rows = (_lib.Camera * 1)(solve.camera(1, cols=1920, rows=0))
    for bad in (bad_model, nan_fx, inf_cy, no_rows):
        assert call(cams_1=bad) == INVALID
    assert call(P=3, offsets=(0, 20, 40, 60)) == CAPACITY           # more problems than the handle was created for
    big = np.zeros((80, 3))
    assert L.ovs_sim3_solve_batch(h._h, 1, vp(np.array([0, 71], np.int32)), vp(big), vp(big), vp(np.ones(80, np.float32)), vp(np.ones(80, np.float32)),
                                  cams, cams, 0, 20, ITERS, SEED, vp(out_i[0]), vp(out_i[1]), vp(out_i[2]), vp(out_d[0]), vp(out_d[1]), vp(out_d[2]),
                                  vp(flags)) == CAPACITY             # more matches
    assert all((a == -7).all() for a in out_i) and all((a == -7.0).all() for a in out_d) and (flags == 9).all()   # nothing truncated, nothing written
    assert call(P=0) == 0 and (out_i[0] == -7).all()                 # no problems: nothing to do
    assert call(P=2, offsets=(0, 2, 2)) == 0                         # n < 3 is not an error
    assert out_i[0][:2].tolist() == [0, 0] and out_i[1][:2].tolist() == [-1, -1]
    assert call(iters=1 << 20, offsets=(0, 3)) == 0                  # the largest max_num_iter, on three matches
    assert ok()
    c = C.c_void_p()
    assert L.ovs_sim3_create(0, 0, 8, C.byref(c)) == INVALID and L.ovs_sim3_create(0, 1 << 20, 8, C.byref(c)) == INVALID
    with pytest.raises(_lib.OvsError):
        solve.solve_sim3_batch([q, q, q], False, handle=h)


# ---- the Python class and the constructor's helper
def test_python_class(solve):
    q = device_problem(solve, problem("n64"))
    s = solve.sim3_solver(q["p1"], q["p2"], q["thr1"], q["thr2"], q["cam_1"], q["cam_2"], False, 20)
    assert not s.solution_is_valid()
    with pytest.raises(RuntimeError):
        s.get_best_rotation_12()
    s.find_via_ransac(ITERS, seed=SEED)
    want = of_reference(expected("n64"))
    got = canon(s.solution_is_valid(), s.get_best_iter(), s.get_num_inliers(), s.get_best_rotation_12(), s.get_best_translation_12(),
                s.get_best_scale_12(), s.get_inlier_flags())
    assert got == want and s.solution_is_valid()
    pair = keyframe_pair("kf20")
    prob, idx1 = sim3_scene_io.problem_of(pair, level_sigma_sq())
    assert len(idx1) == 20 and prob == problem("kf20")
    assert of_device(run(solve, "kf20")) == of_reference(expected("kf20"))


# ---- the C++ class
def test_cpp_class_returns_the_reference_results(tmp_path):
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_sim3_shim"]))
    names = ["kf20", "kf64"]
    sim3_scene_io.write_scene(tmp_path / "scene.bin", [keyframe_pair(k) for k in names], level_sigma_sq(), False, 3, ITERS, SEED)
    r = subprocess.run([os.path.join(cpp, "test_sim3_shim" + SUFFIX), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    got = sim3_scene_io.read_results(tmp_path / "out.bin", len(names))
    for p, k in enumerate(names):
        idx1 = sim3_scene_io.problem_of(keyframe_pair(k), level_sigma_sq())[1]
        assert got["single"][p] == sim3_scene_io.as_bits(expected(k), idx1)
        assert got["batch"][p] == sim3_scene_io.as_bits(expected(k, p=p), idx1)
        assert got["batch"][p]["valid"] == 1
