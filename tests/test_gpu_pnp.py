"""The EPnP RANSAC on the device (csrc/pnp_solve.hip, openvslam_amd.solve, cpp/openvslam/solve/pnp_solver.h) against the sequential reference
tests/pnp_ref.py: valid, best_iter, num_inliers and the flags for equality, R and t as uint64 bit patterns. Every scene is one of
tests/test_pnp_ref.py's CASES, whose distance from the thresholds is asserted there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_ref
import pnp_scene_io
from test_pnp_ref import (BATCH, BATCH_MIN_INLIERS, CASE_ITERS, CASES, EDGE_ITERS, GROW_ITERS, ITERS, SEED, SHIM_CASES, edge_seed, expected,
                          problem, scale_factors, second_seed)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def solve():
    from openvslam_amd import solve
    return solve


def device_problem(prob):
    return dict(bearings=np.array(prob["bearings"], np.float64).reshape(-1, 3), pos_w=np.array(prob["pos_w"], np.float64).reshape(-1, 3),
                max_cos_error=np.array(prob["max_cos_error"], np.float64))


def canon(valid, best_iter, num_inliers, R, t, flags):
    return dict(valid=int(valid), best_iter=int(best_iter), num_inliers=int(num_inliers), R=[pnp_ref.bits(float(v)) for v in np.ravel(R)],
                t=[pnp_ref.bits(float(v)) for v in t], flags=[int(f) for f in flags])


def of_device(r):
    return canon(r["valid"], r["best_iter"], r["num_inliers"], r["rot_cw"], r["trans_cw"], r["inlier_flags"])


def of_reference(r):
    return canon(r["valid"], r["best_iter"], r["num_inliers"], r["R"], r["t"], r["flags"])


def run(solve, name, max_num_iter=None, seed=SEED, handle=None, recompute=True, min_num_inliers=None):
    return solve.solve_pnp_batch([device_problem(problem(name))], CASES[name][1] if min_num_inliers is None else min_num_inliers,
                                 CASE_ITERS.get(name, ITERS) if max_num_iter is None else max_num_iter, recompute, seed, handle=handle)[0]


# ---- the lane-group edge (4, 5), the edges of the match loop's wave (63, 64, 65), the refit's sums with one term per lane (fewer than 64
# inliers), one or two (n100) and two or three (n257), counts that differ per hypothesis, ties, too few inliers
@pytest.mark.parametrize("name", ["n4", "n5", "n63", "n64", "n65", "n100", "n257", "n65_noisy", "clean", "too_few_inliers"])
def test_result_equals_the_reference_bit_for_bit(solve, name):
    got, want = of_device(run(solve, name)), of_reference(expected(name))
    assert got == want
    if name == "clean":             # many hypotheses tie at the full count: the lowest one wins
        assert got["best_iter"] == 0 and got["num_inliers"] == 30
    elif name == "too_few_inliers":
        assert got == of_reference(dict(pnp_ref.INVALID, flags=[0] * 24))
    else:
        assert got["valid"] == 1
    if name == "n257":
        assert got["num_inliers"] > 128
    if name == "n100":
        assert 64 < got["num_inliers"] < 128
    if name in ("n63", "n64", "n65"):
        assert got["num_inliers"] < 64


# ---- rule 5 switched off
@pytest.mark.parametrize("name", ["n65_noisy", "n257"])
def test_without_recompute_the_winner_stays(solve, name):
    got = of_device(run(solve, name, recompute=False))
    assert got == of_reference(expected(name, recompute=False)) and got["valid"] == 1
    again = of_device(run(solve, name))
    assert again["best_iter"] == got["best_iter"] and (again["R"], again["t"]) != (got["R"], got["t"])


# ---- the edges of the hypothesis grid: a workgroup takes one hypothesis
@pytest.mark.parametrize("max_num_iter", EDGE_ITERS)
def test_hypothesis_block_edges(solve, max_num_iter):
    """Under edge_seed the last hypothesis asked for is the winner: one hypothesis too few changes the result."""
    seed = edge_seed(max_num_iter)
    got = of_device(run(solve, "n65_noisy", max_num_iter, seed))
    assert got == of_reference(expected("n65_noisy", max_num_iter, seed)) and got["best_iter"] == max_num_iter - 1


# ---- a batch against its problems one by one
def test_batch_equals_its_problems_solved_alone(solve):
    probs = [device_problem(problem(name)) for name, _ in BATCH]
    assert [len(q["max_cos_error"]) for q in probs] == [65, 0, 4, 3, 64]
    got = solve.solve_pnp_batch(probs, BATCH_MIN_INLIERS, ITERS, True, SEED)
    for (name, p), q, g in zip(BATCH, probs, got):
        alone = solve.solve_pnp_batch([q], BATCH_MIN_INLIERS, ITERS, True, solve.pnp_problem_seed(SEED, p))[0]
        assert of_device(g) == of_device(alone)
        assert of_device(g) == of_reference(expected(name, p=p, min_num_inliers=BATCH_MIN_INLIERS))
    for i in (1, 2, 3):   # n = 0, n < min_num_inliers, n = 3: the invalid-output convention
        assert of_device(got[i]) == of_reference(dict(pnp_ref.INVALID, flags=[0] * len(probs[i]["max_cos_error"])))
    assert got[0]["valid"] and got[4]["valid"]


# ---- the NaN path
@pytest.mark.parametrize("name", ["coplanar", "identical"])
def test_degenerate_landmarks_are_invalid_not_an_error(solve, name):
    got = of_device(run(solve, name))
    n = len(problem(name)["pos_w"])
    assert got == of_reference(dict(pnp_ref.INVALID, flags=[0] * n)) == of_reference(expected(name))
    zero = run(solve, name, min_num_inliers=0)   # "valid" with no inlier: hypothesis 0, whose pose is not a number; the refit changes nothing
    assert zero["valid"] and zero["best_iter"] == 0 and zero["num_inliers"] == 0 and not zero["inlier_flags"].any()
    assert np.isnan(zero["rot_cw"]).all() and np.isnan(zero["trans_cw"]).all()


# ---- seeds
def test_same_seed_same_bytes_other_seed_other_winner(solve):
    h = solve._pnp_handle(2, 128)
    a, b = of_device(run(solve, "n65", handle=h)), of_device(run(solve, "n65", handle=h))
    assert a == b
    c = of_device(run(solve, "n65", seed=second_seed(), handle=h))
    assert c == of_reference(expected("n65", seed=second_seed())) and c["best_iter"] != a["best_iter"]


# ---- the models' buffer grows on a live handle
def test_models_grow_on_a_live_handle(solve):
    """A handle for one problem holds 64 models, one per hypothesis: GROW_ITERS needs 65. The calls before and after it are unchanged."""
    h = solve._pnp_handle(1, 70)
    got = [of_device(run(solve, "n65_noisy", k, handle=h)) for k in (ITERS, GROW_ITERS, ITERS)]
    assert got == [of_reference(expected("n65_noisy", k)) for k in (ITERS, GROW_ITERS, ITERS)]
    assert got[0] == got[2] and got[1]["valid"] == 1


# ---- capacity and argument errors leave the handle usable
def test_error_contract(solve):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = solve._pnp_handle(2, 70)
    ok = lambda: of_device(run(solve, "n65", handle=h)) == of_reference(expected("n65"))
    assert ok()
    q = device_problem(problem("n65"))
    n = 65
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out_i = [np.full(4, -7, np.int32) for _ in range(3)]
    out_d = [np.full(36, -7.0) for _ in range(2)]
    flags = np.full(256, 9, np.uint8)

    def call(P=1, offsets=(0, n), bearings=q["bearings"], pos_w=q["pos_w"], max_cos=q["max_cos_error"], min_inl=10, iters=ITERS, valid=out_i[0],
             rot=out_d[0], flags=flags, handle=h._h):
        off = None if offsets is None else np.array(offsets, np.int32)
        opt = lambda a: None if a is None else vp(a)
        return L.ovs_pnp_solve_batch(handle, P, opt(off), opt(bearings), opt(pos_w), opt(max_cos), min_inl, iters, 1, SEED, opt(valid), vp(out_i[1]),
                                     vp(out_i[2]), opt(rot), vp(out_d[1]), opt(flags))

    assert call(handle=None) == INVALID
    for kw in (dict(offsets=None), dict(bearings=None), dict(pos_w=None), dict(max_cos=None), dict(valid=None), dict(rot=None), dict(flags=None)):
        assert call(**kw) == INVALID, kw
    assert call(P=-1) == INVALID
    assert call(offsets=(1, n)) == INVALID and call(P=2, offsets=(0, 40, 30)) == INVALID
    assert call(iters=0) == INVALID and call(iters=(1 << 20) + 1) == INVALID and call(min_inl=-1) == INVALID
    assert call(P=3, offsets=(0, 20, 40, 60)) == CAPACITY           # more problems than the handle was created for
    big = np.ones((80, 3))
    assert call(offsets=(0, 71), bearings=big, pos_w=big, max_cos=np.ones(80)) == CAPACITY   # more matches
    assert all((a == -7).all() for a in out_i) and all((a == -7.0).all() for a in out_d) and (flags == 9).all()   # nothing truncated, nothing written
    assert call(P=0) == 0 and (out_i[0] == -7).all()                 # no problems: nothing to do
    assert call(P=2, offsets=(0, 3, 3)) == 0                         # n < 4 is not an error
    assert out_i[0][:2].tolist() == [0, 0] and out_i[1][:2].tolist() == [-1, -1]
    assert call(iters=1 << 20, offsets=(0, 3)) == 0                  # the largest max_num_iter, on three matches
    assert ok()
    c = C.c_void_p()
    assert L.ovs_pnp_create(0, 0, 8, C.byref(c)) == INVALID and L.ovs_pnp_create(0, 1 << 20, 8, C.byref(c)) == INVALID
    with pytest.raises(_lib.OvsError):
        solve.solve_pnp_batch([q, q, q], handle=h)


# ---- the Python class and the constructor's mirror
def test_python_class(solve):
    q = problem("n64")
    s = solve.pnp_solver(q["bearings"], q["octaves"], q["pos_w"], scale_factors(), 10)
    assert not s.solution_is_valid()
    with pytest.raises(RuntimeError):
        s.get_best_rotation()
    s.find_via_ransac(ITERS, seed=SEED)
    want = of_reference(expected("n64"))
    got = canon(s.solution_is_valid(), s.get_best_iter(), s.get_num_inliers(), s.get_best_rotation(), s.get_best_translation(), s.get_inlier_flags())
    assert got == want and s.solution_is_valid()
    pose = s.get_best_cam_pose()
    assert pose.shape == (4, 4) and np.array_equal(pose[:3, :3], s.get_best_rotation()) and np.array_equal(pose[:3, 3], s.get_best_translation())
    assert pose[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    s.find_via_ransac(ITERS, recompute=False, seed=SEED)
    assert canon(s.solution_is_valid(), s.get_best_iter(), s.get_num_inliers(), s.get_best_rotation(), s.get_best_translation(),
                 s.get_inlier_flags()) == of_reference(expected("n64", recompute=False))


# ---- the C++ class
def test_cpp_class_returns_the_reference_results(tmp_path):
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_pnp_shim"]))
    pnp_scene_io.write_scene(tmp_path / "scene.bin", [problem(k) for k in SHIM_CASES], scale_factors(), 10, ITERS, True, SEED)
    r = subprocess.run([os.path.join(cpp, "test_pnp_shim" + SUFFIX), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    got = pnp_scene_io.read_results(tmp_path / "out.bin", len(SHIM_CASES))
    for p, k in enumerate(SHIM_CASES):
        assert got["single"][p] == pnp_scene_io.as_bits(expected(k))
        assert got["batch"][p] == pnp_scene_io.as_bits(expected(k, p=p))
        assert got["batch"][p]["valid"] == 1
