"""The monocular initialiser's H and F RANSAC on the device (csrc/two_view_solve.hip, openvslam_amd.solve, cpp/openvslam/solve/
{homography,fundamental}_solver.h) against the sequential reference tests/twoview_ref.py: valid, best_iter, num_inliers, selected and the
flags for equality, the matrices and the scores as uint64 bit patterns. Every scene is one of tests/test_twoview_ref.py's CASES, whose
distance from every decision is asserted there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import twoview_ref as ref
import twoview_scene_io
from test_twoview_ref import BATCH, CASE_ITERS, DEGENERATE, GROW_ITERS, ITER_EDGES, ITERS, SEED, SHIM_CASES, SIZES, expected, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def solve():
    from openvslam_amd import solve
    return solve


def device_problem(prob):
    return dict(x1=np.array(prob["x1"], np.float64).reshape(-1, 2), x2=np.array(prob["x2"], np.float64).reshape(-1, 2))


def of_device(r):
    out = {"selected": r["selected"]}
    for m, name, key in ((ref.H, "H", "H_21"), (ref.F, "F", "F_21")):
        q = r[name]
        out[m] = dict(valid=int(q["valid"]), best_iter=q["best_iter"], num_inliers=q["num_inliers"], score=ref.bits(q["score"]),
                      M=[ref.bits(float(v)) for v in q[key].ravel()], flags=[int(f) for f in q["inlier_flags"]])
    return out


of_reference = twoview_scene_io.as_bits


def run(solve, name, max_num_iter=None, seed=SEED, sigma=1.0, recompute=True, models=3, handle=None):
    return solve.solve_two_view_batch([device_problem(problem(name))], sigma, CASE_ITERS.get(name, ITERS) if max_num_iter is None else max_num_iter,
                                      recompute, seed, models, handle=handle)[0]


# ---- the smallest problem (8, 9), the edges of the match loop's wave (63, 64, 65), two and three terms per lane (129, 200), a plane and a cloud
@pytest.mark.parametrize("name", SIZES)
def test_result_equals_the_reference_bit_for_bit(solve, name):
    got, want = of_device(run(solve, name)), of_reference(expected(name))
    assert got == want
    assert got["selected"] == (1 if name.startswith("p") else 2)
    assert got[ref.F]["valid"] == 1 and got[ref.F]["num_inliers"] >= 8


@pytest.mark.parametrize("max_num_iter", ITER_EDGES)
def test_hypothesis_grid_edges(solve, max_num_iter):
    assert of_device(run(solve, "c65", max_num_iter)) == of_reference(expected("c65", max_num_iter))


@pytest.mark.parametrize("name", ["c65", "p65"])
def test_without_recompute_the_winner_stays(solve, name):
    got = of_device(run(solve, name, recompute=False))
    assert got == of_reference(expected(name, recompute=False))
    again = of_device(run(solve, name))
    for m in (ref.H, ref.F):
        assert again[m]["best_iter"] == got[m]["best_iter"] and (not got[m]["valid"] or again[m]["M"] != got[m]["M"])


@pytest.mark.parametrize("name", ["c65", "p65"])
def test_each_model_alone_equals_its_half_of_both(solve, name):
    both = of_device(run(solve, name))
    assert both == of_reference(expected(name))
    for models, m, other in ((1, ref.H, ref.F), (2, ref.F, ref.H)):
        one = of_device(run(solve, name, models=models))
        assert one == of_reference(expected(name, models=models))
        assert one[m] == both[m] and one[other] == of_reference({ref.H: ref.invalid(65), ref.F: ref.invalid(65), "selected": 0})[other]
        assert one["selected"] == (m + 1 if one[m]["valid"] else 0)


@pytest.mark.parametrize("name", ["c65", "p65"])
def test_sigma_two(solve, name):
    got = of_device(run(solve, name, sigma=2.0))
    assert got == of_reference(expected(name, sigma=2.0)) and got != of_device(run(solve, name))


def test_batch_equals_its_problems_solved_alone(solve):
    probs = [device_problem(problem(name)) for name, _ in BATCH]
    assert [len(q["x1"]) for q in probs] == [65, 0, 63, 7, 65, 129]
    got = solve.solve_two_view_batch(probs, 1.0, ITERS, True, SEED)
    for (name, p), q, g in zip(BATCH, probs, got):
        alone = solve.solve_two_view_batch([q], 1.0, ITERS, True, solve.two_view_problem_seed(SEED, p))[0]
        assert of_device(g) == of_device(alone)
        assert of_device(g) == of_reference(expected(name, ITERS, p=p))
    for i in (1, 3):   # n = 0 and n = 7 in the middle: the invalid form, and the neighbours above are what they are alone
        n = len(probs[i]["x1"])
        assert of_device(got[i]) == of_reference(dict({m: ref.invalid(n) for m in (ref.H, ref.F)}, selected=0))
    assert all(got[i]["F"]["valid"] for i in (0, 2, 4, 5))


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_scenes_return_success(solve, name):
    got = of_device(run(solve, name))
    assert got == of_reference(expected(name))
    if name == "equal":
        assert got == of_reference(dict({m: ref.invalid(20) for m in (ref.H, ref.F)}, selected=0))


def test_same_seed_same_bytes_other_seed_other_result(solve):
    h = solve._two_view_handle(2, 128)
    a, b = of_device(run(solve, "c65", handle=h)), of_device(run(solve, "c65", handle=h))
    assert a == b
    c = of_device(run(solve, "c65", seed=SEED + 1, handle=h))
    assert c == of_reference(expected("c65", seed=SEED + 1)) and c != a


def test_slots_grow_on_a_live_handle(solve):
    """A handle for one problem holds the slots of 32 hypotheses of both models: GROW_ITERS needs 64. The calls before and after it are unchanged."""
    h = solve._two_view_handle(1, 70)
    got = [of_device(run(solve, "c65", k, handle=h)) for k in (ITERS, GROW_ITERS, ITERS)]
    assert got == [of_reference(expected("c65", k)) for k in (ITERS, GROW_ITERS, ITERS)]
    assert got[0] == got[2] and got[1][ref.F]["valid"] == 1


def test_error_contract(solve):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = solve._two_view_handle(2, 70)
    ok = lambda: of_device(run(solve, "c65", ITERS, handle=h)) == of_reference(expected("c65", ITERS))
    assert ok()
    q = device_problem(problem("c65"))
    n = 65
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out_d = [np.full(36, -7.0) for _ in range(3)]       # H, F, scores
    out_i = [np.full(8, -7, np.int32) for _ in range(4)]   # valid, best_iter, num_inliers, selected
    flags = [np.full(256, 9, np.uint8) for _ in range(2)]

    def call(P=1, offsets=(0, n), x1=q["x1"], x2=q["x2"], sigma=1.0, iters=ITERS, models=3, H=out_d[0], valid=out_i[0], selected=out_i[3],
             flags_h=flags[0], flags_f=flags[1], handle=h._h):
        off = None if offsets is None else np.array(offsets, np.int32)
        opt = lambda a: None if a is None else vp(a)
        return L.ovs_twoview_solve_batch(handle, P, opt(off), opt(x1), opt(x2), sigma, iters, 1, SEED, models, opt(H), vp(out_d[1]), vp(out_d[2]),
                                         opt(valid), vp(out_i[1]), vp(out_i[2]), opt(selected), opt(flags_h), opt(flags_f))

    assert call(handle=None) == INVALID
    for kw in (dict(offsets=None), dict(x1=None), dict(x2=None), dict(H=None), dict(valid=None), dict(selected=None), dict(flags_h=None),
               dict(flags_f=None)):
        assert call(**kw) == INVALID, kw
    assert call(P=-1) == INVALID
    assert call(offsets=(1, n)) == INVALID and call(P=2, offsets=(0, 40, 30)) == INVALID
    assert call(iters=0) == INVALID and call(iters=(1 << 20) + 1) == INVALID
    assert call(models=0) == INVALID and call(models=4) == INVALID
    assert call(sigma=0.0) == INVALID and call(sigma=float("nan")) == INVALID and call(sigma=float("inf")) == INVALID
    assert call(P=3, offsets=(0, 20, 40, 60)) == CAPACITY           # more problems than the handle was created for
    big = np.ones((80, 2))
    assert call(offsets=(0, 71), x1=big, x2=big) == CAPACITY        # more matches
    assert all((a == -7).all() for a in out_i) and all((a == -7.0).all() for a in out_d) and all((f == 9).all() for f in flags)   # nothing written
    assert call(P=0) == 0 and (out_i[0] == -7).all()                # no problems: nothing to do
    assert call(P=2, offsets=(0, 7, 7)) == 0                        # n < 8 is not an error
    assert out_i[0][:4].tolist() == [0, 0, 0, 0] and out_i[1][:4].tolist() == [-1, -1, -1, -1] and out_i[3][:2].tolist() == [0, 0]
    assert ok()
    c = C.c_void_p()
    assert L.ovs_twoview_create(0, 0, 8, C.byref(c)) == INVALID and L.ovs_twoview_create(0, 1 << 20, 8, C.byref(c)) == INVALID
    with pytest.raises(_lib.OvsError):
        solve.solve_two_view_batch([q, q, q], handle=h)


# ---- the Python classes
def test_python_classes(solve):
    q = problem("p65")
    n = len(q["x1"])
    kp1, kp2 = np.array(q["x1"], np.float32), np.array(q["x2"], np.float32)[::-1]
    matches = [(i, n - 1 - i) for i in range(n)]
    want = of_reference(expected("p65"))
    for cls, m, getter in ((solve.homography_solver, ref.H, "get_best_H_21"), (solve.fundamental_solver, ref.F, "get_best_F_21")):
        s = cls(kp1, kp2, matches, 1.0)
        assert not s.solution_is_valid()
        with pytest.raises(RuntimeError):
            getattr(s, getter)()
        s.find_via_ransac(ITERS, seed=SEED)
        got = dict(valid=int(s.solution_is_valid()), best_iter=s.get_best_iter(), num_inliers=s.get_num_inliers(), score=ref.bits(s.get_best_score()),
                   M=[ref.bits(float(v)) for v in getattr(s, getter)().ravel()], flags=[int(f) for f in s.get_inlier_matches()])
        assert got == want[m] and s.solution_is_valid()


# ---- the C++ classes and the both-models function
def test_cpp_classes_return_the_reference_results(tmp_path):
    cpp = os.path.join(ROOT, "openvslam_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp] + (["asan"] if SUFFIX else ["test_twoview_shim"]))
    twoview_scene_io.write_scene(tmp_path / "scene.bin", [problem(k) for k in SHIM_CASES], 1.0, ITERS, True, SEED)
    r = subprocess.run([os.path.join(cpp, "test_twoview_shim" + SUFFIX), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    got = twoview_scene_io.read_results(tmp_path / "out.bin", [len(problem(k)["x1"]) for k in SHIM_CASES])
    for p, k in enumerate(SHIM_CASES):
        alone = of_reference(expected(k))
        assert got["single"][p][ref.H] == alone[ref.H] and got["single"][p][ref.F] == alone[ref.F]
        assert got["both"][p] == of_reference(expected(k, p=p))
        assert got["both"][p]["selected"] == (1 if k.startswith("p") else 2)
