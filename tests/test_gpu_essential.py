"""The essential-matrix RANSAC on the device (csrc/essential_solve.hip, openvslam_amd.solve, cpp/openvslam/solve/essential_solver.h) against
the sequential reference tests/essential_ref.py: valid, best_iter, num_inliers and the flags for equality, E_21 and the score as uint64 bit
patterns. Every scene is one of tests/test_essential_ref.py's CASES, whose distance from every decision is asserted there."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import essential_ref as ref
import essential_scene_io as scene_io
from test_essential_ref import (BATCH, CASE_ITERS, GROW_ITERS, ITER_EDGES, ITERS, MARGIN_MIN, SEED, SHIFT, SHIM_CASES, SIZES, SPECIAL, THR, THR_WIDE, expected,
                                problem)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
SUFFIX = os.environ.get("OVS_SHIM_SUFFIX", "")
INVALID, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def solve():
    from openvslam_amd import solve
    return solve


def device_problem(prob):
    return dict(b1=np.array(prob["b1"], np.float64).reshape(-1, 3), b2=np.array(prob["b2"], np.float64).reshape(-1, 3))


def of_device(q):
    return dict(valid=int(q["valid"]), best_iter=q["best_iter"], num_inliers=q["num_inliers"], score=ref.bits(q["score"]),
                E=[ref.bits(float(v)) for v in q["E_21"].ravel()], flags=[int(f) for f in q["inlier_flags"]])


of_reference = ref.as_bits


def run(solve, name, max_num_iter=None, seed=SEED, thr=THR, recompute=True, handle=None):
    return solve.solve_essential_batch([device_problem(problem(name))], thr, CASE_ITERS.get(name, ITERS) if max_num_iter is None else max_num_iter,
                                       recompute, seed, handle=handle)[0]


# ---- the smallest problem (8, 9), the edges of the match loop's wave (63, 64, 65), two and three terms per lane (129, 200), no matches and seven
@pytest.mark.parametrize("recompute", [True, False])
@pytest.mark.parametrize("name", SIZES + SPECIAL + ["empty", "seven"])
def test_result_equals_the_reference_bit_for_bit(solve, name, recompute):
    got, want = of_device(run(solve, name, recompute=recompute)), of_reference(expected(name, recompute=recompute))
    assert got == want
    n = len(problem(name)["b1"])
    if name in SIZES + ["exact", "oblique"]:
        assert got["valid"] == 1 and got["num_inliers"] >= 8
    if name in ("empty", "seven", "equal"):
        assert got == of_reference(ref.invalid(n))


@pytest.mark.parametrize("recompute", [True, False])
@pytest.mark.parametrize("max_num_iter", ITER_EDGES)
def test_hypothesis_grid_edges(solve, max_num_iter, recompute):
    assert of_device(run(solve, "e65", max_num_iter, recompute=recompute)) == of_reference(expected("e65", max_num_iter, recompute=recompute))


def test_without_recompute_the_winner_stays(solve):
    got = of_device(run(solve, "e65", recompute=False))
    again = of_device(run(solve, "e65"))
    assert again["best_iter"] == got["best_iter"] and again["E"] != got["E"] and got["valid"] and again["valid"]


@pytest.mark.parametrize("name,recompute", [("e65", True), ("e65", False), ("e129", True)])
def test_a_wider_threshold(solve, name, recompute):
    got = of_device(run(solve, name, thr=THR_WIDE, recompute=recompute))
    assert got == of_reference(expected(name, thr=THR_WIDE, recompute=recompute)) and got != of_device(run(solve, name, recompute=recompute))


@pytest.mark.parametrize("recompute", [True, False])
def test_batch_equals_its_problems_solved_alone(solve, recompute):
    probs = [device_problem(problem(name)) for name, _ in BATCH]
    assert [len(q["b1"]) for q in probs] == [65, 0, 63, 7, 64, 129]
    got = solve.solve_essential_batch(probs, THR, ITERS, recompute, SEED)
    for (name, p), q, g in zip(BATCH, probs, got):
        alone = solve.solve_essential_batch([q], THR, ITERS, recompute, solve.essential_problem_seed(SEED, p))[0]
        assert of_device(g) == of_device(alone)
        assert of_device(g) == of_reference(expected(name, ITERS, p=p, recompute=recompute))
    for i in (1, 3):   # n = 0 and n = 7 in the middle: the invalid form, and the neighbours above are what they are alone
        assert of_device(got[i]) == of_reference(ref.invalid(len(probs[i]["b1"])))
    assert all(got[i]["valid"] for i in (0, 2, 4, 5))


def test_moving_the_seed_moves_the_hypothesis_numbers(solve):
    whole = of_device(run(solve, "e65", 50, recompute=False))
    part = of_device(run(solve, "e65", 50 - SHIFT, seed=(SEED + 16 * ref.G * SHIFT) & ref.MASK, recompute=False))
    assert part == of_reference(expected("e65", 50 - SHIFT, recompute=False, shift=SHIFT))
    assert part["best_iter"] == whole["best_iter"] - SHIFT and part["E"] == whole["E"] and part["flags"] == whole["flags"]


def test_same_seed_same_bytes_other_seed_other_result(solve):
    h = solve._essential_handle(2, 128)
    a, b = of_device(run(solve, "e65", handle=h)), of_device(run(solve, "e65", handle=h))
    assert a == b
    c = of_device(run(solve, "e65", seed=SEED + 1, handle=h))
    assert c == of_reference(expected("e65", seed=SEED + 1)) and c != a


def test_slots_grow_on_a_live_handle(solve):
    """A handle for one problem holds the slots of 32 hypotheses: 50 need more. The calls before and after it are unchanged."""
    h = solve._essential_handle(1, 70)
    got = [of_device(run(solve, "e65", k, handle=h)) for k in GROW_ITERS]
    assert got == [of_reference(expected("e65", k)) for k in GROW_ITERS]
    assert got[0] == got[2] and got[1]["valid"] == 1


def test_error_contract(solve):
    from openvslam_amd import _lib
    L = _lib.lib()
    h = solve._essential_handle(2, 70)
    ok = lambda: of_device(run(solve, "e65", ITERS, handle=h)) == of_reference(expected("e65", ITERS))
    assert ok()
    q = device_problem(problem("e65"))
    n = 65
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out_d = [np.full(36, -7.0) for _ in range(2)]          # E_21, scores
    out_i = [np.full(8, -7, np.int32) for _ in range(3)]   # valid, best_iter, num_inliers
    flags = np.full(256, 9, np.uint8)

    def call(P=1, offsets=(0, n), b1=q["b1"], b2=q["b2"], thr=THR, iters=ITERS, E=out_d[0], scores=out_d[1], valid=out_i[0], best=out_i[1],
             num=out_i[2], fl=flags, handle=h._h):
        off = None if offsets is None else np.array(offsets, np.int32)
        opt = lambda a: None if a is None else vp(a)
        return L.ovs_essential_solve_batch(handle, P, opt(off), opt(b1), opt(b2), thr, iters, 1, SEED, opt(E), opt(scores), opt(valid), opt(best),
                                           opt(num), opt(fl))

    assert call(handle=None) == INVALID
    for kw in (dict(offsets=None), dict(b1=None), dict(b2=None), dict(E=None), dict(scores=None), dict(valid=None), dict(best=None), dict(num=None),
               dict(fl=None)):
        assert call(**kw) == INVALID, kw
    assert call(P=-1) == INVALID
    assert call(offsets=(1, n)) == INVALID and call(P=2, offsets=(0, 40, 30)) == INVALID
    assert call(iters=0) == INVALID and call(iters=(1 << 20) + 1) == INVALID
    for thr in (0.0, -0.01, 1.0000001, float("nan"), float("inf")):
        assert call(thr=thr) == INVALID, thr
    assert call(P=3, offsets=(0, 20, 40, 60)) == CAPACITY           # more problems than the handle was created for
    big = np.ones((80, 3))
    assert call(offsets=(0, 71), b1=big, b2=big) == CAPACITY        # more matches
    assert all((a == -7).all() for a in out_i) and all((a == -7.0).all() for a in out_d) and (flags == 9).all()   # nothing written
    assert call(P=0) == 0 and (out_i[0] == -7).all()                # no problems: nothing to do
    assert call(P=2, offsets=(0, 7, 7)) == 0                        # n < 8 is not an error
    assert out_i[0][:2].tolist() == [0, 0] and out_i[1][:2].tolist() == [-1, -1] and out_i[2][:2].tolist() == [0, 0]
    assert call(thr=1.0) == 0                                       # the interval's closed end
    assert ok()
    with pytest.raises(_lib.OvsError):
        solve.solve_essential_batch([q, q, q], handle=h)


# ---- the Python class
def test_python_class(solve):
    q = problem("e65")
    n = len(q["b1"])
    bearings_1, bearings_2 = np.array(q["b1"]), np.array(q["b2"])[::-1]
    matches = [(i, n - 1 - i) for i in range(n)]
    s = solve.essential_solver(bearings_1, bearings_2, matches)
    assert not s.solution_is_valid()
    with pytest.raises(RuntimeError):
        s.get_best_E_21()
    s.find_via_ransac(ITERS, seed=SEED)
    got = dict(valid=int(s.solution_is_valid()), best_iter=s.get_best_iter(), num_inliers=s.get_num_inliers(), score=ref.bits(s.get_best_score()),
               E=[ref.bits(float(v)) for v in s.get_best_E_21().ravel()], flags=[int(f) for f in s.get_inlier_matches()])
    assert got == of_reference(expected("e65", ITERS)) and s.solution_is_valid()
    assert solve.essential_problem(bearings_1, bearings_2, matches)["b2"].tolist() == np.array(q["b2"]).tolist()


# ---- the C++ class and its batch entry
def test_cpp_class_returns_the_reference_results_and_the_abis_bytes(solve, tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP, "test_essential_shim"])
    scene_io.write_scene(tmp_path / "scene.bin", [problem(k) for k in SHIM_CASES], THR, ITERS, True, SEED)
    r = subprocess.run([os.path.join(CPP, "test_essential_shim"), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ABI calls failed 0" in r.stdout, r.stdout + r.stderr
    got = scene_io.read_results(tmp_path / "out.bin", [len(problem(k)["b1"]) for k in SHIM_CASES])
    abi = solve.solve_essential_batch([device_problem(problem(k)) for k in SHIM_CASES], THR, ITERS, True, SEED)
    for p, k in enumerate(SHIM_CASES):
        assert got["single"][p] == of_reference(expected(k, ITERS))
        assert got["batch"][p] == of_reference(expected(k, ITERS, p=p)) == of_device(abi[p])
        assert got["batch"][p]["valid"] == 1


# ---- robust::match_frame_and_keyframe through the class
def test_match_frame_and_keyframe_keeps_the_references_inliers(tmp_path):
    """The brute-force pairs the class reports, solved by the reference under the class's own settings (50 iterations, no recompute, its
    default seed and threshold), give the owners the class reports. The scene's distance from every decision is asserted here, on the
    pairs the device matched."""
    from test_gpu_window import _rot
    from openvslam_amd import solve, synth
    subprocess.check_call(["make", "-s", "-C", CPP] + (["asan"] if SUFFIX else ["test_lba_shim"]))
    rng = np.random.default_rng(21)
    n_true, n_wrong = 120, 30
    n = n_true + n_wrong
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(4, 15, n)], 1)
    R2, t2 = _rot((0, 1, 0), 5.0) @ _rot((1, 0, 0), -2.0), np.array([-0.7, 0.1, 0.15])
    b1 = X / np.linalg.norm(X, axis=1, keepdims=True)
    X2 = X @ R2.T + t2
    X2[n_true:] = np.stack([rng.uniform(-4, 4, n_wrong), rng.uniform(-2.5, 2.5, n_wrong), rng.uniform(4, 15, n_wrong)], 1)   # unrelated
    b2 = X2 / np.linalg.norm(X2, axis=1, keepdims=True)
    b1 = b1 + rng.normal(0.0, 0.0005, b1.shape)
    b2 = b2 + rng.normal(0.0, 0.0005, b2.shape)
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 /= np.linalg.norm(b2, axis=1, keepdims=True)
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d2 = np.stack([synth.flip_bits(rng, d1[i], 20) for i in range(n)])
    perm = rng.permutation(n)                 # keyframe keypoints in another order
    d2, b2 = d2[perm], b2[perm]
    ang = np.zeros(n, np.float32)
    has_lm = np.ones(n, np.uint8)
    blob = struct.pack("<3if", n, n, 0, 0.8)
    blob += ang.tobytes() + d1.tobytes() + b1.astype("<f8").tobytes() + ang.tobytes() + d2.tobytes() + b2.astype("<f8").tobytes() + has_lm.tobytes()
    (tmp_path / "mfk.bin").write_bytes(blob)
    subprocess.check_call([os.path.join(CPP, "test_lba_shim" + SUFFIX), "mfk", str(tmp_path / "mfk.bin"), str(tmp_path / "mfk_out.bin")])
    raw = (tmp_path / "mfk_out.bin").read_bytes()
    n_bf, n_inl = (int(v) for v in np.frombuffer(raw[:8], np.int32))
    bf = np.frombuffer(raw[8:8 + 8 * n_bf], np.int32).reshape(n_bf, 2)
    owner = np.frombuffer(raw[8 + 8 * n_bf:], np.int32)
    assert n_bf >= 140 and {(int(a), int(b)) for a, b in bf} <= {(int(perm[j]), j) for j in range(n)}
    prob = dict(b1=[tuple(float(v) for v in b1[a]) for a, _ in bf], b2=[tuple(float(v) for v in b2[b]) for _, b in bf])
    Es = ref.hypotheses(prob, solve.ESSENTIAL_DEFAULT_SEED, 50)
    margin, info = [float("inf")], {}
    want = ref.finish(prob, Es, solve.ESSENTIAL_RESIDUAL_COS_THR, False, margin, None, info)
    best = max(info["scores"])
    assert margin[0] >= MARGIN_MIN and all(s <= best * (1.0 - MARGIN_MIN) for s in info["scores"][:info["scores"].index(best)])
    assert want["valid"] == 1
    got_pairs = {(int(i), int(j)) for i, j in enumerate(owner) if j >= 0}
    assert got_pairs == {(int(a), int(b)) for (a, b), f in zip(bf, want["flags"]) if f} and len(got_pairs) == n_inl == want["num_inliers"]
    kept_true = sum(1 for i, j in got_pairs if i < n_true)
    kept_wrong = sum(1 for i, j in got_pairs if i >= n_true)
    assert kept_true > 0.9 * n_true and kept_wrong < 0.3 * n_wrong
