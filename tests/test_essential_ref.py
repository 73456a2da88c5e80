"""The sequential reference of the essential-matrix RANSAC (tests/essential_ref.py; DESIGN.md 3.16, rules E1 to E8) checked on its own: the
sampler, the round ordering, the planted [t]x R on exact data, the fixed sweeps, an N-version check of the refit against numpy.linalg.svd
-- and the conditions the device tests rest on: every scene they use keeps every residual a relative 1e-9 away from the threshold and
every winner's score as far from an earlier hypothesis's, so that no last-bit difference could flip a flag or a winner. The same algebra
as a plain host program (tests/essential_host.cc over csrc/essential_math.inc) equals the reference bit for bit, and runs clean under
AddressSanitizer and UndefinedBehaviorSanitizer. Plus the C ABI's argument errors, which are decided before the device is touched, and
the C++ class's degraded result when its device is absent."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import essential_ref as ref
import essential_scene_io as scene_io
from essential_scene_io import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
SEED, ITERS = 2468, 16
THR = ref.RESIDUAL_COS_THR            # one degree, upstream's constant
THR_WIDE = 0.03489949670250097        # two degrees
MARGIN_MIN, OFF_MAX = 1e-9, 1e-13
# the refit on exact data against the planted [t]x R (unit Frobenius norm, sign aligned): the reference's own worst error over the scenes
# of test_refit_recovers_the_planted_matrix_on_exact_data per number of matches (measured, 20 scenes each), the bound 100
# times that. Eight matches determine E_21 and no more: the minimal problem's conditioning, not the sweeps, sets its figure.
EXACT_WORST = {8: 2.66e-8, 65: 6.82e-13, 200: 5.86e-13}
EXACT_BOUND = {k: 100.0 * v for k, v in EXACT_WORST.items()}

# every scene the device tests use
CASES = {
    "e8": lambda: scene(8, noise_deg=0.05, outlier_fraction=0.0),
    "e9": lambda: scene(9, noise_deg=0.05, outlier_fraction=0.0),
    "e63": lambda: scene(63),
    "e64": lambda: scene(64),
    "e65": lambda: scene(65),
    "e129": lambda: scene(129),
    "e200": lambda: scene(200),
    "exact": lambda: scene(40, noise_deg=0.0, outlier_fraction=0.0),
    "zero": lambda: scene(40, outlier_fraction=0.0, zero_baseline=True),
    # one bearing everywhere: the system has rank one and every vector of its null space meets every constraint. Along the optical axis the
    # chosen vector maps the bearing to zero and the problem is invalid (n > 0.0 is false); an oblique bearing gives a model that every
    # match fits: valid by the rules, and as meaningless as upstream's
    "equal": lambda: scene(20, all_equal=(0.0, 0.0, 1.0)),
    "oblique": lambda: scene(20, all_equal=(0.0, 0.6, 0.8)),
    "empty": lambda: scene(0),
    "seven": lambda: scene(7, outlier_fraction=0.0),
}
SIZES = ["e8", "e9", "e63", "e64", "e65", "e129", "e200"]
SPECIAL = ["exact", "zero", "equal", "oblique"]
# (eight matches: every sample is the whole problem, in another order, and the scores agree to rounding: one hypothesis. Nine: nine subsets.
# Exact data: every sample gives the planted matrix to rounding and the scores agree as closely: one hypothesis and its refit)
CASE_ITERS = {"e8": 1, "e9": 3, "e65": 50, "exact": 1}
ITER_EDGES = (1, 2, 50)                       # on "e65"
GROW_ITERS = (2, 50, 2)                       # a handle for one problem is created with the slots of 32 hypotheses
SHIFT = 3                                     # the seed-shift test: hypotheses SHIFT .. 49 of "e65" as hypotheses 0 .. 49 - SHIFT
BATCH = [("e65", 0), ("empty", 1), ("e63", 2), ("seven", 3), ("e64", 4), ("e129", 5)]
SHIM_CASES = ["e65", "e64"]                   # the C++ program's problems (positions 0 and 1 of its batch call)


@functools.lru_cache(maxsize=None)
def problem(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def models_of(name, seed=SEED, p=0):
    """([E_21 per h], worst off-diagonal ratio) of a case: computed once, shared by the CPU and the device tests."""
    stats = {}
    Es = ref.hypotheses(problem(name), seed, CASE_ITERS.get(name, ITERS), p, stats)
    return Es, stats.get("off", 0.0)


@functools.lru_cache(maxsize=None)
def _finished(name, max_num_iter, seed, p, thr, recompute, shift):
    Es = models_of(name, seed, p)[0]
    k = CASE_ITERS.get(name, ITERS) if max_num_iter is None else max_num_iter
    assert shift + k <= len(Es) or not Es
    margin, stats, info = [float("inf")], {}, {}
    res = ref.finish(problem(name), Es[shift:shift + k], thr, recompute, margin, stats, info)
    return res, dict(margin=margin[0], off=stats.get("off", 0.0), scores=info["scores"])


def expected(name, max_num_iter=None, seed=SEED, p=0, thr=THR, recompute=True, shift=0):
    """The reference result of a case for the hypotheses shift .. shift + max_num_iter - 1 (they are independent: a slice)."""
    return _finished(name, max_num_iter, seed, p, thr, recompute, shift)[0]


def every_use(name):
    """Every (max_num_iter, seed, p, thr, recompute, shift) under which a device test solves the case."""
    uses = [(None, SEED, 0, THR, True, 0), (None, SEED, 0, THR, False, 0)]
    if name == "e65":
        uses += [(k, SEED, 0, THR, rc, 0) for k in ITER_EDGES for rc in (True, False)]
        uses += [(None, SEED, 0, THR_WIDE, rc, 0) for rc in (True, False)]
        uses += [(ITERS, SEED, 0, THR, True, 0), (None, SEED + 1, 0, THR, True, 0), (50 - SHIFT, SEED, 0, THR, False, SHIFT)]
    if name == "e129":
        uses += [(None, SEED, 0, THR_WIDE, True, 0)]
    if name in SHIM_CASES:
        uses += [(ITERS, SEED, 0, THR, True, 0), (ITERS, SEED, SHIM_CASES.index(name), THR, True, 0)]
    uses += [(ITERS, SEED, p, THR, rc, 0) for case, p in BATCH if case == name for rc in (True, False)]
    return uses


# ---- E1
@pytest.mark.parametrize("n", [8, 9, 10, 64, 1000])
def test_sample_is_eight_distinct_indices_below_n(n):
    for h in range(200):
        idx = ref.sample(SEED, h % 5, h, n)
        assert len(set(idx)) == 8 and all(0 <= i < n for i in idx)
    if n == 8:
        assert sorted(ref.sample(SEED, 0, 0, 8)) == list(range(8))


def test_sample_is_a_function_of_seed_problem_and_hypothesis():
    G, MASK = ref.G, ref.MASK
    a = [ref.sample(SEED, 2, h, 100) for h in range(50)]
    assert a == [ref.sample(SEED, 2, h, 100) for h in range(50)]
    assert a != [ref.sample(SEED + 1, 2, h, 100) for h in range(50)] and a != [ref.sample(SEED, 3, h, 100) for h in range(50)]
    # problem p of a batch draws what problem 0 draws under essential_problem_seed
    assert a == [ref.sample(ref.problem_seed(SEED, 2), 0, h, 100) for h in range(50)]
    # moving the seed by 16 G d moves the hypothesis numbers by d
    assert a[7:] == [ref.sample((SEED + G * 16 * 7) & MASK, 2, h, 100) for h in range(43)]
    from openvslam_amd import solve
    assert solve.essential_problem_seed(SEED, 2) == ref.problem_seed(SEED, 2) == (SEED + G * (2 << 24)) & MASK
    assert solve.ESSENTIAL_RESIDUAL_COS_THR == ref.RESIDUAL_COS_THR == float(np.float32(0.01745240643))


# ---- E3
def test_a_sweep_is_nine_rounds_of_four_disjoint_pairs():
    seen = set()
    for r in range(9):
        pairs = ref.round_pairs(r)
        assert len(pairs) == 4 and all(p < q for p, q in pairs)
        assert sorted(i for pq in pairs for i in pq) == [i for i in range(9) if i != r]   # disjoint, index r idles
        seen.update(pairs)
    assert seen == {(p, q) for p in range(9) for q in range(p + 1, 9)}
    assert ref.round_pairs(0) == [(1, 8), (2, 7), (3, 6), (4, 5)] and ref.round_pairs(8) == [(0, 7), (1, 6), (2, 5), (3, 4)]


def test_the_rounds_diagonalise_and_keep_the_spectrum():
    for n in (8, 9, 65, 300):
        q = scene(n, rng_seed=11)
        N = ref.system([ref.row_of(a, b) for a, b in zip(q["b1"], q["b2"])])
        A, V = ref.jacobi_rounds(N)
        assert ref.off_ratio(N, A) <= OFF_MAX
        A, V, N = np.array(A), np.array(V), np.array(N)
        assert np.abs(V.T @ V - np.eye(9)).max() < 1e-14
        assert np.abs(np.sort(np.diag(A)) - np.linalg.eigvalsh(N)).max() <= 1e-13 * np.abs(N).max()
        assert np.abs(V @ np.diag(np.diag(A)) @ V.T - N).max() <= 1e-13 * np.abs(N).max()
    Z = [[0.0] * 9 for _ in range(9)]
    A, V = ref.jacobi_rounds(Z)       # a pair whose entry is 0.0 does not rotate
    assert A == Z and V == [[1.0 if r == c else 0.0 for c in range(9)] for r in range(9)]


# ---- what makes the bit comparison sound
@pytest.mark.parametrize("name", SIZES + SPECIAL)
def test_every_use_keeps_its_distance_from_every_decision(name):
    assert models_of(name)[1] <= OFF_MAX
    for use in every_use(name):
        k, seed, p, thr, recompute, shift = use
        assert models_of(name, seed, p)[1] <= OFF_MAX
        res, info = _finished(name, k, seed, p, thr, recompute, shift)
        assert info["margin"] >= MARGIN_MIN and info["off"] <= OFF_MAX, (use, info["margin"], info["off"])
        scores = info["scores"]
        best = max((s for s in scores if s == s), default=0.0)
        if best <= 0.0:
            continue
        h = scores.index(best)
        for g, s in enumerate(scores):   # a runner-up within 1e-9 may only be a later hypothesis (an exact tie keeps the lowest h)
            assert g >= h or s != s or s <= best * (1.0 - MARGIN_MIN), (use, h, g)


def test_the_noisy_scenes_are_valid_and_the_degenerate_ones_are_not():
    for name in SIZES + ["exact"]:
        for rc in (True, False):
            r = expected(name, recompute=rc)
            assert r["valid"] == 1 and r["num_inliers"] >= 8 and r["score"] > 0.0 and 0 <= r["best_iter"], name
    for name in ("empty", "seven", "equal"):
        assert expected(name) == ref.invalid(len(problem(name)["b1"])), name
    assert expected("oblique")["num_inliers"] == 20
    a, b = expected("e65", recompute=True), expected("e65", recompute=False)
    assert a["best_iter"] == b["best_iter"] and a["E"] != b["E"]
    assert expected("e65", thr=THR_WIDE)["num_inliers"] >= expected("e65")["num_inliers"]


def test_the_seed_shift_use_moves_the_winner():
    whole, part = expected("e65", 50, recompute=False), expected("e65", 50 - SHIFT, recompute=False, shift=SHIFT)
    assert whole["best_iter"] >= SHIFT and part["best_iter"] == whole["best_iter"] - SHIFT
    assert part["E"] == whole["E"] and part["flags"] == whole["flags"]


def _aligned_error(M, P):
    M, P = np.array(M, np.float64).reshape(3, 3), np.asarray(P)
    M, P = M / np.linalg.norm(M), P / np.linalg.norm(P)
    return min(np.abs(M - P).max(), np.abs(M + P).max())


def test_refit_recovers_the_planted_matrix_on_exact_data():
    """Worst error measured on the CPU, 20 scenes per size: 2.66e-8 at 8 matches, 6.82e-13 at 65, 5.86e-13 at 200."""
    worst = {k: 0.0 for k in EXACT_WORST}
    for n in worst:
        for k in range(20):
            prob = scene(n, noise_deg=0.0, outlier_fraction=0.0, rng_seed=k)
            worst[n] = max(worst[n], _aligned_error(ref.fit(prob, range(n)), scene_io.planted()))
    print("worst error against the planted matrix per number of matches:", {k: "%.3g" % v for k, v in worst.items()})
    assert all(worst[k] <= EXACT_BOUND[k] for k in worst)
    E = ref.fit(problem("exact"), range(40))   # rank two: E_21's determinant is rounding
    assert abs(np.linalg.det(np.array(E).reshape(3, 3))) < 1e-15


def _svd_fit(rows):
    Gm = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Gm)
    return [float(v) for v in (U @ np.diag([S[0], S[1], 0.0]) @ Vt).ravel()]


@pytest.mark.parametrize("name", ["e65", "e200"])
def test_refit_agrees_with_numpy_svd(name):
    """N-version: the refit over the winner's inliers with numpy.linalg.svd in place of the Jacobi rounds and of the rank-two step
    classifies every match as the reference does."""
    prob, want = problem(name), expected(name)
    assert want["valid"]
    flags = ref.check(models_of(name)[0][want["best_iter"]], prob, THR)[0]
    E = ref.fit(prob, [i for i, f in enumerate(flags) if f], eig=_svd_fit)
    assert ref.check(E, prob, THR)[0] == want["flags"]
    assert _aligned_error(want["E"], np.array(E).reshape(3, 3)) < 1e-9


# ---- the same algebra by a plain host compiler
def _scene_file(tmp_path, names, k, thr, recompute):
    path = tmp_path / ("case_%s_%d_%d.bin" % ("_".join(names), k, recompute))
    scene_io.write_scene(path, [problem(n) for n in names], thr, k, recompute, SEED)
    return path


def _host_runs():
    """(names, iterations, threshold, recompute): together every case, both refit settings, both thresholds and a batch position."""
    runs = [([n], CASE_ITERS.get(n, ITERS), THR, rc) for n in SIZES + SPECIAL + ["empty", "seven"] for rc in (True, False)]
    runs += [(["e65"], CASE_ITERS["e65"], THR_WIDE, True), ([n for n, _ in BATCH], ITERS, THR, True)]
    return runs


def test_essential_host_equals_the_reference_bit_for_bit(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP, "essential_host"])
    for names, k, thr, rc in _host_runs():
        out = subprocess.run([os.path.join(CPP, "essential_host"), str(_scene_file(tmp_path, names, k, thr, rc))], capture_output=True, text=True,
                             check=True, timeout=120).stdout
        got = scene_io.read_host(out)
        assert len(got) == len(names)
        for p, n in enumerate(names):
            assert got[p] == ref.as_bits(expected(n, k, p=p, thr=thr, recompute=rc)), (names, p, k, thr, rc)


def test_essential_host_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main on this CPU: AddressSanitizer and UndefinedBehaviorSanitizer linked in; the test puts
    nothing into the child's environment and takes nothing out of it."""
    subprocess.check_call(["make", "-s", "-C", CPP, "essential_host_san"])
    for names, k, thr, rc in [(["e65", "empty", "seven", "equal", "e200"], ITERS, THR, True), (["e8"], 1, THR, False)]:
        r = subprocess.run([os.path.join(CPP, "essential_host_san"), str(_scene_file(tmp_path, names, k, thr, rc))], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert scene_io.read_host(r.stdout)[0] == ref.as_bits(expected(names[0], k, thr=thr, recompute=rc))


# ---- the C ABI's argument errors, decided before the device is touched
def test_argument_errors_need_no_device():
    from openvslam_amd import _lib
    L = _lib.lib()
    INVALID, NO_DEVICE = -1, -2
    h = C.c_void_p()
    assert L.ovs_essential_create(0, 0, 100, C.byref(h)) == INVALID and L.ovs_essential_create(0, 4, 0, C.byref(h)) == INVALID
    assert L.ovs_essential_create(0, 4, 100, None) == INVALID and L.ovs_essential_create(0, 1 << 20, 8, C.byref(h)) == INVALID
    assert L.ovs_essential_create(99, 4, 100, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_essential_create(-1, 4, 100, C.byref(h)) == NO_DEVICE and not h
    assert L.ovs_essential_destroy(None) == INVALID
    args = [None] * 6
    # without a device there is no handle, and a NULL handle is refused whatever else is passed: the checks of max_num_iter and
    # residual_cos_thr need a live one and are exercised by tests/test_gpu_essential.py::test_error_contract
    assert L.ovs_essential_solve_batch(None, 1, None, None, None, THR, 16, 1, SEED, *args) == INVALID


# ---- the C++ class without a device: the failure policy's empty result
def test_cpp_class_degrades_without_its_device(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP, "test_essential_shim"])
    scene_io.write_scene(tmp_path / "scene.bin", [problem(k) for k in SHIM_CASES], THR, ITERS, True, SEED)
    r = subprocess.run([os.path.join(CPP, "test_essential_shim"), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "99"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = scene_io.read_results(tmp_path / "out.bin", [len(problem(k)["b1"]) for k in SHIM_CASES])
    for p, k in enumerate(SHIM_CASES):
        empty = ref.as_bits(ref.invalid(len(problem(k)["b1"])))
        assert got["single"][p] == empty and got["batch"][p] == empty
