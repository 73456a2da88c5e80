"""tests/observe_ref.py -- the sequential statement of search_local_landmarks' visibility rules -- against hand-computed
cases for every gate, against a second, vectorised form of V3 - V5 on the scenes the GPU tests use, those scenes against the conditions they have
to meet, and the resources of k_observe_landmarks that DESIGN quotes. No device."""
import math
import os
import sys

import numpy as np
import pytest

import observe_ref as ref
import observe_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
NL, LSF = scenes.NUM_LEVELS, scenes.LOG_SCALE_FACTOR
UP = (0.0, 0.0, 1.0)   # a normal along the viewing ray of a landmark on the optical axis


def _cam(oracle, cx=0.0, cy=0.0, model=0):
    # fx = fy = 512: u = 512 * x / z + cx scales by a power of two, so bounds can be hit exactly
    return oracle.Camera(model, 0, 512.0, 512.0, cx, cy, 0.0, 0.0, 640, 480), oracle.grid_params(640, 480)


def _see(oracle, X, dmin=0.01, dmax=1000.0, nrm=UP, cx=0.0, cy=0.0, lsf=LSF):
    cam, gp = _cam(oracle, cx, cy)
    return ref.can_observe(oracle, cam, gp, EYE, X, dmin, dmax, nrm, NL, lsf)


def test_behind_the_camera(oracle):
    assert _see(oracle, (0.1, 0.1, -1.0)) == (ref.DEPTH, (0.0, 0.0), -1.0, 0)
    assert _see(oracle, (0.1, 0.1, 0.0))[0] == ref.DEPTH          # pcz <= 0 rejects zero too
    assert _see(oracle, (0.1, 0.1, 5e-324))[0] != ref.DEPTH
    cam, gp = _cam(oracle, model=1)                                # the equirectangular model never rejects
    assert ref.can_observe(oracle, cam, gp, EYE, (0.1, 0.1, -1.0), 0.01, 1000.0, (0.1, 0.1, -1.0), NL, LSF)[0] == ref.OBSERVABLE


def test_one_ulp_either_side_of_each_image_bound(oracle):
    """z = 1, cx = cy = 0: u = 512 x and v = 512 y exactly. Bounds [0, 640] x [0, 480], both ends inside (upstream rejects u < min || u > max)."""
    nrm = lambda X: [c / math.sqrt(sum(a * a for a in X)) for c in X]
    inside = [(1.25, 0.5, 640.0, 256.0), (0.0, 0.5, 0.0, 256.0), (0.5, 0.9375, 256.0, 480.0), (0.5, 0.0, 256.0, 0.0)]
    for x, y, u, v in inside:
        out, uv, _, _ = _see(oracle, (x, y, 1.0), nrm=nrm((x, y, 1.0)))
        assert out == ref.OBSERVABLE and uv == (u, v), (x, y)
    step = lambda a, to: float(np.nextafter(a, to))
    outside = [(step(1.25, 2.0), 0.5), (step(0.0, -1.0), 0.5), (0.5, step(0.9375, 1.0)), (0.5, step(0.0, -1.0))]
    for x, y in outside:
        assert _see(oracle, (x, y, 1.0), nrm=nrm((x, y, 1.0))) == (ref.BOUNDS, (0.0, 0.0), -1.0, 0), (x, y)
    # the projection of the first of them IS one ulp beyond the bound
    cam, gp = _cam(oracle)
    ok, uv, _ = oracle.reproject_to_image(cam, gp, EYE, [outside[0][0], 0.5, 1.0])
    assert not ok and uv[0] == step(640.0, 1000.0)


def test_one_ulp_either_side_of_both_range_limits(oracle):
    """On the optical axis dist = sqrt(z * z) = z exactly. The limits are floats: (float)(0.7 * dmin), (float)(1.3 * dmax)."""
    dmin, dmax = 3.0, 7.0
    lo, hi = ref.range_limits(dmin, dmax)
    assert (lo, hi) == (ref.f32(0.7 * 3.0), ref.f32(1.3 * 7.0)) and lo != 0.7 * 3.0 and hi != 1.3 * 7.0   # the narrowing matters
    step = lambda a, to: float(np.nextafter(a, to))
    see = lambda z: _see(oracle, (0.0, 0.0, z), dmin, dmax, cx=320.0, cy=240.0)[0]
    assert see(lo) == ref.OBSERVABLE and see(step(lo, 0.0)) == ref.RANGE
    assert see(hi) == ref.OBSERVABLE and see(step(hi, 100.0)) == ref.RANGE


def test_one_ulp_either_side_of_the_viewing_angle(oracle):
    """dist = 4 on the axis, normal (0, 0, nz): dot = 4 nz exactly, the threshold 0.5 * 4 = 2."""
    step = lambda a, to: float(np.nextafter(a, to))
    see = lambda nz: _see(oracle, (0.0, 0.0, 4.0), 1.0, 8.0, nrm=(0.0, 0.0, nz), cx=320.0, cy=240.0)[0]
    assert see(0.5) == ref.OBSERVABLE and see(step(0.5, 1.0)) == ref.OBSERVABLE and see(step(0.5, 0.0)) == ref.ANGLE
    assert see(-1.0) == ref.ANGLE


def test_division_form_of_the_angle_gate_agrees_with_the_product_form():
    """Upstream: dot / dist < 0.5. The kernel: dot < 0.5 * dist. 0.5 * dist is exact, and a quotient of doubles whose exact value is below one
    half is at most 0.5 - 2^-54, which cannot round up to 0.5. Checked here on the doubles next to the threshold. (0.5 * dist is exact for every
    dist from 2^-1021 up; below that the halving of a subnormal may round, at distances no landmark has.)"""
    rng = np.random.default_rng(3)
    dist = np.concatenate([rng.uniform(1e-3, 1e3, 20000), 2.0 ** rng.integers(-20, 20, 2000), [2.0 ** -1021, 3e-308, 1e300]])
    half = 0.5 * dist
    for k in range(-3, 4):
        dot = half.copy()
        for _ in range(abs(k)):
            dot = np.nextafter(dot, np.inf if k > 0 else -np.inf)
        with np.errstate(over="ignore", under="ignore"):
            assert np.array_equal(dot / dist < 0.5, dot < half), k
    dot = rng.uniform(-1, 1, len(dist)) * dist
    assert np.array_equal(dot / dist < 0.5, dot < half)


def test_level_on_exact_integers_and_both_clamps(oracle):
    """With log_scale_factor = logf(2) a ratio of 2 gives the quotient 1.0 exactly: ceilf keeps it, the next ratio up goes to level 2."""
    lg2 = ref.f32(float(oracle.detmath_eval(oracle.DETMATH_LOGF, [2.0])[0]))
    assert abs(lg2 - math.log(2.0)) < 1e-7
    level = lambda dmax, dist, lsf=lg2: ref.predict_level(oracle, dmax, dist, NL, lsf)
    assert float(oracle.detmath_eval(oracle.DETMATH_LOGF, [1.0])[0]) == 0.0
    assert level(4.0, 4.0) == 0                                              # ratio 1: logf = 0, level 0
    assert level(float(np.nextafter(np.float32(4.0), np.float32(8.0))), 4.0) == 1   # one float above ratio 1
    assert level(8.0, 4.0) == 1                                              # ratio 2: quotient 1.0 exactly
    assert level(float(np.nextafter(np.float32(8.0), np.float32(16.0))), 4.0) == 2
    assert level(float(np.nextafter(np.float32(8.0), np.float32(0.0))), 4.0) == 1
    # (float)dist: a double distance one ulp above 4 narrows to 4.0f and stays on the integer
    assert level(8.0, float(np.nextafter(4.0, 5.0))) == 1
    # clamps, through the whole gate: ratio 0.8 -> ceilf(-1.22) = -1 -> 0; ratio 1000 -> ceilf(37.9) -> num_levels - 1
    assert _see(oracle, (0.0, 0.0, 1.25), 1.0, 1.0, cx=320.0, cy=240.0) == (ref.OBSERVABLE, (320.0, 240.0), 320.0, 0)
    assert _see(oracle, (0.0, 0.0, 1.0), 1.0, 1000.0, cx=320.0, cy=240.0) == (ref.OBSERVABLE, (320.0, 240.0), 320.0, NL - 1)
    assert level(0.0, 1.0, LSF) == 0     # logf(0) = -inf


def test_not_searched_means_not_observable_with_the_defined_values(oracle):
    sc = scenes.scene(0, 50, 40, 5)
    sc.search[:] = 0
    r = scenes.reference(oracle, ref, sc, 5.0, 0.8)
    assert r["num_observable"] == r["num_matches"] == 0 and (r["outcome"] == ref.SKIPPED).all() and (r["assigned"] == -1).all()
    assert not r["reproj"].any() and (r["x_right"] == -1.0).all() and not r["level"].any()


CASES = [(model, stereo, 300, m) for model, stereo in ((0, False), (0, True), (1, False)) for m in (1, 63, 64, 65, 255, 256, 257)] + \
        [(model, stereo, 2000, 3000) for model, stereo in ((0, False), (0, True), (1, False))]


def seed_of(model, stereo, n, m):
    return 1000 * model + 500 * int(stereo) + m + n


@pytest.fixture(scope="module")
def refs(oracle):
    """The reference of every scene at margin 5, computed once."""
    out = {}
    for model, stereo, n, m in CASES:
        sc = scenes.scene(model, n, m, seed_of(model, stereo, n, m), stereo)
        out[(model, stereo, n, m)] = (sc, scenes.reference(oracle, ref, sc, 5.0, 0.8))
    return out


def check_scene_conditions(oracle, sc, r, margin):
    """What the issue asks of a scene with m >= 256 (fewer landmarks cannot give n / 20 matches): every outcome the camera model can produce at
    least five times -- the equirectangular model never rejects in V2, so there the two V2 outcomes must not occur at all --, more than n / 20
    matches, and a contended keypoint."""
    counts = np.bincount(r["outcome"], minlength=6)
    possible = [ref.SKIPPED, ref.RANGE, ref.ANGLE, ref.OBSERVABLE] + ([ref.DEPTH, ref.BOUNDS] if sc.model == 0 else [])
    assert all(counts[o] >= 5 for o in possible), dict(zip(ref.OUTCOME_NAMES, counts))
    if sc.model == 1:
        assert counts[ref.DEPTH] == counts[ref.BOUNDS] == 0
    assert r["num_matches"] > sc.n // 20, r["num_matches"]
    hit = r["assigned"][r["assigned"] >= 0]
    assert len(np.unique(hit)) == len(hit) == r["num_matches"] and not sc.occupied[hit].any()
    assert len(scenes.contended_keypoints(oracle, sc, r, margin, 0.8)) >= 1


@pytest.mark.parametrize("case", [c for c in CASES if c[3] >= 256], ids=str)
def test_scenes_meet_their_conditions(oracle, refs, case):
    sc, r = refs[case]
    check_scene_conditions(oracle, sc, r, 5.0)
    if sc.x_right is not None:   # the stereo test takes part: without the frame's stereo_x_right the matches differ
        mono = scenes.scene(sc.model, sc.n, sc.m, seed_of(*case), True)
        mono.x_right = None
        assert not np.array_equal(scenes.reference(oracle, ref, mono, 5.0, 0.8)["assigned"], r["assigned"])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_vectorised_gates_equal_the_sequential_ones(oracle, refs, case):
    sc, r = refs[case]
    outcome, level = ref.gates_vectorised(oracle, sc.pose, sc.pos, sc.dmm, sc.nrm, NL, LSF)
    reached = np.isin(r["outcome"], (ref.RANGE, ref.ANGLE, ref.OBSERVABLE))   # the landmarks V1 and V2 let through
    assert np.array_equal(outcome[reached], r["outcome"][reached]) and np.array_equal(level[reached], r["level"][reached])
    assert sc.m < 63 or reached.sum() > sc.m // 2


def test_kernel_appears_once_without_scratch_and_with_the_registers_design_quotes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    rows = [r for r in kr.collect(files={"match_window.hip"}) if "k_observe_landmarks" in r[1]]
    assert len(rows) == 1
    _, _, vgpr, agpr, sgpr, scratch, lds, max_wg = rows[0]
    print("k_observe_landmarks: vgpr", vgpr, "agpr", agpr, "sgpr", sgpr, "scratch", scratch, "lds", lds)
    assert scratch == 0 and lds == 0 and agpr == 0 and max_wg == 256
    # DESIGN.md 3.17 quotes these figures; a change of the source or of the compiler that moves them has to move DESIGN with them
    assert (vgpr, sgpr) == (40, 84)
