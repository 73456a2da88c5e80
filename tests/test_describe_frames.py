"""The frames of tests/describe_frames.py really reach the edges of k_describe they are built for, and the expectation the GPU tests
(tests/test_gpu_describe.py) compare against rests on two legs: the C oracle and the numpy restatement of tests/nversion_numpy.py agree on
every angle (bit pattern), every blurred level (both tap variants) and every descriptor (both trigonometry variants) of every frame.
CPU only. Every condition is asserted by its own name with its own minimum; none may be skipped."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_frames as df   # noqa: E402
import nversion_numpy as nv   # noqa: E402

# condition -> smallest count that will do (the frame is rebuilt until it is reached, never the number lowered)
ORIENTATION = {"m10_zero_m01_zero": 1, "m01_zero_m10_pos": 1, "m01_zero_m10_neg": 1, "m10_zero_m01_pos": 1, "m10_zero_m01_neg": 1,
               "tie_q1": 1, "tie_q2": 1, "tie_q3": 1, "tie_q4": 1, "abs_m10_is_abs_m01_plus_1": 2, "abs_m10_is_abs_m01_minus_1": 2,
               "upper_level_angle_q1": 1, "upper_level_angle_q2": 1, "upper_level_angle_q3": 1, "upper_level_angle_q4": 1,
               "angle_exactly_0": 1, "angle_exactly_90": 1, "angle_exactly_180": 1, "angle_exactly_270": 1}
BORDER = dict({"level0_%s_%s" % (a, b): 1 for a in ("left", "mid", "right") for b in ("top", "mid", "bottom") if (a, b) != ("mid", "mid")},
              **{"level0_residue_%d" % r: 1 for r in range(16)})
SATURATION = {"sampled_blurred_255_taps0": 1000, "sampled_blurred_255_taps1": 1000, "sampled_unclamped_above_255_taps1": 1000,
              "sampled_row_sum_65535_taps1": 1000, "keypoints_taps0": 100, "keypoints_taps1": 100}
# the inverse: blurred zeros everywhere, and the 255 plateaus' centres (few pixels, but sampled)
SATURATION_INVERSE = {"sampled_blurred_0_taps0": 1000, "sampled_blurred_0_taps1": 1000, "sampled_blurred_255_taps0": 1, "sampled_blurred_255_taps1": 1,
                      "sampled_unclamped_above_255_taps1": 1, "sampled_row_sum_65535_taps1": 1, "keypoints_taps0": 100, "keypoints_taps1": 100}
MINIMA = {
    "orientation": ORIENTATION,
    "border_c0": BORDER,
    "border_c4": BORDER,
    "noise": {"upper_level_residues_covered": 16, "keypoints": 200, "levels_with_keypoints": 8},
    "saturation_dark_dots": SATURATION,
    "saturation_bright_dots": SATURATION_INVERSE,
    "level0_empty": {"upper_levels_count": 20, "lower_level_empty_below_a_populated_one": 1},
    "middle_level_empty": {"level0_count": 5, "middle_empty_levels": 1, "upper_levels_count": 3},
    "level0_only": {"level0_count": 20},
}
EXACT = {   # conditions that must hold with exactly this value
    "border_c0": {"level0_no_keypoint_outside_22": 0},
    "border_c4": {"level0_no_keypoint_outside_22": 0},
    "level0_empty": {"level0_count": 0},
    "level0_only": {"upper_levels_count": 0},
}
CASES = [(name, cond) for name in sorted(MINIMA) for cond in sorted(MINIMA[name]) + sorted(EXACT.get(name, {}))]

_cache = {}


def _conditions(oracle, name):
    if name not in _cache:
        img, p = df.FRAMES[name]()
        _cache[name] = df.conditions(oracle, name, img, p)
    return _cache[name]


def test_every_frame_has_its_conditions_listed():
    assert sorted(MINIMA) == sorted(df.FRAMES) == sorted(df.CONDITIONS)


@pytest.mark.parametrize("name,cond", CASES)
def test_frame_reaches_its_condition(oracle, name, cond):
    got = _conditions(oracle, name)
    assert cond in got, (name, cond, sorted(got))
    if cond in EXACT.get(name, {}):
        assert got[cond] == EXACT[name][cond], (name, cond, got[cond])
    else:
        assert got[cond] >= MINIMA[name][cond], (name, cond, got[cond])


def test_frame_sizes_and_keypoint_counts(oracle):
    """264 x 200 to 640 x 480, at most a few hundred keypoints, widths the device entry accepts; the two border widths are the two residues
    of cols % 16 the staging paths split on."""
    for name, build in df.FRAMES.items():
        img, p = build()
        assert img.dtype == np.uint8 and 200 <= img.shape[0] <= 480 and 264 <= img.shape[1] <= 640 and img.shape[1] % 4 == 0, name
        _, kps, _, _ = df.run_oracle(oracle, img, p)
        assert 1 <= len(kps) <= 400, (name, len(kps))
    assert df.FRAMES["border_c0"]()[0].shape[1] % 16 == 0 and df.FRAMES["border_c4"]()[0].shape[1] % 16 == 4


def test_pixels_one_step_outside_the_legal_range_are_no_keypoints(oracle):
    """x = 22 .. cols - 23 (and the same in y) is the whole range: a bright pixel one step further out is not detected."""
    rows, cols = 200, 272
    img = np.full((rows, cols), 100, np.uint8)
    for x, y in ((21, 60), (cols - 22, 100), (90, 21), (150, rows - 22)):
        img[y, x] = 255
    img[140, 140] = 255   # (the control)
    p = df.params(500)
    _, kps, _, counts = df.run_oracle(oracle, img, p)
    xs, ys = df.level_positions(oracle, kps, p)
    l0 = kps["octave"] == 0
    assert counts[0] == 1 and (int(xs[l0][0]), int(ys[l0][0])) == (140, 140)


@pytest.mark.parametrize("name", sorted(df.FRAMES))
def test_oracle_and_numpy_restatement_agree_on_the_frame(oracle, name):
    """ic_angle, the 7x7 blur (both tap variants) and the steered rBRIEF (both trigonometry variants; tests/nversion_numpy.py takes the libm
    variant as numpy's float32 cos / sin) at the oracle's keypoint positions on the oracle's pyramid levels: angles equal by bit pattern,
    blurred levels and descriptors byte for byte. Every keypoint of every level lies at least 22 px from the level's border."""
    img, p = df.FRAMES[name]()
    pat = oracle.orb_pattern()
    n_checked = 0
    for taps in (0, 1):
        for trig in (0, 1):
            ox, kps, desc, counts = df.run_oracle(oracle, img, p, blur_taps=taps, trig=trig)
            xs, ys = df.level_positions(oracle, kps, p)
            assert sum(counts) == len(kps) and np.array_equal(np.repeat(np.arange(p["num_levels"]), counts), kps["octave"])   # level-major
            for l in range(p["num_levels"]):
                sel = np.nonzero(kps["octave"] == l)[0]
                if not len(sel):
                    assert ox.level_blurred(l) is None
                    continue
                lvl = ox.level_image(l)
                x, y = xs[sel], ys[sel]
                assert x.min() >= 22 and x.max() <= lvl.shape[1] - 23 and y.min() >= 22 and y.max() <= lvl.shape[0] - 23, (name, l)
                ang = nv.ic_angle(lvl, x, y)
                assert np.array_equal(ang.view(np.uint32), kps["angle"][sel].view(np.uint32)), (name, taps, trig, l)
                blurred = nv.gaussian_blur_7x7(lvl, taps)
                assert np.array_equal(blurred, ox.level_blurred(l)), (name, taps, l)
                got = nv.orb_descriptors(blurred, x, y, ang, pat, trig_variant=trig)
                assert np.array_equal(got, desc[sel]), (name, taps, trig, l, int((got != desc[sel]).any(1).sum()))
                if trig == 1:   # the single-keypoint entry of the oracle under the libm variant, against the numpy form
                    k = sel[0]
                    assert np.array_equal(oracle.orb_descriptor(ox.level_blurred(l), int(x[0]), int(y[0]), float(kps["angle"][k]), trig_variant=1), got[0])
                n_checked += len(sel)
    assert n_checked > 0


def test_variants_change_the_descriptors_of_the_frames_built_for_them(oracle):
    """The tap variant is no no-op on the saturation frames and the trigonometry variant none on the noise frame (the four variant
    combinations of the GPU tests are four different expectations)."""
    for name, kw in (("saturation_dark_dots", dict(blur_taps=1)), ("saturation_bright_dots", dict(blur_taps=1)), ("noise", dict(trig=1)), ("noise", dict(blur_taps=1))):
        img, p = df.FRAMES[name]()
        _, k0, d0, _ = df.run_oracle(oracle, img, p)
        _, k1, d1, _ = df.run_oracle(oracle, img, p, **kw)
        assert np.array_equal(k0.view(np.uint8), k1.view(np.uint8)) and not np.array_equal(d0, d1), (name, kw)
