"""k_describe (openvslam_amd/csrc/orb_describe.hip) blurs the rows of a keypoint's patch IN PLACE: the row-blurred patch is written over
the pixels it was computed from. The failure that can introduce is a blurred word landing on a pixel that has not been read yet. It is
deterministic per keypoint; it depends on the patch's offset in its aligned row segment ((x - 21) & 15: sixteen values, the sub-word shift
among them), on the patch row, on the staging path and on the tap variant, and it shows only where neighbouring pixels differ. So: white-noise
frames (128 x 160, two levels, ~300 keypoints), one per staging path, through the device entry under the four (blur_taps, trig) variants,
level 0 and a pyramid level, and one batch of nine such frames across the padding to sixteen; counts, keypoint records and descriptors are
compared with the CPU oracle bit for bit. The coverage each case claims is asserted from the oracle's output alone, so that no case can
pass by covering nothing. Fixtures and helpers are those of tests/test_gpu_describe.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_frames as df       # noqa: E402
import test_gpu_describe as tgd    # noqa: E402

pytestmark = pytest.mark.gpu

COLS, ROWS = 160, 128
P = df.params(300, 1.2, 2)
# seeds chosen on the CPU (oracle only) among 1 .. 39: the first ones whose keypoints meet _assert_coverage on both levels
SEEDS = {"aligned": 2, "pitch4": 4, "base4": 5}
BATCH_SEEDS = [2, 4, 5, 9, 11, 15, 16, 22, 24]


@pytest.fixture(scope="module")
def hip():
    from openvslam_amd import feature
    return feature


def _key(seed):
    return "noise_%dx%d_%d" % (COLS, ROWS, seed)


def _level_shapes(oracle, img):
    ox = df.run_oracle(oracle, img, P)[0]
    return [ox.level_image(l).shape for l in range(P["num_levels"])]


def _assert_coverage(oracle, key, want):
    """From the oracle's keypoints alone: on each of the two levels every offset of the patch in its 16-byte-aligned segment occurs, and
    keypoints sit on the first and the last row a keypoint can have (their patches hold the level's first / last rows)."""
    img = tgd._image(key)[0]
    kps = want[0]
    xs, ys = df.level_positions(oracle, kps, P)
    shapes = _level_shapes(oracle, img)
    assert shapes[0] == (ROWS, COLS) and len(shapes) == 2
    for level, (lrows, _) in enumerate(shapes):
        sel = kps["octave"] == level
        residues = np.bincount((xs[sel] - 21) & 15, minlength=16)
        assert (residues > 0).all(), (key, level, residues.tolist())
        assert (ys[sel] == 22).any() and (ys[sel] == lrows - 23).any(), (key, level, int(ys[sel].min()), int(ys[sel].max()), lrows)


@pytest.mark.parametrize("taps,trig", tgd.VARIANTS)
@pytest.mark.parametrize("arrangement", ["aligned", "pitch4", "base4"])
def test_noise_frame_on_each_staging_path(hip, oracle, arrangement, taps, trig):
    """Level 0 staged by the 16-byte loads ("aligned") or by the 4-byte fallback, reached through the pitch alone ("pitch4") or the base
    alone ("base4"); level 1 of the same frame is the pyramid level (the library's own plane). Two frames per call: the frame and its 180
    degree turn."""
    keys = [_key(SEEDS[arrangement]), _key(SEEDS[arrangement]) + "/rot180"]
    want = [tgd._expect(oracle, k, taps, trig, P) for k in keys]
    _assert_coverage(oracle, keys[0], want[0])
    imgs = np.stack([tgd._image(k)[0] for k in keys])
    d_img, _keep = tgd._device_images(imgs, arrangement)
    ex = tgd._extractor(hip, ROWS, COLS, P, taps, trig)
    cnt, kps, desc = tgd._run_dev(ex, d_img, ex.max_keypoints)
    for b, k in enumerate(keys):
        assert min(want[b][2]) > 100, want[b][2]
        tgd._check_frame(cnt, kps, desc, b, want[b])
        assert np.array_equal(ex.debug_level_counts(b), want[b][2]), (k, taps, trig)


def test_nine_noise_frames_across_the_padding_to_sixteen(hip, oracle):
    """launch_describe pads nine frames to sixteen ((batch + 7) & ~7): frame 8 is alone in the second group of eight. Every frame is a
    different noise frame that meets the coverage conditions; rows at and beyond a frame's count and the bytes behind the last frame's
    block keep their fill (asserted in _run_dev)."""
    keys = [_key(s) for s in BATCH_SEEDS]
    assert len(keys) == 9 == tgd.MAX_BATCH
    imgs = np.stack([tgd._image(k)[0] for k in keys])
    d_img, _keep = tgd._device_images(imgs, "aligned")
    for taps, trig in ((0, 0), (1, 1)):
        want = [tgd._expect(oracle, k, taps, trig, P) for k in keys]
        for k, w in zip(keys, want):
            _assert_coverage(oracle, k, w)
        ex = tgd._extractor(hip, ROWS, COLS, P, taps, trig)
        cnt, kps, desc = tgd._run_dev(ex, d_img, ex.max_keypoints)
        for b, k in enumerate(keys):
            tgd._check_frame(cnt, kps, desc, b, want[b])
            assert np.array_equal(ex.debug_level_counts(b), want[b][2]), (k, taps, trig)
