"""k_fast_cells' candidate list holds raw (thread << 5) | bit entries between the list loop and the scoring pass, which decodes them into position
and polarity flags with the thread's flag word (csrc/orb_fast.hip). Every case compares the kernel with the CPU oracle: the NMS survivors of
every level, and the keypoint records and descriptors byte for byte. The shapes are the smallest at which the decode can go wrong: one full
64x64 cell with clipped neighbours, every (thread, bit) position in both polarities, both flags, both list paths, the retry and the batch entry."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fast_list_model as model   # noqa: E402

pytestmark = pytest.mark.gpu

BG = 128
X0 = Y0 = 22   # image coordinates of cell (0, 0)'s first testable pixel: cell position (px, py) <-> image (X0 + px, Y0 + py)
RING = model.RING


@pytest.fixture(scope="module")
def hip():
    from openvslam_amd import feature
    return feature


def _check(hip, oracle, imgs, nfeat=500, levels=1, ini=20, mn=7):
    """Every image through the single-frame entry and the oracle: candidates of every level, keypoints and descriptors. Returns the oracle's level-0
    candidates per image as sets of (x, y)."""
    rows, cols = imgs[0].shape
    ex = hip.orb_extractor(hip.orb_params(nfeat, 1.2, levels, ini, mn), max_rows=rows, max_cols=cols)
    ox = oracle.OrbExtractor(oracle.make_params(nfeat, 1.2, levels, ini, mn))
    found = []
    for n, img in enumerate(imgs):
        gk, gd = ex.extract(img)
        wk, wd = ox.extract(img)
        for level in range(levels):
            gx, gy, gs = ex.debug_candidates(level)
            wx, wy, ws = ox.level_candidates(level)
            assert len(gx) == len(wx), "image %d level %d: %d candidates, oracle %d" % (n, level, len(gx), len(wx))
            assert np.array_equal(gx, wx) and np.array_equal(gy, wy) and np.array_equal(gs, ws), "image %d level %d candidates" % (n, level)
        assert len(gk) == len(wk) and np.array_equal(gk.view(np.uint8), wk.view(np.uint8)) and np.array_equal(gd, wd), "image %d" % n
        wx, wy, _ = ox.level_candidates(0)
        found.append(set(zip(np.asarray(wx).tolist(), np.asarray(wy).tolist())))
    return found


def _testable(rows, cols, x, y):
    return X0 <= x < cols - X0 and Y0 <= y < rows - Y0


def _dots(rows, cols, ox, oy, delta):
    """Flat background with single-pixel dots 8 px apart over the WHOLE image (also outside the testable area and in the clipped cells);
    delta: a number, or a function of the dot's grid index (i, j)."""
    img = np.full((rows, cols), BG, np.uint8)
    want = set()
    for j, y in enumerate(range(oy, rows, 8)):
        for i, x in enumerate(range(ox, cols, 8)):
            img[y, x] = BG + (delta(i, j) if callable(delta) else delta)
            if _testable(rows, cols, x, y):
                want.add((x, y))
    return img, want


@pytest.mark.parametrize("delta", [60, -60])
def test_every_thread_and_bit_position_once_per_polarity(hip, oracle, delta):
    """110 x 110: one full cell, clipped neighbours to the right and below. The dot grid steps through all 64 offsets, so every one of the full
    cell's 4096 positions -- every bit of every thread's mask -- holds the only candidate of its neighbourhood once. A bright dot is a corner of
    the dark polarity (its ring is darker) and a dark dot one of the bright polarity: `dark only` and `bright only` at every position. An isolated
    dot is the only corner around it (a pixel with the dot on its ring has one differing ring pixel), which the oracle confirms."""
    imgs, wants = [], []
    for off in range(64):
        img, want = _dots(110, 110, (X0 + off % 8) % 8, (Y0 + off // 8) % 8, delta)
        imgs.append(img)
        wants.append(want)
    seen = set()
    for want, got in zip(wants, _check(hip, oracle, imgs)):
        assert got == want   # the oracle finds exactly the dots
        seen |= {(x - X0, y - Y0) for x, y in got if x < X0 + 64 and y < Y0 + 64}
    assert len(seen) == 4096


def _arc_patch(img, cx, cy, start, inner, outer):
    """Centre BG; nine contiguous ring pixels from `start` at `inner`, the other seven at `outer`."""
    img[cy - 3:cy + 4, cx - 3:cx + 4] = BG
    for k, (dx, dy) in enumerate(RING):
        img[cy + dy, cx + dx] = inner if (k - start) % 16 < 9 else outer


# cell positions of the patches' centres: thread blocks (run 0, row pair 1), (run 7, row pair 31: the last of both), (run 7, row pair 15),
# (run 3, row pair 31); every arc start moves them by (start % 8, start % 2) inside the block, so all 16 bits of a block are used
BLOCKS = [(0, 2), (56, 62), (56, 30), (24, 62)]


def test_both_tests_passed_flag(hip, oracle):
    """Nine ring pixels at 50 and seven at 200 around a centre of 128 (and the mirror image): the corner exists in ONE polarity (the other arc is
    two short), but for an odd arc start every even diameter has a bright AND a dark end, so both pre-tests pass and the entry carries the `both`
    flag; for an even start the diameter through the start has two ends inside the arc and the entry is single-polarity. A decode that drops the flag
    or swaps it with `dark only` scores the wrong polarity and loses the corner. All 16 starts, both mirror images, four thread blocks."""
    imgs, centres = [], []
    both = 0
    for inner, outer in ((50, 200), (200, 50)):
        for start in range(16):
            img = np.full((110, 110), BG, np.uint8)
            pts = [(bx + start % 8, by + start % 2) for bx, by in BLOCKS]
            for px, py in pts:
                _arc_patch(img, X0 + px, Y0 + py, start, inner, outer)
            b, d = model.cell_masks(img, 20)[0]
            for px, py in pts:
                assert b[py, px] or d[py, px]
                both += bool(b[py, px] and d[py, px])
            imgs.append(img)
            centres.append({(X0 + px, Y0 + py) for px, py in pts})
    assert both == 2 * 8 * len(BLOCKS)   # every odd start, in both mirror images and all blocks
    for want, got in zip(centres, _check(hip, oracle, imgs)):
        assert want <= got   # the centres are corners and survive the NMS: losing one shows in the comparison above


# white noise of amplitude +-AMP around 128, threshold 20: AMP rises from cell to cell so that the pre-test lets through less than the list
# holds in the left cells and more in the right ones (the model's counts are asserted below)
CAP_AMPS = (36, 45, 52, 64, 80)


def test_list_capacity_sparse_and_exhaustive_cells_in_one_group(hip, oracle):
    """Five full cells in a row (one workgroup's group) with uniform noise in [128 - a, 128 + a], a = 36, 45, 52, 64, 80 from left to right
    at ini_fast_thr = 20, min_fast_thr = 7: by the numpy pre-test model at least one cell holds between 1536 and 2048 candidates (the list at
    three quarters or more: all of clist's range is decoded) and at least one more than 2048 (no list, exhaustive scoring)."""
    rng = np.random.default_rng(17)
    rows, cols = 110, 2 * X0 + 64 * len(CAP_AMPS) + 2
    img = np.full((rows, cols), BG, np.uint8)
    for k, a in enumerate(CAP_AMPS):
        x = X0 - 3 + 64 * k if k else 0
        x1 = X0 - 3 + 64 * (k + 1) if k + 1 < len(CAP_AMPS) else cols
        img[:, x:x1] = BG + rng.integers(-a, a + 1, (rows, x1 - x))
    counts = [int((b | d).sum()) for b, d in model.cell_masks(img, 20)]
    print("pre-test candidates per cell:", counts)
    assert any(1536 <= c <= model.LIST_CAP for c in counts[:len(CAP_AMPS)]) and any(c > model.LIST_CAP for c in counts[:len(CAP_AMPS)])
    got = _check(hip, oracle, [img], nfeat=1500, levels=2)
    assert len(got[0]) > 500


def test_retry_with_min_fast_thr_uses_the_retry_flags(hip, oracle):
    """Cell (0, 0) is flat but for dots of +-12 (both polarities alternating): nothing at threshold 20 -- the first pass finds no candidate and
    leaves an all-zero flag word in every thread -- so the cell is run again at threshold 7, where every dot is a candidate. Decoded with the
    first pass's flags, the bright dots (`dark only`) would be scored in the wrong polarity and vanish. Cell (0, 1) holds a +60 dot and +-12
    dots: it has a threshold-20 corner, is not run again, and its weak dots stay undetected."""
    rows, cols = 110, 2 * X0 + 128 + 2
    img, _ = _dots(rows, cols, 3, 5, lambda i, j: 12 if (i + j) % 2 else -12)
    strong = (X0 + 64 + 21, Y0 + 31)
    assert img[strong[1], strong[0]] != BG   # a grid position
    img[strong[1], strong[0]] = BG + 60
    first = model.cell_masks(img, 20)
    assert not (first[0][0] | first[0][1]).any() and (first[1][0] | first[1][1]).sum() == 1
    retry = model.cell_masks(img, 7)[0]
    assert retry[0].sum() >= 16 and retry[1].sum() >= 16
    got = _check(hip, oracle, [img])[0]
    weak0 = {(x, y) for y in range(5, rows, 8) for x in range(3, cols, 8) if _testable(rows, cols, x, y) and x < X0 + 64 and y < Y0 + 64}
    assert {p for p in got if p[0] < X0 + 64 and p[1] < Y0 + 64} == weak0
    assert {p for p in got if X0 + 64 <= p[0] < X0 + 128 and p[1] < Y0 + 64} == {strong}


@pytest.mark.parametrize("rows,cols", [(110, 97), (97, 131)])
def test_clipped_cells(hip, oracle, rows, cols):
    """Last cell column / row with a testable area narrower and lower than 64 (110 x 97: one cell column of width 53; 97 x 131: a second column of
    width 23 and one cell row of height 53). The dot grid covers the whole image: dots in the clipped threads' blocks, on the last testable row and
    column, and just outside them, bright and dark alternating. The oracle finds exactly the dots of the testable area."""
    imgs, wants = [], []
    for off in range(0, 64, 3):
        img, want = _dots(rows, cols, off % 8, off // 8, lambda i, j: 60 if (i + j) % 2 else -60)
        imgs.append(img)
        wants.append(want)
    edge = set()
    for want, got in zip(wants, _check(hip, oracle, imgs)):
        assert got == want
        edge |= {"x" for x, y in got if x == cols - X0 - 1} | {"y" for x, y in got if y == rows - Y0 - 1}
    assert edge == {"x", "y"}   # the last testable column and row held dots


def test_batch_entry_equals_single_frame_extract(hip, oracle):
    """Eight of the small frames above (dots of both polarities, arc patches with the `both` flag, noise) in one extract_batch_dev call, level-0
    split on and off: every frame byte-equal to its own single-frame extract (which the cases above compare with the oracle)."""
    import torch
    rng = np.random.default_rng(5)
    imgs = [_dots(110, 110, 1, 6, 60)[0], _dots(110, 110, 7, 0, -60)[0], _dots(110, 110, 4, 3, lambda i, j: 60 if (i + j) % 2 else -60)[0],
            _dots(110, 110, 2, 2, lambda i, j: 12 if (i + j) % 2 else -12)[0]]
    for inner, outer, start in ((50, 200, 3), (200, 50, 9)):
        img = np.full((110, 110), BG, np.uint8)
        for bx, by in BLOCKS:
            _arc_patch(img, X0 + bx + start % 8, Y0 + by + start % 2, start, inner, outer)
        imgs.append(img)
    imgs.append((BG + rng.integers(-33, 34, (110, 110))).astype(np.uint8))
    imgs.append((BG + rng.integers(-40, 41, (110, 110))).astype(np.uint8))
    imgs = np.stack(imgs)
    B = len(imgs)
    assert B == 8
    one = hip.orb_extractor(hip.orb_params(500, 1.2, 2, 20, 7), max_rows=110, max_cols=110)
    ex = hip.orb_extractor(hip.orb_params(500, 1.2, 2, 20, 7), max_rows=110, max_cols=110, max_batch=B)
    ox = oracle.OrbExtractor(oracle.make_params(500, 1.2, 2, 20, 7))
    want = [one.extract(img) for img in imgs]
    wk, wd = ox.extract(imgs[4])
    assert np.array_equal(want[4][0].view(np.uint8), wk.view(np.uint8)) and np.array_equal(want[4][1], wd)
    cap = ex.max_keypoints
    d_full = torch.zeros((B, 110, 112), dtype=torch.uint8, device="cuda")   # rows at a 4-byte aligned pitch (the ABI's alignment rule)
    d_full[:, :, :110] = torch.from_numpy(imgs).cuda()
    d_img = d_full[:, :, :110]
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((B,), dtype=torch.int32, device="cuda")
    for split in (True, False):
        ex.set_fast_split(split)
        d_cnt.zero_()
        ex.extract_batch_dev(d_img, d_kps, d_desc, d_cnt, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        cnt = d_cnt.cpu().numpy()
        kps = d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
        desc = d_desc.cpu().numpy()
        for b in range(B):
            k, d = want[b]
            assert cnt[b] == len(k) and len(k) > 0, (split, b)
            assert np.array_equal(kps[b, :cnt[b]].reshape(-1), k.view(np.uint8).reshape(-1)) and np.array_equal(desc[b, :cnt[b]], d), (split, b)
