"""k_fast_cells' per-group and per-cell set-up against the CPU oracle on the smallest geometries that reach its edges: the work order
(frame and group from the workgroup index by a host-built magic, groups that straddle a level boundary, a last group shorter than the
rest, workgroups beyond the work list), waves that own no testable row of a bottom-clipped cell (and skip the pre-test, in the retry with
min_fast_thr too), the clipped cell's pixel mask, masked cells, and both staging paths.

Geometry: cols = 192 gives three cell columns, the last 20 pixels wide; rows = 108 + ih gives two cell rows, the second with exactly ih
testable rows (cell origin 19 + 64 i, testable rows 22 + 64 i .. min(85 + 64 i, rows - 23)). Wave w of a cell's workgroup pre-tests rows
16 w .. 16 w + 15, so ih in {1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64} puts every wave on both sides of its skip condition.
Per level the candidate list is compared as a set (list order is free), keypoints and descriptors byte for byte."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS, NFEAT = 192, 300
IHS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
INI_THR, MIN_THR = 20, 7
SLIVER_Y0 = 83 + 3   # first testable row of the second cell row (level 0)

_expected = {}


def rows_of(ih):
    return 108 + ih


def corners_image(ih, seed, flat_sliver=False):
    """Noise plus corners: +-60 squares on a jittered 9-pixel lattice over mild noise, and a row of squares whose top edge is the LAST testable
    row, so that even a one-row sliver holds corners. flat_sliver: from row 81 down (everything the second cell row's rings can read) no
    noise and +-12 squares only: FAST responses between min_fast_thr and ini_fast_thr."""
    rows = rows_of(ih)
    rng = np.random.default_rng(1000 * ih + seed)
    img = 110 + rng.integers(-3, 4, size=(rows, COLS))
    if flat_sliver:
        img[81:] = 110
    last = rows - 23   # last testable row
    spots = [(y + int(rng.integers(0, 4)), x + int(rng.integers(0, 4))) for y in range(4, rows - 6, 9) for x in range(4, COLS - 6, 9)]
    spots += [(last, x) for x in range(24, COLS - 24, 11)]
    for i, (y, x) in enumerate(spots):
        amp = 60 if not (flat_sliver and y + 4 > 81) else 12
        if flat_sliver and y < 81 < y + 4:
            continue   # no square across the border between the two regimes
        img[y:y + 4, x:x + 4] = 110 + (amp if i % 2 == 0 else -amp)
    return np.clip(img, 0, 255).astype(np.uint8)


def corner_mask(ih):
    """removes the top-left corner cell at every level (its corner at the level's (19, 19) is masked) and a strip of keypoints elsewhere"""
    m = np.full((rows_of(ih), COLS), 255, np.uint8)
    m[:40, :40] = 0
    m[60:70, 100:140] = 0
    return m


def expected(oracle, ih, levels, seed, kind):
    """(image, mask or None, oracle keypoints, descriptors, per-level candidate arrays), computed once per case"""
    key = (ih, levels, seed, kind)
    if key not in _expected:
        img = corners_image(ih, seed, flat_sliver=(kind == "flat"))
        mask = corner_mask(ih) if kind == "mask" else None
        ox = oracle.OrbExtractor(oracle.make_params(NFEAT, 1.2, levels, INI_THR, MIN_THR))
        wk, wd = ox.extract(img, mask) if mask is not None else ox.extract(img)
        cands = [np.stack(ox.level_candidates(l)) for l in range(levels)]
        for c in cands:
            c.setflags(write=False)
        _expected[key] = (img, mask, wk, wd, cands)
    return _expected[key]


def cand_set(c):
    return set(map(tuple, np.asarray(c).T.tolist()))


def device_frames(imgs, arrangement):
    """(B, rows, cols) uint8 view on the device: "aligned" = base and pitch multiples of 16 (the 16-byte staging of level 0), "pitch4" = a pitch
    of 4 mod 16 (the 4-byte staging). The layout is asserted."""
    import torch
    B, rows, cols = imgs.shape
    assert cols % 16 == 0
    full = torch.zeros((B, rows, cols + (4 if arrangement == "pitch4" else 0)), dtype=torch.uint8, device="cuda")
    view = full[:, :, :cols]
    view.copy_(torch.from_numpy(imgs).cuda())
    assert (view.data_ptr() % 16, view.stride(1) % 16) == ((0, 4) if arrangement == "pitch4" else (0, 0))
    return view, full


def run_device(feature, imgs, masks, levels, arrangement="aligned"):
    """extract_batch_dev on the frames; per frame (count, keypoint bytes, descriptor bytes, per-level candidate arrays)"""
    import torch
    B, rows, cols = imgs.shape
    ex = feature.orb_extractor(feature.orb_params(NFEAT, 1.2, levels, INI_THR, MIN_THR), max_rows=rows, max_cols=cols, max_batch=B)
    cap = ex.max_keypoints
    d_img, keep = device_frames(imgs, arrangement)
    d_mask, keep_m = device_frames(masks, arrangement) if masks is not None else (None, None)
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ex.extract_batch_dev(d_img, d_kps, d_desc, d_cnt, stream=torch.cuda.current_stream().cuda_stream, d_masks=d_mask)
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    kps = d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    desc = d_desc.cpu().numpy()
    out = []
    for b in range(B):
        assert 0 <= cnt[b] <= cap
        out.append((int(cnt[b]), kps[b, :cnt[b]].copy(), desc[b, :cnt[b]].copy(), [np.stack(ex.debug_candidates(l, frame=b, cap=1 << 15)) for l in range(levels)]))
    return out


def check(got, want, what):
    n, kps, desc, cands = got
    _, _, wk, wd, wc = want
    for l, (g, w) in enumerate(zip(cands, wc)):
        assert g.shape[1] == len(cand_set(g)), "%s: level %d lists a candidate twice" % (what, l)
        assert cand_set(g) == cand_set(w), "%s: level %d candidates (%d against the oracle's %d)" % (what, l, g.shape[1], w.shape[1])
    assert n == len(wk), "%s: %d keypoints against the oracle's %d" % (what, n, len(wk))
    assert np.array_equal(kps.reshape(-1), wk.view(np.uint8).reshape(-1)), "%s: keypoint records" % what
    assert np.array_equal(desc, wd), "%s: descriptors" % what


def assert_not_vacuous(want, ih, what):
    """from the oracle's output alone: the last cell row yields candidates at level 0, and so does a cell above it"""
    c0 = want[4][0]
    ys = c0[1]
    assert int((ys >= SLIVER_Y0).sum()) >= 1 and int(ys.max()) < SLIVER_Y0 + ih, "%s: no candidate in the %d-row sliver" % (what, ih)
    assert int((ys < SLIVER_Y0).sum()) >= 1, "%s: no candidate above the sliver" % what


# ---- no device: the cases mean what they say (the oracle alone)
@pytest.mark.parametrize("ih", IHS)
def test_cases_hold_corners_in_the_sliver_and_above(oracle, ih):
    for levels in (1, 3):
        assert_not_vacuous(expected(oracle, ih, levels, 0, "corners"), ih, "ih %d L %d" % (ih, levels))


def test_flat_sliver_case_is_decided_by_the_retry(oracle):
    for levels in (1, 3):
        want = expected(oracle, 20, levels, 0, "flat")
        assert_not_vacuous(want, 20, "flat")
        xs, ys, sc = want[4][0]
        assert int(sc[ys >= SLIVER_Y0].max()) < INI_THR <= int(sc[ys < SLIVER_Y0].max())   # FAST response = S - 1: below ini_fast_thr means found at min_fast_thr


def test_mask_case_removes_a_corner_cell(oracle):
    want, free = expected(oracle, 17, 3, 0, "mask"), expected(oracle, 17, 3, 0, "corners")
    in_cell = lambda c: int(((c[0] < 22 + 64) & (c[1] < 22 + 64)).sum())
    assert in_cell(free[4][0]) >= 1 and in_cell(want[4][0]) == 0 and want[4][0].shape[1] >= 1


# ---- the device
@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("ih", IHS)
def test_sliver_rows(oracle, ih, levels):
    from openvslam_amd import feature
    want = expected(oracle, ih, levels, 0, "corners")
    assert_not_vacuous(want, ih, "ih %d" % ih)
    got = run_device(feature, want[0][None], None, levels)
    check(got[0], want, "ih %d, %d levels" % (ih, levels))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [3, 9])
@pytest.mark.parametrize("ih", [1, 17, 48])
def test_sliver_rows_in_a_batch(oracle, ih, batch):
    from openvslam_amd import feature
    wants = [expected(oracle, ih, 3, s, "corners") for s in range(batch)]
    got = run_device(feature, np.stack([w[0] for w in wants]), None, 3)
    for b in range(batch):
        check(got[b], wants[b], "ih %d, frame %d of %d" % (ih, b, batch))


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 3])
def test_flat_sliver_is_retried_with_min_fast_thr(oracle, levels):
    from openvslam_amd import feature
    want = expected(oracle, 20, levels, 0, "flat")   # 20 testable rows: waves 2 and 3 idle, in the retry too
    got = run_device(feature, want[0][None], None, levels)
    check(got[0], want, "flat sliver, %d levels" % levels)


@pytest.mark.gpu
def test_masked_corner_cell(oracle):
    from openvslam_amd import feature
    wants = [expected(oracle, 17, 3, 0, "mask"), expected(oracle, 17, 3, 0, "corners")]
    masks = np.stack([wants[0][1], np.full_like(wants[0][1], 255)])   # the second frame unmasked: the mask is the frame's own
    got = run_device(feature, np.stack([w[0] for w in wants]), masks, 3)
    check(got[0], wants[0], "masked frame")
    check(got[1], wants[1], "unmasked frame beside it")


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement", ["aligned", "pitch4"])
def test_both_staging_paths(oracle, arrangement):
    from openvslam_amd import feature
    wants = [expected(oracle, 17, 3, s, "corners") for s in range(3)]
    got = run_device(feature, np.stack([w[0] for w in wants]), None, 3, arrangement)
    for b in range(3):
        check(got[b], wants[b], "%s, frame %d" % (arrangement, b))


def digest(frames):
    h = hashlib.sha256()
    for n, kps, desc, cands in frames:
        h.update(np.int64(n).tobytes() + np.ascontiguousarray(kps).tobytes() + np.ascontiguousarray(desc).tobytes())
        for c in cands:
            h.update(np.array(sorted(cand_set(c)), np.int64).tobytes())
    return h.hexdigest()


CHILD_CASES = [(17, 3, 1), (17, 3, 3), (48, 3, 9), (2, 1, 3)]   # (ih, levels, batch): 10 cells in three levels (groups of three straddle both level boundaries
#                                                                   and leave a last group of one; 24 workgroups for 4 groups x 3 frames), 6 cells in one


def child_digest():
    """the cases above through the device in THIS process (OVS_FAST_CELLS is read once per process); images regenerated, no oracle"""
    from openvslam_amd import feature
    out = []
    for ih, levels, batch in CHILD_CASES:
        out.append(digest(run_device(feature, np.stack([corners_image(ih, s) for s in range(batch)]), None, levels)))
    return " ".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [None, 1, 2, 3, 64])
def test_cells_per_group(oracle, cells):
    want = []
    for ih, levels, batch in CHILD_CASES:
        ws = [expected(oracle, ih, levels, s, "corners") for s in range(batch)]
        want.append(digest([(len(w[2]), w[2].view(np.uint8).reshape(-1, 28), w[3], w[4]) for w in ws]))
    env = {k: v for k, v in os.environ.items() if k != "OVS_FAST_CELLS"}
    if cells is not None:
        env["OVS_FAST_CELLS"] = str(cells)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_fast_setup as t; print('SHA', t.child_digest())" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("SHA")][-1].split()[1:]
    assert line == want, "OVS_FAST_CELLS=%s" % cells
