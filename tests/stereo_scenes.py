"""Constructed scenes for match::stereo::compute (ORACLE_SPEC rule 20): every decision edge of the rule reached ON PURPOSE. Pure numpy, no GPU,
no oracle: images are 240 x 400 (the smallest size the suite extracts on the device), keypoints and descriptors are placed by hand -- the host
entry uploads whatever it is given, and pyramid level 0 is the input image, so an octave-0 keypoint has full control over its two windows.

A scene is (left, right, kps_left, desc_left, kps_right, desc_right, focal_x_baseline, true_baseline, orb_params) plus a name, the probes (label ->
left keypoint, the outcome it was built for and the trace fields that pin the edge) and free-form notes. tests/test_stereo_scenes.py asserts from the
trace of tests/nversion_numpy.py::stereo_compute that every probe still reaches its edge (a scene that stops doing so fails there, not silently)
and that the C oracle agrees with the numpy restatement; tests/test_gpu_stereo.py then holds the HIP path to the oracle on the same inputs.

Descriptors are random 256-bit strings: two unrelated ones are >= 75 bits apart (6.6 sigma below the mean of 128), so probes that share image rows do
not see each other; a probe's right candidates are copies of its left descriptor with an exact number of bits flipped.

Two kinds of images:
  textured  a smooth random texture; right = left moved by an integer disparity (6 px; four row bands of the `edges` scene use 13, 14, 2 and -2), so a
            right keypoint at x_l - disparity aligns the two windows at shift 0 on every pyramid level.
  painted   flat 100 with one 24 x 40 tile per probe. The left window is flat (all zeros once its centre is subtracted), the right strip is flat
            except for bright pixels off the centre row: a pixel of height h in strip column c adds h to the cost of every shift k with
            k <= c <= k + 10, so cost[k+1] - cost[k] = h[k+11] - h[k] and ANY cost profile with cost[0] >= its total descent can be painted exactly.

Unreachable, and therefore not in any scene:
  * |delta| > 1. The chosen shift k is the FIRST minimum, so a = c1 - c2 > 0 and b = c3 - c2 >= 0, and delta = (a - b) / (2 (a + b)) lies in [-0.5, 0.5].
  * the LEFT side of the left window (cx_l - 5 < 0, or == 0 accepted). The gate x_r <= x_l and the monotone rounding give cx_r <= cx_l, so
    cx_l - 5 <= 0 implies cx_r - 10 < 0 and the right-window rule, which is tested first, has already rejected the keypoint.
"""
from typing import NamedTuple

import numpy as np

import nversion_numpy as nv

ROWS, COLS = 240, 400
F = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
ORB_PARAMS = dict(max_num_keypts=500, scale_factor=1.2, num_levels=8)
KITTI = (386.1448, 0.5372)          # max_disp = 718.8 px: wider than the image
VARIANTS = ((False, False), (True, False), (False, True), (True, True))     # (outlier factor 2.1, parabola in double)
SCENE_NAMES = ("edges", "dense", "wide", "shift", "count0", "count1", "count2", "five", "six", "median_zero", "all_equal", "straddle", "big")
HIGH_OCTAVES = (1, 3)               # the two higher octaves of the window probes (7 * 1.2^3 = 12.1 px still fits the `edges` disparity gate)


class Scene(NamedTuple):
    left: np.ndarray
    right: np.ndarray
    kps_left: np.ndarray
    desc_left: np.ndarray
    kps_right: np.ndarray
    desc_right: np.ndarray
    focal_x_baseline: float
    true_baseline: float
    orb_params: dict
    name: str
    probes: dict        # label -> (left keypoint, ST_* code under the default variant or None, {trace field: value})
    notes: dict


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kl, self.dl, self.kr, self.dr, self.probes = [], [], [], [], {}

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flipped(self, d, nbits):
        bits = np.unpackbits(d)
        bits[self.rng.choice(256, nbits, replace=False)] ^= 1
        return np.packbits(bits)

    def left(self, x, y, octave=0, desc=None, label=None, code=None, **checks):
        self.kl.append((x, y, octave))
        self.dl.append(self.desc() if desc is None else desc)
        if label is not None:
            assert label not in self.probes, label
            self.probes[label] = (len(self.kl) - 1, code, checks)
        return len(self.kl) - 1

    def right(self, x, y, octave=0, desc=None):
        self.kr.append((x, y, octave))
        self.dr.append(self.desc() if desc is None else desc)
        return len(self.kr) - 1

    def pair(self, xl, yl, xr, yr=None, octl=0, octr=None, hamming=0, label=None, code=None, **checks):
        d = self.desc()
        il = self.left(xl, yl, octl, d, label, code, **checks)
        ir = self.right(xr, yl if yr is None else yr, octl if octr is None else octr, self.flipped(d, hamming))
        return il, ir

    def scene(self, name, left, right, fxb_b, **notes):
        def kps(rows):
            k = np.zeros(len(rows), KP_DTYPE)
            if rows:
                a = np.array(rows, np.float64)
                k["x"], k["y"], k["octave"] = a[:, 0].astype(F), a[:, 1].astype(F), a[:, 2].astype(np.int32)
            k["size"], k["angle"], k["class_id"] = 31.0, 0.0, -1
            return k
        return Scene(left, right, kps(self.kl), np.array(self.dl, np.uint8).reshape(-1, 32), kps(self.kr), np.array(self.dr, np.uint8).reshape(-1, 32),
                     fxb_b[0], fxb_b[1], dict(ORB_PARAMS), name, self.probes, notes)


def _texture(seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (ROWS, COLS)).astype(np.float64)
    for _ in range(2):     # two 3 x 3 box filters (wrapping): a correlation length of about 3 px, so a misaligned window costs far more than an aligned one
        a = sum(np.roll(np.roll(a, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    a = (a - a.min()) / (a.max() - a.min())
    return np.rint(20.0 + 215.0 * a).astype(np.uint8)


def _moved(left, disparity):
    """right[y, x] = left[y, x + disparity] (wrapping): what the left image shows at x_l, the right one shows at x_l - disparity."""
    return np.roll(left, -disparity, axis=1)


def _coord(target, level, sf, isf):
    """A level-0 coordinate whose rule-20 scaling rint(x * inv_scale[level]) is exactly `target`."""
    x = F(F(target) * sf[level])
    assert int(np.rint(x * isf[level])) == target, (target, level)
    return float(x)


# ---- textured scenes ---------------------------------------------------------------------------------------------------------------------------
EDGE_BANDS = ((120, 140, 13), (140, 160, 14), (160, 180, 2), (180, 200, -2))     # (first row, end row, disparity); 6 everywhere else
EDGE_MAX_DISP = 13.5


def _edges(sf, isf, level_rows, level_cols):
    """Row bands, gates, Hamming, rounding, the window rules on three octaves and the disparity range, on one textured pair. max_disp = 13.5 px."""
    b = _Builder(101)
    left = _texture(1)
    right = _moved(left, 6)
    for r0, r1, d in EDGE_BANDS:
        right[r0:r1] = _moved(left, d)[r0:r1]
    noise = np.random.default_rng(2).integers(-2, 3, right.shape)     # accepted L1 distances of a few hundred, not 0: the median rule keeps the probes
    right = np.clip(right.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    A, OUT = nv.ST_ACCEPTED, None
    # -- row bands (rows 20 .. 40 hold no other right keypoint)
    d = b.desc()
    b.right(244.0, 30.0, 0, d)                                            # band [28, 32]: y -+ 2 * scale is an exact integer at both ends
    b.left(250.0, 32.9, 0, d, "band_last_row", A)                         # row 32
    b.left(250.0, 33.0, 0, d, "band_below", nv.ST_NO_ROW_CANDIDATES)      # row 33: a left row without candidates
    b.left(250.0, 28.0, 0, d, "band_first_row", A)
    b.left(250.0, 27.99, 0, d, "band_above", nv.ST_NO_ROW_CANDIDATES)
    b.pair(250.0, -0.5, 244.0, 1.0, label="y_in_minus1_0", code=nv.ST_LEFT_WINDOW_OUT, cy_l=0)      # (int)y truncates to row 0; right band clipped at row 0
    b.pair(250.0, 239.2, 244.0, 238.5, label="y_last_row", code=nv.ST_LEFT_WINDOW_OUT, cy_l=239)    # right band clipped at row rows - 1
    b.pair(250.0, 240.0, 244.0, 238.5, label="y_ge_rows", code=nv.ST_NO_ROW_CANDIDATES)
    # -- octave gate: right octave l - 2 .. l + 2 for l = 3 and l = 0
    for l, y in ((3, 75.0), (0, 82.0)):
        for dl in (-2, -1, 0, 1, 2):
            if l + dl >= 0:
                b.pair(150.0 + 20 * dl, y, 144.0 + 20 * dl, octl=l, octr=l + dl, label=f"octave_{l}_{dl:+d}", code=A if abs(dl) <= 1 else nv.ST_NO_GATED_CANDIDATE)
    # -- disparity gate: x_r == x_l and x_r == x_l - max_disp exactly, and one ulp outside each (bands with disparity 2 and 13)
    b.pair(150.0, 170.0, 150.0, label="gate_hi_in", code=A)
    b.pair(180.0, 170.0, float(np.nextafter(F(180.0), F(np.inf))), label="gate_hi_out", code=nv.ST_NO_GATED_CANDIDATE)
    b.pair(150.0, 130.0, 136.5, label="gate_lo_in", code=A, half=True)
    b.pair(180.0, 130.0, float(np.nextafter(F(166.5), F(-np.inf))), label="gate_lo_out", code=nv.ST_NO_GATED_CANDIDATE)
    b.pair(-1.0, 90.0, -5.0, label="x_left_negative", code=nv.ST_X_LEFT_NEGATIVE)
    b.pair(-0.0, 90.0, 0.0, label="x_left_minus_zero", code=nv.ST_RIGHT_WINDOW_OUT)     # -0.0 < 0 is false: the keypoint goes on
    # -- Hamming: best distance 0, 74 (accepted) and 75 (rejected)
    for h, code in ((0, A), (74, A), (75, nv.ST_HAMMING)):
        b.pair(100.0 + h, 90.0, 94.0 + h, hamming=h, label=f"hamming_{h}", code=code, best_hamming=h)
    # -- Hamming ties among 40 candidates of one row: the lowest index wins. Only that one aligns (x_l - 6); the others sit at x_l, out of the search's reach.
    for label, y, good_first in (("tie_first_good", 100.0, True), ("tie_first_bad", 106.0, False)):
        d = b.desc()
        first = len(b.kr)
        b.left(200.0, y, 0, d, label, A if good_first else OUT, best_right=first, best_hamming=10, hamming_ties=40)
        for j in range(40):
            b.right(194.0 if (j == 0) == good_first else 200.0 - 0.01 * j, y, 0, b.flipped(d, 10))
    # -- rounding: scaled x_l, y_l, x_r that are exact .5, with an even and with an odd lower neighbour (round half to even goes down, then up)
    b.pair(100.5, 50.5, 94.5, label="half_even", code=A, half=True, cx_l=100, cy_l=50, cx_r=94)
    b.pair(141.5, 51.5, 135.5, label="half_odd", code=A, half=True, cx_l=142, cy_l=52, cx_r=136)
    # -- windows, on octave 0 and two higher ones, placed from the level sizes
    for l in (0,) + HIGH_OCTAVES:
        lr, lc = int(level_rows[l]), int(level_cols[l])
        c = lambda t: _coord(t, l, sf, isf)
        for name, cxr, code in (("right_win_lo_in", 10, A), ("right_win_lo_out", 9, nv.ST_RIGHT_WINDOW_OUT), ("right_win_hi_in", lc - 12, A),
                                ("right_win_hi_out", lc - 11, nv.ST_RIGHT_WINDOW_OUT)):
            b.pair(c(cxr) + 6.0, 60.0 + l, c(cxr), octl=l, label=f"{name}_{l}", code=code, cx_r=cxr)
        for name, cyl, code in (("left_win_top_in", 5, A), ("left_win_top_out", 4, nv.ST_LEFT_WINDOW_OUT), ("left_win_bottom_in", lr - 6, A),
                                ("left_win_bottom_out", lr - 5, nv.ST_LEFT_WINDOW_OUT)):
            b.pair(300.0, c(cyl), 294.0, octl=l, label=f"{name}_{l}", code=code, cy_l=cyl)
        for name, cxl, code in (("left_win_right_in", lc - 6, A), ("left_win_right_out", lc - 5, nv.ST_LEFT_WINDOW_OUT)):
            b.pair(c(cxl), 66.0 + l, c(lc - 12), octl=l, label=f"{name}_{l}", code=code, cx_l=cxl, cx_r=lc - 12)
    # -- disparity range
    b.pair(230.0, 130.0, 217.0, label="disp_under_max", code=A)                          # band 13: 13 - |delta| .. 13 + |delta|, max_disp 13.5
    b.pair(230.0, 150.0, 216.5, label="disp_ge_max", code=nv.ST_DISP_MAX, half=True)       # band 14, the candidate exactly on the gate
    b.pair(230.0, 190.0, 230.0, label="disp_negative", code=nv.ST_DISP_NEGATIVE)           # band -2
    # -- filler: plain octave-3 matches. A level that is not the image itself sees the 6 px as 3.47 of its own, so its accepted distances are around 1000
    #    against 200 on octave 0: with the median among them, the rule keeps every probe above
    for j in range(41):
        b.pair(40.0 + 8 * j, 50.0, 34.0 + 8 * j, octl=3)
    return b.scene("edges", left, right, (EDGE_MAX_DISP, 1.0))


def _dense():
    """More than 2048 accepted matches on octaves 0 .. 2 (the 1024-stride loops wrap twice); the right image's noise grows with the column, so the
    accepted distances spread widely and both outlier factors drop a different set."""
    b = _Builder(202)
    rng = np.random.default_rng(3)
    left = _texture(4)
    amp = np.linspace(0.0, 12.0, COLS)[None, :]
    right = np.clip(np.rint(_moved(left, 6) + rng.uniform(-1.0, 1.0, left.shape) * amp), 0, 255).astype(np.uint8)
    i = 0
    for y in range(10, 231, 7):
        for x in range(24, 387, 5):
            fx, fy = rng.uniform(0, 1, 2)
            b.pair(x + fx, y + fy, x + fx - 6.0, octl=i % 3)
            i += 1
    return b.scene("dense", left, right, KITTI, factor_matters=True, min_accepted=2049)


def _wide():
    """n_right = 65535 (the ABI's limit: the winner's index is packed into 16 bits), winners at 255, 256 and 65534, the first two by a tie
    against a HIGHER index that differs only above bit 7 / bit 8."""
    b = _Builder(303)
    rng = np.random.default_rng(5)
    left = _texture(1)
    right = _moved(left, 6)
    n = 65535
    kr = np.zeros(n, KP_DTYPE)
    kr["x"], kr["y"] = rng.uniform(0, COLS, n).astype(F), rng.uniform(0, ROWS, n).astype(F)
    kr["size"], kr["class_id"] = 31.0, -1
    dr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for label, y, win, lose in (("win_255", 60.0, 255, 511), ("win_256", 120.0, 256, 65534 - 256), ("win_65534", 180.0, 65534, None)):
        d = b.desc()
        b.left(200.0, y, 0, d, label, nv.ST_ACCEPTED, best_right=win, hamming_ties=1 if lose is None else 2)
        for idx, x in ((win, 194.0), (lose, 200.0)):
            if idx is not None:
                kr[idx]["x"], kr[idx]["y"] = x, y
                dr[idx] = b.flipped(d, 5)
    for j in range(5):      # a few plain rows, unmatched
        b.left(50.0 + 60 * j, 30.0 + 40 * j)
    s = b.scene("wide", left, right, KITTI, max_keypoints=65535)
    return s._replace(kps_right=kr, desc_right=dr)


# ---- painted scenes ----------------------------------------------------------------------------------------------------------------------------
_BUMP_ROWS = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)      # never the centre row: the centre value of every right window stays 100


def strip_for_costs(costs):
    """The 11 x 21 right strip whose 11 window costs against a flat left window are exactly `costs`."""
    c = [int(v) for v in costs]
    h = np.zeros(21, np.int64)
    for k in range(10):
        if c[k + 1] > c[k]:
            h[k + 11] = c[k + 1] - c[k]
        else:
            h[k] = c[k] - c[k + 1]
    h[10] = c[0] - h[:10].sum()
    assert h[10] >= 0, "cost[0] must be at least the profile's total descent"
    strip = np.full((11, 21), 100, np.int64)
    for col in range(21):
        rest = int(h[col])
        for r in _BUMP_ROWS:
            t = min(rest, 155)
            strip[r, col] += t
            rest -= t
        assert rest == 0
    return strip.astype(np.uint8)


def vee(minimum):
    """A strict minimum at shift index 5 with equal neighbours: delta = 0."""
    return [minimum + 1100 * abs(k - 5) for k in range(11)]


def big_distance_tile(rest):
    """Left: 255 with centre 0. Right: the centre row 255 under all eleven shifts, the rest of the best window `rest`, 0 outside it.
    cost[5] = 110 * (510 - rest) + 2550 (33350 for 230): a strict interior minimum >= 2^15."""
    win = np.full((11, 11), 255, np.uint8)
    win[5, 5] = 0
    strip = np.zeros((11, 21), np.uint8)
    strip[:, 5:16] = rest
    strip[5, 5:16] = 255
    return win, strip, 110 * (510 - rest) + 2550


def _painted(name, tiles, **notes):
    """tiles: (label, left window or None (flat), right strip, disparity of the right keypoint (0 or 8), code, checks)."""
    b = _Builder(404 + len(tiles))
    left = np.full((ROWS, COLS), 100, np.uint8)
    right = left.copy()
    assert len(tiles) <= 100
    for t, (label, win, strip, dx, code, checks) in enumerate(tiles):
        ty, tx = divmod(t, 10)
        cx, cy = tx * 40 + 25, ty * 24 + 12
        if win is not None:
            left[cy - 5:cy + 6, cx - 5:cx + 6] = win
        right[cy - 5:cy + 6, cx - dx - 10:cx - dx + 11] = strip
        b.pair(float(cx), float(cy), float(cx - dx), label=label, code=code, **checks)
    return b.scene(name, left, right, KITTI, **notes)


def _tile(label, costs, code, dx=8, **checks):
    return (label, None, strip_for_costs(costs), dx, code, dict(costs=[float(v) for v in costs], **checks))


def _distance_scene(name, kept, dropped, **notes):
    """One vee tile per wanted L1 distance; `kept` / `dropped` is the median rule's verdict under the default factor 2.0."""
    tiles = [_tile(f"d{v}_{j}", vee(v), nv.ST_ACCEPTED, shift=5) for j, v in enumerate(kept)]
    tiles += [_tile(f"d{v}_{j}x", vee(v), nv.ST_DROPPED, shift=5) for j, v in enumerate(dropped)]
    return _painted(name, tiles, distances=sorted(kept + dropped), **notes)


_UP = [50, 600, 1100, 1600, 2100, 2600, 3100, 3600, 4100, 4600, 5100]


def _shift():
    A, END = nv.ST_ACCEPTED, nv.ST_END_SHIFT
    up = _UP
    idx1 = [1000] + up[:10]
    tiles = [
        _tile("constant", [0] * 11, END, shift=0),                                                           # all costs 0: index 0 wins, rejected
        _tile("two_minima", [2000, 1500, 1000, 60, 80, 100, 80, 60, 1000, 1500, 2000], A, shift=3),            # equal costs at 3 and 7: the first wins
        _tile("best_1", idx1, A, shift=1),
        _tile("best_9", idx1[::-1], A, shift=9),
        _tile("best_0", up, END, shift=0),
        _tile("best_10", up[::-1], END, shift=10),
        _tile("c3_eq_c2", [3000, 2500, 2000, 1500, 1000, 60, 60, 900, 1500, 2000, 2500], A, shift=5, delta=0.5),
        _tile("zero_minimum", vee(0), A, shift=5, delta=0.0, disp=8.0),
        _tile("disp_zero", vee(0), A, dx=0, shift=5, delta=0.0, disp=0.0, clamped=True),                     # both outputs rewritten by the 0.01 clamp
        _tile("disp_zero_30", vee(30), A, dx=0, shift=5, delta=0.0, disp=0.0, clamped=True),
    ]
    return _painted("shift", tiles)     # accepted distances 0 0 30 50 50 60 60: median 50, everything kept


def _big():
    tiles = []
    for j, rest in enumerate((230, 229, 228, 227, 226)):
        win, strip, cost = big_distance_tile(rest)
        tiles.append((f"big_{j}", win, strip, 8, nv.ST_ACCEPTED, dict(shift=5, delta=0.0)))
    tiles.append(_tile("small", vee(300), nv.ST_ACCEPTED, shift=5))
    return _painted("big", tiles, distances=[300] + [110 * (510 - r) + 2550 for r in (230, 229, 228, 227, 226)])


def build_scenes(scale_factors, inv_scale_factors, level_rows, level_cols):
    """All scenes, in a fixed order. The tables are those of ORB_PARAMS on a 240 x 400 image (the oracle's orb_tables / pyramid_sizes)."""
    sf, isf = np.asarray(scale_factors, F), np.asarray(inv_scale_factors, F)
    return [
        _edges(sf, isf, level_rows, level_cols),
        _dense(),
        _wide(),
        _shift(),
        _painted("count0", [_tile("constant", [0] * 11, nv.ST_END_SHIFT, shift=0), _tile("best_10", _UP[::-1], nv.ST_END_SHIFT, shift=10)], count=0),
        _distance_scene("count1", [70], [], count=1),
        _distance_scene("count2", [10, 40], [], count=2),
        _distance_scene("five", [10, 20, 20, 40], [41], count=5, factor_matters=True),               # median 20: 40 is kept (strict test), 41 dropped
        _distance_scene("six", [10, 20, 20, 30, 60], [61], count=6, factor_matters=True),            # even count: the median is element 3 (30)
        _distance_scene("median_zero", [0, 0, 0], [5, 7], count=5),                                   # median 0: every non-zero distance is dropped
        _distance_scene("all_equal", [30, 30, 30, 30], [], count=4),
        _distance_scene("straddle", [200, 255, 256, 257, 258, 514], [515], count=7),                  # median 257: second element of high byte 1
        _big(),
    ]


_cache = {}


def scenes_from(oracle):
    """build_scenes on the oracle binding's tables, built once per process and shared (read-only) by every test."""
    if "scenes" not in _cache:
        p = oracle.make_params(**ORB_PARAMS)
        tabs = oracle.orb_tables(p)
        lr, lc = oracle.pyramid_sizes(p, ROWS, COLS)
        _cache["scenes"] = build_scenes(tabs["scale_factors"], tabs["inv_scale_factors"], lr, lc)
    return _cache["scenes"]
