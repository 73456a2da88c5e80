"""Small frames that walk k_describe (openvslam_amd/csrc/orb_describe.hip) through its decision edges, and for each frame a conditions()
function that says -- from the CPU oracle's output and from integer moments / blur sums recomputed in numpy on the oracle's own pyramid
levels, never from the HIP code -- which of those edges the frame reaches:

  orientation   cv::fastAtan2's |m10| == |m01| tie, exactly zero moments with either sign of the other one, m10 == m01 == 0
  border        keypoints at the smallest / largest legal position (22 and size - 23), all sixteen values of (x - 21) & 15
  noise         the same sixteen residues on a pyramid level >= 1 (and a few hundred keypoints on every level for the capacity tests)
  saturation    blurred pixels at 255 under both tap variants, the 257-sum variant's clamp really clamping
  level gaps    level 0 empty, a middle level empty, only level 0 populated

No GPU, no pytest. tests/test_describe_frames.py asserts every condition by name; tests/test_gpu_describe.py runs the frames through the kernel."""
import numpy as np

BG = 30                 # flat background of the orientation frame
CORNER = 230
_UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]   # ic_angle's disc (ORACLE_SPEC rule 9)
_TAPS1 = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)             # rule 10, variant 1: the taps sum to 257


def params(max_num_keypts=500, scale_factor=1.2, num_levels=8, ini_fast_thr=20, min_fast_thr=7):
    return dict(max_num_keypts=max_num_keypts, scale_factor=scale_factor, num_levels=num_levels, ini_fast_thr=ini_fast_thr, min_fast_thr=min_fast_thr)


def oracle_params(oracle, p):
    return oracle.make_params(p["max_num_keypts"], p["scale_factor"], p["num_levels"], p["ini_fast_thr"], p["min_fast_thr"])


# ---- builders --------------------------------------------------------------------------------------------------------------------------
# one structure per grid slot: the corner pixel plus (dx, dy, value - BG) companions
_ORIENT_STRUCTURES = [
    [],                                            # lone pixel: m10 = m01 = 0
    [(8, 0, 100)], [(-8, 0, 100)],                 # m01 = 0, m10 > 0 / < 0 (the companion is a keypoint too, with the opposite sign)
    [(0, 8, 100)], [(0, -8, 100)],                 # m10 = 0, m01 > 0 / < 0
    [(7, 7, 100)], [(-7, 7, 100)], [(-7, -7, 100)], [(7, -7, 100)],                       # |m10| == |m01| in the four quadrants
    [(7, 7, 100), (1, 0, 1)], [(7, 7, 100), (0, 1, 1)],                                   # |m10| = |m01| + 1, |m10| = |m01| - 1
    [(-7, -7, 100), (-1, 0, 1)], [(-7, -7, 100), (0, -1, 1)],                             # the same around 225 degrees
    [(-7, 7, 100), (-1, 0, 1)], [(7, -7, 100), (0, -1, 1)],                               # and in the two other quadrants
    [(8, 0, 100), (0, 1, 1)], [(0, 8, 100), (-1, 0, 1)],                                  # one unit off the axes
    [(5, 9, 100)], [(-9, 5, 100)], [(9, -5, 100)],                                        # ordinary angles
]


def orientation_frame():
    """264 x 200: isolated corner pixels on a flat background (the disc's symmetric sums cancel exactly), each with lone companion pixels
    that set the integer moments; weak noise outside every disc so that the descriptors are not trivial."""
    rows, cols = 200, 264
    img = np.full((rows, cols), BG, np.int32)
    flat = np.zeros((rows, cols), bool)
    slots = [(x, y) for y in (32, 76, 120, 164) for x in (32, 80, 128, 176, 224)]
    assert len(slots) >= len(_ORIENT_STRUCTURES)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for (x, y), comps in zip(slots, _ORIENT_STRUCTURES):
        img[y, x] = CORNER
        flat |= (xx - x) ** 2 + (yy - y) ** 2 <= 17 * 17
        for dx, dy, amp in comps:
            img[y + dy, x + dx] = BG + amp
            if amp > 7:
                flat |= (xx - x - dx) ** 2 + (yy - y - dy) ** 2 <= 17 * 17
    noise = np.random.default_rng(5).integers(0, 6, (rows, cols))     # below min_fast_thr: no corner of its own
    img = np.where(flat, img, img + noise)
    return img.astype(np.uint8), params(500)


def _weak_noise(rows, cols, seed, base=100):
    return (base + np.random.default_rng(seed).integers(0, 6, (rows, cols))).astype(np.uint8)


def border_frame(cols=272, rows=200):
    """Single bright pixels at x in {22, cols - 23} x y in {22, rows - 23} (four corners), at the four edge midpoints, and two rows of
    eight pixels 17 px apart whose (x - 21) & 15 runs through all sixteen values; weak noise everywhere (no corner of its own)."""
    img = _weak_noise(rows, cols, 9)
    xs, ys = (22, cols // 2, cols - 23), (22, rows // 2, rows - 23)
    for y in ys:
        for x in xs:
            if (x, y) != (xs[1], ys[1]):
                img[y, x] = 255
    for k in range(8):
        img[64, 40 + 17 * k] = 255      # (x - 21) & 15 = 3 .. 10
        img[136, 48 + 17 * k] = 255     # 11 .. 15, 0 .. 2
    return img, params(500)


def noise_frame(cols=272, rows=200, seed=17):
    """White noise: a few hundred keypoints spread over every level."""
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8), params(300)


def saturation_frame(inverse=False):
    """255 background with dark dots (inverse: 0 background with bright dots and a few 11 x 11 plateaus of 255, whose blurred centres stay at 255)."""
    rows, cols = 200, 264
    rng = np.random.default_rng(23)
    img = np.full((rows, cols), 255, np.int32)
    for y in range(26, rows - 24, 21):
        for x in range(26, cols - 24, 21):
            px, py = x + int(rng.integers(0, 6)), y + int(rng.integers(0, 6))
            img[py, px] = int(rng.integers(0, 160))
            if rng.random() < 0.5:      # a second, weaker dot nearby: angles that are not all zero
                img[py + int(rng.integers(4, 9)), px + int(rng.integers(-8, 9))] = int(rng.integers(100, 220))
    if inverse:
        img = 255 - img
        for x, y in ((60, 50), (150, 120), (210, 60)):
            img[y:y + 11, x:x + 11] = 255
    return img.astype(np.uint8), params(500)


def _blobs(rows, cols, pitch, sigma, amp, base=90, margin=40):
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = np.full((rows, cols), float(base))
    k = 0
    for cy in range(margin, rows - margin + 1, pitch):
        for cx in range(margin, cols - margin + 1, pitch):
            s, a = sigma + 0.25 * (k % 3), amp + 3 * (k % 4)
            img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
            k += 1
    return img


def level0_empty_frame():
    """(a) smooth blobs on a grid (no overlap): too flat for FAST at level 0, corners from some level >= 1 on."""
    return np.rint(_blobs(300, 400, 56, 6.0, 50)).astype(np.uint8), params(500)


def middle_level_empty_frame():
    """(b) three levels at scale 2.0 (each level the 2 x 2 average of the one below). Weak single pixels (+24) are corners at level 0 and
    fade to +6 at level 1; 4 x 4 blocks on the 4-pixel grid are sixteen equal scores at level 0 and four at level 1 -- the strict
    non-maximum suppression drops them all -- and one pixel, a corner, at level 2. So level 1 stays empty between two populated levels."""
    rows, cols = 480, 640
    img = np.full((rows, cols), 100, np.int32)
    for y in range(30, rows - 24, 150):
        for x in range(30, cols - 24, 75):
            img[y, x] += 24
    k = 0
    for y in range(112, rows - 100, 60):
        for x in range(120, cols - 100, 72):
            img[y:y + 4, x:x + 4] += 60 + 10 * (k % 7)
            k += 1
    return img.astype(np.uint8), params(500, 2.0, 3)


def level0_only_frame():
    """(c) weak single pixels on a flat 264 x 200 frame, two levels at scale 2.0: corners at level 0, nothing above."""
    img = np.full((200, 264), 120, np.uint8)
    for y in range(22, 178, 31):
        for x in range(22, 242, 31):
            img[y, x] = 144
    return img, params(500, 2.0, 2)


FRAMES = {
    "orientation": orientation_frame,
    "border_c0": lambda: border_frame(272),       # cols % 16 == 0
    "border_c4": lambda: border_frame(276),       # cols % 16 == 4
    "noise": noise_frame,
    "saturation_dark_dots": saturation_frame,
    "saturation_bright_dots": lambda: saturation_frame(True),
    "level0_empty": level0_empty_frame,
    "middle_level_empty": middle_level_empty_frame,
    "level0_only": level0_only_frame,
}


# ---- what the oracle says about a frame -----------------------------------------------------------------------------------------------------
def level_positions(oracle, kps, p):
    """Integer positions of the oracle's keypoints on their own pyramid level: rint(x / scale_factors[octave]) in float."""
    sf = oracle.orb_tables(oracle_params(oracle, p))["scale_factors"]
    s = sf[kps["octave"]]
    return np.rint(kps["x"] / s).astype(np.int64), np.rint(kps["y"] / s).astype(np.int64)


def moments(level_img, xs, ys):
    """Integer m10, m01 over ic_angle's disc."""
    I = np.asarray(level_img).astype(np.int64)
    m10, m01 = np.zeros(len(xs), np.int64), np.zeros(len(xs), np.int64)
    for v in range(-15, 16):
        u = np.arange(-_UMAX[abs(v)], _UMAX[abs(v)] + 1)
        row = I[(ys + v)[:, None], xs[:, None] + u[None, :]]
        m10 += (row * u).sum(1)
        m01 += v * row.sum(1)
    return m10, m01


def run_oracle(oracle, img, p, blur_taps=0, trig=0):
    """(extractor, kps, desc, level counts) under one variant setting."""
    ox = oracle.OrbExtractor(oracle_params(oracle, p))
    ox.set_variant("blur_taps", blur_taps)
    ox.set_variant("trig", trig)
    kps, desc = ox.extract(img)
    return ox, kps, desc, [ox.level_num_keypts(l) for l in range(p["num_levels"])]


def _all_moments(oracle, ox, kps, p):
    xs, ys = level_positions(oracle, kps, p)
    m10, m01 = np.zeros(len(kps), np.int64), np.zeros(len(kps), np.int64)
    for l in range(p["num_levels"]):
        sel = kps["octave"] == l
        if sel.any():
            m10[sel], m01[sel] = moments(ox.level_image(l), xs[sel], ys[sel])
    return xs, ys, m10, m01


def orientation_conditions(oracle, img, p):
    ox, kps, _, _ = run_oracle(oracle, img, p)
    _, _, m10, m01 = _all_moments(oracle, ox, kps, p)
    a10, a01 = np.abs(m10), np.abs(m01)
    ang, up = kps["angle"], kps["octave"] >= 1
    c = {"m10_zero_m01_zero": (m10 == 0) & (m01 == 0),
         "m01_zero_m10_pos": (m01 == 0) & (m10 > 0), "m01_zero_m10_neg": (m01 == 0) & (m10 < 0),
         "m10_zero_m01_pos": (m10 == 0) & (m01 > 0), "m10_zero_m01_neg": (m10 == 0) & (m01 < 0),
         "abs_m10_is_abs_m01_plus_1": (a10 == a01 + 1) & (a01 > 0), "abs_m10_is_abs_m01_minus_1": (a10 == a01 - 1) & (a10 > 0)}
    tie = (a10 == a01) & (a10 > 0)
    for name, sx, sy in (("q1", 1, 1), ("q2", -1, 1), ("q3", -1, -1), ("q4", 1, -1)):
        c["tie_" + name] = tie & (np.sign(m10) == sx) & (np.sign(m01) == sy)
    for name, lo in (("q1", 0.0), ("q2", 90.0), ("q3", 180.0), ("q4", 270.0)):
        c["upper_level_angle_" + name] = up & (ang > lo) & (ang < lo + 90.0)
    # the exact angles the axis cases must give, from the oracle's own output
    for name, deg, sel in (("angle_exactly_0", 0.0, (m01 == 0) & (m10 > 0)), ("angle_exactly_90", 90.0, (m10 == 0) & (m01 > 0)),
                           ("angle_exactly_180", 180.0, (m01 == 0) & (m10 < 0)), ("angle_exactly_270", 270.0, (m10 == 0) & (m01 < 0))):
        c[name] = sel & (ang == np.float32(deg))
    return {k: int(v.sum()) for k, v in c.items()}


def border_conditions(oracle, img, p):
    rows, cols = img.shape
    ox, kps, _, _ = run_oracle(oracle, img, p)
    xs, ys = level_positions(oracle, kps, p)
    l0 = kps["octave"] == 0
    x0, y0 = xs[l0], ys[l0]
    c = {}
    for nx, vx in (("left", 22), ("mid", cols // 2), ("right", cols - 23)):
        for ny, vy in (("top", 22), ("mid", rows // 2), ("bottom", rows - 23)):
            if (nx, ny) != ("mid", "mid"):
                c["level0_%s_%s" % (nx, ny)] = int(((x0 == vx) & (y0 == vy)).sum())
    res = np.bincount((x0 - 21) & 15, minlength=16)
    for r in range(16):
        c["level0_residue_%d" % r] = int(res[r])
    c["level0_no_keypoint_outside_22"] = int(((x0 < 22) | (x0 > cols - 23) | (y0 < 22) | (y0 > rows - 23)).sum())   # must be 0
    return c


def noise_conditions(oracle, img, p):
    """upper_level_residues_covered: the largest number of distinct (x_level - 21) & 15 that one level >= 1 holds (16 = all)."""
    ox, kps, _, counts = run_oracle(oracle, img, p)
    xs, _ = level_positions(oracle, kps, p)
    best = 0
    for l in range(1, p["num_levels"]):
        best = max(best, len(set(((xs[kps["octave"] == l] - 21) & 15).tolist())))
    return {"upper_level_residues_covered": best, "keypoints": len(kps), "levels_with_keypoints": int(sum(n > 0 for n in counts))}


def _sampled_mask(shape, xs, ys):
    m = np.zeros(shape, bool)
    for x, y in zip(xs, ys):
        m[max(y - 18, 0):y + 19, max(x - 18, 0):x + 19] = True
    return m


def unclamped_blur_257(level_img):
    """Rule 10 variant 1 without the final clamp to 255 (rows still saturate at 16 bits), BORDER_REFLECT_101."""
    P = np.pad(np.asarray(level_img, np.uint8).astype(np.int64), 3, mode="reflect")
    H, W = np.asarray(level_img).shape
    row = np.minimum(sum(_TAPS1[i] * P[:, i:i + W] for i in range(7)), 0xFFFF)
    col = sum(_TAPS1[i] * row[i:i + H, :] for i in range(7))
    return (col + 32768) >> 16, row[3:3 + H]


def saturation_conditions(oracle, img, p):
    c = {}
    for taps in (0, 1):
        ox, kps, _, _ = run_oracle(oracle, img, p, blur_taps=taps)
        xs, ys = level_positions(oracle, kps, p)
        n255 = n0 = nover = nrow = 0
        for l in range(p["num_levels"]):
            sel = kps["octave"] == l
            if not sel.any():
                continue
            m = _sampled_mask(ox.level_image(l).shape, xs[sel], ys[sel])
            b = ox.level_blurred(l)
            n255 += int((b[m] == 255).sum())
            n0 += int((b[m] == 0).sum())
            if taps == 1:
                raw, row = unclamped_blur_257(ox.level_image(l))
                nover += int((raw[m] > 255).sum())
                nrow += int((row[m] == 65535).sum())
        c["sampled_blurred_255_taps%d" % taps] = n255
        c["sampled_blurred_0_taps%d" % taps] = n0
        if taps == 1:
            c["sampled_unclamped_above_255_taps1"] = nover
            c["sampled_row_sum_65535_taps1"] = nrow
        c["keypoints_taps%d" % taps] = len(kps)
    return c


def level_gap_conditions(oracle, img, p):
    _, kps, _, counts = run_oracle(oracle, img, p)
    nz = [l for l, n in enumerate(counts) if n > 0]
    middle_empty = [l for l, n in enumerate(counts) if n == 0 and nz and nz[0] < l < nz[-1]]
    return {"level0_count": counts[0], "upper_levels_count": int(sum(counts[1:])), "middle_empty_levels": len(middle_empty), "keypoints": len(kps),
            "lower_level_empty_below_a_populated_one": int(any(n == 0 for n in counts[:nz[-1]])) if nz else 0}


CONDITIONS = {
    "orientation": orientation_conditions,
    "border_c0": border_conditions,
    "border_c4": border_conditions,
    "noise": noise_conditions,
    "saturation_dark_dots": saturation_conditions,
    "saturation_bright_dots": saturation_conditions,
    "level0_empty": level_gap_conditions,
    "middle_level_empty": level_gap_conditions,
    "level0_only": level_gap_conditions,
}


def conditions(oracle, name, img=None, p=None):
    if img is None:
        img, p = FRAMES[name]()
    return CONDITIONS[name](oracle, img, p)
