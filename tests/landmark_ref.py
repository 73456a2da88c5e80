"""The sequential reference of the landmark upkeep (rules L1 to L9): data::landmark::update_normal_and_depth and
data::landmark::compute_descriptor for one landmark after the other, in numpy scalars (every operation rounded on its own, a division by zero
giving what IEEE says) and Python integers. No vectorised sum, and rule L8 is an explicit sort. Plus the scenes the host program and the
device are held to, as the arrays of the C ABI.

A case is a dict of arrays: offsets i32 [n + 1], pos_w f64 [n, 3], ref_keyfrm i32 [n], ref_level i32 [n], obs_keyfrm i32 [T], obs_desc u8 [T, 32],
obs_use u8 [T] or None, cam_centers f64 [K, 3], scale_factors f32 [L]."""
import math
import random

import numpy as np

NUM_LEVELS = 8
SCALE_FACTORS = np.cumprod(np.concatenate([[np.float32(1.0)], np.full(NUM_LEVELS - 1, np.float32(1.2), np.float32)])).astype(np.float32)
F64, F32 = np.float64, np.float32


# ---- rules L2 to L5
def norm3(d0, d1, d2):
    return np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)


def geometry(pos, centres, ref_centre, sf_ref_level, sf_last_level):
    """pos: 3 floats; centres: the observations' camera centres in list order (not empty). Returns (mean_normal [3 f64], min_valid f32, max_valid f32)."""
    p = [F64(v) for v in pos]
    s = [F64(0.0), F64(0.0), F64(0.0)]
    with np.errstate(all="ignore"):
        for c in centres:
            d = [p[k] - F64(c[k]) for k in range(3)]
            n = norm3(d[0], d[1], d[2])
            for k in range(3):
                s[k] = s[k] + d[k] / n
        mean = [s[k] / F64(len(centres)) for k in range(3)]
        d = [p[k] - F64(ref_centre[k]) for k in range(3)]
        dist = norm3(d[0], d[1], d[2])
        max_valid = F32(dist * F64(F32(sf_ref_level)))
        min_valid = F32(max_valid / F32(sf_last_level))
    return mean, min_valid, max_valid


# ---- rules L6 to L9
def hamming(a, b):
    return bin(int.from_bytes(bytes(a), "little") ^ int.from_bytes(bytes(b), "little")).count("1")


def medians(descs):
    M = len(descs)
    out = []
    for i in range(M):
        row = sorted(hamming(descs[i], descs[j]) for j in range(M))
        out.append(row[int(math.floor(0.5 * (M - 1)))])
    return out


def descriptor(descs, use):
    """descs: the observations' descriptors in list order; use: their flags. Returns the winner's position in the list, or -1."""
    taking_part = [t for t in range(len(descs)) if use[t]]
    if not taking_part:
        return -1
    best, winner = 256, 0
    for i, med in enumerate(medians([descs[t] for t in taking_part])):
        if med < best:
            best, winner = med, i
    return taking_part[winner]


# ---- a whole case
def solve(case):
    """Per landmark: dict status, normal ([3 f64] or None: untouched), min_valid, max_valid, best_obs (None: untouched), desc (bytes or None)."""
    out = []
    off, use = case["offsets"], case["obs_use"]
    for p in range(len(off) - 1):
        a, b = int(off[p]), int(off[p + 1])
        if a == b:
            out.append(dict(status=1, normal=None, min_valid=None, max_valid=None, best_obs=None, desc=None))
            continue
        centres = [case["cam_centers"][int(k)] for k in case["obs_keyfrm"][a:b]]
        sf = case["scale_factors"]
        normal, mn, mx = geometry(case["pos_w"][p], centres, case["cam_centers"][int(case["ref_keyfrm"][p])], sf[int(case["ref_level"][p])], sf[len(sf) - 1])
        descs = [case["obs_desc"][t].tobytes() for t in range(a, b)]
        best = descriptor(descs, [1] * (b - a) if use is None else [int(u) for u in use[a:b]])
        out.append(dict(status=0, normal=normal, min_valid=mn, max_valid=mx, best_obs=best, desc=descs[best] if best >= 0 else None))
    return out


GEO_SENTINEL, RANGE_SENTINEL, BEST_SENTINEL, BYTE_SENTINEL = -7.0, F32(-3.0), -9, 0xA5


def sentinel_outputs(n):
    return dict(mean_normal=np.full((n, 3), GEO_SENTINEL), min_max_dist=np.full((n, 2), RANGE_SENTINEL, np.float32), best_obs=np.full(n, BEST_SENTINEL, np.int32),
                desc=np.full((n, 32), BYTE_SENTINEL, np.uint8), status=np.full(n, BYTE_SENTINEL, np.uint8))


def expected_outputs(case, what=3, solved=None):
    """The five output arrays of the ABI after a call on sentinel-filled arrays."""
    solved = solve(case) if solved is None else solved
    out = sentinel_outputs(len(solved))
    for p, r in enumerate(solved):
        out["status"][p] = r["status"]
        if r["status"] != 0:
            continue
        if what & 1:
            out["mean_normal"][p] = r["normal"]
            out["min_max_dist"][p] = (r["min_valid"], r["max_valid"])
        if what & 2:
            out["best_obs"][p] = r["best_obs"]
            if r["best_obs"] >= 0:
                out["desc"][p] = np.frombuffer(r["desc"], np.uint8)
    return out


def canon_bytes(out):
    """The outputs as they are compared: every byte, but a NaN is a NaN whatever its sign and payload (the host's and the device's default NaNs
    differ in sign)."""
    n = np.ascontiguousarray(out["mean_normal"], np.float64).view(np.uint64).copy()
    n[np.isnan(out["mean_normal"])] = 0x7FF8000000000000
    r = np.ascontiguousarray(out["min_max_dist"], np.float32).view(np.uint32).copy()
    r[np.isnan(out["min_max_dist"])] = 0x7FC00000
    return n.tobytes(), r.tobytes(), np.ascontiguousarray(out["best_obs"], np.int32).tobytes(), np.ascontiguousarray(out["desc"], np.uint8).tobytes(), \
        np.ascontiguousarray(out["status"], np.uint8).tobytes()


# ---- scenes
def flip(desc, *bits):
    d = bytearray(desc)
    for b in bits:
        d[b >> 3] ^= 1 << (b & 7)
    return bytes(d)


def complement(desc):
    return bytes(v ^ 0xFF for v in desc)


def tie_descriptors(rng):
    """Two clusters, rows 1, 2 and 4 tie at a median of 2, rows 0, 3 and 5 at 4: row 1 has to win."""
    x, y = bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(32))
    xs, ys = [flip(x, 1), flip(x, 2), flip(x, 3)], [flip(y, 4, 5), flip(y, 6, 7), flip(y, 8, 9)]
    return [ys[0], xs[0], xs[1], ys[1], xs[2], ys[2]]


def make_case(counts, K=6, seed=0, content="random", use="all", ref_levels=None, at_centre=(), wide_slots=False):
    """counts: observations per landmark. content: random | equal | tie (six observations each) | extremes (a descriptor, itself and its
    complement, repeated). use: all | none | first | last | alt (every other one, from the first). at_centre: landmarks placed on the camera
    centre of their first observation. wide_slots: observations spread over all K slots with repetition (else the first min(K, count) distinct)."""
    rng = random.Random(seed)
    n, T = len(counts), sum(counts)
    centres = np.array([[rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-1, 1)] for _ in range(K)])
    pos = np.array([[rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(4, 10)] for _ in range(n)]).reshape(n, 3)
    offsets = np.cumsum([0] + list(counts)).astype(np.int32)
    obs_kf, descs, flags = [], [], []
    ref_kf, ref_lv = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for p, c in enumerate(counts):
        slots = [rng.randrange(K) for _ in range(c)] if (wide_slots or c > K) else rng.sample(range(K), c)
        obs_kf += slots
        if c:
            ref_kf[p] = slots[rng.randrange(c)]
            if p in at_centre:
                pos[p] = centres[slots[0]]
        ref_lv[p] = rng.randrange(NUM_LEVELS) if ref_levels is None else ref_levels[p % len(ref_levels)]
        if content == "random":
            descs += [bytes(rng.randrange(256) for _ in range(32)) for _ in range(c)]
        elif content == "equal":
            descs += [bytes(rng.randrange(256) for _ in range(32))] * c
        elif content == "tie":
            assert c == 6
            descs += tie_descriptors(rng)
        elif content == "extremes":
            a = bytes(rng.randrange(256) for _ in range(32))
            descs += [(a, a, complement(a))[k % 3] for k in range(c)]
        else:
            raise ValueError(content)
        flags += {"all": [1] * c, "none": [0] * c, "first": [1] + [0] * (c - 1), "last": [0] * (c - 1) + [1], "alt": [1 - (k & 1) for k in range(c)]}[use][:c]
    return dict(offsets=offsets, pos_w=pos, ref_keyfrm=ref_kf, ref_level=ref_lv, obs_keyfrm=np.array(obs_kf, np.int32).reshape(T),
                obs_desc=np.frombuffer(b"".join(descs), np.uint8).reshape(T, 32).copy(), obs_use=None if use == "all" else np.array(flags, np.uint8).reshape(T),
                cam_centers=centres, scale_factors=SCALE_FACTORS.copy())


COUNTS = (0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 130)
BATCHES = (1, 63, 64, 65, 513)
LDS_CENTRES = 256   # csrc/landmark_update.hip: the camera centres a workgroup of k_landmark_geometry holds in LDS


def _batch_counts(n, seed):
    rng = random.Random(seed)
    return [rng.choice((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12)) for _ in range(n)]


def _mixed_counts():
    counts = list(COUNTS) * 2 + [4, 5, 6, 10, 33]
    random.Random(5).shuffle(counts)
    return counts


_MAKERS = {
    **{"n%d" % c: (lambda c=c: make_case([c], seed=100 + c)) for c in COUNTS},
    "mixed": lambda: make_case(_mixed_counts(), seed=7),
    **{"batch%d" % n: (lambda n=n: make_case(_batch_counts(n, n), K=12, seed=200 + n)) for n in BATCHES},
    "use_none": lambda: make_case([0, 3, 9, 1], seed=11, use="none"),
    "use_first": lambda: make_case([1, 5, 9, 70], seed=12, use="first"),
    "use_last": lambda: make_case([1, 5, 9, 70], seed=13, use="last"),
    "use_alt": lambda: make_case([15, 16, 17, 18, 2, 1], seed=14, use="alt"),        # M = 8, 8, 9, 9, 1, 1
    "equal": lambda: make_case([1, 2, 3, 8, 9, 70], seed=15, content="equal"),
    "tie": lambda: make_case([6, 6, 6], seed=16, content="tie"),
    "extremes": lambda: make_case([2, 3, 4, 5, 6, 8, 9, 12, 66], seed=17, content="extremes"),
    "k1": lambda: make_case([1, 4, 9, 0, 2], K=1, seed=18),
    "k300": lambda: make_case([3, 40, 9, 300, 2, 7], K=300, seed=19, wide_slots=True),
    "at_centre": lambda: make_case([1, 4, 9, 3], seed=20, at_centre=(0, 1, 2)),
    "ref_levels": lambda: make_case([3, 3, 5, 5], seed=21, ref_levels=(0, NUM_LEVELS - 1)),
}
CASES = list(_MAKERS)
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _MAKERS[name]()
    return _cache[name]


def solved(name):
    key = ("solved", name)
    if key not in _cache:
        _cache[key] = solve(case(name))
    return _cache[key]


def expected(name, what=3):
    return expected_outputs(case(name), what, solved(name))
