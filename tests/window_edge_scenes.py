"""Scene builders for the window matchers' size edges (tests/test_window_edge_shapes.py on the CPU, tests/test_gpu_window_edges.py on the device):
plain numpy, fixed seeds. Every builder returns the arrays of one matcher call together with the facts the scene was built to have, so that a test can
hold those facts against the oracle without running the code under test.

The lattice: sites 8 px apart; every target sits exactly on a site, every query exactly on a site. With margin 3 at level 0 a query's window takes the
targets of its own site and nothing else, in ascending target index (members of one cell come in keypoint order), so a query's candidate list is known
by construction: n_keys = sum over the valid queries of their site's occupancy. For the BoW matchers the same descriptors serve: unrelated descriptors
are ~128 bits apart, far beyond every rule's dead_from, so a query's live list is again its site's targets."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
PLAN_EXE = os.path.join(CPP, "match_window_plan_host")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
SF = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)]).astype(np.float32)).astype(np.float32)
PITCH = 8.0          # lattice spacing in pixels
MARGIN = 3           # the window of a level-0 query: its own site only
THR_LOW, THR_HIGH = 50, 100
MARK_SIZE = 4096     # the resolver's stamp table (kMarkSize): targets t and t + 4096 share a slot


# ---- the host plan program (tests/match_window_plan_host.cc, built as tests/test_match_window_plan.py builds it) ------------------------------------
def plan(rows):
    """rows -> {row: tuple of ints}"""
    subprocess.check_call(["make", "-s", "-C", CPP, "match_window_plan_host"])
    rows = list(dict.fromkeys(rows))
    r = subprocess.run([PLAN_EXE] + rows, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    return {row: tuple(int(v) for v in line.split()) for row, line in zip(rows, lines)}


def resolve_row(n_q, n_t):
    return "resolve:%d:%d:1024" % (n_q, n_t)


def resolve_form(answer):
    """(offsets_in_lds, key_pool, width) of a resolve row's answer (ok fixed offsets_in_lds lds key_pool width)"""
    assert answer[0] == 1
    return answer[2], answer[4], answer[5]


def grid_row(n, cells):
    return "grid:%d:%d" % (n, cells)


def grid_form(answer):
    """(items_in_lds, raise_attr)"""
    return answer[0], answer[2]


def dead_from(thr, ratio):
    """the plan's dead_from_ratio, restated: the smallest d > thr with fl(d * ratio) >= thr, 257 if there is none"""
    for d in range(thr + 1, 257):
        if np.float32(d) * np.float32(ratio) >= np.float32(thr):
            return d
    return 257


# ---- controlled-distance descriptors ---------------------------------------------------------------------------------------------------------------
def bits_desc(d):
    """32 bytes with exactly the lowest d bits set: its distance from the all-zero descriptor is d (0..256)"""
    assert 0 <= d <= 256
    b = np.zeros(256, np.uint8)
    b[:d] = 1
    return np.packbits(b, bitorder="little")


def hamming(a, b):
    return np.unpackbits(np.bitwise_xor(a, b), axis=-1).sum(-1).astype(np.int32)


def _flip(desc, positions):
    b = np.unpackbits(desc, bitorder="little")
    b[positions] ^= 1
    return np.packbits(b, bitorder="little")


def keypoints(xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"] = 31.0
    k["octave"] = octave
    k["angle"] = angle
    return k


def make_gp(mod, cols, rows, max_x, max_y, min_x=0.0, min_y=0.0):
    """GridParams of `mod` (the oracle binding, or openvslam_amd._lib for the device: same six fields)"""
    return mod.GridParams(min_x, min_y, float(max_x), float(max_y), cols, rows)


# ---- the lattice ------------------------------------------------------------------------------------------------------------------------------------
class Lattice:
    """n_sites sites, `occupancy` targets on each: target t sits on site t % n_sites (so the members of a site are t, t + n_sites, ...: with
    n_sites = 4096 they share a slot of the stamp table). Member k of a site is the site's random base descriptor with bits [step * (k - 1), step * k)
    flipped (k >= 1), so two members are step or 2 * step bits apart; a query is its preferred member with `noise` of the bits 128..255 flipped:
    d(query, preferred) = noise, d(query, other member of the site) = noise + the members' distance, d(query, anything else) ~ 128."""

    def __init__(self, n_t, n_sites, seed, step=24, grid=(64, 48)):
        self.rng = np.random.default_rng(seed)
        self.n_t, self.n_sites, self.step = n_t, n_sites, step
        assert step * (-(-n_t // n_sites) - 1) <= 128
        self.width = int(np.ceil(np.sqrt(n_sites * 4.0 / 3.0)))
        self.t_site = np.arange(n_t) % n_sites
        self.t_member = np.arange(n_t) // n_sites
        self.site_xy = np.stack([PITCH * (1 + np.arange(n_sites) % self.width), PITCH * (1 + np.arange(n_sites) // self.width)], 1).astype(np.float32)
        self.max_x = float(PITCH * (self.width + 1))
        self.max_y = float(PITCH * ((n_sites - 1) // self.width + 2))
        self.grid = grid
        base = self.rng.integers(0, 256, (n_sites, 32), dtype=np.uint8)
        self.t_desc = np.stack([base[s] if k == 0 else _flip(base[s], np.arange(step * (k - 1), step * k)) for s, k in zip(self.t_site, self.t_member)])
        self.t_kps = keypoints(self.site_xy[self.t_site], 0, 0.0)
        self.occupancy = np.bincount(self.t_site, minlength=n_sites)

    def gp(self, mod):
        return make_gp(mod, self.grid[0], self.grid[1], self.max_x, self.max_y)

    def queries(self, pref, noise, valid):
        """queries preferring target pref[q] at distance noise[q]"""
        pref, noise = np.asarray(pref), np.asarray(noise)
        q_desc = np.stack([_flip(self.t_desc[t], 128 + self.rng.permutation(128)[:j]) for t, j in zip(pref, noise)])
        return Queries(self, pref, noise, np.asarray(valid, np.uint8), q_desc)


class Queries:
    def __init__(self, lat, pref, noise, valid, desc):
        self.lat, self.pref, self.noise, self.valid, self.desc = lat, pref, noise, valid, desc
        self.n_q = len(pref)
        self.site = lat.t_site[pref]
        self.xy = np.ascontiguousarray(lat.site_xy[self.site])
        # four rotation bins filled 3 : 2 : 2 : 1: the orientation check drops the last; the last query is in the fullest
        q = np.arange(self.n_q)
        self.angle = (30.0 * np.where(q % 8 == 3, 0, q % 4)).astype(np.float32)
        self.angle[-1] = 0.0

    def n_keys(self, dead):
        """entries of the candidate CSR, counted in numpy: the members of every valid query's site that are nearer than `dead`"""
        lat, total = self.lat, 0
        for k in range(int(lat.occupancy.max())):
            t = self.site + k * lat.n_sites
            ok = (self.valid != 0) & (t < lat.n_t)
            total += int((hamming(self.desc[ok], lat.t_desc[t[ok]]) < dead).sum())
        return total

    def kps(self, invalid_octave=0):
        """as keypoints; the area matcher's invalid queries are those above level 0"""
        k = keypoints(self.xy, 0, self.angle)
        k["octave"] = np.where(self.valid != 0, 0, invalid_octave)
        return k


class Targets:
    """the target side of a call from plain arrays (what the calls below read of a Lattice): gp_args = (cols, rows, max_x, max_y)"""

    def __init__(self, gp_args, t_kps, t_desc):
        self.gp_args, self.t_kps, self.t_desc, self.n_t = gp_args, t_kps, t_desc, len(t_kps)
        self.max_x, self.max_y = gp_args[2], gp_args[3]

    def gp(self, mod):
        return make_gp(mod, *self.gp_args)


class PlainQueries:
    def __init__(self, xy, desc, level=0):
        self.xy, self.desc, self.n_q = np.ascontiguousarray(xy, np.float32), desc, len(xy)
        self.valid = np.ones(self.n_q, np.uint8)
        self.level = np.full(self.n_q, level, np.int32)

    def kps(self, invalid_octave=0):
        return keypoints(self.xy, 0, 0.0)


SPECIAL = (3, 4, 67, 451, 515, 1027)   # q, q + 1 (same wave), q + 64 and q + 448 (other waves of the round), q + 512 and q + 1024 (later rounds)
WIDTH_NQ = [64, 65, 256, 257, 1024, 1025, 1537]
LISTS_M = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049]
RULE_THR = {"projection": THR_HIGH, "area": THR_LOW, "bow": THR_LOW, "bestonly": THR_HIGH, "triang": THR_LOW}


def contended_scene(n_q, seed, n_t=None, step=24):
    """The widths scene. Queries 3, 4, 67, 451, 515 and 1027 -- where they exist -- prefer target 0, at distances 30, 20, 2, 2, 1 and 0: under the
    sequential rules the first claims it, under the area rule 4 steals it from 3 inside one wave, 67 inside one round, 515 and 1027 across rounds.
    From 256 queries on, queries 0..63 all prefer target 0, a chain of 64 consecutive queries with one best, at distances falling from 45 to 3
    (queries 3 and 4 at 43 and 42). The rest prefer random targets of ~n_q / 3 sites with two members each, a tenth of them invalid; the last query
    is valid and alone on a site of its own. Returns (lattice, queries, facts)."""
    n_sites = n_q // 3 + 2
    lat = Lattice(2 * n_sites if n_t is None else n_t, n_sites, seed, step=step)
    rng = lat.rng
    pref = rng.integers(1, lat.n_t, n_q)
    pref[lat.t_site[pref] == n_sites - 1] = 1        # the last site is the last query's
    pref[lat.t_site[pref] == 0] = 1                  # site 0 is the chain's
    noise = rng.integers(0, 41, n_q)
    valid = (rng.random(n_q) >= 0.1).astype(np.uint8)
    chain = np.arange(64) if n_q >= 256 else np.array([3, 4])
    chain = chain[chain < n_q - 1]
    pref[chain], valid[chain] = 0, 1
    noise[chain] = 45 - (2 * chain) // 3 if n_q >= 256 else np.array([30, 20])[:len(chain)]
    for q, j in zip(SPECIAL[2:], (2, 2, 1, 0)):
        if q < n_q - 1:
            pref[q], noise[q], valid[q] = 0, j, 1
    pref[-1], noise[-1], valid[-1] = n_sites - 1, 0, 1
    qs = lat.queries(pref, noise, valid)
    pairs = [(a, b) for a, b in ((3, 4), (3, 67), (3, 451), (3, 515), (3, 1027)) if b < n_q - 1]
    return lat, qs, {"pairs": pairs, "chain": chain, "steals": [(a, b) for a, b in ((2, 3) if n_q >= 256 else (3, 4), (3, 67), (67, 515), (515, 1027)) if b < n_q - 1]}


def collision_scene(n_q, seed):
    """8200 targets on 4096 sites: targets i, i + 4096 and (i < 8) i + 8192 are co-located and share a slot of the stamp table. Consecutive queries
    walk the sites in pairs that prefer different members of one site, so every 64-query window holds >= 32 such pairs; the last third of the
    queries revisits the first sites (other rounds) and prefers the member the first visitor preferred."""
    lat = Lattice(8200, MARK_SIZE, seed, step=24, grid=(64, 64))
    rng = lat.rng
    site = np.repeat(rng.permutation(np.arange(8, MARK_SIZE))[:(n_q + 1) // 2], 2)[:n_q]
    site[:16] = np.repeat(np.arange(8), 2)           # the triples
    member = np.arange(n_q) % 2
    member[:16:4] = 2
    pref = site + MARK_SIZE * member
    late = np.arange(n_q * 2 // 3, n_q)
    pref[late] = pref[late - n_q * 2 // 3]
    valid = np.ones(n_q, np.uint8)
    qs = lat.queries(pref, rng.integers(0, 30, n_q), valid)
    return lat, qs


def congruent_pairs(qs):
    """pairs (q, q') of one 64-query window whose preferred targets differ and are congruent mod MARK_SIZE"""
    n = 0
    for b in range(0, qs.n_q, 64):
        p = qs.pref[b:b + 64]
        same_slot = (p[:, None] % MARK_SIZE) == (p[None, :] % MARK_SIZE)
        n += int((same_slot & (p[:, None] != p[None, :])).sum()) // 2
    return n


def lds_edge_scene(n_q, n_t, n_sites, n_keys, seed, step=24):
    """n_q queries on n_t targets over n_sites sites (occupancy o or o + 1), the valid ones chosen so that the candidate CSR has exactly n_keys
    entries: a on sites of o + 1 members and b on sites of o with (o + 1) a + o b = n_keys. The last query is valid and matched."""
    lat = Lattice(n_t, n_sites, seed, step=step)
    rng = lat.rng
    o = int(lat.occupancy.min())
    hi_sites, lo_sites = np.nonzero(lat.occupancy == o + 1)[0], np.nonzero(lat.occupancy == o)[0]
    if len(hi_sites) == 0:
        assert n_keys % o == 0
        a, b = 0, n_keys // o
    else:
        b = next(b for b in range(o + 1) if (n_keys - o * b) % (o + 1) == 0)
        a = (n_keys - o * b) // (o + 1)
    assert 1 <= a + b <= n_q
    valid = np.zeros(n_q, np.uint8)
    chosen = np.concatenate([rng.permutation(n_q - 1)[:a + b - 1], [n_q - 1]])
    valid[chosen] = 1
    # the last site of either occupancy is kept free for the last query, which prefers its last member at distance 0 and has no competitor:
    # it is matched, so a wrong last list bound shows
    site = rng.integers(0, n_sites, n_q)
    if a:
        site[chosen[:a]] = hi_sites[rng.integers(0, len(hi_sites) - 1, a)]
    if b:
        site[chosen[a:]] = lo_sites[rng.integers(0, len(lo_sites) - 1, b)]
    site[-1] = lo_sites[-1] if b else hi_sites[-1]
    member, noise = rng.integers(0, o, n_q), rng.integers(0, 31, n_q)
    member[-1], noise[-1] = lat.occupancy[site[-1]] - 1, 0   # the site's last member: the last key of the whole CSR is this query's best
    return lat, lat.queries(site + n_sites * member, noise, valid)


def preferred_owner_lost(qs, assigned_of_query, thr):
    """per query: valid, its preferred target within thr, and the oracle gave that target to another query"""
    owner = np.full(qs.lat.n_t, -1)
    m = assigned_of_query >= 0
    owner[assigned_of_query[m]] = np.nonzero(m)[0]
    return (qs.valid != 0) & (qs.noise <= thr) & (owner[qs.pref] >= 0) & (owner[qs.pref] != np.arange(qs.n_q))


# ---- calls: the oracle's side of each entry point on a lattice scene ------------------------------------------------------------------------------
def oracle_projection(oracle, lat, qs, ratio, margin=float(MARGIN)):
    lv = getattr(qs, "level", np.zeros(qs.n_q, np.int32))
    return oracle.projection_match_frame_and_landmarks(lat.gp(oracle), lat.t_kps, lat.t_desc, SF, qs.xy, lv, qs.desc, margin, ratio, lm_valid=qs.valid)


def oracle_area(oracle, lat, qs, ratio, check_orientation, margin=MARGIN):
    """-> (n, matched, prev_matched_xy after the call)"""
    prev = qs.xy.copy()
    n, matched = oracle.area_match_in_consistent_area(lat.gp(oracle), qs.kps(invalid_octave=1), qs.desc, lat.t_kps, lat.t_desc, prev, margin, ratio,
                                                      check_orientation)
    return n, matched, prev


# match_current_and_last_frames with fx = fy = 1, cx = cy = 0 and identity poses: the landmark (u, v, 1) reprojects onto (u, v) exactly
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


def generic_camera(mod, lat):
    return mod.Camera(0, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, int(lat.max_x), int(lat.max_y))


def generic_points(qs):
    return np.concatenate([qs.xy.astype(np.float64), np.ones((qs.n_q, 1))], 1)


def oracle_generic(oracle, lat, qs, check_orientation, margin=float(MARGIN)):
    return oracle.projection_match_current_and_last_frames(generic_camera(oracle, lat), lat.gp(oracle), lat.t_kps, lat.t_desc, IDENTITY, qs.kps(),
                                                           generic_points(qs), qs.desc, IDENTITY, SF, margin, check_orientation, last_valid=qs.valid)


# the BoW matchers: a node per `nodes` entry (node id, first query, end query): its queries and all the targets of their sites
def bow_vectors(lat, qs, nodes=None, absent=()):
    """(keyframe = query side, frame = target side) feature vectors; the nodes in `absent` are missing on the frame side"""
    nodes = [(5, 0, qs.n_q)] if nodes is None else nodes
    fq, ft = {}, {}
    for node, b, e in nodes:
        fq[node] = list(range(b, e))
        if node not in absent:
            ft[node] = [int(t) for t in np.nonzero(np.isin(lat.t_site, np.unique(qs.site[b:e])))[0]]
    return fq, ft


def bow_nodes(n_q):
    """a small first node, a node the frame lacks, the bulk, and a last node that holds the last query"""
    return [(2, 0, 5), (4, 5, 9), (7, 9, n_q - 3), (9, n_q - 3, n_q)], (4,)


def oracle_bow(oracle, lat, qs, ratio, check_orientation, fq_ft=None):
    fq, ft = bow_vectors(lat, qs) if fq_ft is None else fq_ft
    return oracle.bow_match_frame_and_keyframe(qs.kps(), qs.desc, fq, lat.t_kps, lat.t_desc, ft, ratio, check_orientation, qs.valid)


# match_for_triangulation: every bearing (0, 0, 1), E = [t]x with t = (1, 0, 0): E b = (0, -1, 0) is orthogonal to b, the epipolar residual is 0 for
# every pair, and the epipole (1, 0, 0) is 90 degrees from every bearing -- the candidate lists are the node buckets within THR_LOW
TRI_E = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
TRI_EPIPOLE = np.array([1.0, 0.0, 0.0])


def bearings(n):
    return np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))


def oracle_triang(oracle, lat, qs, check_orientation, fq_ft=None):
    fq, ft = bow_vectors(lat, qs) if fq_ft is None else fq_ft
    return oracle.robust_match_for_triangulation(qs.kps(), qs.desc, fq, bearings(qs.n_q), lat.t_kps, lat.t_desc, ft, bearings(lat.n_t), TRI_E, TRI_EPIPOLE,
                                                 SF, check_orientation, (qs.valid == 0).astype(np.uint8), None)


# ---- window cell counts -------------------------------------------------------------------------------------------------------------------------------
# (grid cols, grid rows): with a margin that covers the image every query's window is the whole grid: cols * rows cells, x-major
WINDOW_GRIDS = {63: (9, 7), 64: (8, 8), 65: (13, 5), 128: (16, 8), 129: (43, 3)}


def window_scene(n_cells, seed):
    """One target in every cell of a WINDOW_GRIDS grid (cell 16 px), target index = cell index in the kernel's x-major order, and
    queries in the image centre whose window is the whole grid. Query 0's winner is the target of cell `winner_cell`: the first cell of the second
    pass (64) in the 65- and 128-cell windows, of the third pass (128) in the 129-cell window -- the last cell of the 65- and 129-cell windows --,
    and the last lane of the only pass (63) in the 64-cell window; in the 63-cell window the last cell (62). Query 1 wins the target of cell 0,
    query 2 prefers query 0's winner and loses it. Returns (targets, queries, facts)."""
    cols, rows = WINDOW_GRIDS[n_cells]
    rng = np.random.default_rng(seed)
    winner_cell = {63: 62, 64: 63, 65: 64, 128: 64, 129: 128}[n_cells]
    cx, cy = np.divmod(np.arange(n_cells), rows)
    t_xy = np.stack([16.0 * cx + 4.0, 16.0 * cy + 4.0], 1).astype(np.float32)   # cvRound(x / 16) = cx
    t_desc = rng.integers(0, 256, (n_cells, 32), dtype=np.uint8)
    pref = np.array([winner_cell, 0, winner_cell])
    noise = np.array([5, 7, 9])
    q_desc = np.stack([_flip(t_desc[t], 128 + rng.permutation(128)[:j]) for t, j in zip(pref, noise)])
    q_xy = np.tile(np.array([[8.0 * cols, 8.0 * rows]], np.float32), (3, 1))
    return (Targets((cols, rows, 16.0 * cols, 16.0 * rows), keypoints(t_xy), t_desc), PlainQueries(q_xy, q_desc),
            {"want": np.array([winner_cell, 0, -1], np.int32), "margin": 16 * max(cols, rows)})


def corner_scene(seed):
    """The 8 x 8 grid of window_scene(64) with margin 3: query 0 sits on the target of the last cell (7, 7), where floor((x - r) / 16) = 7 and the upper
    end is clipped to 7 -- a window of a single cell; queries 1..4 lie 50 px outside the grid on each side (no window at all) and carry the exact
    descriptor of a target; query 5 is query 0 again and loses."""
    tg, _, _ = window_scene(64, seed)
    t_desc = tg.t_desc
    q_xy = np.array([[116.0, 116.0], [-50.0, 60.0], [178.0, 60.0], [60.0, -50.0], [60.0, 178.0], [116.0, 116.0]], np.float32)
    q_desc = t_desc[[63, 3, 59, 24, 31, 63]].copy()
    return tg, PlainQueries(q_xy, q_desc), {"want": np.array([63, -1, -1, -1, -1, -1], np.int32), "margin": 3}


# ---- dead_from and rule edges -------------------------------------------------------------------------------------------------------------------------
def rule_edge_scene(thr, ratio, projection):
    """Isolated all-zero queries, each alone on a lattice site with one to three targets of controlled distance (bits_desc): best in
    {thr - 1, thr, thr + 1} x second in {none, dead_from - 2 .. dead_from + 1, 255, 256}, the second before and behind the best in enumeration order;
    best == second; d = 0 and d = 256; a third candidate between the two. Under the projection rule the queries are at level 1 (window levels 0 and
    1), the best at level 1 and the second at level 1 or 0: the ratio test only applies within one level.
    Returns (targets, queries, the per-query (distances, levels) as built)."""
    dead = dead_from(thr, ratio)
    cases = []
    for best in (thr - 1, thr, thr + 1):
        for second in (None, dead - 2, dead - 1, dead, dead + 1, 255, 256):
            if second is not None and second > 256:
                continue
            for same in ((True, False) if (projection and second is not None) else (True,)):
                for second_first in ((False, True) if second is not None else (False,)):
                    cases.append(([second, best] if second_first else [best] + ([] if second is None else [second]),
                                  [(1 if same else 0), 1] if second_first else [1] + ([] if second is None else [1 if same else 0])))
    for d in (0, 1, thr // 2, thr - 1, thr, thr + 1, 256):
        cases.append(([d, d], [1, 1]))            # best == second: the first in enumeration order wins (or nothing does)
        cases.append(([d], [1]))
    cases.append(([0, 256], [1, 1]))
    cases.append(([256, 0], [1, 1]))
    cases.append(([thr, dead - 1, dead], [1, 1, 1]))
    cases.append(([dead, thr, dead - 1], [1, 1, 1]))
    cases.append(([dead - 1, 256, thr - 1], [1, 0, 1]))
    t_xy, t_desc, t_oct, q_xy = [], [], [], []
    width = 32
    for i, (ds, lv) in enumerate(cases):
        xy = (PITCH * (1 + i % width), PITCH * (1 + i // width))
        q_xy.append(xy)
        for d, l in zip(ds, lv):
            t_xy.append(xy)
            t_desc.append(bits_desc(int(d)))
            t_oct.append(l if projection else 0)
    t_kps = keypoints(np.array(t_xy, np.float32), np.array(t_oct), 0.0)
    gp_args = (64, 48, PITCH * (width + 1), PITCH * (len(cases) // width + 2))
    qs = PlainQueries(np.array(q_xy, np.float32), np.zeros((len(cases), 32), np.uint8), level=1 if projection else 0)
    return Targets(gp_args, t_kps, np.stack(t_desc)), qs, cases


RULE_EDGE = [(thr, ratio) for thr in (THR_LOW, THR_HIGH) for ratio in (0.6, 0.75, 0.9, 1.0)]   # thr 50: the area rule, thr 100: the projection rule


# ---- keypoint sets for a grid -------------------------------------------------------------------------------------------------------------------------
GRID_KINDS = ("uniform", "ties", "negmin", "crowded")
MAX_PER_CELL = 256   # the per-cell insertion sort is one lane's and quadratic


def grid_bounds(cols, rows, kind):
    """(min_x, min_y, max_x, max_y): cells of 8 x 8 px, so that (x - min) / 8 is exact in float"""
    if kind == "negmin":
        return -24.0, -16.0, 8.0 * cols - 24.0, 8.0 * rows - 16.0
    return 0.0, 0.0, 8.0 * cols, 8.0 * rows


def cells_of(cols, rows, bounds, x, y):
    """get_cell_indices in numpy: cvRound((pt - min) * inv_cell), round-half-even in float; -1 outside"""
    min_x, min_y, max_x, max_y = (np.float32(v) for v in bounds)
    inv_w = np.float32(np.float64(cols) / np.float64(max_x - min_x))
    inv_h = np.float32(np.float64(rows) / np.float64(max_y - min_y))
    cx = np.rint((x.astype(np.float32) - min_x) * inv_w).astype(np.int64)
    cy = np.rint((y.astype(np.float32) - min_y) * inv_h).astype(np.int64)
    return np.where((0 <= cx) & (cx < cols) & (0 <= cy) & (cy < rows), cx * rows + cy, -1)


def grid_keys(cols, rows, n, kind, seed=0):
    """-> (bounds, keypoints, cell id per keypoint in numpy). Every set has keypoints outside the bounds on all four sides (n >= 8), at most
    MAX_PER_CELL per cell (the excess lies outside), and -- "ties" -- points exactly on cell borders: (x - min) / 8 = k + 0.5, which rounds down to k
    for even k and up to k + 1 for odd k."""
    rng = np.random.default_rng(1000 * cols + 10 * rows + n + seed)
    b = grid_bounds(cols, rows, kind)
    w, h = b[2] - b[0], b[3] - b[1]
    if kind == "crowded":   # few cells, many members each
        k = min(cols * rows, max(2, -(-n // 200)))
        c = rng.integers(0, k, n)
        x = b[0] + 8.0 * (c // rows) + rng.uniform(-3.5, 3.5, n)
        y = b[1] + 8.0 * (c % rows) + rng.uniform(-3.5, 3.5, n)
    else:
        x = rng.uniform(b[0] - 6.0, b[2] + 2.0, n)
        y = rng.uniform(b[1] - 6.0, b[3] + 2.0, n)
        if kind == "ties":
            tie = rng.random(n) < 0.5
            x = np.where(tie, b[0] + 8.0 * rng.integers(0, cols, n) + 4.0, x)
            y = np.where(tie & (rng.random(n) < 0.5), b[1] + 8.0 * rng.integers(0, rows, n) + 4.0, y)
    x, y = x.astype(np.float32), y.astype(np.float32)
    if n >= 8:
        x[:4] = [b[0] - 30.0, b[2] + 30.0, b[0] + 0.25 * w, b[0] + 0.25 * w]
        y[:4] = [b[1] + 0.25 * h, b[1] + 0.25 * h, b[1] - 30.0, b[3] + 30.0]
    elif n == 1:
        x[0], y[0] = b[0] + 1.0, b[1] + 1.0
    cell = cells_of(cols, rows, b, x, y)
    order = np.argsort(cell, kind="stable")
    rank = np.empty(n, np.int64)
    sc = cell[order]
    first = np.searchsorted(sc, sc, side="left")
    rank[order] = np.arange(n) - first
    out = (cell >= 0) & (rank >= MAX_PER_CELL)
    x[out] = b[0] - 50.0
    cell[out] = -1
    kps = keypoints(np.stack([x, y], 1), rng.integers(0, 8, n), 0.0)
    return b, kps, cell


def grid_reference(cols, rows, cell):
    """cell_start and items from the numpy cell ids: members in ascending keypoint index"""
    inside = np.nonzero(cell >= 0)[0]
    order = inside[np.argsort(cell[inside], kind="stable")]
    start = np.zeros(cols * rows + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(cell[inside], minlength=cols * rows))
    return start, order.astype(np.int32)


GRIDS = [(1, 1), (1, 48), (64, 1), (32, 32), (41, 25), (64, 48)]
GRID_N = [0, 1, 1023, 1024, 1025, 8192, 8193, 12000]
GRID_FIXED = [((64, 64), 8191), ((64, 64), 8192), ((128, 128), 4095), ((128, 128), 4096)]
GRID_CASES = [(g, n) for g in GRIDS for n in GRID_N] + GRID_FIXED


# ---- LDS staging edges --------------------------------------------------------------------------------------------------------------------------------
# (n_q, n_t, sites, step between members): one target per site at the two large shapes, 17 or 18 per site at the small one
LDS_SHAPES = [(12295, 2000, 2000, 24), (12296, 2000, 2000, 24), (1000, 1000, 56, 4)]
LDS_DELTAS = [-1, 0, 1, 4]            # n_keys - key_pool: all four residues mod 4 around the edge
LDS_RATIO = 0.6                       # the projection rule at this ratio: dead_from = 167, beyond every distance inside a site


def lds_edge_case(shape, delta, key_pool, seed=7):
    """delta in LDS_DELTAS, or "3x": about three times key_pool on two targets per site (large shapes only)"""
    n_q, n_t, n_sites, step = shape
    if delta == "3x":
        return lds_edge_scene(n_q, n_t, n_t // 2, 2 * ((3 * key_pool) // 2), seed, step), 2 * ((3 * key_pool) // 2)
    return lds_edge_scene(n_q, n_t, n_sites, key_pool + delta, seed, step), key_pool + delta
