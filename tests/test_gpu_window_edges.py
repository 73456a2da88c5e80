"""GPU parity at the window matchers' size edges (openvslam_amd/csrc/match_window.hip): the launch forms and index ranges of k_grid_assign,
k_window_lists, k_bow_lists, k_scan_counts, k_list_resolve and k_cross_check that the workload-shaped tests never execute. Every comparison is exact:
assignments with np.array_equal, the match count, and for the area matcher prev_matched_xy bit for bit. The scenes come from
tests/window_edge_scenes.py; tests/test_window_edge_shapes.py shows without a device which launch form each shape takes and that each scene has
the contention / collisions / key counts it was built for. No environment variable forces a form: the shapes select them."""
import numpy as np
import pytest

import window_edge_scenes as S

pytestmark = pytest.mark.gpu

CAP_T, CAP_Q = 12288, 12304   # one context size for every case: 12 000 grid keypoints, 8200 collision targets, 12 296 queries
COLLISION_NQ = 1280


@pytest.fixture(scope="module")
def match():
    from openvslam_amd import match
    return match


@pytest.fixture(scope="module")
def lib():
    from openvslam_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(match):
    """contexts by (class, ratio, check_orientation), created once"""
    made = {}

    def get(kind, ratio, check_orientation=False):
        key = (kind, ratio, check_orientation)
        if key not in made:
            kw = dict(max_targets=CAP_T, max_queries=CAP_Q)
            if kind == "projection":
                made[key] = match.projection(ratio, check_orientation, **kw)
            elif kind == "area":
                made[key] = match.area(ratio, check_orientation, **kw)
            elif kind == "bow":
                made[key] = match.bow_tree(ratio, check_orientation, **kw)
            else:
                made[key] = match.robust_triangulation(ratio, check_orientation, **kw)
        return made[key]

    return get


# ---- the device's side of each entry point on a scene (the oracle's side: window_edge_scenes.oracle_*) --------------------------------------------
def dev_projection(ctx, lib, tg, qs, ratio, margin=float(S.MARGIN), resident=None):
    lv = getattr(qs, "level", np.zeros(qs.n_q, np.int32))
    w = ctx("projection", ratio)
    if resident is not None:
        return w.match_frame_and_landmarks(None, resident, None, S.SF, qs.xy, lv, qs.desc, margin, lm_valid=qs.valid)
    return w.match_frame_and_landmarks(tg.gp(lib), tg.t_kps, tg.t_desc, S.SF, qs.xy, lv, qs.desc, margin, lm_valid=qs.valid)


def dev_area(ctx, lib, tg, qs, ratio, check_orientation, margin=S.MARGIN):
    prev = qs.xy.copy()
    n, matched = ctx("area", ratio, check_orientation).match_in_consistent_area(tg.gp(lib), qs.kps(invalid_octave=1), qs.desc, tg.t_kps, tg.t_desc, prev,
                                                                                margin)
    return n, matched, prev


def dev_generic(ctx, lib, tg, qs, check_orientation, margin=float(S.MARGIN)):
    return ctx("projection", 0.9, check_orientation).match_current_and_last_frames(
        S.generic_camera(lib, tg), tg.gp(lib), tg.t_kps, tg.t_desc, S.IDENTITY, qs.kps(), S.generic_points(qs), qs.desc, S.IDENTITY, S.SF, margin,
        last_valid=qs.valid)


def dev_bow(ctx, tg, qs, ratio, check_orientation, fq_ft=None):
    fq, ft = S.bow_vectors(tg, qs) if fq_ft is None else fq_ft
    return ctx("bow", ratio, check_orientation).match_frame_and_keyframe(qs.kps(), qs.desc, fq, tg.t_kps, tg.t_desc, ft, qs.valid)


def dev_triang(ctx, tg, qs, check_orientation, fq_ft=None):
    """-> (n, matched_2_in_1) in the oracle's form"""
    fq, ft = S.bow_vectors(tg, qs) if fq_ft is None else fq_ft
    n, pairs = ctx("triang", 0.6, check_orientation).match_for_triangulation(
        qs.kps(), qs.desc, fq, S.bearings(qs.n_q), tg.t_kps, tg.t_desc, ft, S.bearings(tg.n_t), S.TRI_E, S.TRI_EPIPOLE, S.SF,
        (qs.valid == 0).astype(np.uint8), None)
    out = np.full(qs.n_q, -1, np.int32)
    out[pairs[:, 0]] = pairs[:, 1]
    return n, out


def same(got, want):
    """(assignments, count), the two in either order: equal counts and equal assignments"""
    (gn, ga), (wn, wa) = (sorted(got, key=np.ndim), sorted(want, key=np.ndim))
    return int(gn) == int(wn) and np.array_equal(ga, wa)


def area_same(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


def all_rules(ctx, lib, oracle, tg, qs, rules=tuple(S.RULE_THR), fq_ft=None):
    """device == oracle under each rule's entry point; returns the oracle's match counts"""
    counts = {}
    for rule in rules:
        if rule == "projection":
            want = S.oracle_projection(oracle, tg, qs, 0.6)
            assert same(dev_projection(ctx, lib, tg, qs, 0.6), want), rule
            counts[rule] = want[1]
        elif rule == "area":
            for co in (True, False):
                want = S.oracle_area(oracle, tg, qs, 0.9, co)
                assert area_same(dev_area(ctx, lib, tg, qs, 0.9, co), want), (rule, co)
            counts[rule] = want[0]
        elif rule == "bestonly":
            for co in (True, False):
                want = S.oracle_generic(oracle, tg, qs, co)
                assert same(dev_generic(ctx, lib, tg, qs, co), want), (rule, co)
            counts[rule] = want[1]
        elif rule == "bow":
            for co in (True, False):
                want = S.oracle_bow(oracle, tg, qs, 0.75, co, fq_ft)
                assert same(dev_bow(ctx, tg, qs, 0.75, co, fq_ft), want), (rule, co)
            counts[rule] = want[0]
        else:
            for co in (True, False):
                want = S.oracle_triang(oracle, tg, qs, co, fq_ft)
                assert same(dev_triang(ctx, tg, qs, co, fq_ft), want), (rule, co)
            counts[rule] = want[0]
    return counts


# ---- a. k_grid_assign: member lists in LDS | global, the raised LDS attribute, 1..16 cells per thread ---------------------------------------------------
@pytest.mark.parametrize("g,n", S.GRID_CASES, ids=["%dx%d_n%d" % (g[0], g[1], n) for g, n in S.GRID_CASES])
def test_grid_assign(match, ctx, lib, oracle, g, n):
    cols, rows = g
    w = ctx("projection", 0.6)
    for kind in S.GRID_KINDS:
        b, kps, cell = S.grid_keys(cols, rows, n, kind)
        gp, ogp = (S.make_gp(m, cols, rows, b[2], b[3], b[0], b[1]) for m in (lib, oracle))
        start, items = w.assign_keypoints_to_grid(gp, kps)
        want_start, want_items = oracle.assign_keypoints_to_grid(ogp, kps)
        assert np.array_equal(start, want_start) and np.array_equal(items, want_items), kind
        # the resident frame's grid (the same launch_grid_assign), seen through one match on it: landmarks on up to 64 of the keypoints inside
        rng = np.random.default_rng(n)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        inside = np.nonzero(cell >= 0)[0][-64:]
        lm_xy = np.stack([kps["x"][inside], kps["y"][inside]], 1).astype(np.float32).reshape(-1, 2)
        lm_level = kps["octave"][inside].astype(np.int32)
        args = (S.SF, lm_xy, lm_level, desc[inside], 3.0)
        fd = match.frame_dev(gp, kps, desc)
        got = w.match_frame_and_landmarks(None, fd, None, *args)
        want = oracle.projection_match_frame_and_landmarks(ogp, kps, desc, *args, 0.6)
        assert same(got, want), kind
        if len(inside) and n >= 1023:
            assert want[1] > 0


# ---- b. lists and scan: four queries per block, k_scan_counts' per-thread share, the last offset --------------------------------------------------------
@pytest.mark.parametrize("m", S.LISTS_M)
def test_lists_and_scan_sizes(ctx, lib, oracle, m):
    """m queries: the tail of k_window_lists' four-queries-per-block grid (m % 4 = 1, 3, 0), k_scan_counts' per = ceil(m / 1024) at 1024 | 1025 and
    2049, through the projection, area (invalid queries: above level 0) and generic modes. The last query is valid and matched: a wrong last offset
    shows."""
    lat, qs, _ = S.contended_scene(m, seed=m)
    counts = all_rules(ctx, lib, oracle, lat, qs, ("projection", "area", "bestonly"))
    want, _ = S.oracle_projection(oracle, lat, qs, 0.6)
    assert want[-1] >= 0 and qs.valid[-1] and min(counts.values()) >= 1


@pytest.mark.parametrize("n_cells", list(S.WINDOW_GRIDS))
def test_window_cell_counts(ctx, lib, oracle, n_cells):
    """Windows of exactly 63, 64, 65, 128 and 129 cells (k_window_lists takes them 64 per pass). Query 0's winner is the member of window cell 62 /
    63 (the last lane of the only pass) / 64 (the first cell of the second pass; the last cell of the 65-cell window) / 64 / 128 (the first cell of
    the third pass, the last of the window); query 1's is in cell 0; query 2 loses query 0's."""
    tg, qs, facts = S.window_scene(n_cells, seed=n_cells)
    mg = facts["margin"]
    want = S.oracle_projection(oracle, tg, qs, 0.6, float(mg))
    assert np.array_equal(want[0], facts["want"])
    assert same(dev_projection(ctx, lib, tg, qs, 0.6, float(mg)), want)
    assert area_same(dev_area(ctx, lib, tg, qs, 0.9, False, mg), S.oracle_area(oracle, tg, qs, 0.9, False, mg))
    assert same(dev_generic(ctx, lib, tg, qs, False, float(mg)), S.oracle_generic(oracle, tg, qs, False, float(mg)))


def test_single_cell_and_outside_windows(ctx, lib, oracle):
    """a window of one cell (the grid's last), and windows wholly outside the grid on each of the four sides"""
    tg, qs, facts = S.corner_scene(seed=64)
    want = S.oracle_projection(oracle, tg, qs, 0.6, 3.0)
    assert np.array_equal(want[0], facts["want"])
    assert same(dev_projection(ctx, lib, tg, qs, 0.6, 3.0), want)
    assert area_same(dev_area(ctx, lib, tg, qs, 0.9, False, 3), S.oracle_area(oracle, tg, qs, 0.9, False, 3))
    assert same(dev_generic(ctx, lib, tg, qs, False, 3.0), S.oracle_generic(oracle, tg, qs, False, 3.0))


@pytest.mark.parametrize("n_q", [255, 256, 257])
def test_bow_lists_sizes(ctx, lib, oracle, n_q):
    """k_bow_lists (256 queries per block) at 255 | 256 | 257 feature-vector entries: one node only; then four nodes of which the frame lacks one,
    with matches in the first and in the last."""
    lat, qs, _ = S.contended_scene(n_q, seed=n_q)
    counts = all_rules(ctx, lib, oracle, lat, qs, ("bow", "triang"))
    assert min(counts.values()) > n_q // 8
    nodes, absent = S.bow_nodes(n_q)
    fq_ft = S.bow_vectors(lat, qs, nodes, absent)
    all_rules(ctx, lib, oracle, lat, qs, ("bow", "triang"), fq_ft)
    _, of_target = S.oracle_bow(oracle, lat, qs, 0.75, False, fq_ft)
    matched_q = of_target[of_target >= 0]
    assert (matched_q < 5).any() and (matched_q >= n_q - 3).any()


# ---- c. resolver widths: 1 | 4 | 8 waves, competitors in one wave, in other waves of the round, in other rounds -------------------------------------------
@pytest.mark.parametrize("n_q", S.WIDTH_NQ)
@pytest.mark.parametrize("rule", list(S.RULE_THR))
def test_resolver_widths(ctx, lib, oracle, rule, n_q):
    """k_list_resolve<RULE, 1 | 4 | 8> on either side of both width switches (256 | 257, 1024 | 1025) and beyond one round of the widest (1537):
    queries 3, 4, 67, 451, 515 and 1027 compete for target 0 (under the area rule each later one steals it), queries 0..63 are a chain on it from
    256 queries on. At least a quarter of the queries is matched and a quarter loses the target it prefers (tests/test_window_edge_shapes.py)."""
    lat, qs, _ = S.contended_scene(n_q, seed=n_q)
    counts = all_rules(ctx, lib, oracle, lat, qs, (rule,))
    assert 4 * counts[rule] >= n_q


# ---- d. the stamp table's collisions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["projection", "area", "bestonly"])
def test_stamp_table_collisions(ctx, lib, oracle, rule):
    """8200 targets: t, t + 4096 and t + 8192 are co-located and share a slot of the 4096-entry stamp table, and queries of one 64-query window
    prefer different members of one site. A stamp of the wrong member may cost a round, never a different match."""
    lat, qs = S.collision_scene(COLLISION_NQ, seed=3)
    assert S.congruent_pairs(qs) >= 64
    counts = all_rules(ctx, lib, oracle, lat, qs, (rule,))
    assert 4 * counts[rule] >= qs.n_q


# ---- e. list bounds and keys in or out of LDS -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def key_pools():
    rows = [S.resolve_row(*s[:2]) for s in S.LDS_SHAPES]
    ans = S.plan(rows)
    return {s[:2]: S.resolve_form(ans[r]) for s, r in zip(S.LDS_SHAPES, rows)}


# (3 x key_pool entries do not exist at 1000 x 1000 with lists of 18: the large shapes only)
LDS_CASES = [(s, d) for s in S.LDS_SHAPES for d in S.LDS_DELTAS + (["3x"] if s[2] == 2000 else [])]


@pytest.mark.parametrize("shape,delta", LDS_CASES, ids=["q%d_t%d_%s" % (s[0], s[1], d) for s, d in LDS_CASES])
def test_keys_and_bounds_in_or_out_of_lds(ctx, lib, oracle, key_pools, shape, delta):
    """n_keys = key_pool - 1 | key_pool (the last copy into LDS) | key_pool + 1 | key_pool + 4 (keys read from global memory): every residue of
    the uint4 copy's tail; and about 3 x key_pool. At 12 295 queries the list bounds are staged in LDS, at 12 296 they are read from global memory
    (the plan says so in tests/test_window_edge_shapes.py); the small shape has lists of 17 and 18 candidates."""
    offsets_in_lds, key_pool, _ = key_pools[shape[:2]]
    assert offsets_in_lds == (0 if shape[0] == 12296 else 1)
    (lat, qs), n_keys = S.lds_edge_case(shape, delta, key_pool)
    assert qs.n_keys(S.dead_from(S.THR_HIGH, S.LDS_RATIO)) == n_keys
    want = S.oracle_projection(oracle, lat, qs, S.LDS_RATIO)
    assert same(dev_projection(ctx, lib, lat, qs, S.LDS_RATIO), want) and want[1] > 100 and want[0][-1] >= 0


# ---- f. dead_from and the rules' edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr,ratio", S.RULE_EDGE)
def test_dead_from_and_rule_edges(ctx, lib, oracle, thr, ratio):
    """best at thr - 1 | thr | thr + 1 with the second at dead_from - 2 .. dead_from + 1, 255, 256 or absent, before and behind the best, in the
    same and (projection) in the other level; equal distances; d = 0 and d = 256: one call per (rule threshold, ratio)."""
    projection = thr == S.THR_HIGH
    tg, qs, _ = S.rule_edge_scene(thr, ratio, projection)
    if projection:
        want = S.oracle_projection(oracle, tg, qs, ratio)
        assert same(dev_projection(ctx, lib, tg, qs, ratio), want)
        n = want[1]
    else:
        want = S.oracle_area(oracle, tg, qs, ratio, False)
        assert area_same(dev_area(ctx, lib, tg, qs, ratio, False), want)
        n = want[0]
    assert 0 < n < qs.n_q


# ---- k_cross_check -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(63, 100), (64, 63), (65, 64), (255, 300), (256, 255), (257, 256)])
def test_cross_check_sizes(ctx, lib, oracle, n1, n2):
    """projection::match_keyframes_mutually on the lattice (identity poses, landmark (u, v, 1) -> pixel (u, v)): k_cross_check sums the matches per
    wave by ballot, at n1 around one wave and around one block, n2 != n1. A fifth of keyframe 2's landmarks do not find their way back."""
    n = max(n1, n2)
    lat = S.Lattice(n, n, seed=n1)
    rng = lat.rng
    q1 = lat.queries(rng.permutation(n)[:n1], rng.integers(0, 30, n1), np.ones(n1))   # keyframe 1's keypoints, each on a site of its own
    k2, d2 = lat.t_kps[:n2], lat.t_desc[:n2]
    k1, d1 = q1.kps(), q1.desc
    l1 = d1.copy()                                                                    # landmark descriptors: the keypoint's own ...
    l2 = d2.copy()
    wrong = rng.random(n2) < 0.2
    l2[wrong] = rng.integers(0, 256, (int(wrong.sum()), 32), dtype=np.uint8)          # ... or, for some of keyframe 2's, something else
    X1 = S.generic_points(q1)
    X2 = np.concatenate([np.stack([k2["x"], k2["y"]], 1).astype(np.float64), np.ones((n2, 1))], 1)

    def ranges(X):
        dist = np.linalg.norm(X, axis=1)
        return np.ascontiguousarray(np.stack([0.9 * dist, dist], 1), np.float32)

    v1, v2 = (rng.random(n1) < 0.9).astype(np.uint8), (rng.random(n2) < 0.9).astype(np.uint8)
    lsf = float(np.log(np.float32(1.2)))
    args = (k1, d1, S.IDENTITY, X1, ranges(X1), l1, v1, k2, d2, S.IDENTITY, X2, ranges(X2), l2, v2, 1.0, np.eye(3), np.zeros(3), S.SF, lsf, 3.0)
    gn, got = ctx("projection", 0.9).match_keyframes_mutually(S.generic_camera(lib, lat), lat.gp(lib), *args)
    wn, want = oracle.projection_match_keyframes_mutually(S.generic_camera(oracle, lat), lat.gp(oracle), *args)
    assert gn == wn and np.array_equal(got, want)
    assert 0 < wn < min(n1, n2) and wn > min(n1, n2) // 4
