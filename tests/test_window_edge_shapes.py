"""The shapes of tests/test_gpu_window_edges.py without a device. (1) For every shape that file runs, the host plan program
(tests/match_window_plan_host.cc) is asked which launch form the shape takes, and the answer is held to the form the shape was chosen for: "this GPU
test runs the global-bounds form" is checked here, and stays true when the plan's constants move (the test fails and the shape is chosen again).
(2) Every scene of tests/window_edge_scenes.py is held to the facts it was built to have, from the constructed arrays and the CPU oracle alone."""
import numpy as np
import pytest

import window_edge_scenes as S


@pytest.fixture(scope="module")
def plans():
    rows = [S.grid_row(n, g[0] * g[1]) for g, n in S.GRID_CASES]
    rows += [S.resolve_row(n_q, n_t) for n_q, n_t in RESOLVE_FORMS]
    return S.plan(rows)


# ---- (1) launch forms ---------------------------------------------------------------------------------------------------------------------------------
def intended_grid_form(g, n):
    """(items_in_lds, raise_attr) the case was chosen for"""
    special = {((64, 64), 8191): (1, 0),      # exactly the 64 KiB a kernel gets without the attribute, lists in LDS
               ((64, 64), 8192): (1, 1),      # four bytes more: the attribute, lists still in LDS
               ((128, 128), 4095): (1, 1),    # the last LDS form at the largest grid
               ((128, 128), 4096): (0, 1)}    # the first global one, the attribute still raised for histogram and starts
    return special.get((g, n), (1 if n <= 8192 else 0, 0))


@pytest.mark.parametrize("g,n", S.GRID_CASES, ids=["%dx%d_n%d" % (g[0], g[1], n) for g, n in S.GRID_CASES])
def test_grid_launch_form(plans, g, n):
    form = S.grid_form(plans[S.grid_row(n, g[0] * g[1])])
    print("grid %d x %d, n = %d: items_in_lds = %d, raise_attr = %d" % (g[0], g[1], n, form[0], form[1]))
    assert form == intended_grid_form(g, n)


def test_grid_cases_cover_every_form_and_ownership():
    forms = {intended_grid_form(g, n) for g, n in S.GRID_CASES}
    assert forms == {(1, 0), (0, 0), (1, 1), (0, 1)}
    per = {-(-(g[0] * g[1]) // 1024) for g, _ in S.GRID_CASES}   # cells per thread of the scan
    assert per == {1, 2, 3, 4, 16}


# (n_q, n_t) -> (offsets_in_lds, width) intended; key_pool is read from the plan where a test needs it
COLLISION_NQ = 1280
RESOLVE_FORMS = {}
for _n_q in S.WIDTH_NQ:
    RESOLVE_FORMS[(_n_q, 2 * (_n_q // 3 + 2))] = (1, 0 if _n_q <= 256 else (1 if _n_q <= 1024 else 2))
for _m in S.LISTS_M:
    RESOLVE_FORMS[(_m, 2 * (_m // 3 + 2))] = (1, 0 if _m <= 256 else (1 if _m <= 1024 else 2))
RESOLVE_FORMS[(COLLISION_NQ, 8200)] = (1, 2)
RESOLVE_FORMS[(12295, 2000)] = (1, 2)    # the last shape with the list bounds in LDS
RESOLVE_FORMS[(12296, 2000)] = (0, 2)    # the first that reads them from global memory
RESOLVE_FORMS[(1000, 1000)] = (1, 1)


@pytest.mark.parametrize("n_q,n_t", list(RESOLVE_FORMS), ids=["q%d_t%d" % k for k in RESOLVE_FORMS])
def test_resolver_launch_form(plans, n_q, n_t):
    offsets_in_lds, key_pool, width = S.resolve_form(plans[S.resolve_row(n_q, n_t)])
    print("resolve n_q = %d, n_t = %d: offsets_in_lds = %d, key_pool = %d, waves = %d" % (n_q, n_t, offsets_in_lds, key_pool, (1, 4, 8)[width]))
    assert (offsets_in_lds, width) == RESOLVE_FORMS[(n_q, n_t)]


def test_width_switches_are_adjacent(plans):
    w = {n_q: S.resolve_form(plans[S.resolve_row(n_q, 2 * (n_q // 3 + 2))])[2] for n_q in (256, 257, 1024, 1025)}
    assert (w[256], w[257], w[1024], w[1025]) == (0, 1, 1, 2)


# ---- (2) scene facts ------------------------------------------------------------------------------------------------------------------------------------
def per_query(rule, oracle, lat, qs, ratio=None):
    """the oracle's assignment per query, and its match count, under the rule's entry point"""
    if rule == "projection":
        a, n = S.oracle_projection(oracle, lat, qs, 0.6 if ratio is None else ratio)
    elif rule == "area":
        n, a, _ = S.oracle_area(oracle, lat, qs, 0.9 if ratio is None else ratio, True)
    elif rule == "bestonly":
        a, n = S.oracle_generic(oracle, lat, qs, True)
    elif rule == "bow":
        n, of_target = S.oracle_bow(oracle, lat, qs, 0.75, True)
        a = np.full(qs.n_q, -1, np.int32)
        a[of_target[of_target >= 0]] = np.nonzero(of_target >= 0)[0]
    else:
        n, a = S.oracle_triang(oracle, lat, qs, True)
    assert n == int((a >= 0).sum())
    return a, n


@pytest.mark.parametrize("n_q", S.WIDTH_NQ)
@pytest.mark.parametrize("rule", list(S.RULE_THR))
def test_width_scene_facts(oracle, rule, n_q):
    lat, qs, facts = S.contended_scene(n_q, seed=n_q)
    a, n = per_query(rule, oracle, lat, qs)
    lost = S.preferred_owner_lost(qs, a, S.RULE_THR[rule])
    assert 4 * n >= n_q and 4 * int(lost.sum()) >= n_q, (n, int(lost.sum()))
    best = np.array([int(np.argmin(S.hamming(qs.desc[q], lat.t_desc))) for q in np.unique(facts["pairs"])])
    assert (best == 0).all() and facts["pairs"][0] == (3, 4)
    assert a[-1] >= 0 and qs.valid[-1]
    if n_q >= 256:
        assert len(facts["chain"]) == 64 and (qs.pref[facts["chain"]] == 0).all() and (np.diff(facts["chain"]) == 1).all()
    if rule == "area":   # every named later query is strictly nearer than the earlier owner: it steals; the last of them holds target 0
        assert all(qs.noise[b] < qs.noise[a_] for a_, b in facts["steals"])
        assert a[facts["steals"][-1][1]] == 0 and (a[[q for q, _ in facts["steals"]]] != 0).all()
    else:                # sequential claim: one of the queries that prefer target 0 holds it, and it is not the last of them
        holder = np.nonzero(a == 0)[0]
        assert len(holder) == 1 and qs.pref[holder[0]] == 0 and holder[0] < np.nonzero(qs.pref == 0)[0][-1]


@pytest.mark.parametrize("rule", ["projection", "area", "bestonly"])
def test_collision_scene_facts(oracle, rule):
    lat, qs = S.collision_scene(COLLISION_NQ, seed=3)
    assert lat.n_t == 8200 and S.congruent_pairs(qs) >= 64
    assert (lat.t_site[:8] == lat.t_site[8192:]).all() and (lat.t_site[:4096] == lat.t_site[4096:8192]).all()
    a, n = per_query(rule, oracle, lat, qs)
    assert 4 * n >= qs.n_q and (a[a >= 0] >= 4096).sum() > 100 and (a[a >= 0] < 4096).sum() > 100 and (a >= 8192).any()


@pytest.mark.parametrize("shape", S.LDS_SHAPES, ids=["q%d_t%d" % s[:2] for s in S.LDS_SHAPES])
def test_lds_edge_key_counts(oracle, shape):
    key_pool = S.resolve_form(S.plan([S.resolve_row(*shape[:2])])[S.resolve_row(*shape[:2])])[1]
    dead = S.dead_from(S.THR_HIGH, S.LDS_RATIO)
    for delta in S.LDS_DELTAS + (["3x"] if shape[2] == 2000 else []):
        (lat, qs), n_keys = S.lds_edge_case(shape, delta, key_pool)
        assert qs.n_keys(dead) == n_keys and qs.valid[-1]
        if delta == "3x":
            assert n_keys > 2.9 * key_pool
        a, n = S.oracle_projection(oracle, lat, qs, S.LDS_RATIO)
        assert n > 100 and a[-1] >= 0 and (qs.site[:-1][qs.valid[:-1] != 0] != qs.site[-1]).all()


@pytest.mark.parametrize("n_cells", list(S.WINDOW_GRIDS))
def test_window_scene_facts(oracle, n_cells):
    tg, qs, facts = S.window_scene(n_cells, seed=n_cells)
    assert tg.gp_args[0] * tg.gp_args[1] == n_cells == tg.n_t
    # target index == cell id: the grid lists one member per cell, in order
    start, items = oracle.assign_keypoints_to_grid(tg.gp(oracle), tg.t_kps)
    assert np.array_equal(start, np.arange(n_cells + 1)) and np.array_equal(items, np.arange(n_cells))
    a, n = S.oracle_projection(oracle, tg, qs, 0.6, float(facts["margin"]))
    assert np.array_equal(a, facts["want"]) and n == 2
    n2, a2, _ = S.oracle_area(oracle, tg, qs, 0.9, False, facts["margin"])
    assert np.array_equal(a2, facts["want"]) and n2 == 2
    a3, n3 = S.oracle_generic(oracle, tg, qs, False, float(facts["margin"]))
    assert np.array_equal(a3, facts["want"]) and n3 == 2


def test_corner_scene_facts(oracle):
    tg, qs, facts = S.corner_scene(seed=64)
    a, n = S.oracle_projection(oracle, tg, qs, 0.6, float(facts["margin"]))
    assert np.array_equal(a, facts["want"]) and n == 1
    # the single-cell window, restated: get_keypoints_in_cell's cell range for query 0
    x, r, inv = np.float32(116.0), np.float32(3.0), np.float32(8.0 / 128.0)
    assert int(np.floor((x - r) * inv)) == 7 and min(7, int(np.ceil((x + r) * inv))) == 7


@pytest.mark.parametrize("thr,ratio", S.RULE_EDGE)
def test_rule_edge_scene_facts(oracle, thr, ratio):
    projection = thr == S.THR_HIGH
    tg, qs, cases = S.rule_edge_scene(thr, ratio, projection)
    assert 40 < qs.n_q < 400
    if projection:
        a, n = S.oracle_projection(oracle, tg, qs, ratio)
    else:
        n, a, _ = S.oracle_area(oracle, tg, qs, ratio, False)
    assert 0 < n < qs.n_q                        # accepts and rejects
    first = np.cumsum([0] + [len(c[0]) for c in cases])
    for i, (ds, _) in enumerate(cases):          # whatever is accepted is the first of the nearest candidates, and within the threshold
        if a[i] >= 0:
            assert a[i] == first[i] + int(np.argmin(ds)) and min(ds) <= thr
    # both sides of the dead_from edge occur as a second (where the distance exists)
    dead = S.dead_from(thr, ratio)
    seconds = {d for ds, _ in cases for d in ds}
    assert {dead - 1, dead} <= seconds and {thr - 1, thr, thr + 1, 0, 256} <= seconds


@pytest.mark.parametrize("g,n", S.GRID_CASES, ids=["%dx%d_n%d" % (g[0], g[1], n) for g, n in S.GRID_CASES])
def test_grid_key_set_facts(oracle, g, n):
    cols, rows = g
    for kind in S.GRID_KINDS:
        b, kps, cell = S.grid_keys(cols, rows, n, kind)
        counts = np.bincount(cell[cell >= 0], minlength=cols * rows)
        assert counts.max(initial=0) <= S.MAX_PER_CELL
        if n >= 1023:
            if cols * rows == 1:
                assert counts[0] >= 1 and (cell < 0).any()
            else:
                assert (counts > 0).sum() >= 2
            for side in (kps["x"] < b[0], kps["x"] > b[2], kps["y"] < b[1], kps["y"] > b[3]):
                assert side.any()
        if kind == "ties" and n >= 1023 and cols >= 2:
            fx = (kps["x"].astype(np.float64) - b[0]) / 8.0
            half = fx - np.floor(fx) == 0.5
            assert (half & (np.floor(fx) % 2 == 0)).any() and (half & (np.floor(fx) % 2 == 1)).any()   # rounds down | rounds up
        if kind == "negmin":
            assert b[0] < 0 and b[1] < 0
        start, items = oracle.assign_keypoints_to_grid(S.make_gp(oracle, cols, rows, b[2], b[3], b[0], b[1]), kps)
        want_start, want_items = S.grid_reference(cols, rows, cell)
        assert np.array_equal(start, want_start) and np.array_equal(items, want_items)


@pytest.mark.parametrize("n_q", [255, 256, 257])
def test_bow_node_scene_facts(oracle, n_q):
    lat, qs, _ = S.contended_scene(n_q, seed=n_q)
    nodes, absent = S.bow_nodes(n_q)
    fq, ft = S.bow_vectors(lat, qs, nodes, absent)
    assert sorted(fq) == [2, 4, 7, 9] and sorted(ft) == [2, 7, 9]
    n, of_target = S.oracle_bow(oracle, lat, qs, 0.75, False, (fq, ft))
    matched_q = of_target[of_target >= 0]
    assert ((matched_q < 5).any() and (matched_q >= n_q - 3).any() and not ((matched_q >= 5) & (matched_q < 9)).any())   # first, last, absent node
    n1, _ = S.oracle_bow(oracle, lat, qs, 0.75, False)
    assert n1 >= n
