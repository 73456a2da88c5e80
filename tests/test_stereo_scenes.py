"""The constructed stereo scenes (tests/stereo_scenes.py) on the CPU: the C oracle and the numpy restatement of rule 20 agree bit for bit on every
scene under all four variant combinations, and the trace of the restatement shows that every scene still reaches the edges it was built for. This
is the gate that the inputs are right before any kernel sees them (tests/test_gpu_stereo.py runs the same scenes on the device)."""
import numpy as np
import pytest

import nversion_numpy as nv
import stereo_scenes as ss
from stereo_scenes import SCENE_NAMES, VARIANTS


@pytest.fixture(scope="module")
def runs(oracle):
    """Per scene: the oracle extractors (for their pyramids), and per variant the oracle's result and the restatement's result with its trace."""
    out = {}
    for s in ss.scenes_from(oracle):
        oxl, oxr = oracle.OrbExtractor(oracle.make_params(**s.orb_params)), oracle.OrbExtractor(oracle.make_params(**s.orb_params))
        oxl.extract(s.left)
        oxr.extract(s.right)
        tabs = oracle.orb_tables(oxl.params)
        n = oxl.params.num_levels
        pyr_l, pyr_r = [oxl.level_image(l) for l in range(n)], [oxr.level_image(l) for l in range(n)]
        res = {}
        for f21, pdbl in VARIANTS:
            want = oracle.stereo_compute(oxl, oxr, s.kps_left, s.desc_left, s.kps_right, s.desc_right, s.focal_x_baseline, s.true_baseline,
                                         outlier_factor_21=f21, parabola_double=pdbl)
            got = nv.stereo_compute(pyr_l, pyr_r, s.kps_left, s.desc_left, s.kps_right, s.desc_right, tabs["scale_factors"], tabs["inv_scale_factors"],
                                    s.focal_x_baseline, s.true_baseline, 2.1 if f21 else 2.0, pdbl, trace=True)
            res[(f21, pdbl)] = (want, got)
        out[s.name] = (s, pyr_l, res)
    return out


def test_scene_list(oracle):
    scenes = ss.scenes_from(oracle)
    assert tuple(s.name for s in scenes) == SCENE_NAMES
    for s in scenes:
        assert s.left.shape == s.right.shape == (ss.ROWS, ss.COLS) and s.left.dtype == s.right.dtype == np.uint8
        assert len(s.kps_left) == len(s.desc_left) and len(s.kps_right) == len(s.desc_right)
        assert len(s.kps_left) <= 3000, s.name
        assert len(s.kps_right) <= 3000 or s.name == "wide"
    wide = scenes[SCENE_NAMES.index("wide")]
    assert len(wide.kps_right) == 65535 and len(wide.kps_left) <= 16


def test_level_zero_is_the_image(runs):
    for s, pyr_l, _ in runs.values():
        assert np.array_equal(pyr_l[0], s.left), s.name


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_oracle_equals_restatement(runs, name):
    s, _, res = runs[name]
    for v, ((wx, wd, wn), (gx, gd, tr)) in res.items():
        assert np.array_equal(gx.view(np.uint32), wx.view(np.uint32)) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (name, v)
        assert wn == int((tr["code"] == nv.ST_ACCEPTED).sum()) == int((wx >= 0).sum()), (name, v)
        assert np.array_equal(wx >= 0, wd > 0)
        assert not (tr["code"] == nv.ST_DELTA).any()          # unreachable: delta lies in [-0.5, 0.5]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_probes_reach_their_edge(runs, name):
    s, _, res = runs[name]
    tr = res[(False, False)][1][2]
    for label, (il, code, checks) in s.probes.items():
        t = tr[il]
        if code is not None:
            assert t["code"] == code, (name, label, int(t["code"]), code)
        for field, value in checks.items():
            assert np.array_equal(np.asarray(t[field]), np.asarray(value, t[field].dtype)), (name, label, field, t[field], value)
    passed = np.isin(tr["code"], (nv.ST_ACCEPTED, nv.ST_DROPPED))
    dist = np.sort(tr["costs"][passed, tr["shift"][passed]]).astype(np.int64) if passed.any() else np.zeros(0, np.int64)
    if "count" in s.notes:
        assert int(passed.sum()) == s.notes["count"]
    if "distances" in s.notes:
        assert dist.tolist() == list(s.notes["distances"])
    if "min_accepted" in s.notes:
        assert int(passed.sum()) >= s.notes["min_accepted"]
    if s.notes.get("factor_matters"):
        a, b = res[(False, False)][0], res[(True, False)][0]
        assert b[2] > a[2] and not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _accepted(tr):
    return np.isin(tr["code"], (nv.ST_ACCEPTED, nv.ST_DROPPED))


def test_census(runs):
    """What the issue lists as never reached by the noise scenes, counted over the whole scene set (default variant)."""
    traces = {name: r[2][(False, False)][1][2] for name, r in runs.items()}
    tr = np.concatenate(list(traces.values()))
    codes = set(tr["code"].tolist())
    assert codes == set(range(nv.ST_DELTA)), codes                  # every outcome but the unreachable delta gate
    ok = _accepted(tr)
    k = tr["shift"][ok]
    c = tr["costs"][ok]
    rows = np.arange(len(k))
    c1, c2, c3 = c[rows, k - 1], c[rows, k], c[rows, k + 1]
    assert (c1 > c2).all() and (c3 >= c2).all() and (np.abs(tr["delta"][ok]) <= 0.5).all()
    assert (c3 == c2).any() and (c2 == 0).any() and (c2 >= 32768).any() and (k == 1).any() and (k == 9).any()
    assert (tr["code"][tr["shift"] == 0] == nv.ST_END_SHIFT).all() and (tr["shift"] == 0).any() and (tr["shift"] == 10).any()
    searched = tr["shift"] >= 0
    assert (tr["costs"][searched].max(1) == 0).any()                                         # an all-constant window pair
    later = [(t["costs"] == t["costs"][t["shift"]]).sum() > 1 and t["costs"][t["shift"] + 2:].min() == t["costs"][t["shift"]]
             for t in tr[ok]]
    assert any(later)                                                                        # equal minima two or more shifts apart: the first one was taken
    assert (tr["clamped"] & (tr["disp"] == 0)).any() and (tr["code"] == nv.ST_DISP_NEGATIVE).any()
    assert {0, 74, 75} <= set(tr["best_hamming"].tolist()) and tr["hamming_ties"].max() >= 32
    assert (tr["half"] & ok).any()
    # the outlier pass: accepted counts 0, 1, 2, an odd and an even one >= 5, more than 2048
    counts = {name: int(_accepted(t).sum()) for name, t in traces.items()}
    assert {0, 1, 2} <= set(counts.values()) and max(counts.values()) > 2048
    assert any(n >= 5 and n % 2 for n in counts.values()) and any(n >= 5 and n % 2 == 0 for n in counts.values())
    big = traces["big"]
    assert ((big["code"] == nv.ST_ACCEPTED) & (big["costs"][:, 5] >= 32768)).sum() >= 1
    # row bands of the right keypoints
    e = runs["edges"][0]
    band = np.float32(2.0) * np.float32(1.0)
    y0 = e.kps_right["y"][e.kps_right["octave"] == 0]
    assert (np.floor(y0 - band) < 0).any() and (np.ceil(y0 + band) > ss.ROWS - 1).any()
    assert ((y0 - band == np.floor(y0 - band)) & (y0 + band == np.ceil(y0 + band))).any()
    ly = e.kps_left["y"]
    assert ((ly > -1) & (ly < 0)).any() and (ly >= ss.ROWS).any()
    et = traces["edges"]
    assert ((et["code"] == nv.ST_NO_ROW_CANDIDATES) & (ly >= 0) & (ly < ss.ROWS)).any()
    disp = et["disp"][et["code"] == nv.ST_ACCEPTED]
    assert ((disp < ss.EDGE_MAX_DISP) & (disp >= ss.EDGE_MAX_DISP - 1)).any() and (et["disp"][et["code"] == nv.ST_DISP_MAX] >= ss.EDGE_MAX_DISP).all()
