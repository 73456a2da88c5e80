"""GPU parity: match::stereo::compute through the C ABI == CPU oracle. Float outputs (stereo_x_right, depths) are compared by
bit pattern: every float operation of the path is individually rounded on both sides (tolerance 0 ulp)."""
import ctypes as C

import numpy as np
import pytest

import nversion_numpy as nv
import stereo_scenes as ss
from stereo_scenes import SCENE_NAMES, VARIANTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from openvslam_amd import feature, match, synth
    return feature, match, synth


@pytest.mark.parametrize("rows,cols,nfeat,seed", [(376, 1241, 2000, 1), (376, 1241, 2000, 2), (240, 400, 500, 3)])
def test_stereo_compute_kitti_geometry(mods, oracle, rows, cols, nfeat, seed):
    """BASELINE config 3: 1241x376 rectified pair, 2000 features per image, focal_x_baseline 386.1448 (KITTI 00-02)."""
    feature, match, synth = mods
    left, right, _ = synth.synth_stereo_pair(rows, cols, seed=seed)
    el = feature.orb_extractor(feature.orb_params(nfeat), max_rows=rows, max_cols=cols)
    er = feature.orb_extractor(feature.orb_params(nfeat), max_rows=rows, max_cols=cols)
    kl, dl = el.extract(left)
    kr, dr = er.extract(right)
    oxl, oxr = oracle.OrbExtractor(oracle.make_params(nfeat)), oracle.OrbExtractor(oracle.make_params(nfeat))
    wkl, wdl = oxl.extract(left)
    wkr, wdr = oxr.extract(right)
    assert np.array_equal(kl.view(np.uint8), wkl.view(np.uint8)) and np.array_equal(dr, wdr)
    for fxb, b in ((386.1448, 0.5372), (60.0, 1.0)):   # second: max_disp = 60 px cuts the disparity window
        st = match.stereo(el, er, kl, dl, kr, dr, fxb, b)
        xr, dp = st.compute()
        wxr, wdp, wn = oracle.stereo_compute(oxl, oxr, wkl, wdl, wkr, wdr, fxb, b)
        assert st.num_valid_ == wn
        assert np.array_equal(xr.view(np.uint32), wxr.view(np.uint32)) and np.array_equal(dp.view(np.uint32), wdp.view(np.uint32))
        # ORACLE_SPEC rule 20's two L-tagged choices as run-time variants of BOTH sides: bit-equal in every setting, and not no-ops
        changed = 0
        for f21, pdbl in ((True, False), (False, True), (True, True)):
            st.set_variant("outlier_factor", int(f21))
            st.set_variant("parabola", int(pdbl))
            vxr, vdp = st.compute()
            oxr_, odp_, on = oracle.stereo_compute(oxl, oxr, wkl, wdl, wkr, wdr, fxb, b, outlier_factor_21=f21, parabola_double=pdbl)
            assert st.num_valid_ == on and np.array_equal(vxr.view(np.uint32), oxr_.view(np.uint32)) and np.array_equal(vdp.view(np.uint32), odp_.view(np.uint32))
            changed += not np.array_equal(vxr.view(np.uint32), xr.view(np.uint32))
            if f21 and not pdbl:
                assert on >= wn   # a larger factor keeps at least as many matches
        st.set_variant("outlier_factor", 0)
        st.set_variant("parabola", 0)
        assert changed >= 1
    assert wn > len(kl) // 10


def test_stereo_synthetic_keypoints_edge_cases(mods, oracle):
    """Keypoints placed by hand near the image borders / far octaves: exercises the window range checks and the octave filter
    (the extractor itself never emits such keypoints)."""
    feature, match, synth = mods
    rows, cols = 240, 400
    left, right, _ = synth.synth_stereo_pair(rows, cols, seed=9)
    el = feature.orb_extractor(feature.orb_params(300), max_rows=rows, max_cols=cols)
    er = feature.orb_extractor(feature.orb_params(300), max_rows=rows, max_cols=cols)
    kl, dl = el.extract(left)
    kr, dr = er.extract(right)
    oxl, oxr = oracle.OrbExtractor(oracle.make_params(300)), oracle.OrbExtractor(oracle.make_params(300))
    oxl.extract(left)
    oxr.extract(right)
    rng = np.random.default_rng(0)
    kl, kr = kl.copy(), kr.copy()
    kl["x"][:20] = rng.uniform(0, 12, 20)           # left windows that leave the image
    kr["x"][:20] = rng.uniform(0, 14, 20)           # right windows that leave the image
    kr["x"][20:40] = cols - rng.uniform(0, 14, 20)
    kl["octave"][40:60] = 7                          # octave gaps > 1
    dr[:60] = dl[:60]                                # make them attractive matches
    kr["y"][:60] = kl["y"][:60]
    st = match.stereo(el, er, kl, dl, kr, dr, 386.1448, 0.5372)
    xr, dp = st.compute()
    wxr, wdp, wn = oracle.stereo_compute(oxl, oxr, kl, dl, kr, dr, 386.1448, 0.5372)
    assert st.num_valid_ == wn
    assert np.array_equal(xr.view(np.uint32), wxr.view(np.uint32)) and np.array_equal(dp.view(np.uint32), wdp.view(np.uint32))


# ---- constructed scenes (tests/stereo_scenes.py; tests/test_stereo_scenes.py proves on the CPU that each reaches its edges) ----------------------------------
ERR_INVALID, ERR_CAPACITY = -1, -4
ROWS, COLS = ss.ROWS, ss.COLS


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pair(mods):
    """Two device extractors for 240 x 400 images with the scenes' orb_params, shared by the tests below."""
    feature = mods[0]
    return tuple(feature.orb_extractor(feature.orb_params(**ss.ORB_PARAMS), max_rows=ROWS, max_cols=COLS) for _ in range(2))


@pytest.fixture(scope="module")
def oracle_pair(oracle):
    return oracle.OrbExtractor(oracle.make_params(**ss.ORB_PARAMS)), oracle.OrbExtractor(oracle.make_params(**ss.ORB_PARAMS))


def _extract_both(pair, oracle_pair, left, right, levels=range(ss.ORB_PARAMS["num_levels"])):
    """Both images through the device extractors and the oracle's; the device pyramids must be the oracle's (a mismatch here is the extractor's, not
    the matcher's). Returns the device extractors' outputs."""
    (el, er), (oxl, oxr) = pair, oracle_pair
    out = el.extract(left), er.extract(right)
    oxl.extract(left)
    oxr.extract(right)
    for lvl in levels:
        assert np.array_equal(el.image_pyramid(lvl), oxl.level_image(lvl)) and np.array_equal(er.image_pyramid(lvl), oxr.level_image(lvl)), lvl
    return out


def _raw_compute(st, el, er, kl, dl, kr, dr, fxb, b):
    """ovs_stereo_compute on st's handle with any extractors and arrays: (status, stereo_x_right, depths, n_valid)."""
    from openvslam_amd import _lib
    from openvslam_amd.match import KP_DTYPE, _p
    kl, kr = np.ascontiguousarray(kl, KP_DTYPE), np.ascontiguousarray(kr, KP_DTYPE)
    dl, dr = np.ascontiguousarray(dl, np.uint8).reshape(-1, 32), np.ascontiguousarray(dr, np.uint8).reshape(-1, 32)
    xr, dp = np.full(max(len(kl), 1), -7, np.float32), np.full(max(len(kl), 1), -7, np.float32)
    nv = C.c_int32(-7)
    rc = _lib.lib().ovs_stereo_compute(st._h, el._h, er._h, _p(kl), _p(dl), len(kl), _p(kr), _p(dr), len(kr), fxb, b, _p(xr), _p(dp), C.byref(nv))
    return rc, xr[:len(kl)], dp[:len(kl)], nv.value


def _assert_equals_oracle(got, oracle, oracle_pair, kl, dl, kr, dr, fxb, b, f21=False, pdbl=False):
    rc, xr, dp, nv = got
    wxr, wdp, wn = oracle.stereo_compute(oracle_pair[0], oracle_pair[1], kl, dl, kr, dr, fxb, b, outlier_factor_21=f21, parabola_double=pdbl)
    assert rc == 0 and nv == wn, (rc, nv, wn)
    assert np.array_equal(_bits(xr), _bits(wxr)) and np.array_equal(_bits(dp), _bits(wdp)), (np.nonzero(_bits(xr) != _bits(wxr))[0][:8], nv, wn)
    return wxr, wdp, wn


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_stereo_constructed_scene(mods, oracle, pair, oracle_pair, name):
    """HIP == oracle on every constructed scene: stereo_x_right and depths bit for bit and num_valid_, under all four variant combinations."""
    match = mods[1]
    s = ss.scenes_from(oracle)[SCENE_NAMES.index(name)]
    _extract_both(pair, oracle_pair, s.left, s.right)
    st = match.stereo(pair[0], pair[1], s.kps_left, s.desc_left, s.kps_right, s.desc_right, s.focal_x_baseline, s.true_baseline,
                      max_keypoints=s.notes.get("max_keypoints", 8192))
    results = []
    for f21, pdbl in VARIANTS:
        st.set_variant("outlier_factor", int(f21))
        st.set_variant("parabola", int(pdbl))
        xr, dp = st.compute()
        want = _assert_equals_oracle((0, xr, dp, st.num_valid_), oracle, oracle_pair, s.kps_left, s.desc_left, s.kps_right, s.desc_right,
                                     s.focal_x_baseline, s.true_baseline, f21, pdbl)
        results.append(want)
    if s.notes.get("factor_matters"):
        assert results[1][2] > results[0][2]
    if "count" in s.notes:      # what the median rule saw (kept + dropped) is the scene's count; the kept ones are the probes built as accepted
        kept = sorted(il for il, code, _ in s.probes.values() if code == nv.ST_ACCEPTED)
        assert np.nonzero(results[0][0] >= 0)[0].tolist() == kept


@pytest.fixture(scope="module")
def dense_lists(oracle):
    """The `dense` scene's keypoints, with every second left keypoint (`alternate`) or every second run of 16, the first included (`runs`), given a
    fresh random descriptor: unmatched, so its 16 lanes -- or a whole block of the sub-pixel kernel, whole waves of both kernels -- idle."""
    s = ss.scenes_from(oracle)[SCENE_NAMES.index("dense")]
    rng = np.random.default_rng(77)
    i = np.arange(len(s.kps_left))
    lists = {}
    for key, off in (("alternate", i % 2 == 1), ("runs", (i // 16) % 2 == 0)):
        d = s.desc_left.copy()
        d[off] = rng.integers(0, 256, (int(off.sum()), 32), dtype=np.uint8)
        lists[key] = d
    return s, lists


@pytest.mark.parametrize("pattern", ["alternate", "runs"])
def test_stereo_size_edges(mods, oracle, pair, oracle_pair, dense_lists, pattern):
    """n_left around 16 (lanes per keypoint group), 64, 256 (block of the match kernel) and 1024 (stride of the one-block loops), then n_right at 1 and
    around 1024, on a textured scene with matched and unmatched keypoints interleaved."""
    match = mods[1]
    s, lists = dense_lists
    dl = lists[pattern]
    _extract_both(pair, oracle_pair, s.left, s.right, levels=(0, 1, 2))
    st = match.stereo(pair[0], pair[1], s.kps_left[:1], dl[:1], s.kps_right, s.desc_right, *ss.KITTI)
    matched = 0
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        args = (s.kps_left[:n], dl[:n], s.kps_right, s.desc_right) + ss.KITTI
        matched = _assert_equals_oracle(_raw_compute(st, pair[0], pair[1], *args), oracle, oracle_pair, *args)[2]
    assert matched > 256
    for n in (1, 1023, 1024, 1025):
        args = (s.kps_left[:1025], dl[:1025], s.kps_right[:n], s.desc_right[:n]) + ss.KITTI
        _assert_equals_oracle(_raw_compute(st, pair[0], pair[1], *args), oracle, oracle_pair, *args)


def test_stereo_host_entry_contract(mods, oracle, pair, oracle_pair):
    """ovs_stereo_compute's argument checks and its two input paths: empty sides, the capacity and invalid returns -- after each of which the SAME handle
    computes a scene correctly --, extractor outputs used where they are against uploaded copies that differ by one byte, a prefix of the
    extractor's output, and arrays of an extract that a later one on the same handle has superseded."""
    feature, match, synth = mods
    el, er = pair
    sc = {s.name: s for s in ss.scenes_from(oracle)}
    s = sc["shift"]
    scene_args = (s.kps_left, s.desc_left, s.kps_right, s.desc_right, s.focal_x_baseline, s.true_baseline)
    st = match.stereo(el, er, *scene_args, max_rows=ROWS, max_keypoints=64)

    def scene_still_right():
        _extract_both(pair, oracle_pair, s.left, s.right, levels=(0,))
        _assert_equals_oracle(_raw_compute(st, el, er, *scene_args), oracle, oracle_pair, *scene_args)

    scene_still_right()
    # empty sides
    rc, xr, dp, nv = _raw_compute(st, el, er, s.kps_left[:0], s.desc_left[:0], s.kps_right, s.desc_right, *ss.KITTI)
    assert (rc, nv) == (0, 0) and xr.tolist() == [] and dp.tolist() == []
    rc, xr, dp, nv = _raw_compute(st, el, er, s.kps_left, s.desc_left, s.kps_right[:0], s.desc_right[:0], *ss.KITTI)
    assert (rc, nv) == (0, 0) and (xr == -1).all() and (dp == -1).all()
    scene_still_right()
    # capacity: more keypoints than the handle holds, on either side; an image taller than the handle's max_rows
    d = sc["dense"]
    assert _raw_compute(st, el, er, d.kps_left[:65], d.desc_left[:65], s.kps_right, s.desc_right, *ss.KITTI)[0] == ERR_CAPACITY
    scene_still_right()
    assert _raw_compute(st, el, er, s.kps_left, s.desc_left, d.kps_right[:65], d.desc_right[:65], *ss.KITTI)[0] == ERR_CAPACITY
    scene_still_right()
    low = match.stereo(el, er, *scene_args, max_rows=ROWS - 1, max_keypoints=64)
    assert _raw_compute(low, el, er, *scene_args)[0] == ERR_CAPACITY
    tall = feature.orb_extractor(feature.orb_params(**ss.ORB_PARAMS), max_rows=ROWS + 8, max_cols=COLS)
    tall.extract(np.concatenate([s.right, s.right[:8]]))
    assert _raw_compute(st, el, tall, *scene_args)[0] == ERR_INVALID          # extractors with different image sizes
    scene_still_right()
    tall_left = feature.orb_extractor(feature.orb_params(**ss.ORB_PARAMS), max_rows=ROWS + 8, max_cols=COLS)
    tall_left.extract(np.concatenate([s.left, s.left[:8]]))
    assert _raw_compute(st, tall_left, tall, *scene_args)[0] == ERR_CAPACITY      # 248 rows on a 240-row handle
    scene_still_right()
    # resident against uploaded
    st = match.stereo(el, er, *scene_args, max_rows=ROWS)
    left, right, _ = synth.synth_stereo_pair(ROWS, COLS, seed=3)
    (kl, dl), (kr, dr) = _extract_both(pair, oracle_pair, left, right)
    wxr, _, wn = _assert_equals_oracle(_raw_compute(st, el, er, kl, dl, kr, dr, *ss.KITTI), oracle, oracle_pair, kl, dl, kr, dr, *ss.KITTI)
    assert wn > len(kl) // 10
    dl2 = dl.copy()
    dl2[np.nonzero(wxr < 0)[0][0], 31] ^= 0x80
    _assert_equals_oracle(_raw_compute(st, el, er, kl, dl2, kr, dr, *ss.KITTI), oracle, oracle_pair, kl, dl2, kr, dr, *ss.KITTI)
    dr2 = dr.copy()
    dr2[0, 0] ^= 0xFF                                        # the right side is uploaded, the left one stays resident
    _assert_equals_oracle(_raw_compute(st, el, er, kl, dl, kr, dr2, *ss.KITTI), oracle, oracle_pair, kl, dl, kr, dr2, *ss.KITTI)
    h = len(kl) // 2
    _assert_equals_oracle(_raw_compute(st, el, er, kl[:h], dl[:h], kr, dr, *ss.KITTI), oracle, oracle_pair, kl[:h], dl[:h], kr, dr, *ss.KITTI)
    # superseded: the arrays are those of an earlier extract, the pyramids those of the handles' last one
    left2, right2, _ = synth.synth_stereo_pair(ROWS, COLS, seed=4)
    _extract_both(pair, oracle_pair, left2, right2)
    _assert_equals_oracle(_raw_compute(st, el, er, kl, dl, kr, dr, *ss.KITTI), oracle, oracle_pair, kl, dl, kr, dr, *ss.KITTI)


def test_stereo_row_item_overflow(mods, oracle):
    """The row index holds 72 entries per keypoint of the handle (a band of a 16-level x 1.2 pyramid). With scale factor 2.0 and 6 levels the top
    octave's band is 2 * 32 rows either way: a handle sized for exactly n_right keypoints, all of them there, overflows it. The call returns the
    capacity error (the index kernel never writes past its buffer), and the same handle then computes an ordinary list correctly."""
    feature, match, synth = mods
    params = dict(max_num_keypts=300, scale_factor=2.0, num_levels=6)
    left, right, _ = synth.synth_stereo_pair(ROWS, COLS, seed=3)
    el, er = (feature.orb_extractor(feature.orb_params(**params), max_rows=ROWS, max_cols=COLS) for _ in range(2))
    op = oracle.OrbExtractor(oracle.make_params(**params)), oracle.OrbExtractor(oracle.make_params(**params))
    (kl, dl), (kr, dr) = _extract_both((el, er), op, left, right, levels=range(6))
    n = min(len(kl), len(kr), 128)
    kl, dl, kr, dr = kl[:n], dl[:n], kr[:n], dr[:n]
    st = match.stereo(el, er, kl, dl, kr, dr, *ss.KITTI, max_rows=ROWS, max_keypoints=n)
    top = kr.copy()
    top["octave"], top["y"] = 5, 120.0                       # rows 56 .. 184: 129 entries each, 72 provided
    assert _raw_compute(st, el, er, kl, dl, top, dr, *ss.KITTI)[0] == ERR_CAPACITY
    assert _assert_equals_oracle(_raw_compute(st, el, er, kl, dl, kr, dr, *ss.KITTI), oracle, op, kl, dl, kr, dr, *ss.KITTI)[2] > 0


def test_stereo_compute_dev(mods, oracle):
    """ovs_stereo_compute_dev after a batched device extract of (left, right) on ONE handle (frame_left = 0, frame_right = 1): device counts with
    cap > n (the output tail keeps its sentinel), NULL counts with cap == n, and a caller's n_valid on a non-default stream -- each equal to the
    oracle on the downloaded keypoints and to the two-extractor host entry on the same images."""
    import torch
    from openvslam_amd import _lib
    feature, match, synth = mods
    left, right, _ = synth.synth_stereo_pair(ROWS, COLS, seed=3)
    ex = feature.orb_extractor(feature.orb_params(**ss.ORB_PARAMS), max_rows=ROWS, max_cols=COLS, max_batch=2)
    cap = ex.max_keypoints
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_img = torch.from_numpy(np.stack([left, right])).cuda()
        d_kps = torch.zeros((2, cap, 7), dtype=torch.float32, device="cuda")
        d_desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
        ex.extract_batch_dev(d_img, d_kps, d_desc, d_cnt, stream=stream.cuda_stream)
        stream.synchronize()
        nl, nr = (int(v) for v in d_cnt.cpu())
        kps = d_kps.cpu().numpy().view(np.uint8).reshape(2, cap, 28)
        kl, kr = kps[0, :nl].copy().view(feature.KP_DTYPE).reshape(-1), kps[1, :nr].copy().view(feature.KP_DTYPE).reshape(-1)
        dl, dr = d_desc[0, :nl].cpu().numpy(), d_desc[1, :nr].cpu().numpy()
        assert 0 < nl < cap and 0 < nr < cap
        # references: the oracle on the downloaded keypoints, and the host entry with two extractors
        oxl, oxr = oracle.OrbExtractor(oracle.make_params(**ss.ORB_PARAMS)), oracle.OrbExtractor(oracle.make_params(**ss.ORB_PARAMS))
        oxl.extract(left)
        oxr.extract(right)
        wxr, wdp, wn = oracle.stereo_compute(oxl, oxr, kl, dl, kr, dr, *ss.KITTI)
        assert wn > nl // 10
        el = feature.orb_extractor(feature.orb_params(**ss.ORB_PARAMS), max_rows=ROWS, max_cols=COLS)
        er = feature.orb_extractor(feature.orb_params(**ss.ORB_PARAMS), max_rows=ROWS, max_cols=COLS)
        hkl, hdl = el.extract(left)
        hkr, hdr = er.extract(right)
        host = match.stereo(el, er, hkl, hdl, hkr, hdr, *ss.KITTI)
        hxr, hdp = host.compute()
        st = match.stereo(el, er, hkl, hdl, hkr, hdr, *ss.KITTI)      # the handle of the device calls (its host arrays are not used)
        L = _lib.lib()
        for form in ("device_counts", "null_counts", "caller_n_valid"):
            d_xr = torch.full((cap,), -7.0, dtype=torch.float32, device="cuda")
            d_dp = torch.full((cap,), -7.0, dtype=torch.float32, device="cuda")
            d_nv = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            counts = form != "null_counts"
            _lib.check(L.ovs_stereo_compute_dev(st._h, ex._h, 0, ex._h, 1, d_kps[0].data_ptr(), d_desc[0].data_ptr(), d_cnt[0:].data_ptr() if counts else None,
                                                cap if counts else nl, d_kps[1].data_ptr(), d_desc[1].data_ptr(), d_cnt[1:].data_ptr() if counts else None,
                                                cap if counts else nr, ss.KITTI[0], ss.KITTI[1], d_xr.data_ptr(), d_dp.data_ptr(),
                                                d_nv.data_ptr() if form == "caller_n_valid" else None, stream.cuda_stream), "ovs_stereo_compute_dev")
            stream.synchronize()
            xr, dp = d_xr.cpu().numpy(), d_dp.cpu().numpy()
            assert np.array_equal(_bits(xr[:nl]), _bits(wxr)) and np.array_equal(_bits(dp[:nl]), _bits(wdp)), form
            assert (xr[nl:] == -7).all() and (dp[nl:] == -7).all(), form        # nothing written past n
            if form == "caller_n_valid":
                assert int(d_nv.cpu()[0]) == wn
        assert nl == len(hkl) and host.num_valid_ == wn and np.array_equal(_bits(hxr), _bits(wxr)) and np.array_equal(_bits(hdp), _bits(wdp))
