"""Image front end on the device, through the C ABI and the Python mirror: every prepared image byte for byte against the numpy
reference given the library's own fixed map, and the fixed map against the reference's. The sizes are the smallest at which the lane layout
(four pixels per lane, 64 lanes x 4 rows per workgroup) can go wrong."""
import ctypes as C
import threading

import numpy as np
import pytest

import imgprep_ref as ref
import imgprep_scenes as sc

pytestmark = pytest.mark.gpu

MAX_ROWS, MAX_COLS = 240, 320


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.fixture(scope="module")
def L():
    from openvslam_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def prep():
    from openvslam_amd import image
    return image.image_preparer(MAX_ROWS, MAX_COLS)


def padded(img, pad):
    """A copy of img whose rows are `pad` bytes longer than they need to be, filled with 0xEE: (view of the image, row stride)."""
    rows = img.shape[0]
    width = int(np.prod(img.shape[1:]))
    buf = np.full((rows, width + pad), 0xEE, np.uint8)
    buf[:, :width] = img.reshape(rows, width)
    return buf, width + pad


def abi_run(L, prep, images, order, rectify, src_pad=0, out_pad=0):
    """ovs_imgprep_run with the given row paddings; checks that the output's padding bytes are untouched."""
    rows, cols = images[0].shape[:2]
    ch = 1 if images[0].ndim == 2 else images[0].shape[2]
    src = [padded(im, src_pad) for im in images]
    out = [np.full((rows, cols + out_pad), 0xAB, np.uint8) for _ in images]
    st = L.ovs_imgprep_run(prep._h, _p(src[0][0]), _p(src[1][0]) if len(images) == 2 else None, rows, cols, src[0][1], ch, order, 1 if rectify else 0,
                           _p(out[0]), _p(out[1]) if len(images) == 2 else None, cols + out_pad)
    assert st == 0, st
    for o in out:
        assert (o[:, cols:] == 0xAB).all()
    return [o[:, :cols].copy() for o in out]


def random_maps(rows, cols, seed):
    """Float maps around the identity, reaching a few pixels outside the source on every side."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:rows, 0:cols]
    return ((u + rng.uniform(-3, 3, (rows, cols))).astype(np.float32), (v + rng.uniform(-3, 3, (rows, cols))).astype(np.float32))


# ---- widths around the lane group ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(37, 61), (48, 64), (2, 65), (1, 3), (1, 40), (40, 1), (5, 257)])
def test_sizes_strides_and_channels(L, prep, rows, cols):
    maps = [random_maps(rows, cols, 7 + s) for s in range(2)]
    prep.set_maps(maps[0][0], maps[0][1], maps[1][0], maps[1][1])
    fixed = [prep.get_maps(s) for s in range(2)]
    for s in range(2):
        want = ref.fix_maps(*maps[s])
        assert np.array_equal(fixed[s][0], want[0]) and np.array_equal(fixed[s][1], want[1])
    for ch, order in ((1, ref.GRAY), (3, ref.BGR), (4, ref.RGB)):
        images = [sc.noise_image(rows, cols, ch, 31 + s) for s in range(2)]
        for rectify in (False, True):
            want = [ref.prepare(images[s], order, fixed[s] if rectify else None) for s in range(2)]
            for src_pad, out_pad in ((0, 0), (3, 5), (4, 0), (0, 1)):
                got = abi_run(L, prep, images, order, rectify, src_pad, out_pad)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (ch, rectify, src_pad, out_pad)


# ---- map edges -------------------------------------------------------------------------------------------------------------------------
def test_map_edges(L, prep):
    n = 16
    def coords(size):
        return [-1.0, -0.5, 0.0, size - 1.0, size - 0.5, float(size), 31 / 32, 2 + 1 / 64, 3 + 1 / 64, 5 + 31 / 32, 40000.0, -40000.0, float("nan"), 1e30, float("inf"), 7.25]
    cx, cy = coords(n), coords(n)
    map_x = np.tile(np.array(cx, np.float32)[None, :], (n, 1))
    map_y = np.tile(np.array(cy, np.float32)[:, None], (1, n))
    prep.set_maps(map_x, map_y)
    ixy, fxy = prep.get_maps(0)
    want = ref.fix_maps(map_x, map_y)
    assert np.array_equal(ixy, want[0]) and np.array_equal(fxy, want[1])
    # the rule's own words: ties to even (2 + 1/64 and 3 + 1/64 both round down / up to the even count of 32nds), saturation, far outside
    assert ixy[0, :, 0].tolist() == [-1, -1, 0, n - 1, n - 1, n, 0, 2, 3, 5, 32767, -32768, -32768, -32768, -32768, 7]
    assert fxy[0, :, 0].tolist() == [0, 16, 0, 0, 16, 0, 31, 0, 0, 31, 0, 0, 0, 0, 0, 8]
    for ch, order in ((1, ref.GRAY), (3, ref.RGB), (4, ref.BGR)):
        img = sc.noise_image(n, n, ch, 5) | 1   # no zero byte: a tap that reads 0 was outside
        got, = abi_run(L, prep, [img], order, True)
        assert np.array_equal(got, ref.prepare(img, order, (ixy, fxy)))
        if ch == 1:
            assert got[2, 2] == img[0, 0] and got[3, 3] == img[n - 1, n - 1]          # integer coordinates return the source pixel
            assert got[0, 0] == 0 and got[5, 5] == 0 and (got[10:15] == 0).all()         # all four taps outside
            assert got[2, 1] == (16 * 32 * int(img[0, 0]) + 512) >> 10                 # x = -0.5: two taps outside


# ---- channels and order ----------------------------------------------------------------------------------------------------------------
def test_order_of_remap_and_gray(L, prep):
    rows, cols = 24, 40
    img = np.zeros((rows, cols, 3), np.uint8)
    u = np.arange(cols)
    for c, on in enumerate((u % 2 == 0, u % 2 == 1, (u // 2) % 2 == 0)):   # columns of 0 and 255, another pattern in every channel
        img[:, on, c] = 255
    maps = random_maps(rows, cols, 3)
    prep.set_maps(*maps)
    fixed = prep.get_maps(0)
    for order in (ref.RGB, ref.BGR):
        first, second = ref.prepare(img, order, fixed), ref.prepare_gray_first(img, order, fixed)
        assert not np.array_equal(first, second)   # the two orders differ on this image
        got, = abi_run(L, prep, [img], order, True)
        assert np.array_equal(got, first)
    assert not np.array_equal(ref.prepare(img, ref.RGB, fixed), ref.prepare(img, ref.BGR, fixed))
    with_alpha = np.concatenate([img, np.full((rows, cols, 1), 77, np.uint8)], -1)
    assert np.array_equal(abi_run(L, prep, [with_alpha], ref.RGB, True)[0], ref.prepare(img, ref.RGB, fixed))   # alpha is ignored


# ---- both rig models -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["identity", "persp5", "persp8", "fisheye"])
def test_rigs(prep, name):
    r = sc.rig(name)
    prep.set_rectifier(sc.ROWS, sc.COLS, r["left"], r["right"], r["P"])
    fixed = [prep.get_maps(s) for s in range(2)]
    for s in range(2):
        assert sc.maps_agree(fixed[s][0], fixed[s][1], name, s) == []
    for ch, order in ((1, ref.GRAY), (3, ref.BGR)):
        images = [sc.noise_image(sc.ROWS, sc.COLS, ch, 40 + s) for s in range(2)]
        got = prep.run(images[0], images[1], order, True)
        for s in range(2):
            assert np.array_equal(got[s], ref.prepare(images[s], order, fixed[s]))
        if name == "identity" and ch == 1:
            assert np.array_equal(got[0], images[0])


def test_single_camera_map_and_python_mirror(prep):
    from openvslam_amd import image
    r = sc.rig("persp5")
    prep.set_rectifier(sc.ROWS, sc.COLS, r["left"], None, r["P"])
    img = sc.noise_image(sc.ROWS, sc.COLS, 3, 9)
    fixed = prep.get_maps(0)
    assert np.array_equal(prep.run(img, None, "rgb", True), ref.prepare(img, ref.RGB, fixed))
    with pytest.raises(RuntimeError):
        prep.get_maps(1)
    with pytest.raises(RuntimeError):
        prep.run(img, img, "rgb", True)   # a pair on a single camera's map
    assert np.array_equal(image.convert_to_grayscale(img, "bgr", prep), ref.gray(img, ref.BGR))
    assert np.array_equal(image.convert_to_grayscale(img[..., 0], "gray", prep), img[..., 0])
    cfg = dict(model="perspective", rows=sc.ROWS, cols=sc.COLS, fx=r["P"][0], fy=r["P"][1], cx=r["P"][2], cy=r["P"][3])
    for s in ("left", "right"):
        cfg.update({"K_" + s: r[s]["K"], "D_" + s: r[s]["D"], "R_" + s: r[s]["R"]})
    rect = image.stereo_rectifier(cfg, preparer=prep)
    img_r = sc.noise_image(sc.ROWS, sc.COLS, 3, 10)
    out_l, out_r = rect.rectify(img, img_r)
    assert np.array_equal(out_l, ref.remap(img, *prep.get_maps(0))) and np.array_equal(out_r, ref.remap(img_r, *prep.get_maps(1)))


# ---- the forms agree -------------------------------------------------------------------------------------------------------------------
def test_host_device_and_single_forms_agree(prep):
    import torch
    r = sc.rig("persp8")
    prep.set_rectifier(sc.ROWS, sc.COLS, r["left"], r["right"], r["P"])
    rows, cols = sc.ROWS, sc.COLS
    for ch, order, rectify in ((3, ref.BGR, True), (4, ref.RGB, False), (1, ref.GRAY, True)):
        images = [sc.noise_image(rows, cols, ch, 50 + s) for s in range(2)]
        pair = prep.run(images[0], images[1], order, rectify)
        d_src = [torch.from_numpy(im.reshape(rows, cols * ch)).cuda() for im in images]
        d_out = torch.zeros((2, rows, cols), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            prep.run_dev(d_src[0], d_src[1], ch, order, rectify, d_out[0], d_out[1], stream.cuda_stream)
        stream.synchronize()
        dev = d_out.cpu().numpy()
        assert np.array_equal(dev[0], pair[0]) and np.array_equal(dev[1], pair[1])
        if rectify:
            assert np.array_equal(prep.run(images[0], None, order, True), pair[0])   # a single image takes the left map
        else:
            assert np.array_equal(prep.run(images[1], None, order, False), pair[1])


@pytest.fixture(scope="module")
def stereo_scene(prep):
    """A 320 x 240 colour pair with corners, the rig and everything the two-step path computes from it."""
    from openvslam_amd import feature
    from openvslam_amd.synth import synth_frame
    rows, cols = 240, 320
    g = [synth_frame(rows, cols, seed=5, n_rect=80), synth_frame(rows, cols, seed=5, n_rect=80, shift=(6, 0), noise_seed=8)]
    raw = [np.stack([np.roll(x, 1, 1), x, np.roll(x, 1, 0)], -1).copy() for x in g]
    r = sc.scaled(sc.rig("persp5"), 2.0)
    ex = feature.orb_extractor(feature.orb_params(500), max_rows=rows, max_cols=cols, max_batch=2)
    mask = np.full((rows, cols), 255, np.uint8)
    mask[60:120, 100:200] = 0
    return dict(rows=rows, cols=cols, raw=raw, rig=r, ex=ex, mask=mask)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("with_gray", [False, True])
def test_fused_pair_equals_prepare_then_extract_pair(prep, stereo_scene, masked, with_gray):
    from openvslam_amd import match
    m = stereo_scene
    r, ex = m["rig"], m["ex"]
    prep.set_rectifier(m["rows"], m["cols"], r["left"], r["right"], r["P"])
    masks = (m["mask"], m["mask"]) if masked else (None, None)
    gray = prep.run(m["raw"][0], m["raw"][1], ref.BGR, True)
    fixed = [prep.get_maps(s) for s in range(2)]
    assert all(np.array_equal(gray[s], ref.prepare(m["raw"][s], ref.BGR, fixed[s])) for s in range(2))
    want = ex.extract_pair(gray[0], gray[1], *masks)
    st = match.stereo(ex, ex, want[0][0], want[0][1], want[1][0], want[1][1], 120.0, 0.1, max_rows=m["rows"])
    want_stereo = st.compute()
    got = ex.extract_pair_prepared(prep, m["raw"][0], m["raw"][1], ref.BGR, True, masks[0], masks[1], return_gray=with_gray)
    assert len(want[0][0]) > 100 and len(want[1][0]) > 100
    for s in range(2):
        assert np.array_equal(got[s][0], want[s][0]) and np.array_equal(got[s][1], want[s][1])
    if with_gray:
        assert np.array_equal(got[2], gray[0]) and np.array_equal(got[3], gray[1])
    got_stereo = st.compute()   # the same device pyramid after the fused call
    assert np.array_equal(got_stereo[0], want_stereo[0]) and np.array_equal(got_stereo[1], want_stereo[1])


@pytest.mark.parametrize("rectify", [False, True])
def test_fused_single_equals_prepare_then_extract(prep, stereo_scene, rectify):
    m = stereo_scene
    r, ex = m["rig"], m["ex"]
    prep.set_rectifier(m["rows"], m["cols"], r["left"], None, r["P"])
    gray = prep.run(m["raw"][0], None, ref.RGB, rectify)
    want = ex.extract(gray, m["mask"])
    kps, desc, out = ex.extract_prepared(prep, m["raw"][0], ref.RGB, rectify, m["mask"], return_gray=True)
    assert len(want[0]) > 100 and np.array_equal(kps, want[0]) and np.array_equal(desc, want[1]) and np.array_equal(out, gray)
    kps, desc = ex.extract_prepared(prep, m["raw"][0], ref.RGB, rectify, m["mask"])
    assert np.array_equal(kps, want[0]) and np.array_equal(desc, want[1])


# ---- argument errors on a live handle --------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(L, prep, stereo_scene):
    r = sc.rig("persp5")
    prep.set_rectifier(sc.ROWS, sc.COLS, r["left"], r["right"], r["P"])
    rows, cols = sc.ROWS, sc.COLS
    img = sc.noise_image(rows, cols, 3, 1)
    out = np.full((rows, cols), 0x5A, np.uint8)
    run = lambda **kw: L.ovs_imgprep_run(prep._h, _p(kw.get("src", img)), None, kw.get("rows", rows), kw.get("cols", cols), kw.get("stride", cols * 3),
                                         kw.get("ch", 3), kw.get("order", ref.RGB), kw.get("rectify", 0), _p(kw.get("out", out)), None, kw.get("ostride", cols))
    assert run() == 0
    out[:] = 0x5A
    for kw in (dict(ch=2), dict(order=3), dict(order=ref.GRAY), dict(stride=cols * 3 - 1), dict(ostride=cols - 1), dict(rows=rows + 1, rectify=1), dict(rows=-1)):
        assert run(**kw) == -1, kw
    assert run(rows=MAX_ROWS + 1) == -4 and run(cols=MAX_COLS + 1, stride=3 * (MAX_COLS + 1)) == -4
    assert L.ovs_imgprep_run(prep._h, None, None, rows, cols, cols * 3, 3, ref.RGB, 0, _p(out), None, cols) == -1
    assert L.ovs_imgprep_run(prep._h, _p(img), _p(img), rows, cols, cols * 3, 3, ref.RGB, 0, _p(out), None, cols) == -1
    assert run(rows=0) == 0 and run(cols=0, stride=0) == 0
    assert (out == 0x5A).all()
    assert L.ovs_imgprep_get_maps(prep._h, 2, None, None) == -1
    from openvslam_amd import image
    side, P = image.rectify_side(r["left"]), (C.c_double * 4)(*r["P"])
    bad = image.rectify_side(dict(r["left"], n_dist=6))
    assert L.ovs_imgprep_set_rectifier(prep._h, rows, cols, C.byref(bad), None, P) == -1
    assert L.ovs_imgprep_set_rectifier(prep._h, rows, cols, C.byref(side), None, None) == -1
    assert L.ovs_imgprep_set_rectifier(prep._h, MAX_ROWS + 1, cols, C.byref(side), None, P) == -4
    assert prep.get_maps(1)[0].shape == (rows, cols, 2)   # the refused calls left the pair's maps as they were
    # the fused entry: the preparer's refusals before anything is written
    ex = stereo_scene["ex"]
    n, buf = C.c_int32(9), np.zeros(64, np.uint8)
    assert L.ovs_orb_extract_prepared(ex._h, prep._h, _p(img), rows, cols, cols * 3, 5, ref.RGB, 0, None, 0, _p(buf), _p(buf), 1, C.byref(n), None, 0) == -1
    assert L.ovs_orb_extract_prepared(ex._h, prep._h, _p(img), MAX_ROWS + 1, cols, cols * 3, 3, ref.RGB, 0, None, 0, _p(buf), _p(buf), 1, C.byref(n), None, 0) == -4
    assert n.value == 0 and not buf.any()


# ---- lifetime and retry ----------------------------------------------------------------------------------------------------------------
def test_lifetime_two_handles_and_injected_failure(L):
    from openvslam_amd import image
    live = L.ovs_debug_live_resources()
    img = sc.noise_image(sc.ROWS, sc.COLS, 3, 2)
    r = sc.rig("persp5")
    results, errors = [None, None], []

    def work(i):
        try:
            p = image.image_preparer(sc.ROWS, sc.COLS)
            p.set_rectifier(sc.ROWS, sc.COLS, r["left"], r["right"], r["P"])
            fixed = p.get_maps(i)
            outs = [p.run(img, img, ref.RGB, True)[i] for _ in range(4)]
            results[i] = all(np.array_equal(o, ref.prepare(img, ref.RGB, fixed)) for o in outs)
            del p
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and results == [True, True]
    p = image.image_preparer(sc.ROWS, sc.COLS)
    assert L.ovs_debug_live_resources() == live + 9   # a stream and four blocks per side
    want = ref.gray(img, ref.BGR)
    try:
        L.ovs_debug_inject_hip_failures(0, 1)
        with pytest.raises(RuntimeError):
            p.run(img, None, ref.BGR, False)
    finally:
        L.ovs_debug_inject_hip_failures(0, 0)
    assert np.array_equal(p.run(img, None, ref.BGR, False), want)   # the next call is correct
    del p
    assert L.ovs_debug_live_resources() == live
