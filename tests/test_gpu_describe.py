"""GPU parity of k_describe (openvslam_amd/csrc/orb_describe.hip) at its decision edges: the frames of tests/describe_frames.py -- which
tests/test_describe_frames.py shows to reach those edges, from oracle and numpy data alone -- through the host entry and the device-batch
entry, under the four (blur_taps, trig) variant combinations, on both patch-staging load paths, at batch sizes around the XCD group of
eight and with output capacities below the keypoint count. Keypoint records (raw bytes: angles by bit pattern), descriptors and level counts
are compared with the CPU oracle by np.array_equal; tolerance zero."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_frames as df   # noqa: E402

pytestmark = pytest.mark.gpu

VARIANTS = [(0, 0), (1, 0), (0, 1), (1, 1)]   # (blur_taps, trig)
SENTINEL = 0xA5
GUARD = 4096                                  # bytes behind the last frame's block of every output
MAX_BATCH = 9
OVS_ERR_CAPACITY = -4

_extractors, _expected, _images = {}, {}, {}


@pytest.fixture(scope="module")
def hip():
    from openvslam_amd import feature
    return feature


def _image(key):
    """'name' or 'name/transform': the frames and the rolls / flips of them that the batches hold."""
    if key not in _images:
        name, _, tr = key.partition("/")
        if name.startswith("noise"):   # noise_<cols>x<rows>_<seed>: a busy frame of any size (the params come from the caller)
            if name == "noise":
                img, p = df.FRAMES["noise"]()
            else:
                size, seed = name.split("_")[1:]
                cols, rows = (int(v) for v in size.split("x"))
                img, p = df.noise_frame(cols, rows, int(seed))
        else:
            img, p = df.FRAMES[name]()
        img = {"": lambda a: a, "flipud": lambda a: a[::-1], "fliplr": lambda a: a[:, ::-1], "rot180": lambda a: a[::-1, ::-1],
               "right1": lambda a: np.roll(a, 1, 1), "left1": lambda a: np.roll(a, -1, 1), "down1": lambda a: np.roll(a, 1, 0),
               "up1": lambda a: np.roll(a, -1, 0), "roll75": lambda a: np.roll(a, (7, 5), (0, 1))}[tr](img)
        _images[key] = (np.ascontiguousarray(img), p)
    return _images[key]


TRANSFORMS = ["", "flipud", "fliplr", "rot180", "right1", "left1", "down1", "up1", "roll75"]


def _pkey(p):
    return tuple(sorted(p.items()))


def _expect(oracle, key, taps, trig, p=None):
    """(kps, desc, level counts) of the oracle, computed once per (image, params, variant)."""
    img, p0 = _image(key)
    p = p or p0
    k = (key, _pkey(p), taps, trig)
    if k not in _expected:
        _, kps, desc, counts = df.run_oracle(oracle, img, p, blur_taps=taps, trig=trig)
        _expected[k] = (kps, desc, counts)
    return _expected[k]


def _extractor(hip, rows, cols, p, taps, trig):
    """One extractor per (frame size, params), reused across tests and variants."""
    k = (rows, cols, _pkey(p))
    if k not in _extractors:
        _extractors[k] = hip.orb_extractor(hip.orb_params(p["max_num_keypts"], p["scale_factor"], p["num_levels"], p["ini_fast_thr"], p["min_fast_thr"]),
                                           max_rows=rows, max_cols=cols, max_batch=MAX_BATCH)
    ex = _extractors[k]
    ex.set_variant("blur_taps", taps)
    ex.set_variant("trig", trig)
    return ex


def _device_images(imgs, arrangement):
    """(B, rows, cols) uint8 view on the device in one of the layouts the patch staging distinguishes, with the layout asserted."""
    import torch
    B, rows, cols = imgs.shape
    p16 = (cols + 15) // 16 * 16
    src = torch.from_numpy(imgs).cuda()
    if arrangement == "aligned":          # pitch % 16 == 0, base % 16 == 0: the 16-byte loads
        full = torch.zeros((B, rows, p16), dtype=torch.uint8, device="cuda")
        view = full[:, :, :cols]
        want = (0, 0)
    elif arrangement == "pitch4":         # a tensor 4 bytes wider: pitch % 16 == 4 fails the first condition alone
        full = torch.zeros((B, rows, p16 + 4), dtype=torch.uint8, device="cuda")
        view = full[:, :, :cols]
        want = (0, 4)
    elif arrangement == "base4":          # from column 4 of a wider tensor: base % 16 == 4 fails the second condition alone
        full = torch.zeros((B, rows, p16 + 16), dtype=torch.uint8, device="cuda")
        view = full[:, :, 4:4 + cols]
        want = (4, 0)
    else:                                 # "tight": contiguous, the last frame's last pixel is the last byte of the tensor's storage
        assert arrangement == "tight"
        full = torch.empty((B, rows, cols), dtype=torch.uint8, device="cuda")
        view = full
        want = (0, cols % 16)
        assert full.untyped_storage().nbytes() == B * rows * cols and view.is_contiguous()
    view.copy_(src)
    assert (view.data_ptr() % 16, view.stride(1) % 16) == want and view.stride(2) == 1 and view.stride(0) == rows * view.stride(1)
    return view, full


def _run_dev(ex, d_img, cap):
    """extract_batch_dev into views over the front of larger sentinel-filled allocations. Returns (counts, kps (B, cap, 28) u8, desc (B, cap, 32))
    after asserting that the guard bytes behind the last frame's block and every row at or beyond counts[b] still hold the sentinel."""
    import torch
    B = d_img.shape[0]
    flat_k = torch.full((B * cap * 28 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    flat_d = torch.full((B * cap * 32 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    flat_c = torch.full((B * 4 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_kps, d_desc, d_cnt = flat_k[:B * cap * 28].view(B, cap, 28), flat_d[:B * cap * 32].view(B, cap, 32), flat_c[:B * 4].view(torch.int32)
    assert d_kps.data_ptr() == flat_k.data_ptr() and d_desc.data_ptr() == flat_d.data_ptr() and d_cnt.data_ptr() == flat_c.data_ptr()
    ex.extract_batch_dev(d_img, d_kps, d_desc, d_cnt, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    k, d, c = flat_k.cpu().numpy(), flat_d.cpu().numpy(), flat_c.cpu().numpy()
    for name, a, used in (("kps", k, B * cap * 28), ("desc", d, B * cap * 32), ("counts", c, B * 4)):
        assert (a[used:] == SENTINEL).all(), "guard bytes behind %s" % name
    cnt = c[:B * 4].view(np.int32)
    kps, desc = k[:B * cap * 28].reshape(B, cap, 28), d[:B * cap * 32].reshape(B, cap, 32)
    for b in range(B):
        assert 0 <= cnt[b] <= cap, (b, cnt[b])
        assert (kps[b, cnt[b]:] == SENTINEL).all() and (desc[b, cnt[b]:] == SENTINEL).all(), "frame %d: rows beyond its count" % b
    return cnt, kps, desc


def _check_frame(cnt, kps, desc, b, want, cap=None):
    wk, wd, _ = want
    n = len(wk) if cap is None else min(len(wk), cap)
    assert cnt[b] == n, (b, cnt[b], n)
    assert np.array_equal(kps[b, :n].reshape(-1), wk[:n].view(np.uint8).reshape(-1)), "frame %d keypoint records" % b
    assert np.array_equal(desc[b, :n], wd[:n]), "frame %d descriptors" % b


FRAME_NAMES = sorted(df.FRAMES)


@pytest.mark.parametrize("taps,trig", VARIANTS)
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_host_entry(hip, oracle, name, taps, trig):
    img, p = _image(name)
    ex = _extractor(hip, img.shape[0], img.shape[1], p, taps, trig)
    wk, wd, counts = _expect(oracle, name, taps, trig)
    gk, gd = ex.extract(img)
    assert len(gk) == len(wk) > 0
    assert np.array_equal(gk.view(np.uint8), wk.view(np.uint8))
    assert np.array_equal(gd, wd)
    assert np.array_equal(ex.debug_level_counts(), counts)


@pytest.mark.parametrize("arrangement", ["aligned", "pitch4", "base4", "tight"])
@pytest.mark.parametrize("name", FRAME_NAMES)
def test_device_entry_on_each_load_path(hip, oracle, name, arrangement):
    """Two frames (the frame and its 180 degree turn) per call, level-0 rows laid out so that the 16-byte path runs ("aligned"; "tight" too
    when cols % 16 == 0, then with the last frame ending on the last byte of the tensor's storage) or the 4-byte fallback runs because of the
    pitch alone ("pitch4") or of the base alone ("base4"); all four variant combinations."""
    keys = [name, name + "/rot180"]
    imgs = np.stack([_image(k)[0] for k in keys])
    p = _image(name)[1]
    d_img, _keep = _device_images(imgs, arrangement)
    for taps, trig in VARIANTS:
        ex = _extractor(hip, imgs.shape[1], imgs.shape[2], p, taps, trig)
        cnt, kps, desc = _run_dev(ex, d_img, ex.max_keypoints)
        for b, k in enumerate(keys):
            want = _expect(oracle, k, taps, trig)
            _check_frame(cnt, kps, desc, b, want)
            assert np.array_equal(ex.debug_level_counts(b), want[2]), (k, taps, trig)


def test_tight_layout_of_the_border_frame_takes_the_16_byte_path():
    """The arrangement the comment in k_describe on reading past a row's end is about: cols % 16 == 0, contiguous, base aligned."""
    img, _ = _image("border_c0")
    d_img, _keep = _device_images(np.stack([img, img]), "tight")
    assert d_img.stride(1) % 16 == 0 and d_img.data_ptr() % 16 == 0 and (d_img.data_ptr() + d_img.stride(0)) % 16 == 0


@pytest.mark.parametrize("name", ["border_c0", "border_c4"])
@pytest.mark.parametrize("B", [1, 7, 8, 9])
def test_batch_sizes_around_the_xcd_group(hip, oracle, name, B):
    """launch_describe pads the batch to a multiple of eight frames (frame 8 g + x on XCD x): one frame, a group one short, a full group and a
    group plus one. Every frame is a different roll or flip of the border frame and is compared with the oracle; rows beyond a frame's count and
    the bytes behind the last frame keep their fill (_run_dev)."""
    keys = [name + ("/" + t if t else "") for t in TRANSFORMS[:B]]
    imgs = np.stack([_image(k)[0] for k in keys])
    p = _image(name)[1]
    d_img, _keep = _device_images(imgs, "tight")
    for taps, trig in VARIANTS:
        ex = _extractor(hip, imgs.shape[1], imgs.shape[2], p, taps, trig)
        cnt, kps, desc = _run_dev(ex, d_img, ex.max_keypoints)
        for b, k in enumerate(keys):
            want = _expect(oracle, k, taps, trig, p)
            _check_frame(cnt, kps, desc, b, want)
            assert np.array_equal(ex.debug_level_counts(b), want[2]), (k, taps, trig)


def _caps(counts):
    """n - 1, the middle of a level, a level boundary, 1."""
    n = sum(counts)
    assert counts[0] > 2 and counts[1] > 2 and n > counts[0] + counts[1]
    return [("n_minus_1", n - 1), ("mid_level_1", counts[0] + counts[1] // 2), ("end_of_level_1", counts[0] + counts[1]), ("end_of_level_0", counts[0]), ("one", 1)]


@pytest.mark.parametrize("which", ["n_minus_1", "mid_level_1", "end_of_level_1", "end_of_level_0", "one"])
@pytest.mark.parametrize("name", ["noise", "border_c0"])
def test_capacity_below_the_count_device_entry(hip, oracle, name, which):
    """d_kps / d_desc of capacity cap < n: counts[b] == cap, rows [0, cap) are the oracle's first cap keypoints (the output is level-major),
    frame 1's block holds frame 1's own first rows and nothing of frame 0's overflow, nothing is written behind the last block."""
    keys = [name, name + "/fliplr"]
    imgs = np.stack([_image(k)[0] for k in keys])
    p = _image(name)[1]
    want = [_expect(oracle, k, 0, 0) for k in keys]
    cap = dict(_caps(want[0][2]))[which]
    assert 1 <= cap < len(want[0][0])
    ex = _extractor(hip, imgs.shape[1], imgs.shape[2], p, 0, 0)
    d_img, _keep = _device_images(imgs, "aligned")
    cnt, kps, desc = _run_dev(ex, d_img, cap)
    assert cnt[0] == cap
    for b in range(2):
        _check_frame(cnt, kps, desc, b, want[b], cap)


@pytest.mark.parametrize("which", ["n_minus_1", "mid_level_1", "end_of_level_1", "end_of_level_0", "one"])
def test_capacity_below_the_count_host_entry(hip, oracle, which):
    """ovs_orb_extract with cap < n (include/ovslam_hip.h: "*n_out = number written", OVS_ERR_CAPACITY = "output larger than the ... buffer"):
    the status says so, n_out == cap, the first cap rows are the oracle's, and the caller's arrays are untouched beyond them."""
    img, p = _image("noise")
    wk, wd, counts = _expect(oracle, "noise", 0, 0)
    cap = dict(_caps(counts))[which]
    ex = _extractor(hip, img.shape[0], img.shape[1], p, 0, 0)
    kps = np.full((len(wk) + 8) * 28, SENTINEL, np.uint8)
    desc = np.full((len(wk) + 8, 32), SENTINEL, np.uint8)
    n = C.c_int32(-5)
    st = ex._L.ovs_orb_extract(ex._h, img.ctypes.data_as(C.c_void_p), img.shape[0], img.shape[1], img.strides[0], None, 0,
                               kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    assert st == OVS_ERR_CAPACITY and n.value == cap
    assert np.array_equal(kps[:cap * 28], wk[:cap].view(np.uint8).reshape(-1)) and np.array_equal(desc[:cap], wd[:cap])
    assert (kps[cap * 28:] == SENTINEL).all() and (desc[cap:] == SENTINEL).all()
    # and with room for all of them, through the same arrays
    st = ex._L.ovs_orb_extract(ex._h, img.ctypes.data_as(C.c_void_p), img.shape[0], img.shape[1], img.strides[0], None, 0,
                               kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), len(wk), C.byref(n))
    assert st == 0 and n.value == len(wk) and np.array_equal(kps[:len(wk) * 28], wk.view(np.uint8).reshape(-1)) and np.array_equal(desc[:len(wk)], wd)


@pytest.mark.parametrize("name", ["level0_empty", "middle_level_empty", "level0_only"])
def test_level_gap_frame_between_busy_frames(hip, oracle, name):
    """A frame with an empty level (level 0: the kslot == 0 workgroup has no keypoint to describe and still owes counts[b]; a middle level:
    out_idx sums a zero) as frame 1 of a batch whose frames 0 and 2 are busy on every level, under the gap frame's parameters."""
    img, p = _image(name)
    rows, cols = img.shape
    keys = ["noise_%dx%d_31" % (cols, rows), name, "noise_%dx%d_32" % (cols, rows), name + "/rot180"]
    imgs = np.stack([_image(k)[0] for k in keys])
    d_img, _keep = _device_images(imgs, "aligned")
    for taps, trig in ((0, 0), (1, 1)):
        ex = _extractor(hip, rows, cols, p, taps, trig)
        want = [_expect(oracle, k, taps, trig, p) for k in keys]
        assert all(c > 0 for c in want[0][2]) and all(c > 0 for c in want[2][2]) and 0 in want[1][2]
        cnt, kps, desc = _run_dev(ex, d_img, ex.max_keypoints)
        for b in range(len(keys)):
            _check_frame(cnt, kps, desc, b, want[b])
            assert np.array_equal(ex.debug_level_counts(b), want[b][2]), (keys[b], taps, trig)
