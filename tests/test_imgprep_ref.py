"""Image front end, CPU tier: the numpy reference on its own, the host program (tests/imgprep_host.cc over
csrc/image_prep_plan.inc, g++ -ffp-contract=off) against the reference, and the argument errors of the C ABI, decided without a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import imgprep_ref as ref
import imgprep_scenes as sc

ROWS, COLS = sc.ROWS, sc.COLS


# ---- 1. the reference on its own ---------------------------------------------------------------------------------------------------------
def test_gray_of_white_and_black():
    for order in (ref.RGB, ref.BGR):
        assert ref.gray(np.full((1, 1, 3), 255, np.uint8), order)[0, 0] == 255
        assert ref.gray(np.zeros((1, 1, 4), np.uint8), order)[0, 0] == 0
    img = np.array([[[200, 100, 50, 7]]], np.uint8)
    assert ref.gray(img, ref.RGB)[0, 0] == (200 * 4899 + 100 * 9617 + 50 * 1868 + 8192) >> 14
    assert ref.gray(img, ref.BGR)[0, 0] == (50 * 4899 + 100 * 9617 + 200 * 1868 + 8192) >> 14
    assert ref.gray(img, ref.RGB)[0, 0] != ref.gray(img, ref.BGR)[0, 0]


def test_identity_rig_reproduces_the_source():
    fixed, _ = sc.fixed_maps("identity")
    for ch in (1, 3):
        img = sc.noise_image(ROWS, COLS, ch, 3)
        ixy, fxy = fixed[0]
        v, u = np.mgrid[0:ROWS, 0:COLS]
        assert np.array_equal(ixy[..., 0], u) and np.array_equal(ixy[..., 1], v) and not fxy.any()
        assert np.array_equal(ref.remap(img, ixy, fxy), img)


def test_integer_shift_of_the_map_shifts_the_image_and_fills_with_zero():
    img = sc.noise_image(ROWS, COLS, 1, 4) | 1   # no zero byte in the source
    v, u = np.mgrid[0:ROWS, 0:COLS]
    for dx, dy in ((5, 0), (-3, 7), (0, -ROWS), (COLS - 1, 2)):
        fixed = ref.fix_maps((u + dx).astype(np.float32), (v + dy).astype(np.float32))
        out = ref.remap(img, *fixed)
        want = np.zeros_like(img)
        vv, uu = v + dy, u + dx
        inside = (vv >= 0) & (vv < ROWS) & (uu >= 0) & (uu < COLS)
        want[inside] = img[vv[inside], uu[inside]]
        assert np.array_equal(out, want), (dx, dy)
        assert (out == 0).sum() == (~inside).sum() > 0


def test_blend_equals_exact_rational_arithmetic():
    rng = np.random.default_rng(11)
    for fx in range(32):
        for fy in range(32):
            p = rng.integers(0, 256, 4)
            assert ref.blend(p, fx, fy) == ref.blend_exact(p, fx, fy), (fx, fy, p)
    for p in ((255, 255, 255, 255), (0, 0, 0, 0), (255, 0, 0, 255), (0, 255, 255, 0)):
        assert all(ref.blend(p, fx, fy) == ref.blend_exact(p, fx, fy) for fx in range(32) for fy in range(32))
    assert ref.blend((37, 1, 2, 3), 0, 0) == 37   # an integer coordinate returns the source pixel


def test_fix_coord_ties_saturation_and_far_outside():
    m = np.array([0.0, 2 + 1 / 64, 3 + 1 / 64, -1.0, -0.5, 31 / 32, 40000.0, -40000.0, np.nan, np.inf, 2.0 ** 26, -2.0 ** 26, 2.0 ** 24], np.float32)
    ip, fr = ref.fix_coord(m)
    # 2 + 1/64 -> 64.5 -> 64 (even), 3 + 1/64 -> 96.5 -> 96 (even); 2^26 * 32 = 2^31 lies beyond 2^30; 2^24 * 32 = 2^29 saturates
    assert ip.tolist() == [0, 2, 3, -1, -1, 0, 32767, -32768, -32768, -32768, -32768, -32768, 32767]
    assert fr.tolist() == [0, 0, 0, 0, 16, 31, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("name", ["fisheye"])
def test_the_fisheye_rigs_have_few_near_tie_pixels(name):
    _, fm = sc.fixed_maps(name)
    for mx, my in fm:
        assert ref.near_tie(mx, my).sum() <= 0.001 * mx.size


# ---- 2. the host program against the reference -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    return sc.host_program()


def run_host(host, tmp_path, images, order, rectify, rig):
    sc.write_case(tmp_path / "case.bin", images, order, rectify, rig["P"], [rig["left"], rig["right"]])
    subprocess.run([host, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], check=True)
    rows, cols = images[0].shape[:2]
    return sc.read_out(tmp_path / "out.bin", rows, cols, len(images), rectify)


@pytest.mark.parametrize("name", ["identity", "persp5", "persp8", "fisheye"])
@pytest.mark.parametrize("channels,order", [(1, ref.GRAY), (3, ref.BGR), (4, ref.RGB)])
def test_host_program_equals_the_reference(host, tmp_path, name, channels, order):
    images = [sc.noise_image(ROWS, COLS, channels, 20 + s) for s in range(2)]
    got = run_host(host, tmp_path, images, order, True, sc.rig(name))
    for s, (ixy, fxy, out) in enumerate(got):
        assert sc.maps_agree(ixy, fxy, name, s) == []
        assert np.array_equal(out, ref.prepare(images[s], order, (ixy, fxy)))   # given the program's own map: everywhere


def test_host_program_gray_alone_and_odd_sizes(host, tmp_path):
    for rows, cols, ch, order in ((1, 3, 3, ref.RGB), (2, 65, 4, ref.BGR), (37, 61, 1, ref.GRAY)):
        img = sc.noise_image(rows, cols, ch, rows)
        (_, _, out), = run_host(host, tmp_path, [img], order, False, sc.rig("identity"))
        assert np.array_equal(out, ref.gray(img, order))


def test_launch_geometry_covers_the_image(host):
    for rows, cols, sides in ((1, 1, 1), (37, 61, 2), (2, 65, 1), (240, 257, 2), (1080, 1920, 2)):
        gx, gy, gz, bx, by = map(int, subprocess.run([host, "--launch", str(rows), str(cols), str(sides)], check=True, capture_output=True, text=True).stdout.split())
        assert (bx, by, gz) == (64, 4, sides)
        assert (gx - 1) * 256 < cols <= gx * 256 and (gy - 1) * 4 < rows <= gy * 4


# ---- 3. argument errors, decided before the device is touched --------------------------------------------------------------------------
def status(host, rows, cols, stride, channels, order, rectify, sides, max_rows=480, max_cols=752, map_rows=0, map_cols=0, map_sides=0):
    args = [rows, cols, stride, channels, order, rectify, sides, max_rows, max_cols, map_rows, map_cols, map_sides]
    return int(subprocess.run([host, "--status"] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout)


def test_run_status_of_the_plan(host):
    assert status(host, 480, 752, 752 * 3, 3, ref.BGR, 0, 2) == 0
    assert status(host, 0, 752, 752, 1, ref.GRAY, 0, 1) == 0 and status(host, 480, 0, 0, 1, ref.GRAY, 0, 1) == 0
    for channels in (0, 2, 5):
        assert status(host, 480, 752, 752 * 5, channels, ref.RGB, 0, 1) == -1
    for order in (-1, 3):
        assert status(host, 480, 752, 752 * 3, 3, order, 0, 1) == -1
    assert status(host, 480, 752, 752 * 3, 3, ref.GRAY, 0, 1) == -1      # a colour image needs a colour order
    assert status(host, 480, 752, 752 * 3 - 1, 3, ref.RGB, 0, 1) == -1    # a stride below cols * channels
    assert status(host, 481, 752, 752, 1, ref.GRAY, 0, 1) == -4 and status(host, 480, 753, 753, 1, ref.GRAY, 0, 1) == -4
    assert status(host, 480, 752, 752, 1, ref.GRAY, 1, 1) == -1           # rectify without a map
    assert status(host, 480, 752, 752, 1, ref.GRAY, 1, 1, map_rows=240, map_cols=752, map_sides=2) == -1   # a map of another size
    assert status(host, 480, 752, 752, 1, ref.GRAY, 1, 2, map_rows=480, map_cols=752, map_sides=1) == -1   # a pair on a single camera's map
    assert status(host, 480, 752, 752, 1, ref.GRAY, 1, 2, map_rows=480, map_cols=752, map_sides=2) == 0


def bad_rigs():
    good = sc.rig("persp5")
    def with_(**kw):
        return dict(good, left=dict(good["left"], **kw))
    nan = float("nan")
    yield "model", with_(model=2)
    for n in (1, 3, 6, 9):
        yield "n_dist %d" % n, with_(n_dist=n)
    yield "fisheye n_dist 5", with_(model=1, n_dist=5)
    yield "K nan", with_(K=[nan] + good["left"]["K"][1:])
    yield "D inf", with_(D=[float("inf")] + good["left"]["D"][1:])
    yield "R nan", with_(R=good["left"]["R"][:8] + [nan])
    yield "P nan", dict(good, P=[148.0, nan, 80.0, 60.0])
    yield "singular", with_(R=[1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    yield "singular P", dict(with_(R=sc.IDENT), P=[0.0, 148.0, 80.0, 60.0])


@pytest.mark.parametrize("what,rig", list(bad_rigs()), ids=[w for w, _ in bad_rigs()])
def test_host_program_refuses_a_bad_rig(host, tmp_path, what, rig):
    img = sc.noise_image(8, 8, 1, 1)
    sc.write_case(tmp_path / "case.bin", [img], ref.GRAY, True, rig["P"], [rig["left"], rig["right"]])
    r = subprocess.run([host, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 3 and "refused" in r.stdout, what


class RectifySide(C.Structure):
    _fields_ = [("model", C.c_int32), ("n_dist", C.c_int32), ("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9)]


def test_abi_argument_errors_without_a_handle():
    from openvslam_amd import _lib, image
    L = _lib.lib()
    h = C.c_void_p()
    for rows, cols in ((0, 752), (480, 0), (-1, 752), (480, 16385)):
        assert L.ovs_imgprep_create(0, rows, cols, C.byref(h)) == -1 and not h
    assert L.ovs_imgprep_create(0, 480, 752, None) == -1
    assert L.ovs_imgprep_create(-1, 480, 752, C.byref(h)) == -2 and not h
    assert L.ovs_imgprep_destroy(None) == 0
    buf = (C.c_uint8 * 64)()
    side = image.rectify_side(sc.rig("persp5")["left"])
    P = (C.c_double * 4)(148.0, 148.0, 80.0, 60.0)
    assert C.sizeof(side) == C.sizeof(RectifySide) == 216
    # a NULL handle is a NULL required pointer, for every entry
    assert L.ovs_imgprep_set_rectifier(None, 8, 8, C.byref(side), None, P) == -1
    assert L.ovs_imgprep_set_maps(None, 8, 8, buf, buf, None, None) == -1
    assert L.ovs_imgprep_get_maps(None, 0, buf, buf) == -1
    assert L.ovs_imgprep_run(None, buf, None, 8, 8, 8, 1, 0, 0, buf, None, 8) == -1
    assert L.ovs_imgprep_run_dev(None, buf, None, 8, 8, 8, 1, 0, 0, buf, None, 8, None) == -1
    n = C.c_int32(7)
    assert L.ovs_orb_extract_prepared(None, None, buf, 8, 8, 8, 1, 0, 0, None, 0, buf, buf, 1, C.byref(n), None, 0) == -1
    assert L.ovs_orb_extract_pair_prepared(None, None, buf, buf, 8, 8, 8, 1, 0, 0, None, None, 0, buf, buf, C.byref(n), buf, buf, C.byref(n), 1, None, None, 0) == -1
    if L.ovs_device_count() == 0:
        assert L.ovs_imgprep_create(0, 480, 752, C.byref(h)) == -2 and not h
        with pytest.raises(_lib.OvsError):
            image.image_preparer(480, 752)
