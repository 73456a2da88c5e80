"""util::stereo_rectifier, util::convert_to_grayscale and feature::orb_extractor::extract_pair_prepared through the class layer
(openvslam_amd/cpp/test_imgprep_shim.cc) against arrays the reference wrote; and the classes' degraded result, with or without a device."""
import os
import subprocess

import numpy as np
import pytest

import imgprep_ref as ref
import imgprep_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
SHIM = os.path.join(CPP, "test_imgprep_shim")


@pytest.fixture(scope="module")
def shim():
    subprocess.check_call(["make", "-C", CPP, "test_imgprep_shim"])
    return SHIM


def scene(tmp_path, rows, cols, channels, order):
    from openvslam_amd.synth import synth_frame
    g = [synth_frame(rows, cols, seed=5, n_rect=80), synth_frame(rows, cols, seed=5, n_rect=80, shift=(6, 0), noise_seed=8)]
    raw = [x if channels == 1 else np.stack([np.roll(x, 1, 1), x, np.roll(x, 1, 0)] + [x] * (channels - 3), -1).copy() for x in g]
    r = sc.scaled(sc.rig("persp5"), rows / sc.ROWS)
    sc.write_case(tmp_path / "case.bin", raw, order, True, r["P"], [r["left"], r["right"]])
    return raw, r


def test_classes_degrade_to_the_empty_result(shim, tmp_path):
    scene(tmp_path, 120, 160, 3, ref.BGR)
    out = subprocess.run([shim, str(tmp_path / "case.bin"), "--degraded"], capture_output=True, text=True)
    assert out.returncode == 0 and "degraded ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("channels,order", [(3, ref.BGR), (1, ref.GRAY)])
def test_classes_equal_the_reference(shim, tmp_path, channels, order):
    rows, cols = 240, 320
    raw, r = scene(tmp_path, rows, cols, channels, order)
    out = subprocess.run([shim, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout + out.stderr
    data = np.fromfile(tmp_path / "out.bin", np.uint8)
    n, nc = rows * cols, rows * cols * channels
    fixed = [ref.fix_maps(*ref.float_map(r[s], r["P"], rows, cols)) for s in ("left", "right")]   # perspective rigs: the library's map is the reference's
    for s in range(2):
        want = ref.remap(raw[s], *fixed[s])
        assert np.array_equal(data[s * nc:(s + 1) * nc].reshape(want.shape), want)                               # stereo_rectifier::rectify
        assert np.array_equal(data[2 * nc + s * n:2 * nc + (s + 1) * n].reshape(rows, cols), ref.gray(raw[s], order))   # convert_to_grayscale
        assert np.array_equal(data[2 * nc + (2 + s) * n:2 * nc + (3 + s) * n].reshape(rows, cols), ref.prepare(raw[s], order, fixed[s]))   # the fused call
    counts = data[2 * nc + 4 * n:].view(np.int32)
    assert counts.size == 2 and (counts > 100).all()
