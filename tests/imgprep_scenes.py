"""Rigs and images for the image front end's tests, and the file formats of tests/imgprep_host.cc. The rigs are chosen so that the share of
pixels the fisheye comparison may excuse (imgprep_ref.near_tie) stays far below its cap; test_imgprep_ref.py checks that."""
import os
import struct
import subprocess

import numpy as np

import imgprep_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "openvslam_amd", "cpp")
ROWS, COLS = 120, 160


def rot(rx, ry, rz):
    """Rodrigues' formula for the rotation vector (rx, ry, rz), row-major 9 doubles."""
    v = np.array([rx, ry, rz], np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3).ravel().tolist()
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)).ravel().tolist()


def K(fx, fy, cx, cy):
    return [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0]


def side(model, Kv, D, R):
    return dict(model=model, K=list(Kv), D=list(D), R=list(R))


IDENT = np.eye(3).ravel().tolist()
P_RECT = [148.0, 148.0, 80.5, 59.25]
RIGS = {
    # D = 0, R = I, K = the rectified camera: the map is the identity
    "identity": dict(P=[150.0, 150.0, 80.0, 60.0], left=side(0, K(150.0, 150.0, 80.0, 60.0), [], IDENT), right=side(0, K(150.0, 150.0, 80.0, 60.0), [0, 0, 0, 0], IDENT)),
    "persp5": dict(P=P_RECT, left=side(0, K(151.3, 150.7, 79.2, 61.1), [-0.283, 0.0739, 1.9e-4, 1.8e-5, -0.011], rot(0.004, -0.003, 0.001)),
                   right=side(0, K(150.2, 151.9, 81.7, 58.6), [-0.291, 0.0801, -4.1e-4, 2.3e-4, 0.0], rot(-0.011, 0.023, -0.006))),
    "persp8": dict(P=P_RECT, left=side(0, K(151.3, 150.7, 79.2, 61.1), [0.12, -0.05, 3e-4, -2e-4, 0.01, 0.3, -0.02, 0.004], IDENT),
                   right=side(0, K(150.2, 151.9, 81.7, 58.6), [0.11, -0.04, -1e-4, 5e-4, 0.02, 0.28, -0.01, 0.002], rot(0.02, -0.015, 0.03))),
    "fisheye": dict(P=[95.0, 95.0, 80.0, 60.0], left=side(1, K(101.3, 100.9, 79.6, 60.4), [-0.013, 0.0051, -0.0023, 4.1e-4], rot(0.002, 0.001, -0.003)),
                    right=side(1, K(100.4, 101.7, 80.9, 59.2), [-0.011, 0.0043, -0.0019, 3.7e-4], rot(-0.015, 0.02, 0.01))),
}


def rig(name):
    return RIGS[name]


def scaled(r, k):
    """The rig for images k times as large: focal lengths and principal points times k."""
    def sk(Kv):
        return [Kv[0] * k, 0.0, Kv[2] * k, 0.0, Kv[4] * k, Kv[5] * k, 0.0, 0.0, 1.0]
    return dict(P=[v * k for v in r["P"]], left=dict(r["left"], K=sk(r["left"]["K"])), right=dict(r["right"], K=sk(r["right"]["K"])))


def noise_image(rows, cols, channels, seed):
    """Smooth structure plus noise: neighbouring taps differ, so a wrong tap or weight changes bytes."""
    rng = np.random.default_rng(seed)
    shape = (rows, cols) if channels == 1 else (rows, cols, channels)
    y, x = np.mgrid[0:rows, 0:cols]
    base = (96 + 64 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0)).astype(np.int64)
    if channels > 1:
        base = base[..., None] + np.arange(channels) * 17
    return np.clip(base + rng.integers(-60, 61, shape), 0, 255).astype(np.uint8)


def fixed_maps(name, rows=ROWS, cols=COLS):
    """[(ixy, fxy) left, (ixy, fxy) right] and the float maps [(mx, my), ...] of a rig by the reference."""
    r = rig(name)
    fm = [ref.float_map(r[s], r["P"], rows, cols) for s in ("left", "right")]
    return [ref.fix_maps(*m) for m in fm], fm


def maps_agree(got_ixy, got_fxy, name_or_maps, side_idx, rows=ROWS, cols=COLS, cap=0.001):
    """The fixed map of a side against the reference: identical, except (fisheye only) at the reference's near-tie pixels, at most `cap` of all.
    Returns the list of complaints."""
    fixed, fm = fixed_maps(name_or_maps, rows, cols) if isinstance(name_or_maps, str) else name_or_maps
    want_ixy, want_fxy = fixed[side_idx]
    differs = np.any(got_ixy != want_ixy, -1) | np.any(got_fxy != want_fxy, -1)
    fisheye = isinstance(name_or_maps, str) and rig(name_or_maps)["left"]["model"] == ref.FISHEYE
    if not fisheye:
        return [] if not differs.any() else ["%d entries differ" % differs.sum()]
    tie = ref.near_tie(*fm[side_idx])
    out = []
    if tie.sum() > cap * tie.size:
        out.append("the reference itself has %d near-tie pixels" % tie.sum())
    if (differs & ~tie).any():
        out.append("%d entries differ away from a tie" % (differs & ~tie).sum())
    return out


def side_bytes(s):
    D = list(s["D"]) + [0.0] * (8 - len(s["D"]))
    return struct.pack("<ii", s["model"], s.get("n_dist", len(s["D"]))) + struct.pack("<9d", *s["K"]) + struct.pack("<8d", *D) + struct.pack("<9d", *s["R"])


def write_case(path, images, order, rectify, P, sides):
    """A case file of imgprep_host: images = [left] or [left, right], dense uint8 arrays of one shape."""
    rows, cols = images[0].shape[:2]
    channels = 1 if images[0].ndim == 2 else images[0].shape[2]
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", rows, cols, channels, order, 1 if rectify else 0, len(images)))
        f.write(struct.pack("<4d", *P))
        for s in sides[:len(images)]:
            f.write(side_bytes(s))
        for im in images:
            f.write(np.ascontiguousarray(im).tobytes())


def read_out(path, rows, cols, nsides, rectify):
    """[(ixy | None, fxy | None, gray)] per side from imgprep_host's output file."""
    raw = np.fromfile(path, np.uint8)
    out, off, n = [], 0, rows * cols
    for _ in range(nsides):
        ixy = fxy = None
        if rectify:
            ixy = raw[off:off + 4 * n].view(np.int16).reshape(rows, cols, 2)
            off += 4 * n
            fxy = raw[off:off + 2 * n].reshape(rows, cols, 2)
            off += 2 * n
        out.append((ixy, fxy, raw[off:off + n].reshape(rows, cols)))
        off += n
    assert off == raw.size
    return out


def host_program():
    """Builds (by name) and returns openvslam_amd/cpp/imgprep_host."""
    subprocess.run(["make", "-C", CPP, "imgprep_host"], check=True, capture_output=True)
    return os.path.join(CPP, "imgprep_host")
