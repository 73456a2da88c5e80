"""The image front end's rules I1 to I8 restated in numpy, every f64 operation rounded on its own and every sum taken from left
to right, plus a second restatement of rule I7 in exact rational arithmetic. The tests hold the host program (tests/imgprep_host.cc), the library
and the class layers to this file. The fisheye model's atan here is numpy's, the library's is include/ovs_detmath.h's: near_tie() names the pixels
where that may show."""
import math
from fractions import Fraction

import numpy as np

GRAY, RGB, BGR = 0, 1, 2
PERSPECTIVE, FISHEYE = 0, 1
FAR = -32768


def gray_weights(order):
    return {RGB: (4899, 9617, 1868), BGR: (1868, 9617, 4899)}[order]


def gray(img, order):
    """I1: (rows, cols) passes through; (rows, cols, 3 | 4) by the integer weights, alpha ignored."""
    img = np.asarray(img)
    if img.ndim == 2:
        return img.copy()
    w = gray_weights(order)
    c = img.astype(np.int64)
    return ((c[..., 0] * w[0] + c[..., 1] * w[1] + c[..., 2] * w[2] + 8192) >> 14).astype(np.uint8)


def inverse_PR(R, P):
    """I3: (P R)^-1 by the adjugate over the determinant, or None for a singular product. R: 9 doubles row-major, P: fx fy cx cy."""
    R = [np.float64(v) for v in R]
    fx, fy, cx, cy = (np.float64(v) for v in P)
    M = [None] * 9
    for j in range(3):
        M[j] = fx * R[j] + cx * R[6 + j]
        M[3 + j] = fy * R[3 + j] + cy * R[6 + j]
        M[6 + j] = R[6 + j]
    c = [M[4] * M[8] - M[5] * M[7], M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
         M[5] * M[6] - M[3] * M[8], M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
         M[3] * M[7] - M[4] * M[6], M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]]
    det = M[0] * c[0] + M[1] * c[3] + M[2] * c[6]
    if not np.isfinite(det) or det == 0.0:
        return None
    with np.errstate(all="ignore"):
        iR = [v / det for v in c]
    return iR if all(np.isfinite(v) for v in iR) else None


def float_map(side, P, rows, cols):
    """I3 / I4: (map_x, map_y) as float32 arrays. side: dict(model, K (9), D (0, 4, 5 or 8 values), R (9))."""
    iR = inverse_PR(side["R"], P)
    assert iR is not None
    K = [np.float64(v) for v in side["K"]]
    k = [np.float64(v) for v in list(side["D"]) + [0.0] * (8 - len(side["D"]))]
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        X = iR[0] * u + iR[1] * v + iR[2]
        Y = iR[3] * u + iR[4] * v + iR[5]
        W = iR[6] * u + iR[7] * v + iR[8]
        x, y = X / W, Y / W
        fxK, fyK, cxK, cyK = K[0], K[4], K[2], K[5]
        if side["model"] == PERSPECTIVE:
            k1, k2, p1, p2, k3, k4, k5, k6 = k
            r2 = x * x + y * y
            kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            mx, my = fxK * xd + cxK, fyK * yd + cyK
        else:
            r = np.sqrt(x * x + y * y)
            th = np.arctan(r)
            t2 = th * th
            thd = th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
            scale = np.where(r == 0.0, 1.0, thd / r)
            mx, my = fxK * x * scale + cxK, fyK * y * scale + cyK
        return mx.astype(np.float32), my.astype(np.float32)


def fix_coord(m):
    """I5 for one coordinate array (float32): (integer part saturated to int16, 5-bit fraction)."""
    with np.errstate(all="ignore"):
        s = np.asarray(m, np.float32) * np.float32(32.0)
        far = ~(np.abs(s) <= np.float32(2.0 ** 30))
    q = np.rint(np.where(far, np.float32(0), s)).astype(np.int64)   # ties to even
    ip = np.clip(q >> 5, -32768, 32767)
    fr = q & 31
    return np.where(far, FAR, ip).astype(np.int16), np.where(far, 0, fr).astype(np.uint8)


def fix_maps(map_x, map_y):
    """The resident map as the ABI's getter returns it: ixy (rows, cols, 2) int16 and fxy (rows, cols, 2) uint8."""
    ix, fx = fix_coord(map_x)
    iy, fy = fix_coord(map_y)
    return np.stack([ix, iy], -1), np.stack([fx, fy], -1)


def near_tie(map_x, map_y, eps=1e-6):
    """Pixels whose 32 * map lies within eps of a rounding tie of I5 in either coordinate."""
    out = np.zeros(np.shape(map_x), bool)
    for m in (map_x, map_y):
        with np.errstate(all="ignore"):
            s = (np.asarray(m, np.float32) * np.float32(32.0)).astype(np.float64)
        ok = np.isfinite(s)
        frac = np.where(ok, s - np.floor(np.where(ok, s, 0.0)), 0.0)
        out |= ok & (np.abs(frac - 0.5) <= eps)
    return out


def remap(src, ixy, fxy):
    """I6 + I7 on every channel of src ((rows, cols) or (rows, cols, channels)), rounded to bytes."""
    src = np.asarray(src)
    rows, cols = src.shape[:2]
    s = src.reshape(rows, cols, -1).astype(np.int64)
    ix, iy = ixy[..., 0].astype(np.int64), ixy[..., 1].astype(np.int64)
    fx, fy = fxy[..., 0].astype(np.int64), fxy[..., 1].astype(np.int64)

    def tap(x, y):
        inside = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
        v = s[np.where(inside, y, 0), np.where(inside, x, 0)]
        return np.where(inside[..., None], v, 0)

    w = [(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy]
    t = [tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)]
    acc = w[0][..., None] * t[0]
    for k in (1, 2, 3):
        acc = acc + w[k][..., None] * t[k]
    out = ((acc + 512) >> 10).astype(np.uint8)
    return out.reshape(src.shape)


def prepare(src, order, fixed=None):
    """The whole front end for one image: I2's order (remap every channel, round, then gray)."""
    return gray(remap(src, *fixed) if fixed is not None else src, order)


def prepare_gray_first(src, order, fixed):
    """The OTHER order (gray, then remap): what rule I2 says the library does not compute."""
    return remap(gray(src, order), *fixed)


def blend_exact(p, fx, fy):
    """I7 in exact rational arithmetic: floor(sum of w_k p_k / 1024 + 1/2), weights as fractions of 32."""
    a, b = Fraction(int(fx), 32), Fraction(int(fy), 32)
    v = (1 - a) * (1 - b) * int(p[0]) + a * (1 - b) * int(p[1]) + (1 - a) * b * int(p[2]) + a * b * int(p[3])
    return math.floor(v + Fraction(1, 2))


def blend(p, fx, fy):
    """I7 in the integers, for four taps."""
    fx, fy = int(fx), int(fy)
    return ((32 - fx) * (32 - fy) * int(p[0]) + fx * (32 - fy) * int(p[1]) + (32 - fx) * fy * int(p[2]) + fx * fy * int(p[3]) + 512) >> 10
