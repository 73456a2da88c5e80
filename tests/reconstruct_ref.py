"""Sequential restatement of the monocular initialiser's pose recovery, initialize::perspective's reconstruct_with_H / reconstruct_with_F with
check_pose and find_most_plausible_pose, as DESIGN.md 3.15 fixes them (rules R1 to R12): one hypothesis after the other, one match after the
other. Pure Python on purpose: a Python float is an IEEE f64 and every operation below rounds once, so the results are the bits the rules ask
for; the few float values are narrowed with struct. No numpy in the arithmetic; imports nothing of the product.

A problem is a dict: model (1: H_21, 2: F_21), mat (9, row-major), cam (fx, fy, cx, cy), inlier (n flags), kp1, kp2 (n 2-tuples: the
undistorted keypoints of the reference and the current frame), b1, b2 (n 3-tuples: their bearings)."""
import math
import struct

from pnp_ref import jacobi, off_ratio
from sim3_ref import _div, _sqrt, bits, dot3, f32

SWEEPS = 8
MODEL_H, MODEL_F = 1, 2
COS_SMALL = f32(0.99996192306)
RATIO_MIN = 1.00001
PARALLAX_INDEX = 50
PI = 3.14159265358979323846
NAN = float("nan")


# ---- the conventions: a 3 x 3 matrix is a list of 9, row-major
def mul3(A, B):
    return [dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]) for r in range(3) for c in range(3)]


def transpose3(A):
    return [A[3 * c + r] for r in range(3) for c in range(3)]


def det3(M):
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6])


def _from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


# ---- ovs_det_acos of include/ovs_detmath.h, operation for operation
def _asin_pq(t):
    p = t * (1.66666666666666657415e-01 + t * (-3.25565818622400915405e-01 + t * (2.01212532134862925881e-01 + t * (
        -4.00555345006794114027e-02 + t * (7.91534994289814532176e-04 + t * 3.47933107596021167570e-05)))))
    q = 1.0 + t * (-2.40339491173441421878e+00 + t * (2.02094576023350569471e+00 + t * (-6.88283971605453293030e-01 + t * 7.70381505559019352791e-02)))
    return p / q


def det_acos(x):
    pi, pio2_hi, pio2_lo = 3.14159265358979311600e+00, 1.57079632679489655800e+00, 6.12323399573676603587e-17
    if x != x:
        return x + x
    ax, neg = abs(x), math.copysign(1.0, x) < 0.0
    if ax >= 1.0:
        if ax == 1.0:
            return pi + 2.0 * pio2_lo if neg else 0.0
        return NAN
    if ax < 0.5:
        if ax < 6.938893903907228e-18:
            return pio2_hi + pio2_lo
        z = x * x
        r = _asin_pq(z)
        return pio2_hi - (x - (pio2_lo - x * r))
    if neg:
        z = (1.0 + x) * 0.5
        r = _asin_pq(z)
        s = math.sqrt(z)
        w = r * s - pio2_lo
        return pi - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = _from_bits(bits(s) & 0xffffffff00000000)
    c = (z - df * df) / (s + df)
    r = _asin_pq(z)
    w = r * s + c
    return 2.0 * (df + w)


# ---- R2
def svd3(M, cross_third, stats=None, eig=None):
    """(U, V, d) of M = U diag(d) V^T: U and V lists of 9, row-major. `eig`, if given, replaces the sweeps: M^T M -> (diagonal, V rows)."""
    B = [[dot3(M[i], M[3 + i], M[6 + i], M[j], M[3 + j], M[6 + j]) for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(i):
            B[i][j] = B[j][i]
    A, V = jacobi(B, SWEEPS)
    if stats is not None:
        stats["off"] = max(stats.get("off", 0.0), off_ratio(B, A))
    lam = [A[0][0], A[1][1], A[2][2]]
    for a, b in ((0, 1), (1, 2), (0, 1)):
        if lam[a] < lam[b]:
            lam[a], lam[b] = lam[b], lam[a]
            for r in range(3):
                V[r][a], V[r][b] = V[r][b], V[r][a]
    d = [_sqrt(v) for v in lam]
    U = [_div(dot3(M[3 * r], M[3 * r + 1], M[3 * r + 2], V[0][k], V[1][k], V[2][k]), d[k]) for r in range(3) for k in range(3)]
    if cross_third:
        U[2] = U[3] * U[7] - U[6] * U[4]
        U[5] = U[6] * U[1] - U[0] * U[7]
        U[8] = U[0] * U[4] - U[3] * U[1]
    return U, [V[r][k] for r in range(3) for k in range(3)], d


def _hyp(R, t):
    c = [-dot3(R[k], R[3 + k], R[6 + k], t[0], t[1], t[2]) for k in range(3)]
    return dict(R=R, t=t, c=c)


def _K(cam):
    fx, fy, cx, cy = cam
    return [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0]


# ---- R3, R4
def hypotheses_of_H(prob, stats=None, margin=None):
    fx, fy, cx, cy = prob["cam"]
    ifx, ify = _div(1.0, fx), _div(1.0, fy)
    Kinv = [ifx, 0.0, -(cx * ifx), 0.0, ify, -(cy * ify), 0.0, 0.0, 1.0]
    A = mul3(Kinv, mul3(prob["mat"], _K(prob["cam"])))
    U, V, d = svd3(A, False, stats)
    Vt = transpose3(V)
    sign = det3(U) * det3(Vt)
    d1, d2, d3 = d
    ratios = (_div(d1, d2), _div(d2, d3))
    if margin is not None:
        for v in ratios:
            if math.isfinite(v):
                margin["ratio"] = min(margin.get("ratio", math.inf), abs(v - RATIO_MIN) / RATIO_MIN)
    if ratios[0] < RATIO_MIN or ratios[1] < RATIO_MIN:
        return []
    q1, q2, q3 = d1 * d1, d2 * d2, d3 * d3
    aux1, aux3 = _sqrt(_div(q1 - q2, q1 - q3)), _sqrt(_div(q2 - q3, q1 - q3))
    root = _sqrt((q1 - q2) * (q2 - q3))
    out = []
    for h in range(8):
        x1 = -aux1 if h & 2 else aux1
        x3 = -aux3 if h & 1 else aux3
        minus, second = ((h >> 1) ^ h) & 1, h >= 4
        den = (d1 - d3) * d2 if second else (d1 + d3) * d2
        aux_s = _div(root, den)
        sn = -aux_s if minus else aux_s
        cs = _div(d1 * d3 - q2, den) if second else _div(q2 + d1 * d3, den)
        Rp = [cs, 0.0, sn if second else -sn, 0.0, -1.0 if second else 1.0, 0.0, sn, 0.0, -cs if second else cs]
        R = [sign * v for v in mul3(U, mul3(Rp, Vt))]
        scale = d1 + d3 if second else d1 - d3
        tp = (x1 * scale, 0.0 * scale, (x3 if second else -x3) * scale)
        t = [dot3(U[3 * r], U[3 * r + 1], U[3 * r + 2], *tp) for r in range(3)]
        nrm = _sqrt(dot3(t[0], t[1], t[2], t[0], t[1], t[2]))
        out.append(_hyp(R, [_div(v, nrm) for v in t]))
    return out


# ---- R5
def hypotheses_of_F(prob, stats=None):
    K = _K(prob["cam"])
    E = mul3(transpose3(K), mul3(prob["mat"], K))
    U, V, d = svd3(E, True, stats)
    Vt = transpose3(V)
    t = [U[2], U[5], U[8]]
    nrm = _sqrt(dot3(t[0], t[1], t[2], t[0], t[1], t[2]))
    t = [_div(v, nrm) for v in t]
    out = []
    for h in range(4):
        w = -1.0 if h & 2 else 1.0
        R = mul3(U, mul3([0.0, -w, 0.0, w, 0.0, 0.0, 0.0, 0.0, 1.0], Vt))
        if det3(R) < 0.0:
            R = [-v for v in R]
        out.append(_hyp(R, [-v for v in t] if h & 1 else t[:]))
    return out


def hypotheses(prob, stats=None, margin=None):
    return hypotheses_of_H(prob, stats, margin) if prob["model"] == MODEL_H else hypotheses_of_F(prob, stats)


def _note(margin, key, value, threshold):
    """The smallest relative distance of a finite value from its threshold (absolute where the threshold is 0)."""
    if margin is not None and math.isfinite(value):
        scale = abs(threshold) if threshold != 0.0 else 1.0
        margin[key] = min(margin.get(key, math.inf), abs(value - threshold) / scale)


# ---- R6 to R9
def check_match(prob, hyp, i, thr_sq, margin=None):
    """None, or (pos, cos, small) of match i under the hypothesis."""
    R, t, c = hyp["R"], hyp["t"], hyp["c"]
    fx, fy, cx, cy = prob["cam"]
    b1, bc = prob["b1"][i], prob["b2"][i]
    b2 = [dot3(R[k], R[3 + k], R[6 + k], bc[0], bc[1], bc[2]) for k in range(3)]
    d12 = dot3(b1[0], b1[1], b1[2], *b2)
    a00, a01, a10, a11 = dot3(b1[0], b1[1], b1[2], *b1), -d12, d12, -dot3(b2[0], b2[1], b2[2], *b2)
    r0, r1 = dot3(b1[0], b1[1], b1[2], *c), dot3(b2[0], b2[1], b2[2], *c)
    det = a00 * a11 - a01 * a10
    lam0, lam1 = _div(a11 * r0 - a01 * r1, det), _div(a00 * r1 - a10 * r0, det)
    pos = [_div((lam0 * b1[k] + lam1 * b2[k]) + c[k], 2.0) for k in range(3)]
    if not all(math.isfinite(v) for v in pos):
        return None
    n2 = [pos[k] - c[k] for k in range(3)]
    cosd = _div(dot3(pos[0], pos[1], pos[2], *n2), _sqrt(dot3(pos[0], pos[1], pos[2], *pos)) * _sqrt(dot3(n2[0], n2[1], n2[2], *n2)))
    if cosd != cosd:
        return None
    cosf = f32(cosd)
    _note(margin, "cos", cosd, COS_SMALL)
    small = COS_SMALL <= cosf
    pc = [dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], *pos) + t[r] for r in range(3)]
    if not small:
        _note(margin, "depth", pos[2], 0.0)
        if not pos[2] > 0.0:
            return None
        _note(margin, "depth", pc[2], 0.0)
        if not pc[2] > 0.0:
            return None
    ex, ey = (_div(fx * pos[0], pos[2]) + cx) - prob["kp1"][i][0], (_div(fy * pos[1], pos[2]) + cy) - prob["kp1"][i][1]
    err = ex * ex + ey * ey
    _note(margin, "reproj", err, thr_sq)
    if not err <= thr_sq:
        return None
    ex, ey = (_div(fx * pc[0], pc[2]) + cx) - prob["kp2"][i][0], (_div(fy * pc[1], pc[2]) + cy) - prob["kp2"][i][1]
    err = ex * ex + ey * ey
    _note(margin, "reproj", err, thr_sq)
    if not err <= thr_sq:
        return None
    return pos, cosf, small


def key_of(x):
    """R10: the order-preserving integer key of a float."""
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def parallax_deg(cosines, info=None):
    """R10 over a hypothesis's list of float cosines."""
    if not cosines:
        return 0.0
    ordered = sorted(cosines, key=key_of)
    idx = min(PARALLAX_INDEX, len(ordered) - 1)
    if info is not None:
        around = ordered[max(0, idx - 1):idx + 2]
        info["distinct"] = info.get("distinct", True) and len(set(around)) == len(around)
    return f32(_div(det_acos(ordered[idx]) * 180.0, PI))


def check_pose(prob, hyp, thr_sq, margin=None, info=None):
    """(count, parallax, pos per match, flag per match) of one hypothesis."""
    n = len(prob["inlier"])
    pts, flags, cosines = [[0.0, 0.0, 0.0] for _ in range(n)], [0] * n, []
    for i in range(n):
        if not prob["inlier"][i]:
            continue
        got = check_match(prob, hyp, i, thr_sq, margin)
        if got is None:
            continue
        pts[i], cos, small = got[0], got[1], got[2]
        flags[i] = 0 if small else 1
        cosines.append(cos)
    return len(cosines), parallax_deg(cosines, info), pts, flags


def failed(n):
    return dict(success=0, best=-1, R=[0.0] * 9, t=[0.0] * 3, counts=[0] * 8, parallax=[0.0] * 8, pts=[[0.0, 0.0, 0.0] for _ in range(n)], flags=[0] * n)


# ---- R11
def most_plausible(counts, parallax, parallax_deg_thr, min_num_triangulated, margin=None):
    if not counts:
        return -1
    best = 0
    for h in range(1, len(counts)):
        if counts[best] < counts[h]:
            best = h
    most = counts[best]
    if most < min_num_triangulated:
        return -1
    for c in counts:
        _note(margin, "similar", 0.8 * float(most), float(c)) if c else None
    if sum(1 for c in counts if 0.8 * float(most) < float(c)) > 1:
        return -1
    _note(margin, "parallax", parallax[best], parallax_deg_thr)
    if not parallax[best] >= parallax_deg_thr:
        return -1
    return best


def reconstruct(prob, reproj_err_thr=4.0, parallax_deg_thr=1.0, min_num_triangulated=50, margin=None, stats=None, info=None):
    """The whole call for one problem: dict success, best, R, t, counts (8), parallax (8, floats held as f64), pts (n x 3), flags (n)."""
    n = len(prob["inlier"])
    thr = f32(reproj_err_thr)
    thr_sq = f32(thr * thr)
    hyps = hypotheses(prob, stats, margin)
    res = [check_pose(prob, hyp, thr_sq, margin, info) for hyp in hyps]
    out = failed(n)
    for h, r in enumerate(res):
        out["counts"][h], out["parallax"][h] = r[0], r[1]
    best = most_plausible([r[0] for r in res], [r[1] for r in res], f32(parallax_deg_thr), min_num_triangulated, margin)
    if best >= 0:
        out.update(success=1, best=best, R=hyps[best]["R"][:], t=hyps[best]["t"][:], pts=res[best][2], flags=res[best][3])
    return out


def as_bits(r):
    """A result with its doubles as uint64 bit patterns (the parallaxes are floats: their f64 value compares as it is)."""
    return dict(success=r["success"], best=r["best"], R=[bits(v) for v in r["R"]], t=[bits(v) for v in r["t"]], counts=list(r["counts"]),
                parallax=[bits(float(v)) for v in r["parallax"]], pts=[[bits(v) for v in p] for p in r["pts"]], flags=list(r["flags"]))
