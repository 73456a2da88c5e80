"""Sequential restatement of solve::sim3_solver::find_via_ransac as DESIGN.md 3.9 fixes it (rules 1 to 4): one hypothesis after the other, one
match after the other. Pure Python on purpose: a Python float is an IEEE f64 and every operation below rounds once, so the results are the
bits the rules ask for. No numpy in the arithmetic; imports nothing of the product. asin / atan2 of the equirectangular projection are
include/ovs_detmath.h's, evaluated through the oracle library.

A problem is a dict: p1, p2 (lists of 3-tuples), thr1, thr2 (lists of floats that hold f32 values), cam_1, cam_2 (dicts: model 0 with
fx fy cx cy, or model 1 with cols rows)."""
import math
import struct

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def f32(x):
    """(float)x: narrow an f64 to the nearest f32, returned as the f64 that holds it."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- rule 1
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, p, h, n):
    base = (seed + G * ((((p << 20) + h) * 4 + 1) & MASK)) & MASK
    r = [mix((base + G * c) & MASK) for c in range(3)]
    i0 = r[0] % n
    i1 = r[1] % (n - 1)
    if i1 >= i0:
        i1 += 1
    i2 = r[2] % (n - 2)
    if i2 >= min(i0, i1):
        i2 += 1
    if i2 >= max(i0, i1):
        i2 += 1
    return i0, i1, i2


# ---- rule 2
def horn_N(a, b):
    """The symmetric 4 x 4 matrix of Horn's method from the centred points a (side 1) and b (side 2), as a full matrix."""
    M = [[(b[0][r] * a[0][c] + b[1][r] * a[1][c]) + b[2][r] * a[2][c] for c in range(3)] for r in range(3)]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2]
    N[0][1] = M[1][2] - M[2][1]
    N[0][2] = M[2][0] - M[0][2]
    N[0][3] = M[0][1] - M[1][0]
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2]
    N[1][2] = M[0][1] + M[1][0]
    N[1][3] = M[2][0] + M[0][2]
    N[2][2] = (-M[0][0] + M[1][1]) - M[2][2]
    N[2][3] = M[1][2] + M[2][1]
    N[3][3] = (-M[0][0] - M[1][1]) + M[2][2]
    for r in range(4):
        for c in range(r):
            N[r][c] = N[c][r]
    return N


def jacobi(N, sweeps=SWEEPS):
    """Cyclic Jacobi, the rotation of csrc/jacobi_math.inc (jacobi_angle), a fixed number of sweeps: (A, V), A nearly diagonal, V's columns the vectors."""
    A = [row[:] for row in N]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(4):
                akp, akq = A[k][p], A[k][q]
                A[k][p] = c * akp - s * akq
                A[k][q] = s * akp + c * akq
            for k in range(4):
                apk, aqk = A[p][k], A[q][k]
                A[p][k] = c * apk - s * aqk
                A[q][k] = s * apk + c * aqk
            for k in range(4):
                vkp, vkq = V[k][p], V[k][q]
                V[k][p] = c * vkp - s * vkq
                V[k][q] = s * vkp + c * vkq
    return A, V


def rotation_of(w, x, y, z):
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else float("nan")   # (math.sqrt raises where IEEE returns NaN; NaN >= 0 is false too)


def _div(a, b):
    """IEEE a / b where Python raises: x / 0 is +-inf, 0 / 0 and NaN / 0 are NaN."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def horn(P1, P2, fix_scale, eig=None):
    """Horn's closed form on three point pairs: dict with R (9, row-major), t12, s12, s21, t21, N, A (the matrix after the sweeps).
    `eig`, if given, replaces the Jacobi iteration: N -> quaternion (w, x, y, z) (the N-version check)."""
    c1 = [((P1[0][x] + P1[1][x]) + P1[2][x]) / 3.0 for x in range(3)]
    c2 = [((P2[0][x] + P2[1][x]) + P2[2][x]) / 3.0 for x in range(3)]
    a = [[P1[k][x] - c1[x] for x in range(3)] for k in range(3)]
    b = [[P2[k][x] - c2[x] for x in range(3)] for k in range(3)]
    N = horn_N(a, b)
    A = None
    if eig is None:
        A, V = jacobi(N)
        best = 0
        for i in range(1, 4):
            if A[i][i] > A[best][best]:
                best = i
        q0, q1, q2, q3 = V[0][best], V[1][best], V[2][best], V[3][best]
    else:
        q0, q1, q2, q3 = eig(N)
    nrm = _sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
    w, x, y, z = _div(q0, nrm), _div(q1, nrm), _div(q2, nrm), _div(q3, nrm)
    R = rotation_of(w, x, y, z)
    if fix_scale:
        s12 = 1.0
    else:
        num, den = [], []
        for k in range(3):
            r0 = dot3(R[0], R[1], R[2], *b[k])
            r1 = dot3(R[3], R[4], R[5], *b[k])
            r2 = dot3(R[6], R[7], R[8], *b[k])
            num.append(dot3(a[k][0], a[k][1], a[k][2], r0, r1, r2))
            den.append(dot3(r0, r1, r2, r0, r1, r2))
        s12 = _div((num[0] + num[1]) + num[2], (den[0] + den[1]) + den[2])
    t12 = [c1[r] - s12 * dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], *c2) for r in range(3)]
    s21 = _div(1.0, s12)
    t21 = [-s21 * dot3(R[r], R[3 + r], R[6 + r], *t12) for r in range(3)]
    return dict(R=R, t12=t12, s12=s12, s21=s21, t21=t21, N=N, A=A)


# ---- rule 3
def _detmath(fn, a, b=None):
    from oracle import binding as ob
    return float(ob.detmath_eval(fn, [a], None if b is None else [b])[0])


def project(cam, x, y, z):
    if cam["model"] == 0:
        return _div(cam["fx"] * x, z) + cam["cx"], _div(cam["fy"] * y, z) + cam["cy"]
    L = _sqrt((x * x + y * y) + z * z)
    theta = _detmath(3, x, z)               # OVS_DETMATH_ATAN2
    phi = -_detmath(1, _div(y, L))          # OVS_DETMATH_ASIN
    return float(cam["cols"]) * (0.5 + theta / (2.0 * math.pi)), float(cam["rows"]) * (0.5 - phi / math.pi)


def inlier(prob, obs, m, i):
    """(is inlier, e1, e2) of match i under model m; obs[i] = (u1, u2), the match's own projections."""
    p1, p2, R = prob["p1"][i], prob["p2"][i], m["R"]
    x1 = m["s12"] * dot3(R[0], R[1], R[2], *p2) + m["t12"][0]
    y1 = m["s12"] * dot3(R[3], R[4], R[5], *p2) + m["t12"][1]
    z1 = m["s12"] * dot3(R[6], R[7], R[8], *p2) + m["t12"][2]
    x2 = m["s21"] * dot3(R[0], R[3], R[6], *p1) + m["t21"][0]
    y2 = m["s21"] * dot3(R[1], R[4], R[7], *p1) + m["t21"][1]
    z2 = m["s21"] * dot3(R[2], R[5], R[8], *p1) + m["t21"][2]
    v1 = project(prob["cam_1"], x1, y1, z1)
    v2 = project(prob["cam_2"], x2, y2, z2)
    (u1, u2) = obs[i]
    d1x, d1y, d2x, d2y = u1[0] - v1[0], u1[1] - v1[1], u2[0] - v2[0], u2[1] - v2[1]
    e1 = d1x * d1x + d1y * d1y
    e2 = d2x * d2x + d2y * d2y
    ok = e1 < prob["thr1"][i] and e2 < prob["thr2"][i]
    if prob["cam_1"]["model"] == 0:
        ok = ok and p1[2] > 0.0 and z1 > 0.0
    if prob["cam_2"]["model"] == 0:
        ok = ok and p2[2] > 0.0 and z2 > 0.0
    return ok, e1, e2


def observations(prob):
    return [(project(prob["cam_1"], *prob["p1"][i]), project(prob["cam_2"], *prob["p2"][i])) for i in range(len(prob["p1"]))]


def hypothesis(prob, seed, p, h, fix_scale, eig=None):
    n = len(prob["p1"])
    idx = sample(seed, p, h, n)
    return horn([prob["p1"][i] for i in idx], [prob["p2"][i] for i in idx], fix_scale, eig)


def flags_of(prob, obs, m):
    return [1 if inlier(prob, obs, m, i)[0] else 0 for i in range(len(prob["p1"]))]


def evaluate(prob, seed, max_num_iter, fix_scale, p=0, eig=None):
    """Every hypothesis h < max_num_iter of problem index p: (inlier counts per h, margin, worst off-diagonal ratio), margin being the smallest
    |e - thr| / thr over every (hypothesis, match, side) with a finite e, the ratio the largest off-diagonal norm of the swept matrix over max|N|."""
    n = len(prob["p1"])
    if n < 3:
        return [], float("inf"), 0.0
    obs = observations(prob)
    counts, margin, off = [], float("inf"), 0.0
    for h in range(max_num_iter):
        m = hypothesis(prob, seed, p, h, fix_scale, eig)
        if m["A"] is not None:
            scale = max(abs(v) for row in m["N"] for v in row)
            norm = math.sqrt(sum(m["A"][r][c] ** 2 for r in range(4) for c in range(4) if r != c))
            if scale > 0.0 and norm == norm:
                off = max(off, norm / scale)
        c = 0
        for i in range(n):
            ok, e1, e2 = inlier(prob, obs, m, i)
            c += 1 if ok else 0
            for e, thr in ((e1, prob["thr1"][i]), (e2, prob["thr2"][i])):
                if math.isfinite(e) and thr > 0.0:
                    margin = min(margin, abs(e - thr) / thr)
        counts.append(c)
    return counts, margin, off


INVALID = dict(valid=0, best_iter=-1, num_inliers=0, R=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], t=[0.0, 0.0, 0.0], s=1.0)


def finish(prob, counts, seed, fix_scale, min_num_inliers, p=0):
    """Rule 4 over the counts of hypotheses 0 .. len(counts) - 1: the result dict (valid, best_iter, num_inliers, R, t, s, flags)."""
    n = len(prob["p1"])
    best_iter, best = -1, -1
    for h, c in enumerate(counts):
        if best < c:            # strict: the lowest h of a tie stays
            best, best_iter = c, h
    if not (n >= 3 and n >= min_num_inliers and best >= min_num_inliers):
        return dict(INVALID, flags=[0] * n)
    m = hypothesis(prob, seed, p, best_iter, fix_scale)
    return dict(valid=1, best_iter=best_iter, num_inliers=best, R=m["R"], t=m["t12"], s=m["s12"], flags=flags_of(prob, observations(prob), m))


def find_via_ransac(prob, max_num_iter, seed, fix_scale, min_num_inliers=20, p=0):
    """The whole solver: (result dict, margin)."""
    counts, margin, _ = evaluate(prob, seed, max_num_iter, fix_scale, p)
    return finish(prob, counts, seed, fix_scale, min_num_inliers, p), margin
