"""Sequential restatement of solve::pnp_solver::find_via_ransac as DESIGN.md 3.10 fixes it (rules 1 to 6): one hypothesis after the other, one
match after the other. Pure Python on purpose: a Python float is an IEEE f64 and every operation below rounds once, so the results are the
bits the rules ask for. No numpy in the arithmetic; imports nothing of the product.

A problem is a dict: bearings, pos_w (lists of 3-tuples), max_cos_error (list of floats)."""
import math

from sim3_ref import G, MASK, _div, _sqrt, bits, dot3, mix, rotation_of   # the shared pieces: the mixer, IEEE division and square root

SWEEPS = 8                 # every symmetric eigenproblem: 3 x 3, 12 x 12 and Horn's 4 x 4
LANES = 64                 # rule 6: the number of strided partial sums
PAIRS6 = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
NAN = float("nan")


# ---- rule 1
def sample(seed, p, h, n):
    base = (seed + G * ((((p << 20) + h) * 8 + 1) & MASK)) & MASK
    idx = []
    for c in range(4):
        i = mix((base + G * c) & MASK) % (n - c)
        for e in sorted(idx):
            if i >= e:
                i += 1
        idx.append(i)
    return tuple(idx)


# ---- rule 6
def tsum(terms):
    """The one order of every sum over matches: 64 partial sums, partial j over the terms j, j + 64, ... in rank order from 0.0, then the
    pairwise tree part[j] += part[j + d] for d = 32, 16, ... 1."""
    part = [0.0] * LANES
    for i, t in enumerate(terms):
        part[i % LANES] = part[i % LANES] + t
    d = LANES // 2
    while d:
        for j in range(d):
            part[j] = part[j] + part[j + d]
        d //= 2
    return part[0]


# ---- rule 2
def jacobi(N, sweeps=SWEEPS):
    """Cyclic Jacobi of any size, the rotation of DESIGN.md 3.9 rule 2, row-major pair order, a fixed number of sweeps: (A, V)."""
    m = len(N)
    A = [row[:] for row in N]
    V = [[1.0 if r == c else 0.0 for c in range(m)] for r in range(m)]
    for _ in range(sweeps):
        for p in range(m - 1):
            for q in range(p + 1, m):
                apq = A[p][q]
                if apq == 0.0:          # (a NaN is not 0: it rotates and spreads)
                    continue
                theta = _div(A[q][q] - A[p][p], 2.0 * apq)
                t = _div(1.0 if theta >= 0 else -1.0, abs(theta) + _sqrt(theta * theta + 1.0))
                c = _div(1.0, _sqrt(t * t + 1.0))
                s = t * c
                for k in range(m):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(m):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                for k in range(m):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return A, V


def off_ratio(N, A):
    scale = max(abs(v) for row in N for v in row)
    m = len(N)
    norm = math.sqrt(sum(A[r][c] * A[r][c] for r in range(m) for c in range(m) if r != c))
    return norm / scale if scale > 0.0 and norm == norm and scale != float("inf") else 0.0


def ls_solve(rows, b):
    """min |rows x - b| for 6 rows of K columns: the normal equations, every entry a left-to-right sum of its six products, Gaussian elimination
    without pivoting, back substitution."""
    K = len(rows[0])

    def acc(f):
        s = f(0)
        for i in range(1, 6):
            s = s + f(i)
        return s
    N = [[acc(lambda i: rows[i][r] * rows[i][c]) for c in range(K)] for r in range(K)]
    g = [acc(lambda i: rows[i][r] * b[i]) for r in range(K)]
    for k in range(K):
        for r in range(k + 1, K):
            f = _div(N[r][k], N[k][k])
            for c in range(k + 1, K):
                N[r][c] = N[r][c] - f * N[k][c]
            g[r] = g[r] - f * g[k]
    x = [0.0] * K
    for r in range(K - 1, -1, -1):
        s = g[r]
        for c in range(r + 1, K):
            s = s - N[r][c] * x[c]
        x[r] = _div(s, N[r][r])
    return x


def inverse3(C):
    m00 = C[1][1] * C[2][2] - C[1][2] * C[2][1]
    m01 = C[1][2] * C[2][0] - C[1][0] * C[2][2]
    m02 = C[1][0] * C[2][1] - C[1][1] * C[2][0]
    det = (C[0][0] * m00 + C[0][1] * m01) + C[0][2] * m02
    return [[_div(m00, det), _div(C[0][2] * C[2][1] - C[0][1] * C[2][2], det), _div(C[0][1] * C[1][2] - C[0][2] * C[1][1], det)],
            [_div(m01, det), _div(C[0][0] * C[2][2] - C[0][2] * C[2][0], det), _div(C[0][2] * C[1][0] - C[0][0] * C[1][2], det)],
            [_div(m02, det), _div(C[0][1] * C[2][0] - C[0][0] * C[2][1], det), _div(C[0][0] * C[1][1] - C[0][1] * C[1][0], det)]]


def betas_approx(which, L, rho, lsq):
    if which == 0:
        b4 = lsq([[r[0], r[1], r[3], r[6]] for r in L], rho)
        if b4[0] < 0:
            b0 = _sqrt(-b4[0])
            return [b0, _div(-b4[1], b0), _div(-b4[2], b0), _div(-b4[3], b0)]
        b0 = _sqrt(b4[0])
        return [b0, _div(b4[1], b0), _div(b4[2], b0), _div(b4[3], b0)]
    if which == 1:
        b3 = lsq([[r[0], r[1], r[2]] for r in L], rho)
    else:
        b3 = lsq([[r[0], r[1], r[2], r[3], r[4]] for r in L], rho)
    if b3[0] < 0:
        b0 = _sqrt(-b3[0])
        b1 = _sqrt(-b3[2]) if b3[2] < 0 else 0.0
    else:
        b0 = _sqrt(b3[0])
        b1 = _sqrt(b3[2]) if b3[2] > 0 else 0.0
    if b3[1] < 0:
        b0 = -b0
    return [b0, b1, 0.0 if which == 1 else _div(b3[3], b0), 0.0]


def gauss_newton(L, rho, b, lsq):
    for _ in range(5):
        rows, res = [], []
        for i in range(6):
            l = L[i]
            rows.append([((2.0 * l[0] * b[0] + l[1] * b[1]) + l[3] * b[2]) + l[6] * b[3],
                         ((l[1] * b[0] + 2.0 * l[2] * b[1]) + l[4] * b[2]) + l[7] * b[3],
                         ((l[3] * b[0] + l[4] * b[1]) + 2.0 * l[5] * b[2]) + l[8] * b[3],
                         ((l[6] * b[0] + l[7] * b[1]) + l[8] * b[2]) + 2.0 * l[9] * b[3]])
            res.append(rho[i] - (((((((((l[0] * b[0] * b[0] + l[1] * b[0] * b[1]) + l[2] * b[1] * b[1]) + l[3] * b[0] * b[2]) + l[4] * b[1] * b[2])
                                     + l[5] * b[2] * b[2]) + l[6] * b[0] * b[3]) + l[7] * b[1] * b[3]) + l[8] * b[2] * b[3]) + l[9] * b[3] * b[3]))
        x = lsq(rows, res)
        b = [b[k] + x[k] for k in range(4)]
    return b


def epnp(pws, uvs, stats=None, eig=None, lsq=None):
    """EPnP (rule 2) over the points pws with image coordinates uvs, in the given order: (R (9, row-major), t (3)). `stats`: a dict whose
    "off" collects the largest off-diagonal ratio of the swept matrices. `eig` / `lsq` replace the Jacobi iteration (N -> (A, V)) and the
    least-squares method (the N-version check)."""
    eig = eig or jacobi
    lsq = lsq or ls_solve
    n = len(pws)
    nan_pose = ([NAN] * 9, [NAN] * 3)
    if n == 0:
        return nan_pose

    def swept(N):
        A, V = eig(N)
        if stats is not None:
            stats["off"] = max(stats.get("off", 0.0), off_ratio(N, A))
        return A, V
    fn = float(n)
    # 1. control points
    c0 = [_div(tsum([p[x] for p in pws]), fn) for x in range(3)]
    d = [[p[x] - c0[x] for x in range(3)] for p in pws]
    S = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(r, 3):
            S[r][c] = S[c][r] = tsum([q[r] * q[c] for q in d])
    A, V = swept(S)
    lam = [A[k][k] for k in range(3)]
    order = [0, 0, 0]   # by descending eigenvalue, the lowest index first on a tie
    for k in range(3):
        rank = sum(1 for j in range(3) if lam[j] > lam[k] or (lam[j] == lam[k] and j < k))
        order[rank] = k
    cw = [c0]
    for k in range(3):
        vec = [V[x][order[k]] for x in range(3)]
        big = vec[0]   # the sign that makes the component of the largest magnitude positive (the first of equals)
        for x in (1, 2):
            if abs(vec[x]) > abs(big):
                big = vec[x]
        if big < 0.0:
            vec = [-y for y in vec]
        kk = _sqrt(_div(lam[order[k]], fn))
        cw.append([c0[x] + kk * vec[x] for x in range(3)])
    # 2. barycentric coordinates
    inv = inverse3([[cw[k + 1][x] - c0[x] for k in range(3)] for x in range(3)])
    alphas = []
    for q in d:
        a1, a2, a3 = dot3(inv[0][0], inv[0][1], inv[0][2], *q), dot3(inv[1][0], inv[1][1], inv[1][2], *q), dot3(inv[2][0], inv[2][1], inv[2][2], *q)
        alphas.append((((1.0 - a1) - a2) - a3, a1, a2, a3))
    # 3. M^T M
    rows1, rows2 = [], []
    for a, (u, v) in zip(alphas, uvs):
        m1, m2 = [], []
        for j in range(4):
            m1 += [a[j], 0.0, -(a[j] * u)]
            m2 += [0.0, a[j], -(a[j] * v)]
        rows1.append(m1)
        rows2.append(m2)
    MtM = [[0.0] * 12 for _ in range(12)]
    for r in range(12):
        for c in range(r, 12):
            MtM[r][c] = MtM[c][r] = tsum([m1[r] * m1[c] + m2[r] * m2[c] for m1, m2 in zip(rows1, rows2)])
    # 4. the four eigenvectors of the smallest eigenvalues, the smallest first; ties: the lowest index first
    A, V = swept(MtM)
    diag = [A[i][i] for i in range(12)]
    sel = [0, 0, 0, 0]
    for i in range(12):
        rank = sum(1 for j in range(12) if diag[j] < diag[i] or (diag[j] == diag[i] and j < i))
        if rank < 4:
            sel[rank] = i
    v = [[V[j][sel[k]] for j in range(12)] for k in range(4)]
    # 5. L and rho
    L, rho = [], []
    for a, b in PAIRS6:
        dv = [[v[k][3 * a + x] - v[k][3 * b + x] for x in range(3)] for k in range(4)]
        dd = lambda i, j: dot3(dv[i][0], dv[i][1], dv[i][2], dv[j][0], dv[j][1], dv[j][2])
        L.append([dd(0, 0), 2.0 * dd(0, 1), dd(1, 1), 2.0 * dd(0, 2), 2.0 * dd(1, 2), dd(2, 2), 2.0 * dd(0, 3), 2.0 * dd(1, 3), 2.0 * dd(2, 3), dd(3, 3)])
        e = [cw[a][x] - cw[b][x] for x in range(3)]
        rho.append(dot3(e[0], e[1], e[2], e[0], e[1], e[2]))
    # 6 to 8
    best_err, best = float("inf"), nan_pose
    for which in range(3):
        b = gauss_newton(L, rho, betas_approx(which, L, rho, lsq), lsq)
        cc = [[((b[0] * v[0][3 * i + x] + b[1] * v[1][3 * i + x]) + b[2] * v[2][3 * i + x]) + b[3] * v[3][3 * i + x] for x in range(3)] for i in range(4)]
        a = alphas[0]
        if ((a[0] * cc[0][2] + a[1] * cc[1][2]) + a[2] * cc[2][2]) + a[3] * cc[3][2] < 0.0:
            cc = [[-y for y in row] for row in cc]
        pcs = [[((a[0] * cc[0][x] + a[1] * cc[1][x]) + a[2] * cc[2][x]) + a[3] * cc[3][x] for x in range(3)] for a in alphas]
        pc0 = [_div(tsum([q[x] for q in pcs]), fn) for x in range(3)]
        M = [[tsum([d[i][r] * (pcs[i][c] - pc0[c]) for i in range(n)]) for c in range(3)] for r in range(3)]
        R = horn_rotation(M, swept)
        t = [pc0[r] - dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], *c0) for r in range(3)]
        errs = []
        for p, (u, w) in zip(pws, uvs):
            x, y, z = (dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], *p) + t[r] for r in range(3))
            du, dw = u - _div(x, z), w - _div(y, z)
            errs.append(_sqrt(du * du + dw * dw))
        err = _div(tsum(errs), fn)
        if err < best_err:
            best_err, best = err, (R, t)
    return best


def horn_rotation(M, swept):
    """Horn's quaternion form with the scale fixed: the rotation (9, row-major) that maximises tr(R M); M[r][c] = sum b[r] a[c], a = R b."""
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
    A, V = swept(N)
    best = 0
    for i in range(1, 4):
        if A[i][i] > A[best][best]:
            best = i
    q0, q1, q2, q3 = V[0][best], V[1][best], V[2][best], V[3][best]
    nrm = _sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
    return rotation_of(_div(q0, nrm), _div(q1, nrm), _div(q2, nrm), _div(q3, nrm))


def image_coords(prob):
    return [(_div(b[0], b[2]), _div(b[1], b[2])) for b in prob["bearings"]]


# ---- rule 3
def cosine(prob, R, t, i):
    p, b = prob["pos_w"][i], prob["bearings"][i]
    x, y, z = (dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], *p) + t[r] for r in range(3))
    return _div(dot3(x, y, z, *b), _sqrt(dot3(x, y, z, x, y, z)))


def flags_of(prob, R, t, margin=None):
    out = []
    for i in range(len(prob["pos_w"])):
        c, thr = cosine(prob, R, t, i), prob["max_cos_error"][i]
        out.append(1 if c > thr else 0)
        if margin is not None and math.isfinite(c):
            margin[0] = min(margin[0], abs(c - thr))
    return out


def hypothesis(prob, seed, p, h, stats=None):
    idx = sample(seed, p, h, len(prob["pos_w"]))
    uv = image_coords(prob)
    return epnp([prob["pos_w"][i] for i in idx], [uv[i] for i in idx], stats)


def evaluate(prob, seed, max_num_iter, p=0):
    """Every hypothesis h < max_num_iter of problem index p: (inlier counts per h, margin, worst off-diagonal ratio); margin is the smallest
    |cos - max_cos_error| over every (hypothesis, match) with a finite cosine."""
    n = len(prob["pos_w"])
    if n < 4:
        return [], float("inf"), 0.0
    counts, margin, stats = [], [float("inf")], {}
    for h in range(max_num_iter):
        R, t = hypothesis(prob, seed, p, h, stats)
        counts.append(sum(flags_of(prob, R, t, margin)))
    return counts, margin[0], stats.get("off", 0.0)


INVALID = dict(valid=0, best_iter=-1, num_inliers=0, R=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], t=[0.0, 0.0, 0.0])


def refit(prob, flags, stats=None, eig=None, lsq=None):
    """Rule 5's EPnP over the flagged matches, in match order."""
    uv = image_coords(prob)
    idx = [i for i, f in enumerate(flags) if f]
    return epnp([prob["pos_w"][i] for i in idx], [uv[i] for i in idx], stats, eig, lsq)


def finish(prob, counts, seed, min_num_inliers, recompute, p=0, info=None):
    """Rules 4 and 5 over the counts of hypotheses 0 .. len(counts) - 1: the result dict (valid, best_iter, num_inliers, R, t, flags).
    `info`: a dict that receives the refit's margin and off-diagonal ratio."""
    n = len(prob["pos_w"])
    best_iter, best = -1, -1
    for h, c in enumerate(counts):
        if best < c:            # strict: the lowest h of a tie stays
            best, best_iter = c, h
    if not (n >= 4 and n >= min_num_inliers and best >= min_num_inliers):
        return dict(INVALID, flags=[0] * n)
    R, t = hypothesis(prob, seed, p, best_iter)
    flags = flags_of(prob, R, t)
    count = best
    if recompute:
        stats, margin = {}, [float("inf")]
        R2, t2 = refit(prob, flags, stats)
        if all(math.isfinite(x) for x in R2 + t2):
            R, t = R2, t2
            flags = flags_of(prob, R, t, margin)
            count = sum(flags)
        if info is not None:
            info.update(margin=margin[0], off=stats.get("off", 0.0))
    return dict(valid=1, best_iter=best_iter, num_inliers=count, R=R, t=t, flags=flags)


def find_via_ransac(prob, max_num_iter, seed, min_num_inliers=10, recompute=True, p=0):
    """The whole solver: (result dict, margin of the hypotheses)."""
    counts, margin, _ = evaluate(prob, seed, max_num_iter, p)
    return finish(prob, counts, seed, min_num_inliers, recompute, p), margin


def max_cos_error(scale_factor):
    """The constructor's value per octave: cos(scale_factors[octave] * 1 degree), evaluated in f64 by the host's libm."""
    return math.cos(scale_factor * (math.pi / 180.0))


def pose_bits(R, t):
    return [bits(x) for x in R] + [bits(x) for x in t]

