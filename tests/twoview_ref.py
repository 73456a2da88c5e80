"""Sequential restatement of the monocular initialiser's two RANSACs, solve::homography_solver and solve::fundamental_solver, as DESIGN.md 3.13
fixes them (rules 1 to 9): one hypothesis after the other, one match after the other. Pure Python on purpose: a Python float is an IEEE f64
and every operation below rounds once, so the results are the bits the rules ask for. No numpy in the arithmetic; imports nothing of the
product.

A problem is a dict: x1, x2 (lists of 2-tuples: the undistorted keypoint of the reference and of the current frame, per match)."""
import math

from pnp_ref import inverse3, jacobi, off_ratio, tsum   # rule 6's sum, the cyclic Jacobi of any size, the cofactor inverse of 3.10 rule 2.2
from sim3_ref import G, MASK, _div, bits, dot3, mix

SWEEPS = 8
H, F = 0, 1                      # a model's index; its bit in `models` is 1 << index
CHI_H, CHI_F, SCORE = 5.991, 3.841, 5.991
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
NAN = float("nan")


# ---- rule 2
def sample(seed, p, h, n):
    base = (seed + G * ((((p << 20) + h) * 16 + 1) & MASK)) & MASK
    idx = []
    for c in range(8):
        i = mix((base + G * c) & MASK) % (n - c)
        for e in sorted(idx):
            if i >= e:
                i += 1
        idx.append(i)
    return tuple(idx)


def problem_seed(seed, p):
    return (seed + G * (p << 24)) & MASK


# ---- the conventions: a 3 x 3 matrix is a list of 9, row-major
def mul3(A, B):
    return [dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]) for r in range(3) for c in range(3)]


def transpose3(A):
    return [A[3 * c + r] for r in range(3) for c in range(3)]


# ---- rule 1
def normalisation(pts):
    """One side of a problem: mean, dev, s per axis, T and Tinv."""
    fn = float(len(pts))
    mean = [_div(tsum([q[a] for q in pts]), fn) for a in (0, 1)]
    dev = [_div(tsum([abs(q[a] - mean[a]) for q in pts]), fn) for a in (0, 1)]
    s = [_div(1.0, dev[a]) for a in (0, 1)]
    return dict(mean=mean, dev=dev, s=s, T=[s[0], 0.0, -(mean[0] * s[0]), 0.0, s[1], -(mean[1] * s[1]), 0.0, 0.0, 1.0],
                Tinv=[dev[0], 0.0, mean[0], 0.0, dev[1], mean[1], 0.0, 0.0, 1.0])


def normalised(N, q):
    return ((q[0] - N["mean"][0]) * N["s"][0], (q[1] - N["mean"][1]) * N["s"][1])


# ---- rule 3
def rows_of(model, a, b):
    """The rows of the design matrix of one match: a, b the normalised points of side 1 and 2."""
    x1, y1, x2, y2 = a[0], a[1], b[0], b[1]
    if model == H:
        return ([0.0, 0.0, 0.0, -x1, -y1, -1.0, y2 * x1, y2 * y1, y2], [x1, y1, 1.0, 0.0, 0.0, 0.0, -(x2 * x1), -(x2 * y1), -x2])
    return ([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0],)


def smallest(diag):
    best = 0
    for i in range(1, len(diag)):
        if diag[i] < diag[best]:
            best = i
    return best


def null_vector(model, pairs, stats=None, eig=None):
    """The 3 x 3 matrix G of the smallest diagonal entry after the sweeps over A^T A of the normalised pairs, in their order. `eig`, if
    given, replaces everything after the rows: rows -> 9-vector (the N-version check)."""
    rows = [rows_of(model, a, b) for a, b in pairs]
    if eig is not None:
        return eig([r for per_match in rows for r in per_match])
    AtA = [[0.0] * 9 for _ in range(9)]
    for r in range(9):
        for c in range(r, 9):
            if model == H:
                AtA[r][c] = AtA[c][r] = tsum([m1[r] * m1[c] + m2[r] * m2[c] for m1, m2 in rows])
            else:
                AtA[r][c] = AtA[c][r] = tsum([m[r] * m[c] for (m,) in rows])
    A, V = jacobi(AtA, SWEEPS)
    if stats is not None:
        stats["off"] = max(stats.get("off", 0.0), off_ratio(AtA, A))
    k = smallest([A[i][i] for i in range(9)])
    return [V[j][k] for j in range(9)]


# ---- rule 4
def rank_two(Gm, stats=None):
    GtG = mul3(transpose3(Gm), Gm)
    M = [GtG[0:3], GtG[3:6], GtG[6:9]]
    A, V = jacobi(M, SWEEPS)
    if stats is not None:
        stats["off"] = max(stats.get("off", 0.0), off_ratio(M, A))
    k = smallest([A[i][i] for i in range(3)])
    v3 = [V[j][k] for j in range(3)]
    w = [dot3(Gm[3 * r], Gm[3 * r + 1], Gm[3 * r + 2], *v3) for r in range(3)]
    return [Gm[3 * r + c] - w[r] * v3[c] for r in range(3) for c in range(3)]


# ---- rules 3 to 5
def fit(model, prob, norm, idx, stats=None, eig=None):
    """The model over the matches idx, in that order, under the problem's normalisation norm = (side 1, side 2): 9 doubles, row-major."""
    N1, N2 = norm
    Gm = null_vector(model, [(normalised(N1, prob["x1"][i]), normalised(N2, prob["x2"][i])) for i in idx], stats, eig)
    if model == H:
        return mul3(N2["Tinv"], mul3(Gm, N1["T"]))
    return mul3(transpose3(N2["T"]), mul3(rank_two(Gm, stats), N1["T"]))


# ---- rule 6
def transfer_chi(M, src, dst, inv_sigma_sq):
    w = _div(1.0, dot3(M[6], M[7], M[8], src[0], src[1], 1.0))
    u = dot3(M[0], M[1], M[2], src[0], src[1], 1.0) * w
    v = dot3(M[3], M[4], M[5], src[0], src[1], 1.0) * w
    du, dv = dst[0] - u, dst[1] - v
    return (du * du + dv * dv) * inv_sigma_sq


def epipolar_chi(M, src, dst, inv_sigma_sq):
    l0, l1, l2 = (dot3(M[3 * k], M[3 * k + 1], M[3 * k + 2], src[0], src[1], 1.0) for k in range(3))
    num = dot3(l0, l1, l2, dst[0], dst[1], 1.0)
    return _div(num * num, l0 * l0 + l1 * l1) * inv_sigma_sq


def check(model, M, prob, sigma, margin=None):
    """(flags, score) of the model M over every match. margin: a one-element list that keeps the smallest relative distance of a finite
    chi from its threshold."""
    inv_sigma_sq = _div(1.0, sigma * sigma)
    if model == H:
        inv = inverse3([M[0:3], M[3:6], M[6:9]])
        dirs = ((inv[0] + inv[1] + inv[2], 1), (M, 0))     # direction 1 transfers x2 by H_12, direction 2 x1 by H_21
        chi_of, thr = transfer_chi, CHI_H
    else:
        dirs = ((M, 0), (transpose3(M), 1))                # direction 1: F_21 x1 against x2, direction 2: F_21^T x2 against x1
        chi_of, thr = epipolar_chi, CHI_F
    flags, terms = [], []
    for a, b in zip(prob["x1"], prob["x2"]):
        pts = (a, b)
        term, passed = 0.0, 0
        for Md, s in dirs:
            chi = chi_of(Md, pts[s], pts[1 - s], inv_sigma_sq)
            if margin is not None and math.isfinite(chi):
                margin[0] = min(margin[0], abs(chi - thr) / thr)
            if not chi <= thr:       # a NaN fails
                break
            term = term + (SCORE - chi)
            passed += 1
        flags.append(1 if passed == 2 else 0)
        terms.append(term)
    return flags, tsum(terms)


def invalid(n):
    return dict(valid=0, best_iter=-1, num_inliers=0, score=0.0, M=IDENTITY[:], flags=[0] * n)


def hypotheses(prob, seed, max_num_iter, p=0, models=3, stats=None):
    """The models of every hypothesis h < max_num_iter of problem index p: {model: [M per h]}; empty lists below eight matches."""
    n = len(prob["x1"])
    out = {m: [] for m in (H, F) if models >> m & 1}
    if n < 8:
        return out
    norm = (normalisation(prob["x1"]), normalisation(prob["x2"]))
    for h in range(max_num_iter):
        idx = sample(seed, p, h, n)
        for m in out:
            out[m].append(fit(m, prob, norm, idx, stats))
    return out


def finish(model, prob, Ms, sigma, recompute, margin=None, stats=None, info=None):
    """Rules 6 to 8 of one model over the hypotheses' matrices Ms. info: a dict that receives the scores per hypothesis."""
    n = len(prob["x1"])
    best, best_iter, scores = 0.0, -1, []
    for h, M in enumerate(Ms):
        score = check(model, M, prob, sigma, margin)[1]
        scores.append(score)
        if best < score:             # strict: the lowest h of a tie stays; a NaN never wins
            best, best_iter = score, h
    if info is not None:
        info["scores"] = scores
    if best_iter < 0:
        return invalid(n)
    M = Ms[best_iter]
    flags, score = check(model, M, prob, sigma)
    count = sum(flags)
    if not (n >= 8 and score > 0.0 and count >= 8):
        return invalid(n)
    if recompute:
        norm = (normalisation(prob["x1"]), normalisation(prob["x2"]))
        M2 = fit(model, prob, norm, [i for i, f in enumerate(flags) if f], stats)
        if all(math.isfinite(v) for v in M2):
            M = M2
            flags, score = check(model, M, prob, sigma, margin)
            count = sum(flags)
            if not (score > 0.0 and count >= 8):
                return invalid(n)
    return dict(valid=1, best_iter=best_iter, num_inliers=count, score=score, M=M, flags=flags)


def select(res, models=3):
    """Rule 9 over {model: result}."""
    if models != 3:
        m = H if models == 1 else F
        return m + 1 if res[m]["valid"] else 0
    rel = _div(res[H]["score"], res[H]["score"] + res[F]["score"])
    if res[H]["valid"] and 0.40 < rel:
        return 1
    return 2 if res[F]["valid"] else 0


def relative_score(res):
    return _div(res[H]["score"], res[H]["score"] + res[F]["score"])


def solve(prob, sigma=1.0, max_num_iter=100, recompute=True, seed=0, models=3, p=0):
    """The whole call for one problem: dict H, F (the requested ones) and selected."""
    Ms = hypotheses(prob, seed, max_num_iter, p, models)
    res = {m: finish(m, prob, Ms[m], sigma, recompute) for m in Ms}
    return dict(res, selected=select(res, models))


def matrix_bits(M):
    return [bits(x) for x in M]
