"""Sequential restatement of solve::essential_solver, the bearing-vector eight-point RANSAC of robust::match_frame_and_keyframe, as DESIGN.md
3.16 fixes it (rules E1 to E8): one hypothesis after the other, one match after the other. Pure Python on purpose: a Python float is an IEEE
f64 and every operation below rounds once, so the results are the bits the rules ask for. No numpy in the arithmetic; imports nothing of
the product.

A problem is a dict: b1, b2 (lists of 3-tuples: the bearing of the match's keypoint in frame 1 and in frame 2)."""
import math

from pnp_ref import jacobi, off_ratio, tsum          # the sequential 3 x 3 sweeps of E4, the off-diagonal measure, rule 6's sum
from sim3_ref import G, MASK, _div, _sqrt, bits, dot3, f32, mix

SWEEPS = 8
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
# upstream's constant as recalled: the float 0.01745240643f widened to double (the class default of every layer)
RESIDUAL_COS_THR = f32(0.01745240643)


# ---- E1
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


# ---- E2
def row_of(b1, b2):
    return [b2[r] * b1[c] for r in range(3) for c in range(3)]


def system(rows):
    AtA = [[0.0] * 9 for _ in range(9)]
    for i in range(9):
        for j in range(i, 9):
            AtA[i][j] = AtA[j][i] = tsum([a[i] * a[j] for a in rows])
    return AtA


# ---- E3
def round_pairs(r):
    """The four disjoint pairs of round r, the smaller index first; index r idles."""
    return [tuple(sorted(((r + 9 - k) % 9, (r + k) % 9))) for k in (1, 2, 3, 4)]


def jacobi_rounds(N, sweeps=SWEEPS):
    """Cyclic Jacobi on the 9 x 9 matrix N in the round ordering: (A, V). Within a round the four rotations are taken from the matrix as it
    stands, then come the four column updates, the four row updates and the four column updates of V."""
    A = [row[:] for row in N]
    V = [[1.0 if r == c else 0.0 for c in range(9)] for r in range(9)]
    for _ in range(sweeps):
        for r in range(9):
            rots = []
            for p, q in round_pairs(r):
                apq = A[p][q]
                if apq == 0.0:          # (a NaN is not 0: it rotates and spreads)
                    continue
                theta = _div(A[q][q] - A[p][p], 2.0 * apq)
                t = _div(1.0 if theta >= 0 else -1.0, abs(theta) + _sqrt(theta * theta + 1.0))
                c = _div(1.0, _sqrt(t * t + 1.0))
                rots.append((p, q, c, t * c))
            for p, q, c, s in rots:
                for k in range(9):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
            for p, q, c, s in rots:
                for k in range(9):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
            for p, q, c, s in rots:
                for k in range(9):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return A, V


def smallest(diag):
    best = 0
    for i in range(1, len(diag)):
        if diag[i] < diag[best]:
            best = i
    return best


def null_vector(rows, stats=None):
    AtA = system(rows)
    A, V = jacobi_rounds(AtA)
    if stats is not None:
        stats["off"] = max(stats.get("off", 0.0), off_ratio(AtA, A))
    k = smallest([A[i][i] for i in range(9)])
    return [V[j][k] for j in range(9)]


# ---- E4
def rank_two(Gm):
    GtG = [[dot3(Gm[r], Gm[3 + r], Gm[6 + r], Gm[c], Gm[3 + c], Gm[6 + c]) for c in range(3)] for r in range(3)]
    A, V = jacobi(GtG, SWEEPS)
    k = smallest([A[i][i] for i in range(3)])
    v3 = [V[j][k] for j in range(3)]
    w = [dot3(Gm[3 * r], Gm[3 * r + 1], Gm[3 * r + 2], *v3) for r in range(3)]
    return [Gm[3 * r + c] - w[r] * v3[c] for r in range(3) for c in range(3)]


# ---- E2 to E4
def fit(prob, idx, stats=None, eig=None):
    """E_21 over the matches idx, in that order: 9 doubles, row-major. `eig`, if given, replaces everything after the rows: rows -> E_21
    (the N-version check)."""
    rows = [row_of(prob["b1"][i], prob["b2"][i]) for i in idx]
    if eig is not None:
        return eig(rows)
    return rank_two(null_vector(rows, stats))


# ---- E5
def residual(pl, b):
    n = _sqrt((pl[0] * pl[0] + pl[1] * pl[1]) + pl[2] * pl[2])
    return abs(_div(dot3(pl[0], pl[1], pl[2], *b), n)), n


def check(E, prob, thr, margin=None):
    """(flags, score) of E_21 over every match. margin: a one-element list that keeps the smallest relative distance of a finite residual
    from the threshold."""
    flags, terms = [], []
    for b1, b2 in zip(prob["b1"], prob["b2"]):
        r2, n2 = residual([dot3(E[3 * r], E[3 * r + 1], E[3 * r + 2], *b1) for r in range(3)], b2)
        r1, n1 = residual([dot3(E[r], E[3 + r], E[6 + r], *b2) for r in range(3)], b1)
        if margin is not None:
            for r in (r2, r1):
                if math.isfinite(r):
                    margin[0] = min(margin[0], abs(r - thr) / thr)
        term, passed = 0.0, 0
        for r, n in ((r2, n2), (r1, n1)):     # direction 2 first; direction 1 counts only after it passed
            if not (n > 0.0 and r <= thr):    # a NaN fails
                break
            d = thr - r
            term = term + d * d
            passed += 1
        flags.append(1 if passed == 2 else 0)
        terms.append(term)
    return flags, tsum(terms)


def invalid(n):
    return dict(valid=0, best_iter=-1, num_inliers=0, score=0.0, E=IDENTITY[:], flags=[0] * n)


def hypotheses(prob, seed, max_num_iter, p=0, stats=None):
    """E_21 of every hypothesis h < max_num_iter of problem index p; an empty list below eight matches."""
    n = len(prob["b1"])
    if n < 8:
        return []
    return [fit(prob, sample(seed, p, h, n), stats) for h in range(max_num_iter)]


# ---- E6 and E7
def finish(prob, Es, thr, recompute, margin=None, stats=None, info=None):
    """Rules E5 to E7 over the hypotheses' matrices Es. info: a dict that receives the scores per hypothesis."""
    n = len(prob["b1"])
    best, best_iter, scores = 0.0, -1, []
    for h, E in enumerate(Es):
        score = check(E, prob, thr, margin)[1]
        scores.append(score)
        if best < score:             # strict: the lowest h of a tie stays; a NaN never wins
            best, best_iter = score, h
    if info is not None:
        info["scores"] = scores
    if best_iter < 0:
        return invalid(n)
    E = Es[best_iter]
    flags, score = check(E, prob, thr)
    count = sum(flags)
    if not (n >= 8 and score > 0.0 and count >= 8):
        return invalid(n)
    if recompute:
        E2 = fit(prob, [i for i, f in enumerate(flags) if f], stats)
        if all(math.isfinite(v) for v in E2):
            E = E2
            flags, score = check(E, prob, thr, margin)
            count = sum(flags)
            if not (score > 0.0 and count >= 8):
                return invalid(n)
    return dict(valid=1, best_iter=best_iter, num_inliers=count, score=score, E=E, flags=flags)


def solve(prob, thr=RESIDUAL_COS_THR, max_num_iter=50, recompute=False, seed=0, p=0):
    """The whole call for one problem."""
    return finish(prob, hypotheses(prob, seed, max_num_iter, p), thr, recompute)


def as_bits(r):
    """A result with its doubles as uint64 bit patterns: what the device tests compare."""
    return dict(valid=r["valid"], best_iter=r["best_iter"], num_inliers=r["num_inliers"], score=bits(r["score"]), E=[bits(v) for v in r["E"]],
                flags=list(r["flags"]))
