"""Sequential reference of the reduced camera system's conjugate-gradient solver: DESIGN.md 3.20 rules P1 to P5 restated in numpy / Python
floats, every operation rounded on its own (numpy's elementwise kernels do not fuse a multiply into an add). The product and the tree are
vectorised over rows and over the 64 partials; inside a partial the terms are added one after the other in ascending column order, as
rule P2 says. tests/test_ba_pcg_ref.py holds openvslam_amd/csrc/ba_pcg_math.inc (through a plain host compiler) to these bits and
tests/test_gpu_global_ba.py the device."""
import math

import numpy as np

TOL = 1e-10


class Failed(Exception):
    """Rule P5: p.q is not > 0 or not finite, or a pivot of a diagonal block is not > 0."""


def tree_sum(val):
    """3.10 rule 6: partial j of 64 takes the items j, j + 64, ... from 0.0, then part[j] += part[j + d] for d = 32 .. 1."""
    val = np.asarray(val, np.float64)
    part = np.zeros(64)
    for t in range(0, len(val), 64):
        c = val[t:t + 64]
        part[:len(c)] = part[:len(c)] + c
    d = 32
    while d:
        part[:d] = part[:d] + part[d:2 * d]
        d >>= 1
    return float(part[0])


def factor6(A):
    """P1: Cholesky of a 6x6 block in solve6's loop order, Python floats. None when a pivot is not > 0."""
    L = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i + 1):
            s = float(A[i][j])
            for c in range(j):
                s = s - L[i][c] * L[j][c]
            if i == j:
                if not s > 0:
                    return None
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    return L


def apply6(L, r):
    y = [0.0] * 6
    for i in range(6):
        s = float(r[i])
        for c in range(i):
            s = s - L[i][c] * y[c]
        y[i] = s / L[i][i]
    z = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for c in range(i + 1, 6):
            s = s - L[c][i] * z[c]
        z[i] = s / L[i][i]
    return z


def dot6(a, b):
    s = float(a[0]) * float(b[0])
    for c in range(1, 6):
        s = s + float(a[c]) * float(b[c])
    return s


def block_dot(a, b):
    """P3: per block the six products left to right, then rule 6 over the block index."""
    return tree_sum(block_terms(a, b))


def product(S, p):
    """P2: q_i = sum_j S_ij p_j; partial l adds the terms j = l, l + 64, ... in ascending order from 0.0, then the tree."""
    n = len(p)
    part = np.zeros((n, 64))
    for t in range(0, n, 64):
        w = min(64, n - t)
        part[:, :w] = part[:, :w] + S[:, t:t + w] * p[None, t:t + w]
    d = 32
    while d:
        part[:, :d] = part[:, :d] + part[:, d:2 * d]
        d >>= 1
    return part[:, 0].copy()


def precondition(Ls, r):
    """z = M^-1 r: apply6 over all blocks at once (vectorised over the blocks, the order inside a block is apply6's)."""
    L = np.asarray(Ls, np.float64)
    rb = np.asarray(r, np.float64).reshape(-1, 6)
    y = np.zeros_like(rb)
    for i in range(6):
        s_ = rb[:, i].copy()
        for c in range(i):
            s_ = s_ - L[:, i, c] * y[:, c]
        y[:, i] = s_ / L[:, i, i]
    z = np.zeros_like(rb)
    for i in range(5, -1, -1):
        s_ = y[:, i].copy()
        for c in range(i + 1, 6):
            s_ = s_ - L[:, c, i] * z[:, c]
        z[:, i] = s_ / L[:, i, i]
    return z.reshape(-1)


def block_terms(a, b):
    """dot6 over all blocks at once"""
    a, b = np.asarray(a, np.float64).reshape(-1, 6), np.asarray(b, np.float64).reshape(-1, 6)
    s_ = a[:, 0] * b[:, 0]
    for c in range(1, 6):
        s_ = s_ + a[:, c] * b[:, c]
    return s_


def solve(S, g, tol=TOL, max_iter=0):
    """S x = g by rules P1 to P5. Returns (x, (iterations, stopped at the cap, last dn / d0)). Raises Failed."""
    S = np.ascontiguousarray(S, np.float64)
    g = np.ascontiguousarray(g, np.float64)
    n = len(g)
    assert S.shape == (n, n) and n % 6 == 0 and n > 0
    if max_iter == 0:
        max_iter = 12 * (n // 6)
    Ls = [factor6(S[k:k + 6, k:k + 6]) for k in range(0, n, 6)]
    if any(L is None for L in Ls):
        raise Failed("pivot")
    x = np.zeros(n)
    r = g.copy()
    z = precondition(Ls, r)
    p = None
    dn = block_dot(r, z)
    d0 = dn
    dn_prev = dn
    k = 0
    while dn > (tol * tol) * d0 and k < max_iter:
        p = z.copy() if k == 0 else z + (dn / dn_prev) * p
        q = product(S, p)
        pq = block_dot(p, q)
        if not (pq > 0.0 and pq < math.inf):
            raise Failed("p.q")
        alpha = dn / pq
        x = x + alpha * p
        r = r - alpha * q
        z = precondition(Ls, r)
        dn_prev = dn
        dn = block_dot(r, z)
        k += 1
    capped = bool(dn > (tol * tol) * d0)
    return x, (k, capped, dn / d0 if d0 > 0.0 else 0.0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the systems the tests share -------------------------------------------------------------------------------------------------
def spd(rng, n, cond):
    """tests/test_gpu_ba.py's _spd: random orthogonal basis, log-spaced spectrum."""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.logspace(0, np.log10(cond), n)
    S = (q * w) @ q.T
    return 0.5 * (S + S.T)


# below / above 64 entries per row, 64 / 65 blocks, both sides of the Cholesky's limit, 256 / 257 blocks: one full workgroup of the lane-per-block
# kernels, and a second one holding one lane
SIZES = (6, 12, 60, 66, 384, 390, 1020, 1026, 1032, 1536, 1542)
BLOCK_SIZES = (3078, 6144)   # block_case: 513 blocks (three workgroups, the last with one lane) and the capacity (four full ones, pitch == n)
_cache = {}


def case(n, cond=1e3):
    """(S, g) of size n, and the reference's solution of it: computed once, shared, not to be written to."""
    key = (n, cond)
    if key not in _cache:
        rng = np.random.default_rng(7000 + n)
        S = spd(rng, n, cond)
        g = S @ rng.standard_normal(n)
        S.setflags(write=False)
        g.setflags(write=False)
        _cache[key] = (S, g)
    return _cache[key]


def solved(n, cond=1e3, max_iter=0):
    key = ("x", n, cond, max_iter)
    if key not in _cache:
        S, g = case(n, cond)
        _cache[key] = solve(S, g, TOL, max_iter)
    return _cache[key]


def failure_cases(n):
    """Rule P5's failures placed in the LAST block of case(n) (at n = 1542 block 256: lane 0 of the second workgroup of the lane-per-block
    kernels): name -> (S, g). Every one makes solve raise Failed."""
    S0, g0 = case(n)
    b = n // 6 - 1
    assert b >= 1
    out = {}
    S = np.array(S0)
    S[6 * b + 1, 6 * b + 1] = -1.0
    out["bad pivot"] = (S, g0)
    S = np.array(S0)
    S[1, 6 * b + 2] = S[6 * b + 2, 1] = np.nan
    out["nan off the diagonal blocks"] = (S, g0)
    S = np.array(S0)
    S[6 * b + 3, 6 * b + 3] = np.nan
    out["nan on the diagonal"] = (S, g0)
    # positive definite blocks, a coupling of -3 between the last two: p = g in the first pass, p.q = 12 - 36
    S = np.eye(n)
    i = np.arange(6 * (b - 1), 6 * b)
    S[i, i + 6] = S[i + 6, i] = -3.0
    g = np.zeros(n)
    g[6 * (b - 1):] = 1.0
    out["indefinite"] = (S, g)
    return out


def block_spd(rng, n):
    """A block-dominant system, what block-Jacobi is made for (spd() needs a QR of the whole matrix and then some 300 iterations: too slow at
    thousands of unknowns): a dense coupling of rank 8 and weight 0.5, and on every 6x6 diagonal block a random Gram matrix plus 6 .. 60 on the
    diagonal, the blocks drawn in ascending order."""
    W = rng.standard_normal((n, 8))
    S = (0.5 / 8) * W @ W.T
    for b in range(n // 6):
        A = rng.standard_normal((6, 6))
        S[6 * b:6 * b + 6, 6 * b:6 * b + 6] += A @ A.T + 6 * np.eye(6) * (1 + 9 * rng.random())
    return 0.5 * (S + S.T)


def block_case(n):
    """(S, g) of the block-dominant family: computed once, shared, not to be written to."""
    key = ("block", n)
    if key not in _cache:
        rng = np.random.default_rng(7000 + n)
        S = block_spd(rng, n)
        g = S @ rng.standard_normal(n)
        S.setflags(write=False)
        g.setflags(write=False)
        _cache[key] = (S, g)
    return _cache[key]


def block_solved(n):
    key = ("block x", n)
    if key not in _cache:
        S, g = block_case(n)
        _cache[key] = solve(S, g, TOL, 0)
    return _cache[key]
