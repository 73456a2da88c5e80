"""Extended-precision reference for the dense solver's tests (a plain helper module): a Cholesky solve and a backward-error evaluator in
long double (x86-64: 64-bit mantissa, eps 1.08e-19; where long double is no wider than that, mpmath up to 96 unknowns), and the
generators of the systems the tests solve.

The criterion of the tests: a backward-stable solve of S x = b has a normwise backward error

    berr(x) = max_i |b - S x|_i / (||S||_inf ||x||_inf + ||b||_inf)

of a small multiple of the f64 eps WHATEVER the condition number, while the forward error grows with it; the device solver is held to
10 x the backward error LAPACK reaches on the same system, both evaluated by backward_error() below."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)                     # 2.22e-16
EXTENDED = float(np.finfo(LD).eps) < 1e-18                # long double is wider than double by enough to judge f64 residuals
MPMATH_MAX_N = 96


def available(n):
    """None if a reference exists for n unknowns, else the reason (the tests skip with it). On x86-64 nothing is skipped."""
    if EXTENDED or n <= MPMATH_MAX_N:
        return None
    return "long double has eps %.1e here: no extended-precision reference beyond n = %d (mpmath)" % (float(np.finfo(LD).eps), MPMATH_MAX_N)


def _sym_lower(S):
    """What the solver reads: the lower triangle, mirrored."""
    S = np.asarray(S)
    return np.tril(S) + np.tril(S, -1).T


def chol_solve_ld(S, b):
    """x of S x = b by Cholesky in long double (left-looking, one column per step), from the lower triangle of S."""
    if not EXTENDED:
        return _chol_solve_mp(S, b)
    n = len(b)
    L = np.tril(np.asarray(S)).astype(LD)
    for j in range(n):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        if not L[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite at pivot %d" % j)
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    y = np.asarray(b).astype(LD)
    for j in range(n):        # L y = b, column-oriented
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):   # L^T x = y
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def backward_error(S, x, b):
    """max |b - S x| / (||S||_inf ||x||_inf + ||b||_inf), evaluated in extended precision; S is taken from its lower triangle."""
    if not EXTENDED:
        return _backward_error_mp(S, x, b)
    A = _sym_lower(S).astype(LD)
    x, b = np.asarray(x).astype(LD), np.asarray(b).astype(LD)
    r = np.abs(b - A @ x).max()
    den = np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    return float(r / den) if den > 0 else float(r)


def _chol_solve_mp(S, b):
    import mpmath as mp
    assert len(b) <= MPMATH_MAX_N
    with mp.workdps(40):
        x = mp.cholesky_solve(mp.matrix(_sym_lower(S).tolist()), mp.matrix([float(v) for v in b]))
        return np.array([LD(mp.nstr(v, 25)) for v in x])


def _backward_error_mp(S, x, b):
    import mpmath as mp
    assert len(b) <= MPMATH_MAX_N
    with mp.workdps(40):
        A = mp.matrix(_sym_lower(S).tolist())
        xv, bv = mp.matrix([mp.mpf(str(v)) if isinstance(v, LD) else mp.mpf(float(v)) for v in x]), mp.matrix([float(v) for v in b])
        r = max(abs(v) for v in (bv - A * xv))
        den = mp.mnorm(A, mp.inf) * max(abs(v) for v in xv) + max(abs(v) for v in bv)
        return float(r / den) if den > 0 else float(r)


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def spd_random_orthogonal(rng, n, cond):
    """Dense symmetric positive definite, random orthogonal basis, log-spaced spectrum 1 .. cond (the family of test_dense_solve_matches_numpy)."""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = np.logspace(0, np.log10(cond), n)
    S = (q * w) @ q.T
    return 0.5 * (S + S.T)


def ba_reduced_system(rng, n_kf, rows_per_pair=10, band=3, extra_pairs=None):
    """A reduced-camera-system look-alike of 6 n_kf unknowns: S = J^T J + 1e-4 diag(J^T J), every row of J touching the 6-wide blocks of two
    keyframes (a shared landmark), rotation : translation column scales 1 : 300. Keyframes pair with their `band` successors and with a few
    random others, so most off-diagonal 6 x 6 blocks are EXACTLY zero. Returns (S, pairs)."""
    pairs = {(i, j) for i in range(n_kf) for j in range(i + 1, min(n_kf, i + 1 + band))}
    for _ in range(n_kf // 4 if extra_pairs is None else extra_pairs):
        i, j = sorted(rng.choice(n_kf, 2, replace=False).tolist())
        pairs.add((i, j))
    pairs = sorted(pairs)
    scale = np.tile(np.array([1.0, 1.0, 1.0, 300.0, 300.0, 300.0]), n_kf)
    J = np.zeros((len(pairs) * rows_per_pair, 6 * n_kf))
    for p, (i, j) in enumerate(pairs):
        rows = slice(p * rows_per_pair, (p + 1) * rows_per_pair)
        J[rows, 6 * i:6 * i + 6] = rng.standard_normal((rows_per_pair, 6))
        J[rows, 6 * j:6 * j + 6] = rng.standard_normal((rows_per_pair, 6))
    J *= scale
    S = J.T @ J
    S = 0.5 * (S + S.T)
    S[np.diag_indices_from(S)] *= 1.0 + 1e-4
    return S, pairs


def zero_blocks(S, bs=6):
    """Number of off-diagonal bs x bs blocks of S that are exactly zero (lower triangle)."""
    nb = len(S) // bs
    return sum(1 for i in range(nb) for j in range(i) if not S[bs * i:bs * i + bs, bs * j:bs * j + bs].any())


BLOCK_SIZES = {96: (6, 30, 17, 43), 288: (6, 30, 17, 38, 59, 65, 73), 304: (6, 30, 17, 38, 59, 65, 89)}


def block_diagonal(rng, sizes, cond=1e4, panel=16):
    """Block-diagonal SPD system, blocks of spd_random_orthogonal; no interior block boundary lies on the solver's `panel`-column grid.
    Returns (S, [slice per block])."""
    n = int(sum(sizes))
    S, at, blocks = np.zeros((n, n)), 0, []
    for m in sizes:
        S[at:at + m, at:at + m] = spd_random_orthogonal(rng, m, cond)
        blocks.append(slice(at, at + m))
        at += m
        assert at == n or at % panel, "block boundary %d on the panel grid" % at
    return S, blocks


def integer_factor_system(rng, n, per_row=3):
    """(S, L) with S = L L^T EXACT in f64 and every intermediate of its Cholesky factorisation an integer: L lower triangular, powers of two
    (1, 2, 4) on the diagonal -- so that square roots, reciprocal square roots and the divisions by the pivots are exact -- and `per_row`
    entries of -1 / +1 left of it. Subtracting L[k][k]^2 from S[k][k] then makes pivot k exactly zero."""
    L = np.zeros((n, n))
    L[np.diag_indices(n)] = rng.choice([1.0, 2.0, 4.0], n)
    for i in range(1, n):
        cols = rng.choice(i, min(i, per_row), replace=False)
        L[i, cols] = rng.choice([-1.0, 1.0], len(cols))
    return L @ L.T, L


def pivot_classes(n):
    """The pivots of the refusal tests: first, 14, 15 (last lane of a 16-row block), 16, 31, first / second row of the last 17, last two."""
    return sorted({k for k in (0, 14, 15, 16, 31, n - 17, n - 16, n - 2, n - 1) if 0 <= k < n})


def blocked_cholesky_solve(S, b, nb=16, drop=None, by=1.0):
    """Right-looking blocked Cholesky solve in f64 numpy (the shape of the device kernels: panel, rows below it, trailing tile updates).
    drop = (panel, tile row, tile column): of that one nb x nb trailing update only (1 - by) is applied -- the deliberately broken solvers
    the tests must catch: by = 1 skips the update, a small `by` is an update that is wrong in its last digits."""
    A = np.tril(np.asarray(S, np.float64)).copy()
    n = len(A)
    for p, j0 in enumerate(range(0, n, nb)):
        j1 = min(j0 + nb, n)
        A[j0:j1, j0:j1] = np.linalg.cholesky(A[j0:j1, j0:j1] + np.tril(A[j0:j1, j0:j1], -1).T)
        if j1 == n:
            break
        A[j1:, j0:j1] = np.linalg.solve(A[j0:j1, j0:j1], A[j1:, j0:j1].T).T
        for ti, r0 in enumerate(range(j1, n, nb), p + 1):
            for tj, c0 in enumerate(range(j1, r0 + 1, nb), p + 1):
                r1, c1 = min(r0 + nb, n), min(c0 + nb, n)
                A[r0:r1, c0:c1] -= (1.0 - by if drop == (p, ti, tj) else 1.0) * (A[r0:r1, j0:j1] @ A[c0:c1, j0:j1].T)
    L = np.tril(A)
    y = np.linalg.solve(L, np.asarray(b, np.float64))
    return np.linalg.solve(L.T, y)
