"""The references the dense solver's device tests lean on (tests/dense_ref.py), checked on the CPU: on every generated system LAPACK's f64
solve has a backward error below one eps and the long-double Cholesky solve a smaller one still, so `10 x LAPACK's backward error` is a
bound a correct f64 solver meets and a wrong one does not -- shown on a blocked Cholesky with one 16 x 16 trailing update tampered with."""
import numpy as np
import pytest

import dense_ref as dr

OLD_TOL = lambda cond: 50 * cond * 2.2e-16 + 1e-13   # noqa: E731  (test_dense_solve_matches_numpy's forward-error tolerance)


def _systems():
    for n in (1, 6, 17, 48, 150, 288, 304):
        for cond in (1e2, 1e8, 1e12):
            rng = np.random.default_rng(100 + n)
            S = dr.spd_random_orthogonal(rng, n, cond)
            yield "orthogonal n=%d cond=%g" % (n, cond), S, S @ rng.standard_normal(n)
    for kf in (8, 48, 100):
        rng = np.random.default_rng(kf)
        S, _ = dr.ba_reduced_system(rng, kf)
        yield "reduced camera system, %d keyframes" % kf, S, rng.standard_normal(6 * kf)
    for n, sizes in dr.BLOCK_SIZES.items():
        rng = np.random.default_rng(n)
        S, _ = dr.block_diagonal(rng, sizes)
        yield "block diagonal n=%d" % n, S, rng.standard_normal(n)
    for n in (17, 48, 288, 304, 600):
        rng = np.random.default_rng(n)
        S, _ = dr.integer_factor_system(rng, n)
        yield "integer factor n=%d" % n, S, rng.standard_normal(n)


def test_lapack_is_below_one_eps_and_long_double_below_lapack():
    for tag, S, b in _systems():
        if dr.available(len(b)):
            continue
        lap = dr.backward_error(S, np.linalg.solve(S, b), b)
        ref = dr.backward_error(S, dr.chol_solve_ld(S, b), b)
        print("%-40s LAPACK %.4f eps, long double %.2e eps" % (tag, lap / dr.EPS, ref / dr.EPS))
        assert lap < dr.EPS, (tag, lap)
        assert ref < lap or ref == 0.0, (tag, ref, lap)
        assert ref < 1e-2 * dr.EPS, (tag, ref)


def test_generators_have_the_structure_they_promise():
    for kf in (8, 48, 100):
        S, pairs = dr.ba_reduced_system(np.random.default_rng(kf), kf)
        assert np.array_equal(S, S.T) and dr.zero_blocks(S) == kf * (kf - 1) // 2 - len(pairs) > 0
        d = np.diag(S).reshape(kf, 6)
        assert d[:, 3:].min() > 1e3 * d[:, :3].max()        # translation columns 300 x the rotation columns: 9e4 on the diagonal
    for n, sizes in dr.BLOCK_SIZES.items():
        S, blocks = dr.block_diagonal(np.random.default_rng(n), sizes)
        assert len(S) == n and all(b.stop % 16 for b in blocks[:-1])
        mask = np.ones_like(S, bool)
        for b in blocks:
            mask[b, b] = False
        assert not S[mask].any()
    for n in (17, 48, 288, 304, 600):
        S, L = dr.integer_factor_system(np.random.default_rng(n), n)
        assert np.array_equal(np.linalg.cholesky(S), L)      # exact in f64
        for k in dr.pivot_classes(n):
            Z = S.copy()
            Z[k, k] -= L[k, k] ** 2
            with pytest.raises(np.linalg.LinAlgError, match="pivot %d$" % k):
                dr.chol_solve_ld(Z, np.ones(n))
    assert dr.pivot_classes(17) == [0, 1, 14, 15, 16] and dr.pivot_classes(304) == [0, 14, 15, 16, 31, 287, 288, 302, 303]


@pytest.mark.parametrize("n", [96, 288])
def test_a_tampered_tile_update_fails_the_backward_error_criterion(n):
    """The blocked numpy Cholesky is within the criterion as it stands. With the first panel's update of the first trailing 16 x 16 tile
    (a) dropped, (b) applied 1e-12 short (a tile update wrong from its 12th digit on: 4500 ulp) it exceeds 10 x LAPACK's backward error at
    every condition number. Measured: (a) 5e5 .. 1e14 x, and its forward error is O(1), so the old forward-error tolerance 50 cond eps
    of test_dense_solve_matches_numpy refuses it too; (b) 95 .. 1660 x, while its forward error at cond 1e8 (3.9e-7 at n = 96, 1.5e-7 at
    n = 288) PASSES the old tolerance of 1.1e-6 -- as it does at cond 1e2 and 1e12."""
    for cond in (1e2, 1e8, 1e12):
        rng = np.random.default_rng(n)
        S = dr.spd_random_orthogonal(rng, n, cond)
        b = S @ rng.standard_normal(n)
        want = np.linalg.solve(S, b)
        lap = dr.backward_error(S, want, b)
        fwd = lambda x: np.abs(x - want).max() / np.abs(want).max()   # noqa: E731
        good = dr.blocked_cholesky_solve(S, b)
        assert dr.backward_error(S, good, b) <= 10 * lap and fwd(good) < OLD_TOL(cond)
        dropped = dr.blocked_cholesky_solve(S, b, drop=(0, 1, 1))
        short = dr.blocked_cholesky_solve(S, b, drop=(0, 1, 1), by=1e-12)
        rd, rs = dr.backward_error(S, dropped, b) / lap, dr.backward_error(S, short, b) / lap
        print("n=%d cond=%g: dropped update %.3g x LAPACK's backward error (forward %.2e), 1e-12 short %.3g x (forward %.2e), old tolerance %.2e"
              % (n, cond, rd, fwd(dropped), rs, fwd(short), OLD_TOL(cond)))
        assert rd > 1e3 and rs > 50, (cond, rd, rs)          # both far beyond the x 10 margin
        assert fwd(dropped) > OLD_TOL(cond)                  # the old test sees a dropped update ...
        assert fwd(short) < OLD_TOL(cond)                    # ... and not one wrong from the 12th digit on


def test_backward_error_of_exact_and_of_perturbed_solutions():
    """The evaluator itself: zero for an exactly representable solution, ~delta for a solution perturbed by delta, and it reads the lower
    triangle only."""
    S = np.array([[4.0, 2.0], [2.0, 3.0]])
    x = np.array([1.0, -2.0])
    b = S @ x
    assert dr.backward_error(S, x, b) == 0.0
    got = dr.backward_error(S, x * (1 + 1e-10), b)
    assert 1e-11 < got < 1e-10
    S2 = S.copy()
    S2[0, 1] = 1e300
    assert dr.backward_error(S2, x, b) == 0.0 and np.array_equal(dr.chol_solve_ld(S2, b).astype(float), x)
    assert dr.backward_error(S, np.zeros(2), np.zeros(2)) == 0.0
