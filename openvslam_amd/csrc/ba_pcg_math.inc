// ba_pcg_math.inc -- the arithmetic of the reduced camera system's conjugate-gradient solver (DESIGN.md 3.20 rules P1 to P5), for the device
// (ba_pcg.hip) and for a plain host compiler alike: tests/test_ba_pcg_ref.py builds a stand-alone program from this file with
// g++ -ffp-contract=off and holds its bits to the sequential reference (tests/ba_pcg_ref.py), so that only the lane layout and the split
// into launches are left to the device. Everything is f64, every operation rounded on its own. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <stdint.h>

#include "../../include/ovs_detmath.h"

#define PCG_FN OVS_DM_FN

namespace pcg {

constexpr double kTol = 1e-10;   // rule P4

// P1: the Cholesky factor of the k-th diagonal block of S (pitch doubles per row) in solve6's loop order; L is 36 doubles, row-major, the
// lower triangle written. False when a pivot is not > 0 (a NaN included); the factor is then not to be used.
PCG_FN bool factor6(const double* S, size_t pitch, int k, double* Lout) {
    const double* A = S + (size_t)6 * k * pitch + (size_t)6 * k;
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[(size_t)i * pitch + j];
#pragma unroll
            for (int c = 0; c < j; ++c) s = s - L[i][c] * L[j][c];
            if (i == j) {
                ok = ok && s > 0;
                L[i][i] = ovs_dm::sqrt_d(s);
            } else {
                L[i][j] = s / L[j][j];
            }
            Lout[6 * i + j] = L[i][j];
        }
    return ok;
}

// P1: z = (L L^T)^-1 r by the two substitutions
PCG_FN void apply6(const double* L, const double (&r)[6], double (&z)[6]) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = r[i];
#pragma unroll
        for (int c = 0; c < i; ++c) s = s - L[6 * i + c] * y[c];
        y[i] = s / L[6 * i + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int c = i + 1; c < 6; ++c) s = s - L[6 * c + i] * z[c];
        z[i] = s / L[6 * i + i];
    }
}

// P3: a block's six products, left to right
PCG_FN double dot6(const double* a, const double* b) {
    double s = a[0] * b[0];
#pragma unroll
    for (int c = 1; c < 6; ++c) s = s + a[c] * b[c];
    return s;
}

// P4: entry j of the search direction of iteration k: z_j at k = 0, z_j + beta p_j afterwards
PCG_FN double direction(int k, double z, double beta, double p_old) { return k == 0 ? z : z + beta * p_old; }

// P2: partial l of 64 of row i: the terms j = l, l + 64, ... < n in ascending order from 0.0; p_of(j) is the direction's entry
template <class P>
PCG_FN double row_partial(const double* Srow, int n, int l, P p_of) {
    double s = 0.0;
    for (int j = l; j < n; j += 64) s = s + Srow[j] * p_of(j);
    return s;
}

// P4's loop test and P5's failure test
PCG_FN bool goes_on(double dn, double d0, double tol, int k, int max_iter) { return dn > (tol * tol) * d0 && k < max_iter; }
PCG_FN bool curvature_ok(double pq) { return pq > 0.0 && pq < __builtin_inf(); }

// what a solve reports: iterations run, 1.0 when it stopped at the cap with the loop test still true, the last dn / d0 (0.0 when d0 is not > 0)
PCG_FN void report(int k, double dn, double d0, double tol, double* info) {
    info[0] = (double)k;
    info[1] = dn > (tol * tol) * d0 ? 1.0 : 0.0;
    info[2] = d0 > 0.0 ? dn / d0 : 0.0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// 3.10 rule 6 over val[0 .. n): partial j of 64 takes the items j, j + 64, ... from 0.0, then part[j] += part[j + d], d = 32 .. 1
inline double tree_sum(const double* val, int n) {
    double part[64];
    for (int j = 0; j < 64; ++j) {
        part[j] = 0.0;
        for (int i = j; i < n; i += 64) part[j] = part[j] + val[i];
    }
    for (int d = 32; d; d >>= 1)
        for (int j = 0; j < d; ++j) part[j] = part[j] + part[j + d];
    return part[0];
}

// The whole solve, the lanes one after the other: S x = g, S dense with `pitch` doubles per row, n = 6 nb unknowns. work: solve_seq_work_doubles(n)
// doubles. Returns false on FAILED (P5); x is then unspecified. info: see report().
inline bool solve_seq(const double* S, size_t pitch, const double* g, int n, double tol, int max_iter, double* x, double* work, double* info) {
    const int nb = n / 6;
    double* L = work;
    double *r = L + (size_t)36 * nb, *z = r + n, *p = z + n, *pn = p + n, *q = pn + n, *part = q + n;
    bool ok = true;
    for (int b = 0; b < nb; ++b) ok = factor6(S, pitch, b, L + (size_t)36 * b) && ok;
    info[0] = info[1] = info[2] = 0.0;
    if (!ok) return false;
    for (int b = 0; b < nb; ++b) {
        double rb[6], zb[6];
        for (int c = 0; c < 6; ++c) {
            x[6 * b + c] = 0.0;
            rb[c] = r[6 * b + c] = g[6 * b + c];
        }
        apply6(L + (size_t)36 * b, rb, zb);
        for (int c = 0; c < 6; ++c) z[6 * b + c] = zb[c];
        part[b] = dot6(r + 6 * b, z + 6 * b);
    }
    double dn = tree_sum(part, nb), dn_prev = dn;
    const double d0 = dn;
    int k = 0;
    for (; goes_on(dn, d0, tol, k, max_iter); ++k) {
        const double beta = k == 0 ? 0.0 : dn / dn_prev;
        for (int j = 0; j < n; ++j) pn[j] = direction(k, z[j], beta, p[j]);
        for (int i = 0; i < n; ++i) {
            double lane[64];
            for (int l = 0; l < 64; ++l) lane[l] = row_partial(S + (size_t)i * pitch, n, l, [&](int j) { return pn[j]; });
            for (int d = 32; d; d >>= 1)
                for (int l = 0; l < d; ++l) lane[l] = lane[l] + lane[l + d];
            q[i] = lane[0];
        }
        for (int j = 0; j < n; ++j) p[j] = pn[j];
        for (int b = 0; b < nb; ++b) part[b] = dot6(p + 6 * b, q + 6 * b);
        const double pq = tree_sum(part, nb);
        if (!curvature_ok(pq)) return false;
        const double alpha = dn / pq;
        for (int b = 0; b < nb; ++b) {
            double rb[6], zb[6];
            for (int c = 0; c < 6; ++c) {
                x[6 * b + c] = x[6 * b + c] + alpha * p[6 * b + c];
                rb[c] = r[6 * b + c] = r[6 * b + c] - alpha * q[6 * b + c];
            }
            apply6(L + (size_t)36 * b, rb, zb);
            for (int c = 0; c < 6; ++c) z[6 * b + c] = zb[c];
            part[b] = dot6(r + 6 * b, z + 6 * b);
        }
        dn_prev = dn;
        dn = tree_sum(part, nb);
    }
    report(k, dn, d0, tol, info);
    return true;
}
inline size_t solve_seq_work_doubles(int n) { return (size_t)36 * (n / 6) + (size_t)5 * n + (size_t)(n / 6); }
#endif

}   // namespace pcg
