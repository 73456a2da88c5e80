// essential_math.inc -- the algebra of solve::essential_solver (DESIGN.md 3.16, rules E2 to E5) for the device and for a plain host compiler
// alike: a match's row of the eight-point system, the round schedule of the parallel Jacobi ordering, the inlier test with its contribution
// to the score, and the sequential form of the null vector (E3) and of the rank-two step (E4). essential_solve.hip runs the rounds on a matrix
// in LDS (jacobi_lds_rounds of solve_internal.inc, which takes its pairs from round_pair here) and everything else from here;
// tests/essential_host.cc runs all of it one hypothesis and one match after the other. Every operation is rounded on its own (both are
// built with -ffp-contract=off); sqrt and fabs are correctly rounded on both sides. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#endif

#include "jacobi_math.inc"

#if defined(__HIPCC__) || defined(__HIP__)
#define OVS_ESS_FN __host__ __device__ __forceinline__
#else
#define OVS_ESS_FN inline
#endif

namespace ess {

constexpr int kSweeps = 8;        // E3 and E4: a fixed number, no convergence test
constexpr int kRounds = 9;        // E3: rounds per sweep
constexpr int kRoundPairs = 4;    // E3: disjoint pairs per round

OVS_ESS_FN double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// E2: a[3 r + c] = b2[r] * b1[c]
OVS_ESS_FN void row_of(const double* b1, const double* b2, double (&a)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        a[3 * r] = b2[r] * b1[0];
        a[3 * r + 1] = b2[r] * b1[1];
        a[3 * r + 2] = b2[r] * b1[2];
    }
}

// E3's ordering: pair k = 1 .. 4 of round r = 0 .. 8 is {(r + 9 - k) % 9, (r + k) % 9}, the smaller index first (index r idles)
OVS_ESS_FN void round_pair(int r, int k, int& p, int& q) {
    int a = r + 9 - k, b = r + k;
    a = a >= 9 ? a - 9 : a;
    b = b >= 9 ? b - 9 : b;
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// E3, sequentially: the sweeps of the round ordering on the symmetric 9 x 9 matrix A with its vectors V (V = identity on entry). Within a
// round: the four rotations from the matrix as it stands, the four column updates, the four row updates, the four column updates of V.
inline void jacobi_rounds(double (&A)[9][9], double (&V)[9][9]) {
    for (int sweep = 0; sweep < kSweeps; ++sweep)
        for (int r = 0; r < kRounds; ++r) {
            int p[kRoundPairs], q[kRoundPairs];
            bool rot[kRoundPairs];
            double c[kRoundPairs], s[kRoundPairs];
            for (int j = 0; j < kRoundPairs; ++j) {
                round_pair(r, j + 1, p[j], q[j]);
                const double apq = A[p[j]][q[j]];
                rot[j] = apq != 0.0;
                c[j] = 1.0, s[j] = 0.0;
                if (rot[j]) ovs_jacobi::jacobi_angle(A[p[j]][p[j]], A[q[j]][q[j]], apq, c[j], s[j]);
            }
            for (int j = 0; j < kRoundPairs; ++j)
                for (int k = 0; k < 9 && rot[j]; ++k) {
                    const double akp = A[k][p[j]], akq = A[k][q[j]];
                    A[k][p[j]] = c[j] * akp - s[j] * akq;
                    A[k][q[j]] = s[j] * akp + c[j] * akq;
                }
            for (int j = 0; j < kRoundPairs; ++j)
                for (int k = 0; k < 9 && rot[j]; ++k) {
                    const double apk = A[p[j]][k], aqk = A[q[j]][k];
                    A[p[j]][k] = c[j] * apk - s[j] * aqk;
                    A[q[j]][k] = s[j] * apk + c[j] * aqk;
                }
            for (int j = 0; j < kRoundPairs; ++j)
                for (int k = 0; k < 9 && rot[j]; ++k) {
                    const double vkp = V[k][p[j]], vkq = V[k][q[j]];
                    V[k][p[j]] = c[j] * vkp - s[j] * vkq;
                    V[k][q[j]] = s[j] * vkp + c[j] * vkq;
                }
        }
}

// E4: the vector v3 of the smallest diagonal entry of G^T G after the sequential 3 x 3 sweeps (lowest index on a tie; selects, no indexed
// read), projected out of G: G -= (G v3) v3^T. G is 9 doubles, row-major; the result is E_21.
OVS_ESS_FN void rank_two(const double (&G)[9], double (&E)[9]) {
    double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int r = 0; r < 3; ++r) {   // G^T G, rows times columns by dot3
        A[r][0] = dot3(G[r], G[3 + r], G[6 + r], G[0], G[3], G[6]);
        A[r][1] = dot3(G[r], G[3 + r], G[6 + r], G[1], G[4], G[7]);
        A[r][2] = dot3(G[r], G[3 + r], G[6 + r], G[2], G[5], G[8]);
    }
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        ovs_jacobi::jacobi_rotate<3, 0, 1>(A, V);
        ovs_jacobi::jacobi_rotate<3, 0, 2>(A, V);
        ovs_jacobi::jacobi_rotate<3, 1, 2>(A, V);
    }
    double smallest = A[0][0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0];
    {
        const bool take = A[1][1] < smallest;
        smallest = take ? A[1][1] : smallest;
        v0 = take ? V[0][1] : v0, v1 = take ? V[1][1] : v1, v2 = take ? V[2][1] : v2;
    }
    {
        const bool take = A[2][2] < smallest;
        v0 = take ? V[0][2] : v0, v1 = take ? V[1][2] : v1, v2 = take ? V[2][2] : v2;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double w = dot3(G[3 * r], G[3 * r + 1], G[3 * r + 2], v0, v1, v2);
        E[3 * r] = G[3 * r] - w * v0;
        E[3 * r + 1] = G[3 * r + 1] - w * v1;
        E[3 * r + 2] = G[3 * r + 2] - w * v2;
    }
}

// E5, one direction: |cos| of the angle between the bearing b and the normal pl of its partner's epipolar plane; n = |pl|
OVS_ESS_FN double residual(double pl0, double pl1, double pl2, const double* b, double& n) {
    n = sqrt((pl0 * pl0 + pl1 * pl1) + pl2 * pl2);
    return fabs(dot3(pl0, pl1, pl2, b[0], b[1], b[2]) / n);
}

// E5: a match's contribution to the score and whether it is an inlier. Direction 2 (E_21 b1 against b2) first; direction 1 (E_21^T b2
// against b1) counts only after it passed. A NaN fails both comparisons. r2 / r1 return the residuals for the reference's margin.
OVS_ESS_FN double match_term(const double (&E)[9], const double* b1, const double* b2, double thr, bool& inlier, double& r2, double& r1) {
    double n2, n1;
    r2 = residual(dot3(E[0], E[1], E[2], b1[0], b1[1], b1[2]), dot3(E[3], E[4], E[5], b1[0], b1[1], b1[2]), dot3(E[6], E[7], E[8], b1[0], b1[1], b1[2]),
                  b2, n2);
    r1 = residual(dot3(E[0], E[3], E[6], b2[0], b2[1], b2[2]), dot3(E[1], E[4], E[7], b2[0], b2[1], b2[2]), dot3(E[2], E[5], E[8], b2[0], b2[1], b2[2]),
                  b1, n1);
    const bool pass2 = n2 > 0.0 && r2 <= thr;
    const bool pass1 = pass2 && n1 > 0.0 && r1 <= thr;
    const double d2 = thr - r2, d1 = thr - r1;
    double term = 0.0;
    term = pass2 ? term + d2 * d2 : term;
    term = pass1 ? term + d1 * d1 : term;
    inlier = pass1;
    return term;
}

}   // namespace ess
