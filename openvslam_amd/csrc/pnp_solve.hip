// pnp_solve.hip -- solve::pnp_solver (expected: src/openvslam/solve/pnp_solver.{h,cc}): find_via_ransac over a batch of relocalisation
// candidates (module::relocalizer runs it once per candidate between bow_tree::match_frame_and_keyframe and the pose optimiser).
// Rules: DESIGN.md 3.10.
//
// A problem is one (frame, candidate keyframe) pair with n matches: the keypoint's bearing, the landmark in the world and max_cos_error.
// Everything is f64, every operation rounded on its own (the unit is built with -ffp-contract=off).
//
// One wavefront solves one EPnP (epnp_wave), the four-point hypothesis and the n-point refit alike. What does not depend on the match
// (3 x 3 eigenproblem, control points, L, rho, the betas, Gauss-Newton, Horn's form) every lane computes for itself in registers, on
// compile-time indices: the values are wave-uniform and nothing is indexed dynamically, so nothing goes to scratch. The sums over the
// matches (rule 6) give lane j the matches j, j + 64, ... in rank order and end in a butterfly of x + shfl_xor(x, d), d = 32 .. 1 (wave_sum of solve_internal.inc): lane 0
// holds the rule's pairwise tree, and as IEEE addition commutes every lane holds the same bits. The 12 x 12 eigenproblem lives in LDS:
// the rotation's angle in every lane, its 12 column pairs, 12 row pairs and 12 vector pairs one per lane.
//
// k_pnp_hypotheses: grid (hypotheses, problems), one wavefront per workgroup and hypothesis. After EPnP the lanes walk the matches, the
// inlier count of a round of 64 is ballot + popcount. The key is (count << 32) | (0xFFFFFFFF - h); lane 0 saves the wave's model (12
// doubles) and publishes the key with ONE integer atomicMax. No floating-point atomics, no waiting between workgroups.
// k_pnp_finish: one workgroup (one wavefront) per problem: rule 4 on the key, the winner's model read back from its wave's record, the
// flags and the inliers compacted by rank (ballot + prefix popcount), rule 5's EPnP over them, the flags again, the result.
#include <cmath>
#include <cstring>

#include "ovs_common.h"
#include "solve_internal.inc"

namespace {

constexpr int kSweeps = 8;          // every symmetric eigenproblem (DESIGN.md 3.10 rule 2)
constexpr int kModelDoubles = 12;   // R 9, t 3
// the staged block of one call: solve_plan.inc
using splan::pnp::Layout;
using splan::pnp::layout_of;

// one wavefront's LDS: the 12 x 12 matrix and its vectors (row-major), the four chosen eigenvectors, a hypothesis's four indices
struct Lds {
    double A[144], V[144], vec[48];
    int32_t idx[4];
};

// min |rows x - b| over 6 rows of K columns: the normal equations, every entry a left-to-right sum of its six products, Gaussian
// elimination without pivoting, back substitution. A zero pivot gives Inf / NaN, which flow on.
template <int K>
__device__ __forceinline__ void ls_solve(const double (&rows)[6][K], const double (&b)[6], double (&x)[K]) {
    double N[K][K], g[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            double s = rows[0][r] * rows[0][c];
#pragma unroll
            for (int i = 1; i < 6; ++i) s = s + rows[i][r] * rows[i][c];
            N[r][c] = s;
        }
        double s = rows[0][r] * b[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) s = s + rows[i][r] * b[i];
        g[r] = s;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int r = k + 1; r < K; ++r) {
            const double f = N[r][k] / N[k][k];
#pragma unroll
            for (int c = k + 1; c < K; ++c) N[r][c] = N[r][c] - f * N[k][c];
            g[r] = g[r] - f * g[k];
        }
#pragma unroll
    for (int r = K - 1; r >= 0; --r) {
        double s = g[r];
#pragma unroll
        for (int c = r + 1; c < K; ++c) s = s - N[r][c] * x[c];
        x[r] = s / N[r][r];
    }
}

// what turns a world point into its barycentric coordinates: the centroid and the inverse of the control-point matrix
struct Control {
    double c0[3], inv[3][3];
};
__device__ __forceinline__ void centred(const Control& k, const double* __restrict__ p, double (&d)[3]) {
#pragma unroll
    for (int x = 0; x < 3; ++x) d[x] = p[x] - k.c0[x];
}
__device__ __forceinline__ void alphas_of(const Control& k, const double (&d)[3], double (&a)[4]) {
    a[1] = dot3(k.inv[0][0], k.inv[0][1], k.inv[0][2], d[0], d[1], d[2]);
    a[2] = dot3(k.inv[1][0], k.inv[1][1], k.inv[1][2], d[0], d[1], d[2]);
    a[3] = dot3(k.inv[2][0], k.inv[2][1], k.inv[2][2], d[0], d[1], d[2]);
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

__device__ __forceinline__ double select3(int which, double a, double b, double c) { return which == 0 ? a : which == 1 ? b : c; }

// rule 2: EPnP over the n matches idx[0 .. n) of a problem (bearings / pos_w: the problem's first match), by one wavefront. Every lane
// returns the same R, t: all NaN when no approximation has a comparable error. idx may point into LDS or memory.
__device__ __forceinline__ void epnp_wave(const double* __restrict__ bearings, const double* __restrict__ pos_w, const int32_t* idx, int n, Lds& sh,
                                          int lane, double (&R_best)[9], double (&t_best)[3]) {
    const double fn = (double)n;
    Control ctl;
    double cw[4][3];
    // 1. control points: the centroid, then along the eigenvectors of PW0^T PW0
    {
        double a[3] = {0.0, 0.0, 0.0};
        for (int i = lane; i < n; i += 64) {
            const double* p = pos_w + 3 * (size_t)idx[i];
#pragma unroll
            for (int x = 0; x < 3; ++x) a[x] = a[x] + p[x];
        }
#pragma unroll
        for (int x = 0; x < 3; ++x) ctl.c0[x] = wave_sum(a[x]) / fn;
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        for (int i = lane; i < n; i += 64) {
            double d[3];
            centred(ctl, pos_w + 3 * (size_t)idx[i], d);
            s[0] = s[0] + d[0] * d[0];
            s[1] = s[1] + d[0] * d[1];
            s[2] = s[2] + d[0] * d[2];
            s[3] = s[3] + d[1] * d[1];
            s[4] = s[4] + d[1] * d[2];
            s[5] = s[5] + d[2] * d[2];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = wave_sum(s[k]);
        double A[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
        double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll 1
        for (int sweep = 0; sweep < kSweeps; ++sweep) {
            jacobi_rotate<3, 0, 1>(A, V);
            jacobi_rotate<3, 0, 2>(A, V);
            jacobi_rotate<3, 1, 2>(A, V);
        }
#pragma unroll
        for (int x = 0; x < 3; ++x) cw[0][x] = ctl.c0[x];
        // by descending eigenvalue (the lowest index first on a tie), each vector with its largest component positive: selects, no indexed read
        double lam[3] = {A[0][0], A[0][0], A[0][0]}, vec[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int x = 0; x < 3; ++x) vec[r][x] = V[x][0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) rank += (A[j][j] > A[k][k] || (A[j][j] == A[k][k] && j < k)) ? 1 : 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const bool take = rank == r;
                lam[r] = take ? A[k][k] : lam[r];
#pragma unroll
                for (int x = 0; x < 3; ++x) vec[r][x] = take ? V[x][k] : vec[r][x];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double big = vec[k][0];
            big = fabs(vec[k][1]) > fabs(big) ? vec[k][1] : big;
            big = fabs(vec[k][2]) > fabs(big) ? vec[k][2] : big;
            const bool neg = big < 0.0;
            const double kk = sqrt(lam[k] / fn);
#pragma unroll
            for (int x = 0; x < 3; ++x) cw[k + 1][x] = ctl.c0[x] + kk * (neg ? -vec[k][x] : vec[k][x]);
        }
    }
    // 2. the inverse of the control-point matrix C[x][k] = cw[k + 1][x] - c0[x], by cofactors
    {
        double C[3][3];
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int k = 0; k < 3; ++k) C[x][k] = cw[k + 1][x] - ctl.c0[x];
        const double m00 = C[1][1] * C[2][2] - C[1][2] * C[2][1];
        const double m01 = C[1][2] * C[2][0] - C[1][0] * C[2][2];
        const double m02 = C[1][0] * C[2][1] - C[1][1] * C[2][0];
        const double det = (C[0][0] * m00 + C[0][1] * m01) + C[0][2] * m02;
        ctl.inv[0][0] = m00 / det;
        ctl.inv[0][1] = (C[0][2] * C[2][1] - C[0][1] * C[2][2]) / det;
        ctl.inv[0][2] = (C[0][1] * C[1][2] - C[0][2] * C[1][1]) / det;
        ctl.inv[1][0] = m01 / det;
        ctl.inv[1][1] = (C[0][0] * C[2][2] - C[0][2] * C[2][0]) / det;
        ctl.inv[1][2] = (C[0][2] * C[1][0] - C[0][0] * C[1][2]) / det;
        ctl.inv[2][0] = m02 / det;
        ctl.inv[2][1] = (C[0][1] * C[2][0] - C[0][0] * C[2][1]) / det;
        ctl.inv[2][2] = (C[0][0] * C[1][1] - C[0][1] * C[1][0]) / det;
    }
    // 3. M^T M: per match the rows (a_j, 0, -(a_j u)) and (0, a_j, -(a_j v)), j = 0 .. 3; entry (r, c), r <= c, sums m1[r] m1[c] + m2[r] m2[c]
    {
        double acc[78];
#pragma unroll
        for (int k = 0; k < 78; ++k) acc[k] = 0.0;
        for (int i = lane; i < n; i += 64) {
            const size_t m = (size_t)idx[i];
            double d[3], a[4], m1[12], m2[12];
            centred(ctl, pos_w + 3 * m, d);
            alphas_of(ctl, d, a);
            const double u = bearings[3 * m] / bearings[3 * m + 2], v = bearings[3 * m + 1] / bearings[3 * m + 2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m1[3 * j] = a[j], m1[3 * j + 1] = 0.0, m1[3 * j + 2] = -(a[j] * u);
                m2[3 * j] = 0.0, m2[3 * j + 1] = a[j], m2[3 * j + 2] = -(a[j] * v);
            }
            int k = 0;
#pragma unroll
            for (int r = 0; r < 12; ++r)
#pragma unroll
                for (int c = r; c < 12; ++c, ++k) acc[k] = acc[k] + (m1[r] * m1[c] + m2[r] * m2[c]);
        }
        __syncthreads();   // the previous EPnP of this wavefront has left sh
        int k = 0;
#pragma unroll
        for (int r = 0; r < 12; ++r)
#pragma unroll
            for (int c = r; c < 12; ++c, ++k) {
                const double s = wave_sum(acc[k]);
                if (lane == 0) sh.A[r * 12 + c] = sh.A[c * 12 + r] = s;
            }
        for (int i = lane; i < 144; i += 64) sh.V[i] = (i / 12 == i % 12) ? 1.0 : 0.0;
        __syncthreads();
    }
    // 4. the eigenvectors of the four smallest eigenvalues, the smallest first, the lowest index first on a tie
    jacobi_lds<12, kSweeps>(sh.A, sh.V, lane);
    {
        double diag[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) diag[i] = sh.A[i * 13];
        int sel[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < 12; ++j) rank += (diag[j] < diag[i] || (diag[j] == diag[i] && j < i)) ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) sel[k] = rank == k ? i : sel[k];
        }
        if (lane < 48) {
            const int k = lane / 12, j = lane % 12;
            const int s = k == 0 ? sel[0] : k == 1 ? sel[1] : k == 2 ? sel[2] : sel[3];
            sh.vec[lane] = sh.V[j * 12 + s];
        }
        __syncthreads();
    }
    // 5. L (6 x 10) and rho over the control-point pairs
    double L[6][10], rho[6];
    {
        constexpr int PA[6] = {0, 0, 0, 1, 1, 2}, PB[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double dv[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int x = 0; x < 3; ++x) dv[k][x] = sh.vec[k * 12 + 3 * PA[p] + x] - sh.vec[k * 12 + 3 * PB[p] + x];
#define DD(i, j) dot3(dv[i][0], dv[i][1], dv[i][2], dv[j][0], dv[j][1], dv[j][2])
            L[p][0] = DD(0, 0);
            L[p][1] = 2.0 * DD(0, 1);
            L[p][2] = DD(1, 1);
            L[p][3] = 2.0 * DD(0, 2);
            L[p][4] = 2.0 * DD(1, 2);
            L[p][5] = DD(2, 2);
            L[p][6] = 2.0 * DD(0, 3);
            L[p][7] = 2.0 * DD(1, 3);
            L[p][8] = 2.0 * DD(2, 3);
            L[p][9] = DD(3, 3);
#undef DD
            const double e0 = cw[PA[p]][0] - cw[PB[p]][0], e1 = cw[PA[p]][1] - cw[PB[p]][1], e2 = cw[PA[p]][2] - cw[PB[p]][2];
            rho[p] = dot3(e0, e1, e2, e0, e1, e2);
        }
    }
    // 6. the three beta approximations with the public code's sign rules
    double ba[4], bb[4], bc[4];
    {
        double r4[6][4], r3[6][3], r5[6][5], x4[4], x3[3], x5[5];
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            r4[p][0] = L[p][0], r4[p][1] = L[p][1], r4[p][2] = L[p][3], r4[p][3] = L[p][6];
#pragma unroll
            for (int c = 0; c < 3; ++c) r3[p][c] = L[p][c];
#pragma unroll
            for (int c = 0; c < 5; ++c) r5[p][c] = L[p][c];
        }
        ls_solve<4>(r4, rho, x4);
        ls_solve<3>(r3, rho, x3);
        ls_solve<5>(r5, rho, x5);
        if (x4[0] < 0) {
            ba[0] = sqrt(-x4[0]);
            ba[1] = -x4[1] / ba[0], ba[2] = -x4[2] / ba[0], ba[3] = -x4[3] / ba[0];
        } else {
            ba[0] = sqrt(x4[0]);
            ba[1] = x4[1] / ba[0], ba[2] = x4[2] / ba[0], ba[3] = x4[3] / ba[0];
        }
        if (x3[0] < 0) {
            bb[0] = sqrt(-x3[0]);
            bb[1] = x3[2] < 0 ? sqrt(-x3[2]) : 0.0;
        } else {
            bb[0] = sqrt(x3[0]);
            bb[1] = x3[2] > 0 ? sqrt(x3[2]) : 0.0;
        }
        if (x3[1] < 0) bb[0] = -bb[0];
        bb[2] = 0.0, bb[3] = 0.0;
        if (x5[0] < 0) {
            bc[0] = sqrt(-x5[0]);
            bc[1] = x5[2] < 0 ? sqrt(-x5[2]) : 0.0;
        } else {
            bc[0] = sqrt(x5[0]);
            bc[1] = x5[2] > 0 ? sqrt(x5[2]) : 0.0;
        }
        if (x5[1] < 0) bc[0] = -bc[0];
        bc[2] = x5[3] / bc[0], bc[3] = 0.0;
    }
    // 7, 8. per approximation: Gauss-Newton, the pose, its error; the smallest error wins, the lowest index on a tie, never a NaN
    double best_err = INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) R_best[k] = NAN;
    t_best[0] = t_best[1] = t_best[2] = NAN;
    const size_t first = n > 0 ? (size_t)idx[0] : 0;
#pragma unroll 1
    for (int which = 0; which < 3; ++which) {
        double b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = select3(which, ba[k], bb[k], bc[k]);
#pragma unroll 1
        for (int it = 0; it < 5; ++it) {
            double rows[6][4], res[6], x[4];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double(&l)[10] = L[i];
                rows[i][0] = ((2.0 * l[0] * b[0] + l[1] * b[1]) + l[3] * b[2]) + l[6] * b[3];
                rows[i][1] = ((l[1] * b[0] + 2.0 * l[2] * b[1]) + l[4] * b[2]) + l[7] * b[3];
                rows[i][2] = ((l[3] * b[0] + l[4] * b[1]) + 2.0 * l[5] * b[2]) + l[8] * b[3];
                rows[i][3] = ((l[6] * b[0] + l[7] * b[1]) + l[8] * b[2]) + 2.0 * l[9] * b[3];
                res[i] = rho[i] - (((((((((l[0] * b[0] * b[0] + l[1] * b[0] * b[1]) + l[2] * b[1] * b[1]) + l[3] * b[0] * b[2]) + l[4] * b[1] * b[2]) +
                                       l[5] * b[2] * b[2]) + l[6] * b[0] * b[3]) + l[7] * b[1] * b[3]) + l[8] * b[2] * b[3]) + l[9] * b[3] * b[3]);
            }
            ls_solve<4>(rows, res, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = b[k] + x[k];
        }
        double cc[4][3];   // the control points in the camera
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int x = 0; x < 3; ++x)
                cc[i][x] = ((b[0] * sh.vec[3 * i + x] + b[1] * sh.vec[12 + 3 * i + x]) + b[2] * sh.vec[24 + 3 * i + x]) + b[3] * sh.vec[36 + 3 * i + x];
        {
            double d[3], a[4];
            centred(ctl, pos_w + 3 * first, d);
            alphas_of(ctl, d, a);
            if (((a[0] * cc[0][2] + a[1] * cc[1][2]) + a[2] * cc[2][2]) + a[3] * cc[3][2] < 0.0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int x = 0; x < 3; ++x) cc[i][x] = -cc[i][x];
            }
        }
        double pc0[3] = {0.0, 0.0, 0.0};
        for (int i = lane; i < n; i += 64) {
            double d[3], a[4];
            centred(ctl, pos_w + 3 * (size_t)idx[i], d);
            alphas_of(ctl, d, a);
#pragma unroll
            for (int x = 0; x < 3; ++x) pc0[x] = pc0[x] + (((a[0] * cc[0][x] + a[1] * cc[1][x]) + a[2] * cc[2][x]) + a[3] * cc[3][x]);
        }
#pragma unroll
        for (int x = 0; x < 3; ++x) pc0[x] = wave_sum(pc0[x]) / fn;
        double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        for (int i = lane; i < n; i += 64) {
            double d[3], a[4], e[3];
            centred(ctl, pos_w + 3 * (size_t)idx[i], d);
            alphas_of(ctl, d, a);
#pragma unroll
            for (int x = 0; x < 3; ++x) e[x] = ((((a[0] * cc[0][x] + a[1] * cc[1][x]) + a[2] * cc[2][x]) + a[3] * cc[3][x])) - pc0[x];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) M[r][c] = M[r][c] + d[r] * e[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[r][c] = wave_sum(M[r][c]);
        double R[9], t[3];
        horn_rotation(M, R);
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = pc0[r] - dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], ctl.c0[0], ctl.c0[1], ctl.c0[2]);
        double err = 0.0;
        for (int i = lane; i < n; i += 64) {
            const size_t m = (size_t)idx[i];
            const double* p = pos_w + 3 * m;
            const double u = bearings[3 * m] / bearings[3 * m + 2], v = bearings[3 * m + 1] / bearings[3 * m + 2];
            const double x = dot3(R[0], R[1], R[2], p[0], p[1], p[2]) + t[0];
            const double y = dot3(R[3], R[4], R[5], p[0], p[1], p[2]) + t[1];
            const double z = dot3(R[6], R[7], R[8], p[0], p[1], p[2]) + t[2];
            const double du = u - x / z, dw = v - y / z;
            err = err + sqrt(du * du + dw * dw);
        }
        err = wave_sum(err) / fn;
        const bool take = err < best_err;
        best_err = take ? err : best_err;
#pragma unroll
        for (int k = 0; k < 9; ++k) R_best[k] = take ? R[k] : R_best[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t_best[k] = take ? t[k] : t_best[k];
    }
}

// rule 3: a NaN anywhere leaves the comparison false
__device__ __forceinline__ bool is_inlier(const double (&R)[9], const double (&t)[3], const double* __restrict__ p, const double* __restrict__ b,
                                          double max_cos) {
    const double x = dot3(R[0], R[1], R[2], p[0], p[1], p[2]) + t[0];
    const double y = dot3(R[3], R[4], R[5], p[0], p[1], p[2]) + t[1];
    const double z = dot3(R[6], R[7], R[8], p[0], p[1], p[2]) + t[2];
    return dot3(x, y, z, b[0], b[1], b[2]) / sqrt(dot3(x, y, z, x, y, z)) > max_cos;
}

__global__ __launch_bounds__(64) void k_pnp_hypotheses(uint8_t* __restrict__ block, int P, int T, int max_iter, uint64_t seed,
                                                       double* __restrict__ wave_models) {
    __shared__ Lds sh;
    const Layout lay = layout_of(P, T);
    const int p = blockIdx.y, h = blockIdx.x, lane = threadIdx.x;
    const auto [off, n] = problem_span(block, lay.offsets, p);
    if (n < 4) return;   // rule 4: invalid, k_pnp_finish says so
    const double* bearings = reinterpret_cast<const double*>(block + lay.bearings) + 3 * (size_t)off;
    const double* pos_w = reinterpret_cast<const double*>(block + lay.pos_w) + 3 * (size_t)off;
    const double* max_cos = reinterpret_cast<const double*>(block + lay.max_cos) + off;
    if (lane == 0) {
        uint32_t i[4];
        sample_distinct<4, 8>(seed, (uint32_t)p, (uint32_t)h, (uint32_t)n, i);   // rule 1
#pragma unroll
        for (int k = 0; k < 4; ++k) sh.idx[k] = (int32_t)i[k];
    }
    __syncthreads();
    double R[9], t[3];
    epnp_wave(bearings, pos_w, sh.idx, 4, sh, lane, R, t);
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool inl = i < n && is_inlier(R, t, pos_w + 3 * (size_t)(i < n ? i : 0), bearings + 3 * (size_t)(i < n ? i : 0), max_cos[i < n ? i : 0]);
        count += __popcll(__ballot(inl));
    }
    if (lane == 0) {
        double* dst = wave_models + ((size_t)p * max_iter + h) * kModelDoubles;
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[9 + k] = t[k];
        atomicMax(reinterpret_cast<unsigned long long*>(block + lay.keys) + p, hypothesis_key(count, (uint32_t)h));
    }
}

__global__ __launch_bounds__(64) void k_pnp_finish(const uint8_t* __restrict__ block, int P, int T, int min_inliers, int max_iter, int recompute,
                                                   const double* __restrict__ wave_models, int32_t* __restrict__ inlier_idx,
                                                   ResultRec* __restrict__ out, uint8_t* __restrict__ out_flags) {
    __shared__ Lds sh;
    const Layout lay = layout_of(P, T);
    const int p = blockIdx.x, lane = threadIdx.x;
    const auto [off, n] = problem_span(block, lay.offsets, p);
    const unsigned long long key = reinterpret_cast<const unsigned long long*>(block + lay.keys)[p];
    int count = key_count(key);
    const uint32_t h = key_iter(key);
    const bool valid = n >= 4 && n >= min_inliers && count >= min_inliers;   // rule 4 (n < 4: the key is still zero and never read)
    if (!valid) {
        write_invalid(out_flags + off, n, 64, out + p);
        return;
    }
    const double* bearings = reinterpret_cast<const double*>(block + lay.bearings) + 3 * (size_t)off;
    const double* pos_w = reinterpret_cast<const double*>(block + lay.pos_w) + 3 * (size_t)off;
    const double* max_cos = reinterpret_cast<const double*>(block + lay.max_cos) + off;
    const double* md = wave_models + ((size_t)p * max_iter + h) * kModelDoubles;   // the doubles the hypothesis kernel counted with
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = md[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = md[9 + k];
    int32_t* list = inlier_idx + off;
    int found = 0;   // the winner's inliers, compacted in match order
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool inl = i < n && is_inlier(R, t, pos_w + 3 * (size_t)(i < n ? i : 0), bearings + 3 * (size_t)(i < n ? i : 0), max_cos[i < n ? i : 0]);
        const unsigned long long mask = __ballot(inl);
        if (i < n) out_flags[off + i] = inl ? 1 : 0;
        if (inl) list[found + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        found += __popcll(mask);
    }
    if (recompute) {   // rule 5
        __syncthreads();
        double R2[9], t2[3];
        epnp_wave(bearings, pos_w, list, found, sh, lane, R2, t2);
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) finite = finite && __builtin_isfinite(R2[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) finite = finite && __builtin_isfinite(t2[k]);
        if (finite) {
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = R2[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = t2[k];
            count = 0;
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                const bool inl = i < n && is_inlier(R, t, pos_w + 3 * (size_t)(i < n ? i : 0), bearings + 3 * (size_t)(i < n ? i : 0), max_cos[i < n ? i : 0]);
                if (i < n) out_flags[off + i] = inl ? 1 : 0;
                count += __popcll(__ballot(inl));
            }
        }
    }
    if (lane == 0) {
        ResultRec r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.rot[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) r.trans[k] = t[k];
        r.scale = 1.0;
        r.valid = 1;
        r.best_iter = (int32_t)h;
        r.num_inliers = count;
        r.pad = 0;
        out[p] = r;
    }
}

}   // namespace

struct ovs_pnp : batch_handle {
    int32_t* d_inlier_idx = nullptr;   // [max_total_matches] the winner's inliers by rank, per problem at its offset
};

extern "C" {

ovs_status ovs_pnp_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_pnp** out) {
    return batch_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes,
                        (size_t)max_problems * 64,   // 64 iterations per problem without growing
                        kModelDoubles, sizeof(ResultRec), out, [&](ovs_pnp* s) {
                            OVS_HIP_TRY(s->res.dev(&s->d_inlier_idx, sizeof(int32_t) * (size_t)max_total_matches));
                            return OVS_OK;
                        });
}

ovs_status ovs_pnp_destroy(ovs_pnp* s) { return batch_destroy(s); }

ovs_status ovs_pnp_solve_batch(ovs_pnp* s, int32_t n_problems, const int32_t* offsets, const double* bearings, const double* pos_w,
                               const double* max_cos_errors, int32_t min_num_inliers, int32_t max_num_iter, int32_t recompute, uint64_t seed,
                               int32_t* out_valid, int32_t* out_best_iter, int32_t* out_num_inliers, double* out_rot_cw, double* out_trans_cw,
                               uint8_t* out_inlier_flags) {
    const splan::pnp::Call call{s != nullptr, n_problems, offsets, bearings, pos_w, max_cos_errors, min_num_inliers, max_num_iter, out_valid,
                                out_best_iter, out_num_inliers, out_rot_cw, out_trans_cw, out_inlier_flags};
    const splan::Checked checked = splan::pnp::check(call, caps_of(s));
    const Layout lay = layout_of(n_problems, checked.T);
    const auto hypotheses = [&](hipStream_t st, int, int32_t T) {
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3(max_num_iter, n_problems), dim3(64), 0, st, s->d_block, n_problems, T, max_num_iter, seed, s->d_records);
    };
    const auto finish = [&](hipStream_t st, int, int32_t T) {
        hipLaunchKernelGGL(k_pnp_finish, dim3(n_problems), dim3(64), 0, st, s->d_block, n_problems, T, min_num_inliers, max_num_iter, recompute ? 1 : 0,
                           s->d_records, s->d_inlier_idx, s->m_rec<ResultRec>(), s->m_flags);
    };
    return run_batch(s, checked, lay.bytes, n_problems, max_num_iter, 1,
                     {out_valid, out_best_iter, out_num_inliers, out_rot_cw, out_trans_cw, nullptr, out_inlier_flags},
                     [&] { splan::pnp::stage(call, lay, s->h_block); }, hypotheses, finish);
}

}   // extern "C"
