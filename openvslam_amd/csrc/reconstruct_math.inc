// reconstruct_math.inc -- initialize::perspective's reconstruct_with_H / reconstruct_with_F, check_pose and find_most_plausible_pose (DESIGN.md
// 3.15, rules R1 to R12) for ONE problem, ONE hypothesis and ONE match over plain doubles, for the device (two_view_reconstruct.hip) and for a
// plain host compiler alike: tests/test_reconstruct_ref.py builds a stand-alone program from this file with g++ -ffp-contract=off and holds its
// bits to the sequential Python reference. A match is one lane's work, so there is no lane policy here. Everything is f64 unless a rule says
// float, every operation rounded on its own. No local array is indexed by a run-time value: the hypothesis number only drives selects, and on
// the device everything stays in registers. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <stdint.h>

#include "../../include/ovs_detmath.h"
#include "jacobi_math.inc"

#if defined(__HIPCC__) || defined(__HIP__)
#define REC_FN __host__ __device__ __forceinline__
#else
#define REC_FN inline
#endif

namespace rec {

constexpr int kMaxHypotheses = 8;
constexpr int kSweeps = 8;
constexpr float kCosSmallParallax = 0.99996192306f;   // cos(0.5 degrees), upstream's constant
constexpr double kRatioMin = 1.00001;
constexpr int kParallaxIndex = 50;
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;   // above every key of a cosine that is not a NaN

// per problem as the host stages it: the chosen model's matrix (row-major), the perspective camera and the model (1: H_21, 2: F_21)
struct Problem {
    double mat[9];
    double fx, fy, cx, cy;
    int32_t model, pad;
};

// one pose hypothesis: rot_ref_to_cur (row-major), trans_ref_to_cur and the current camera's centre in the reference frame, -R^T t (R6)
struct Hyp {
    double R[9], t[3], c[3];
};

struct Match {
    double kp1[2], kp2[2], b1[3], b2[3];
};

// a match under a hypothesis: ok where it survives every gate of R7 to R9; then pos, cos and small are what upstream stores
struct Point {
    double pos[3];
    float cos;
    bool ok, small;
};

REC_FN double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// a 3 x 3 product, rows times columns by dot3, zeros multiplied like any value
REC_FN void mul3(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]);
}
REC_FN void transpose3(const double (&A)[9], double (&At)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) At[3 * r + c] = A[3 * c + r];
}
REC_FN double det3(const double (&M)[9]) {
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
REC_FN bool finite_d(double x) { return (ovs_dm::bits_of(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// R2: M = U diag(d) V^T. V and d^2 by the cyclic Jacobi sweeps on M^T M, the pairs by descending d^2 through a three-exchange network
// (strict "<": equal values and a NaN stay where they are); column k of U is M v_k / d_k, the third one the cross product of the first two
// where `cross_third` says so (an essential matrix: d_3 is next to zero).
struct Svd {
    double U[9], V[9], d[3];   // row-major: column k of U is U[k], U[3 + k], U[6 + k]
};
REC_FN void svd3(const double (&M)[9], bool cross_third, Svd& out) {
    double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) A[i][j] = A[j][i] = dot3(M[i], M[3 + i], M[6 + i], M[j], M[3 + j], M[6 + j]);
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        ovs_jacobi::jacobi_rotate<3, 0, 1>(A, V);
        ovs_jacobi::jacobi_rotate<3, 0, 2>(A, V);
        ovs_jacobi::jacobi_rotate<3, 1, 2>(A, V);
    }
    double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
#define REC_EXCHANGE(la, lb, a, b)                  \
    {                                               \
        const bool sw = la < lb;                    \
        const double hi = sw ? lb : la;             \
        lb = sw ? la : lb;                          \
        la = hi;                                    \
        _Pragma("unroll") for (int r = 0; r < 3; ++r) { \
            const double va = V[r][a], vb = V[r][b]; \
            V[r][a] = sw ? vb : va;                 \
            V[r][b] = sw ? va : vb;                 \
        }                                           \
    }
    REC_EXCHANGE(l0, l1, 0, 1)
    REC_EXCHANGE(l1, l2, 1, 2)
    REC_EXCHANGE(l0, l1, 0, 1)
#undef REC_EXCHANGE
    out.d[0] = ovs_dm::sqrt_d(l0), out.d[1] = ovs_dm::sqrt_d(l1), out.d[2] = ovs_dm::sqrt_d(l2);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out.V[3 * r + k] = V[r][k];
            out.U[3 * r + k] = dot3(M[3 * r], M[3 * r + 1], M[3 * r + 2], V[0][k], V[1][k], V[2][k]) / out.d[k];
        }
    if (cross_third) {
        out.U[2] = out.U[3] * out.U[7] - out.U[6] * out.U[4];
        out.U[5] = out.U[6] * out.U[1] - out.U[0] * out.U[7];
        out.U[8] = out.U[0] * out.U[4] - out.U[3] * out.U[1];
    }
}

REC_FN void set_centre(Hyp& hyp) {
#pragma unroll
    for (int c = 0; c < 3; ++c) hyp.c[c] = -dot3(hyp.R[c], hyp.R[3 + c], hyp.R[6 + c], hyp.t[0], hyp.t[1], hyp.t[2]);
}

// R3, R4: hypothesis h of 8 of a homography; false where the singular values say there is none
REC_FN bool hypothesis_of_H(const Problem& q, int h, Hyp& hyp) {
    const double ifx = 1.0 / q.fx, ify = 1.0 / q.fy;
    const double K[9] = {q.fx, 0.0, q.cx, 0.0, q.fy, q.cy, 0.0, 0.0, 1.0};
    const double Kinv[9] = {ifx, 0.0, -(q.cx * ifx), 0.0, ify, -(q.cy * ify), 0.0, 0.0, 1.0};
    double HK[9], A[9];
    mul3(q.mat, K, HK);
    mul3(Kinv, HK, A);
    Svd s;
    svd3(A, false, s);
    double Vt[9];
    transpose3(s.V, Vt);
    const double sign = det3(s.U) * det3(Vt);
    const double d1 = s.d[0], d2 = s.d[1], d3 = s.d[2];
    if (d1 / d2 < kRatioMin || d2 / d3 < kRatioMin) return false;
    const double q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
    const double aux1 = ovs_dm::sqrt_d((q1 - q2) / (q1 - q3)), aux3 = ovs_dm::sqrt_d((q2 - q3) / (q1 - q3));
    const double x1 = (h & 2) ? -aux1 : aux1, x3 = (h & 1) ? -aux3 : aux3;
    const bool minus = ((h >> 1) ^ h) & 1;   // the sine's signs + - - +
    const bool second = h >= 4;               // d' = -d2
    const double root = ovs_dm::sqrt_d((q1 - q2) * (q2 - q3));
    const double den = second ? (d1 - d3) * d2 : (d1 + d3) * d2;
    const double aux_s = root / den;
    const double sn = minus ? -aux_s : aux_s;
    const double cs = second ? (d1 * d3 - q2) / den : (q2 + d1 * d3) / den;
    const double Rp[9] = {cs, 0.0, second ? sn : -sn, 0.0, second ? -1.0 : 1.0, 0.0, sn, 0.0, second ? -cs : cs};
    double RpVt[9], URpVt[9];
    mul3(Rp, Vt, RpVt);
    mul3(s.U, RpVt, URpVt);
#pragma unroll
    for (int k = 0; k < 9; ++k) hyp.R[k] = sign * URpVt[k];
    const double scale = second ? d1 + d3 : d1 - d3;
    const double tp0 = x1 * scale, tp1 = 0.0 * scale, tp2 = (second ? x3 : -x3) * scale;
    double t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = dot3(s.U[3 * r], s.U[3 * r + 1], s.U[3 * r + 2], tp0, tp1, tp2);
    const double nrm = ovs_dm::sqrt_d(dot3(t[0], t[1], t[2], t[0], t[1], t[2]));
#pragma unroll
    for (int r = 0; r < 3; ++r) hyp.t[r] = t[r] / nrm;
    set_centre(hyp);
    return true;
}

// R5: hypothesis h of 4 of a fundamental matrix; false for h >= 4
REC_FN bool hypothesis_of_F(const Problem& q, int h, Hyp& hyp) {
    if (h >= 4) return false;
    const double K[9] = {q.fx, 0.0, q.cx, 0.0, q.fy, q.cy, 0.0, 0.0, 1.0};
    double Kt[9], FK[9], E[9];
    transpose3(K, Kt);
    mul3(q.mat, K, FK);
    mul3(Kt, FK, E);
    Svd s;
    svd3(E, true, s);
    double Vt[9];
    transpose3(s.V, Vt);
    const bool second = (h & 2) != 0;   // R2 = U W^T V^T
    const double w = second ? -1.0 : 1.0;
    const double W[9] = {0.0, -w, 0.0, w, 0.0, 0.0, 0.0, 0.0, 1.0};
    double WVt[9], R[9];
    mul3(W, Vt, WVt);
    mul3(s.U, WVt, R);
    const bool flip = det3(R) < 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) hyp.R[k] = flip ? -R[k] : R[k];
    const double t0 = s.U[2], t1 = s.U[5], t2 = s.U[8];
    const double nrm = ovs_dm::sqrt_d(dot3(t0, t1, t2, t0, t1, t2));
    const double n0 = t0 / nrm, n1 = t1 / nrm, n2 = t2 / nrm;
    hyp.t[0] = (h & 1) ? -n0 : n0;
    hyp.t[1] = (h & 1) ? -n1 : n1;
    hyp.t[2] = (h & 1) ? -n2 : n2;
    set_centre(hyp);
    return true;
}

REC_FN bool hypothesis(const Problem& q, int h, Hyp& hyp) { return q.model == 1 ? hypothesis_of_H(q, h, hyp) : hypothesis_of_F(q, h, hyp); }

// R11's threshold: reproj_err_thr squared in float
REC_FN float threshold_sq(float reproj_err_thr) { return reproj_err_thr * reproj_err_thr; }

// R6 to R9: one inlier match under one hypothesis
REC_FN Point check_match(const Problem& q, const Hyp& hyp, const Match& m, float thr_sq) {
    Point out;
    out.pos[0] = out.pos[1] = out.pos[2] = 0.0;
    out.cos = 0.0f;
    out.ok = false;
    out.small = false;
    const double(&R)[9] = hyp.R;
    // R6: the midpoint of the two rays
    double b2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) b2[c] = dot3(R[c], R[3 + c], R[6 + c], m.b2[0], m.b2[1], m.b2[2]);
    const double d12 = dot3(m.b1[0], m.b1[1], m.b1[2], b2[0], b2[1], b2[2]);
    const double a00 = dot3(m.b1[0], m.b1[1], m.b1[2], m.b1[0], m.b1[1], m.b1[2]), a01 = -d12, a10 = d12;
    const double a11 = -dot3(b2[0], b2[1], b2[2], b2[0], b2[1], b2[2]);
    const double r0 = dot3(m.b1[0], m.b1[1], m.b1[2], hyp.c[0], hyp.c[1], hyp.c[2]), r1 = dot3(b2[0], b2[1], b2[2], hyp.c[0], hyp.c[1], hyp.c[2]);
    const double det = a00 * a11 - a01 * a10;
    const double lam0 = (a11 * r0 - a01 * r1) / det, lam1 = (a00 * r1 - a10 * r0) / det;
    double pos[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = ((lam0 * m.b1[c] + lam1 * b2[c]) + hyp.c[c]) / 2.0;
    if (!(finite_d(pos[0]) && finite_d(pos[1]) && finite_d(pos[2]))) return out;
    // R7: the parallax between the rays from the two centres
    const double n2x = pos[0] - hyp.c[0], n2y = pos[1] - hyp.c[1], n2z = pos[2] - hyp.c[2];
    const double cosd = dot3(pos[0], pos[1], pos[2], n2x, n2y, n2z) /
                        (ovs_dm::sqrt_d(dot3(pos[0], pos[1], pos[2], pos[0], pos[1], pos[2])) * ovs_dm::sqrt_d(dot3(n2x, n2y, n2z, n2x, n2y, n2z)));
    const float cosf = (float)cosd;
    if (cosf != cosf) return out;
    const bool small = kCosSmallParallax <= cosf;
    // R8: in front of both cameras, unless the parallax is small
    const double pc0 = dot3(R[0], R[1], R[2], pos[0], pos[1], pos[2]) + hyp.t[0];
    const double pc1 = dot3(R[3], R[4], R[5], pos[0], pos[1], pos[2]) + hyp.t[1];
    const double pc2 = dot3(R[6], R[7], R[8], pos[0], pos[1], pos[2]) + hyp.t[2];
    if (!small && !(pos[2] > 0.0)) return out;
    if (!small && !(pc2 > 0.0)) return out;
    // R9: the reprojection errors, the reference's pose the identity
    const double thr = (double)thr_sq;
    const double ex1 = ((q.fx * pos[0]) / pos[2] + q.cx) - m.kp1[0], ey1 = ((q.fy * pos[1]) / pos[2] + q.cy) - m.kp1[1];
    if (!(ex1 * ex1 + ey1 * ey1 <= thr)) return out;
    const double ex2 = ((q.fx * pc0) / pc2 + q.cx) - m.kp2[0], ey2 = ((q.fy * pc1) / pc2 + q.cy) - m.kp2[1];
    if (!(ex2 * ex2 + ey2 * ey2 <= thr)) return out;
    out.pos[0] = pos[0], out.pos[1] = pos[1], out.pos[2] = pos[2];
    out.cos = cosf;
    out.ok = true;
    out.small = small;
    return out;
}

// R10: the order-preserving integer key of a float (ascending keys are ascending floats, -0 before +0)
REC_FN uint32_t key_of(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
REC_FN float float_of_key(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}
// R10: which element of the ascending list of n >= 1 cosines names the parallax, and the parallax of that cosine in degrees
REC_FN int parallax_rank(int n) { return n - 1 < kParallaxIndex ? n - 1 : kParallaxIndex; }
REC_FN float parallax_deg(float cos_parallax) { return (float)((ovs_det_acos((double)cos_parallax) * 180.0) / 3.14159265358979323846); }

// R11: the winner of the hypotheses' records, or -1. A hypothesis that does not exist has the count 0 and the parallax 0.
REC_FN int most_plausible(const int32_t (&count)[kMaxHypotheses], const float (&parallax)[kMaxHypotheses], int n_hypotheses, float parallax_deg_thr,
                          int32_t min_num_triangulated) {
    if (n_hypotheses < 1) return -1;
    int best = 0;
    int32_t most = count[0];
    float best_parallax = parallax[0];
#pragma unroll
    for (int h = 1; h < kMaxHypotheses; ++h) {
        const bool take = h < n_hypotheses && most < count[h];
        most = take ? count[h] : most;
        best = take ? h : best;
        best_parallax = take ? parallax[h] : best_parallax;
    }
    if (most < min_num_triangulated) return -1;
    int similar = 0;
#pragma unroll
    for (int h = 0; h < kMaxHypotheses; ++h) similar += (h < n_hypotheses && 0.8 * (double)most < (double)count[h]) ? 1 : 0;
    if (similar > 1) return -1;
    if (!(best_parallax >= parallax_deg_thr)) return -1;
    return best;
}

// how many hypotheses a problem has (R4, R5): H's depends on the singular values, so the caller asks hypothesis(q, 0, .) for it
REC_FN int hypotheses_of_model(int model) { return model == 1 ? 8 : 4; }

}   // namespace rec
