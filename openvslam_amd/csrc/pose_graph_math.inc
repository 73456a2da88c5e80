// pose_graph_math.inc -- the algebra of optimize::graph_optimizer (DESIGN.md 3.19 rules G1 to G11), for the device (pose_graph.hip) and for a
// plain host compiler alike: tests/test_posegraph_ref.py builds a stand-alone program from this file with g++ -ffp-contract=off and holds its
// bits to the sequential Python reference (tests/posegraph_ref.py), so that only the lane layout is left to the device. Everything is f64,
// every operation rounded on its own. No local array is indexed by a run-time value: what a loop indexes lies in the handle's memory.
//
// The optimisation (pg_optimize) is written once over a policy X that says how the lanes exist: X::kLanes, x.each(f) runs f(lane) for every
// lane (a lane takes the items lane, lane + kLanes, ...), x.sync() separates a phase's writes from the next phase's reads, and
// x.sum(n, val, skip) is rule 6's sum of val[0 .. n) without the items whose skip byte is set (skip may be null): partial j of 64 takes the
// items j, j + 64, ... from 0.0, then part[j] += part[j + d], d = 32 .. 1. It begins with a sync of its own (val is written by the phase
// before it) and returns the same bits to every lane. The device's X is one workgroup (pose_graph.hip); the host's runs the lanes one after
// the other. Rule 2's exponential, the state with its inverse and the finiteness test are sim3_opt_math.inc's, used and not copied.
// (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <stdint.h>

#include "sim3_opt_math.inc"

namespace pg {

using s3::dot3;
using s3::State;

constexpr double kEps = 1e-5;         // G3's small-angle / small-scale switch
constexpr double kDelta = 1e-9;       // G6's step
constexpr double kTol = 1e-6;         // G8: g2o's PCG tolerance
constexpr double kLambda0 = 1e-16;    // G9: upstream's setUserLambdaInit
constexpr double kDblMax = 1.7976931348623157e308;
constexpr int kMaxTrials = 10;
constexpr int kStateDoubles = 13;                 // R (9, row-major), t (3), s
constexpr int kEdgeDoubles = 7 + 49 + 49 + 49;    // per edge in the arena: e, J_i [row][column], J_j, A_ij [a][b]

// per call
struct Params {
    int fix_scale, num_iter, pcg_max_iter;
};

// One call's arrays. The host plan (pose_graph_plan.inc) places them; V holds the vertices on entry and the result on return.
struct Problem {
    int n_v, n_e, n_free;
    const uint8_t* fixed;      // [n_v] 1 = outside the system
    const int32_t* edge_ij;    // [2 n_e]
    const double* meas;        // [13 n_e] M_ji
    const int32_t* inc_row;    // [n_v + 1] the incidence CSR: vertex v owns inc[inc_row[v] .. inc_row[v + 1])
    const int32_t* inc;        // [2 n_e] 2 * edge + side (0: the vertex is the edge's i, 1: its j), ascending
    double *V, *Vt;            // [13 n_v] the vertices and their trial copy
    double* edge;              // [kEdgeDoubles n_e]
    double* chi_e;             // [n_e]
    double *Hd, *Lf;           // [49 n_v] diagonal blocks and their Cholesky factors
    double *g, *x, *r, *z, *p, *q;   // [7 n_v]
    double* val;               // [n_v] a phase's terms for rule 6
};

S3_FN State load_state(const double* p) {
    State S;
#pragma unroll
    for (int k = 0; k < 9; ++k) S.R[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) S.t[k] = p[9 + k];
    S.s = p[12];
    s3::set_inverse(S);
    return S;
}

S3_FN void store_state(double* p, const State& S) {
#pragma unroll
    for (int k = 0; k < 9; ++k) p[k] = S.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[9 + k] = S.t[k];
    p[12] = S.s;
}

// G1's product A B (R, t, s only)
S3_FN void compose(const State& A, const State& B, State& out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out.R[3 * i + j] = (A.R[3 * i] * B.R[j] + A.R[3 * i + 1] * B.R[3 + j]) + A.R[3 * i + 2] * B.R[6 + j];
        out.t[i] = A.s * dot3(A.R[3 * i], A.R[3 * i + 1], A.R[3 * i + 2], B.t[0], B.t[1], B.t[2]) + A.t[i];
    }
    out.s = A.s * B.s;
}

// A B^-1 with G1's inverse of B: (R_B read by columns, t21, s21)
S3_FN void compose_inverse(const State& A, const State& B, State& out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out.R[3 * i + j] = (A.R[3 * i] * B.R[3 * j] + A.R[3 * i + 1] * B.R[3 * j + 1]) + A.R[3 * i + 2] * B.R[3 * j + 2];
        out.t[i] = A.s * dot3(A.R[3 * i], A.R[3 * i + 1], A.R[3 * i + 2], B.t21[0], B.t21[1], B.t21[2]) + A.t[i];
    }
    out.s = A.s * B.s21;
}

// G3: e = (omega, upsilon, sigma) of T (R, t, s). The 3 x 3 solve is the adjugate over the determinant expanded along row 0.
S3_FN void log_of(const State& T, double (&e)[7]) {
    const double* R = T.R;
    const double s = T.s;
    const double sigma = ovs_det_log(s);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double r0 = R[7] - R[5], r1 = R[2] - R[6], r2 = R[3] - R[1];
    const bool small_t = d > 1.0 - kEps, small_s = ovs_dm::abs_d(sigma) < kEps;
    double theta = 0.0, kf = 0.5;
    if (!small_t) {
        theta = ovs_det_acos(d);
        kf = theta / (2.0 * ovs_dm::sqrt_d(1.0 - d * d));
    }
    const double w0 = kf * r0, w1 = kf * r1, w2 = kf * r2;
    const double Om[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double Om2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
    double sn, cs;
    ovs_dm::sincos_d(theta, sn, cs);
    const double th2 = theta * theta;
    double A, B, C;
    if (small_s) {
        C = 1.0;
        A = small_t ? 0.5 : (1.0 - cs) / th2;
        B = small_t ? 1.0 / 6.0 : (theta - sn) / (th2 * theta);
    } else {
        C = (s - 1.0) / sigma;
        const double sg2 = sigma * sigma;
        if (small_t) {
            A = ((sigma - 1.0) * s + 1.0) / sg2;
            B = ((0.5 * sg2 - sigma + 1.0) * s - 1.0) / (sg2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, c = th2 + sg2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) / th2;
        }
    }
    double W[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) W[k] = (A * Om[k] + B * Om2[k]) + C * ((k % 4 == 0) ? 1.0 : 0.0);
    const double c00 = W[4] * W[8] - W[5] * W[7], c01 = W[5] * W[6] - W[3] * W[8], c02 = W[3] * W[7] - W[4] * W[6];
    const double c10 = W[2] * W[7] - W[1] * W[8], c11 = W[0] * W[8] - W[2] * W[6], c12 = W[1] * W[6] - W[0] * W[7];
    const double c20 = W[1] * W[5] - W[2] * W[4], c21 = W[2] * W[3] - W[0] * W[5], c22 = W[0] * W[4] - W[1] * W[3];
    const double det = dot3(W[0], W[1], W[2], c00, c01, c02);
    e[0] = w0, e[1] = w1, e[2] = w2;
    e[3] = dot3(c00, c10, c20, T.t[0], T.t[1], T.t[2]) / det;
    e[4] = dot3(c01, c11, c21, T.t[0], T.t[1], T.t[2]) / det;
    e[5] = dot3(c02, c12, c22, T.t[0], T.t[1], T.t[2]) / det;
    e[6] = sigma;
}

// G5: e = log(M S_i S_j^-1)
S3_FN void edge_error(const State& M, const State& Si, const State& Sj, double (&e)[7]) {
    State T1, T2;
    compose(M, Si, T1);
    compose_inverse(T1, Sj, T2);
    log_of(T2, e);
}

S3_FN double chi_of(const double (&e)[7]) {
    return (((((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]) + e[4] * e[4]) + e[5] * e[5]) + e[6] * e[6];
}

// the unit step +-Delta along d
S3_FN void unit_step(int d, double step, double (&u)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = k == d ? step : 0.0;
}

// G5 and G6 for one edge: e, chi_e and the columns of its free ends into the edge's record
S3_FN void linearize_edge(const Problem& P, const Params& prm, int ei) {
    const int i = P.edge_ij[2 * ei], j = P.edge_ij[2 * ei + 1];
    double* rec = P.edge + (size_t)kEdgeDoubles * ei;
    const State M = load_state(P.meas + (size_t)kStateDoubles * ei);
    const State Si = load_state(P.V + (size_t)kStateDoubles * i), Sj = load_state(P.V + (size_t)kStateDoubles * j);
    const double k = 1.0 / (2.0 * kDelta);
    {
        double e[7];
        edge_error(M, Si, Sj, e);
#pragma unroll
        for (int r = 0; r < 7; ++r) rec[r] = e[r];
        P.chi_e[ei] = chi_of(e);
    }
    if (!P.fixed[i]) {
#pragma unroll 1
        for (int d = 0; d < 7; ++d) {
            double u[7], ep[7], em[7];
            State Sp;
            unit_step(d, kDelta, u);
            s3::exp_apply(u, prm.fix_scale, Si, Sp);
            edge_error(M, Sp, Sj, ep);
            unit_step(d, -kDelta, u);
            s3::exp_apply(u, prm.fix_scale, Si, Sp);
            edge_error(M, Sp, Sj, em);
#pragma unroll
            for (int r = 0; r < 7; ++r) rec[7 + 7 * r + d] = k * (ep[r] - em[r]);
        }
    }
    if (!P.fixed[j]) {
#pragma unroll 1
        for (int d = 0; d < 7; ++d) {
            double u[7], ep[7], em[7];
            State Sp;
            unit_step(d, kDelta, u);
            s3::exp_apply(u, prm.fix_scale, Sj, Sp);
            edge_error(M, Si, Sp, ep);
            unit_step(d, -kDelta, u);
            s3::exp_apply(u, prm.fix_scale, Sj, Sp);
            edge_error(M, Si, Sp, em);
#pragma unroll
            for (int r = 0; r < 7; ++r) rec[56 + 7 * r + d] = k * (ep[r] - em[r]);
        }
    }
}

// the 7-term sum of G7, left to right: column a of X against column b of Y (both [row][column])
S3_FN double col_dot(const double* X, int a, const double* Y, int b) {
    double s = X[a] * Y[b];
#pragma unroll
    for (int r = 1; r < 7; ++r) s = s + X[7 * r + a] * Y[7 * r + b];
    return s;
}

// G7: entry c of vertex v's 49 + 7: its diagonal block's (c / 7, c % 7) or its right-hand side's c - 49, over its incident edges in
// ascending edge index from 0.0
S3_FN void assemble_entry(const Problem& P, int v, int c) {
    double s = 0.0;
    for (int q = P.inc_row[v]; q < P.inc_row[v + 1]; ++q) {
        const int code = P.inc[q];
        const double* rec = P.edge + (size_t)kEdgeDoubles * (code >> 1);
        const double* J = rec + 7 + 49 * (code & 1);
        if (c < 49) {
            s = s + col_dot(J, c / 7, J, c % 7);
        } else {
            const int a = c - 49;
            double t = J[a] * rec[0];
#pragma unroll
            for (int r = 1; r < 7; ++r) t = t + J[7 * r + a] * rec[r];
            s = s + -t;
        }
    }
    if (c < 49) P.Hd[(size_t)49 * v + c] = s;
    else P.g[(size_t)7 * v + (c - 49)] = s;
}

// G7: entry c of edge ei's off-diagonal block A_ij = J_i^T J_j (read only when both ends are free)
S3_FN void offdiag_entry(const Problem& P, int ei, int c) {
    double* rec = P.edge + (size_t)kEdgeDoubles * ei;
    rec[105 + c] = col_dot(rec + 7, c / 7, rec + 56, c % 7);
}

// G8's preconditioner: the Cholesky factor of H_vv + lambda I in solve6's loop order (rule 7's); false when a pivot is not positive
S3_FN bool factor_vertex(const Problem& P, int v, double lambda) {
    const double* Hv = P.Hd + (size_t)49 * v;
    double* Lv = P.Lf + (size_t)49 * v;
    double L[7][7];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = i == j ? Hv[7 * i + j] + lambda : Hv[7 * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            if (i == j) {
                ok = ok && s > 0;
                L[i][i] = ovs_dm::sqrt_d(s);
            } else {
                L[i][j] = s / L[j][j];
            }
            Lv[7 * i + j] = L[i][j];
        }
    return ok;
}

// z = (L L^T)^-1 r by the two substitutions
S3_FN void apply_factor(const double* Lv, const double (&r)[7], double (&z)[7]) {
    double y[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double s = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - Lv[7 * i + k] * y[k];
        y[i] = s / Lv[7 * i + i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; ++k) s = s - Lv[7 * k + i] * z[k];
        z[i] = s / Lv[7 * i + i];
    }
}

S3_FN double dot7(const double (&a)[7], const double (&b)[7]) {
    double s = a[0] * b[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) s = s + a[k] * b[k];
    return s;
}

S3_FN void load7(const double* p, double (&a)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) a[k] = p[k];
}
S3_FN void store7(double* p, const double (&a)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) p[k] = a[k];
}

// G8: q_v = (H_vv + lambda I) p_v, then the incident edges in ascending edge index: A_ij p_j, or A_ij^T p_i from the other end
S3_FN void apply_system(const Problem& P, int v, double lambda, double (&q)[7]) {
    const double* Hv = P.Hd + (size_t)49 * v;
    double pv[7];
    load7(P.p + (size_t)7 * v, pv);
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        double s = (a == 0 ? Hv[7 * a] + lambda : Hv[7 * a]) * pv[0];
#pragma unroll
        for (int b = 1; b < 7; ++b) s = s + (a == b ? Hv[7 * a + b] + lambda : Hv[7 * a + b]) * pv[b];
        q[a] = s;
    }
    for (int k = P.inc_row[v]; k < P.inc_row[v + 1]; ++k) {
        const int code = P.inc[k], ei = code >> 1, side = code & 1;
        const int other = P.edge_ij[2 * ei + (1 - side)];
        if (P.fixed[other]) continue;
        const double* A = P.edge + (size_t)kEdgeDoubles * ei + 105;
        double po[7];
        load7(P.p + (size_t)7 * other, po);
        const int sa = side ? 1 : 7, sb = side ? 7 : 1;   // A[a][b] for the i end, A[b][a] for the j end
#pragma unroll
        for (int a = 0; a < 7; ++a) {
            double t = A[sa * a] * po[0];
#pragma unroll
            for (int b = 1; b < 7; ++b) t = t + A[sa * a + sb * b] * po[b];
            q[a] = q[a] + t;
        }
    }
}

// Rules G5 to G9 and G11 over one graph. info: G's out_info. P.V is the input on entry and the result on return.
template <class X>
S3_FN void pg_optimize(X& x, const Problem& P, const Params& prm, double (&info)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) info[k] = 0.0;
    if (P.n_free == 0 || P.n_e == 0) {
        info[7] = 1.0;
        return;
    }
    const int cap = prm.pcg_max_iter > 0 ? prm.pcg_max_iter : 7 * P.n_free;
    double lambda = kLambda0, nu = 2.0, chi = 0.0, chi0 = 0.0, status = 0.0;
    int it = 0, trials = 0, pcg_total = 0, pcg_last = 0;
#pragma unroll 1
    for (; it < prm.num_iter;) {
        x.each([&](int lane) {
            for (int ei = lane; ei < P.n_e; ei += X::kLanes) linearize_edge(P, prm, ei);
        });
        x.sync();
        x.each([&](int lane) {
            for (int w = lane; w < 56 * P.n_v; w += X::kLanes)
                if (!P.fixed[w / 56]) assemble_entry(P, w / 56, w % 56);
            for (int w = lane; w < 49 * P.n_e; w += X::kLanes) {
                const int ei = w / 49;
                if (!P.fixed[P.edge_ij[2 * ei]] && !P.fixed[P.edge_ij[2 * ei + 1]]) offdiag_entry(P, ei, w % 49);
            }
        });
        chi = x.sum(P.n_e, P.chi_e, nullptr);
        if (it == 0) chi0 = chi;
        if (!s3::is_finite(chi)) {   // G11
            status = 2.0;
            break;
        }
        ++it;
        double rho = 0.0;
        int qmax = 0;
#pragma unroll 1
        do {
            x.each([&](int lane) {
                for (int v = lane; v < P.n_v; v += X::kLanes)
                    if (!P.fixed[v]) P.val[v] = factor_vertex(P, v, lambda) ? 0.0 : 1.0;
            });
            bool failed = x.sum(P.n_v, P.val, P.fixed) != 0.0;
            int iters = 0;
            if (!failed) {
                x.each([&](int lane) {
                    for (int v = lane; v < P.n_v; v += X::kLanes)
                        if (!P.fixed[v]) {
                            double r[7], z[7];
                            load7(P.g + (size_t)7 * v, r);
                            apply_factor(P.Lf + (size_t)49 * v, r, z);
                            store7(P.r + (size_t)7 * v, r);
                            store7(P.z + (size_t)7 * v, z);
                            store7(P.p + (size_t)7 * v, z);
#pragma unroll
                            for (int k = 0; k < 7; ++k) P.x[(size_t)7 * v + k] = 0.0;
                            P.val[v] = dot7(r, z);
                        }
                });
                double dn = x.sum(P.n_v, P.val, P.fixed);
                const double d0 = dn;
#pragma unroll 1
                while (dn > (kTol * kTol) * d0 && iters < cap) {
                    x.each([&](int lane) {
                        for (int v = lane; v < P.n_v; v += X::kLanes)
                            if (!P.fixed[v]) {
                                double q[7], pv[7];
                                apply_system(P, v, lambda, q);
                                load7(P.p + (size_t)7 * v, pv);
                                store7(P.q + (size_t)7 * v, q);
                                P.val[v] = dot7(pv, q);
                            }
                    });
                    const double pq = x.sum(P.n_v, P.val, P.fixed);
                    if (!(pq > 0.0) || !s3::is_finite(pq)) {
                        failed = true;
                        break;
                    }
                    const double alpha = dn / pq;
                    x.each([&](int lane) {
                        for (int v = lane; v < P.n_v; v += X::kLanes)
                            if (!P.fixed[v]) {
                                double xv[7], r[7], z[7], pv[7], q[7];
                                load7(P.x + (size_t)7 * v, xv);
                                load7(P.r + (size_t)7 * v, r);
                                load7(P.p + (size_t)7 * v, pv);
                                load7(P.q + (size_t)7 * v, q);
#pragma unroll
                                for (int k = 0; k < 7; ++k) {
                                    xv[k] = xv[k] + alpha * pv[k];
                                    r[k] = r[k] - alpha * q[k];
                                }
                                apply_factor(P.Lf + (size_t)49 * v, r, z);
                                store7(P.x + (size_t)7 * v, xv);
                                store7(P.r + (size_t)7 * v, r);
                                store7(P.z + (size_t)7 * v, z);
                                P.val[v] = dot7(r, z);
                            }
                    });
                    const double dn2 = x.sum(P.n_v, P.val, P.fixed);
                    const double beta = dn2 / dn;
                    x.each([&](int lane) {
                        for (int v = lane; v < P.n_v; v += X::kLanes)
                            if (!P.fixed[v]) {
#pragma unroll
                                for (int k = 0; k < 7; ++k) P.p[(size_t)7 * v + k] = P.z[(size_t)7 * v + k] + beta * P.p[(size_t)7 * v + k];
                            }
                    });
                    x.sync();
                    dn = dn2;
                    ++iters;
                }
            }
            pcg_total += iters;
            pcg_last = iters;
            double chi_new = kDblMax, scale = 0.0;
            if (!failed) {
                x.each([&](int lane) {
                    for (int v = lane; v < P.n_v; v += X::kLanes) {
                        const State S = load_state(P.V + (size_t)kStateDoubles * v);
                        if (P.fixed[v]) {
                            store_state(P.Vt + (size_t)kStateDoubles * v, S);
                        } else {
                            double u[7];
                            load7(P.x + (size_t)7 * v, u);
                            const double* gv = P.g + (size_t)7 * v;
                            double sv = 0.0;
#pragma unroll
                            for (int k = 0; k < 7; ++k) sv = sv + u[k] * (lambda * u[k] + gv[k]);
                            P.val[v] = sv;
                            State Sn;
                            s3::exp_apply(u, prm.fix_scale, S, Sn);
                            store_state(P.Vt + (size_t)kStateDoubles * v, Sn);
                        }
                    }
                });
                scale = x.sum(P.n_v, P.val, P.fixed);
                x.each([&](int lane) {
                    for (int ei = lane; ei < P.n_e; ei += X::kLanes) {
                        const State M = load_state(P.meas + (size_t)kStateDoubles * ei);
                        const State Si = load_state(P.Vt + (size_t)kStateDoubles * P.edge_ij[2 * ei]);
                        const State Sj = load_state(P.Vt + (size_t)kStateDoubles * P.edge_ij[2 * ei + 1]);
                        double e[7];
                        edge_error(M, Si, Sj, e);
                        P.chi_e[ei] = chi_of(e);
                    }
                });
                chi_new = x.sum(P.n_e, P.chi_e, nullptr);
            }
            rho = (chi - chi_new) / (scale + 1e-3);
            if (rho > 0 && s3::is_finite(chi_new)) {
                const double xx = 2.0 * rho - 1.0;
                double alpha = 1.0 - (xx * xx) * xx;
                alpha = (2.0 / 3.0 < alpha) ? 2.0 / 3.0 : alpha;
                lambda = lambda * ((1.0 / 3.0 < alpha) ? alpha : 1.0 / 3.0);
                nu = 2.0;
                chi = chi_new;
                x.each([&](int lane) {
                    for (int w = lane; w < kStateDoubles * P.n_v; w += X::kLanes) P.V[w] = P.Vt[w];
                });
                x.sync();
            } else {
                lambda = lambda * nu;
                nu = nu * 2.0;
            }
            ++qmax;
            ++trials;
        } while (rho < 0 && qmax < kMaxTrials);
        if (qmax == kMaxTrials || rho == 0) break;
    }
    info[0] = (double)it, info[1] = (double)trials, info[2] = chi0, info[3] = chi, info[4] = lambda;
    info[5] = (double)pcg_total, info[6] = (double)pcg_last, info[7] = status;
}

// G10: landmark p with the non-corrected and the optimised state of its reference vertex
S3_FN void correct_landmark(const State& nc, const State& opt, const double* p, double* out) {
    double q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = nc.s * dot3(nc.R[3 * i], nc.R[3 * i + 1], nc.R[3 * i + 2], p[0], p[1], p[2]) + nc.t[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = opt.s21 * dot3(opt.R[i], opt.R[3 + i], opt.R[6 + i], q[0], q[1], q[2]) + opt.t21[i];
}

}   // namespace pg
