// sim3_opt_math.inc -- the algebra of optimize::transform_optimizer (DESIGN.md 3.11 rules 1 to 8), for the device (sim3_opt.hip) and for a
// plain host compiler alike: tests/test_transform_ref.py builds a stand-alone program from this file with g++ -ffp-contract=off and holds
// its bits to the sequential Python reference, so that only the lane layout is left to the device. Everything is f64, every operation
// rounded on its own. No local array is indexed by a run-time value: on the device what is not in LDS stays in registers.
//
// The optimisation itself (s3_optimize) is written once over a policy X that says how 64 lanes exist: X::each(f) runs f(lane) for the
// lanes, X::sum<K>(f, out) lets every lane accumulate its matches into K partial sums from 0.0 and adds the 64 partials by rule 6's tree,
// X::sync() separates a write to the shared perturbed states from the reads, X::jacobian(lane) is a lane's room for 28 doubles,
// X::kJacobianStride apart, X::count(f, out) adds the lanes' integers. The device's X is one wavefront (each = this lane, sum = the shfl_xor
// butterfly); the host's runs the lanes one after the other. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <stdint.h>

#include "../../include/ovs_detmath.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define S3_FN __host__ __device__ __forceinline__
#else
#define S3_FN inline
#endif

namespace s3 {

constexpr double kEps = 1e-5;              // rule 2's small-angle / small-scale switch
constexpr double kDelta = 1e-9;            // rule 5's step
constexpr double kDblMax = 1.7976931348623157e308;
constexpr int kMinSurvivors = 10, kRound1Iters = 5, kMaxTrials = 10;

// one side's camera: perspective (fx, fy, cx, cy) or equirectangular ((double)cols, (double)rows, -, -)
struct Cam {
    double a, b, c, d;
    int32_t model, pad;
};

// rule 1: S12 with its inverse (R21 is R read by columns)
struct State {
    double R[9], t[3], s, s21, t21[3];
};

// one match as the edges read it
struct Match {
    double p1[3], p2[3], o1[2], o2[2], w1, w2;
};

// per call
struct Params {
    int fix_scale, num_iter;
    double chi_sq, delta, delta_sq;   // (double)chi_sq, (double)sqrtf(chi_sq) and its square
};

// per problem: what out_info reports, then the result
struct Result {
    double info[8];
    State est;
    int num_inliers;
};

S3_FN double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

S3_FN void set_inverse(State& S) {
    S.s21 = 1.0 / S.s;
#pragma unroll
    for (int r = 0; r < 3; ++r) S.t21[r] = (-S.s21) * dot3(S.R[r], S.R[3 + r], S.R[6 + r], S.t[0], S.t[1], S.t[2]);
}

// rule 2: out = exp(u) * S (out may not alias S), with the inverse
S3_FN void exp_apply(const double (&u)[7], int fix_scale, const State& S, State& out) {
    const double w0 = u[0], w1 = u[1], w2 = u[2];
    const double sigma = fix_scale ? 0.0 : u[6];
    const double theta = ovs_dm::sqrt_d(dot3(w0, w1, w2, w0, w1, w2));
    const double Om[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double Om2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = (Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j]) + Om[3 * i + 2] * Om[6 + j];
    const double se = ovs_det_exp(sigma);
    double sn, cs;
    ovs_dm::sincos_d(theta, sn, cs);
    const double th2 = theta * theta;
    const bool small_t = theta < kEps, small_s = ovs_dm::abs_d(sigma) < kEps;
    double Re[9], A, B, C;
    {
        const double ka = sn / theta, kb = (1.0 - cs) / th2;   // (0 / 0 when theta is zero: not selected then)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double I = (k % 4 == 0) ? 1.0 : 0.0;
            Re[k] = small_t ? (I + Om[k]) + Om2[k] / 2.0 : (I + ka * Om[k]) + kb * Om2[k];
        }
    }
    if (small_s) {
        C = 1.0;
        A = small_t ? 0.5 : (1.0 - cs) / th2;
        B = small_t ? 1.0 / 6.0 : (theta - sn) / (th2 * theta);
    } else {
        C = (se - 1.0) / sigma;
        const double sg2 = sigma * sigma;
        if (small_t) {
            A = ((sigma - 1.0) * se + 1.0) / sg2;
            B = ((0.5 * sg2 - sigma + 1.0) * se - 1.0) / (sg2 * sigma);
        } else {
            const double a = se * sn, b = se * cs, c = th2 + sg2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) / th2;
        }
    }
    double W[9], te[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) W[k] = (A * Om[k] + B * Om2[k]) + C * ((k % 4 == 0) ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) te[i] = dot3(W[3 * i], W[3 * i + 1], W[3 * i + 2], u[3], u[4], u[5]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) out.R[3 * i + j] = (Re[3 * i] * S.R[j] + Re[3 * i + 1] * S.R[3 + j]) + Re[3 * i + 2] * S.R[6 + j];
        out.t[i] = se * dot3(Re[3 * i], Re[3 * i + 1], Re[3 * i + 2], S.t[0], S.t[1], S.t[2]) + te[i];
    }
    out.s = se * S.s;
    set_inverse(out);
}

// 3.9 rule 3's projections
S3_FN void project(const Cam& cam, double x, double y, double z, double& u, double& v) {
    if (cam.model == 0) {
        u = cam.a * x / z + cam.c;
        v = cam.b * y / z + cam.d;
    } else {
        const double kPi = 3.14159265358979323846;
        const double L = ovs_dm::sqrt_d((x * x + y * y) + z * z);
        const double theta = ovs_det_atan2(x, z);
        const double phi = -ovs_det_asin(y / L);
        u = cam.a * (0.5 + theta / (2.0 * kPi));
        v = cam.b * (0.5 - phi / kPi);
    }
}

// rule 4: both edges of a match under S; z1 / z2 are the depths the classification reads
struct Edges {
    double e1[2], e2[2], z1, z2;
};
S3_FN Edges edges_of(const Cam& cam1, const Cam& cam2, const State& S, const Match& m) {
    Edges e;
    const double x1 = S.s * dot3(S.R[0], S.R[1], S.R[2], m.p2[0], m.p2[1], m.p2[2]) + S.t[0];
    const double y1 = S.s * dot3(S.R[3], S.R[4], S.R[5], m.p2[0], m.p2[1], m.p2[2]) + S.t[1];
    e.z1 = S.s * dot3(S.R[6], S.R[7], S.R[8], m.p2[0], m.p2[1], m.p2[2]) + S.t[2];
    const double x2 = S.s21 * dot3(S.R[0], S.R[3], S.R[6], m.p1[0], m.p1[1], m.p1[2]) + S.t21[0];
    const double y2 = S.s21 * dot3(S.R[1], S.R[4], S.R[7], m.p1[0], m.p1[1], m.p1[2]) + S.t21[1];
    e.z2 = S.s21 * dot3(S.R[2], S.R[5], S.R[8], m.p1[0], m.p1[1], m.p1[2]) + S.t21[2];
    double u, v;
    project(cam1, x1, y1, e.z1, u, v);
    e.e1[0] = m.o1[0] - u, e.e1[1] = m.o1[1] - v;
    project(cam2, x2, y2, e.z2, u, v);
    e.e2[0] = m.o2[0] - u, e.e2[1] = m.o2[1] - v;
    return e;
}
S3_FN double chi_of(const double (&e)[2], double w) { return w * (e[0] * e[0] + e[1] * e[1]); }

S3_FN void huber(double chi, const Params& P, double& rho0, double& rho1) {
    if (chi > P.delta_sq) {
        const double r = ovs_dm::sqrt_d(chi);
        rho0 = 2.0 * r * P.delta - P.delta_sq;
        rho1 = P.delta / r;
    } else {
        rho0 = chi;
        rho1 = 1.0;
    }
}

// the robust chi-square of one match (rule 6's chi term)
S3_FN double robust_chi_of(const Cam& cam1, const Cam& cam2, const State& S, const Match& m, const Params& P) {
    const Edges e = edges_of(cam1, cam2, S, m);
    double a0, a1, b0, b1;
    huber(chi_of(e.e1, m.w1), P, a0, a1);
    huber(chi_of(e.e2, m.w2), P, b0, b1);
    return a0 + b0;
}

// rule 8's inlier test
S3_FN bool is_inlier(const Cam& cam1, const Cam& cam2, const State& S, const Match& m, const Params& P) {
    const Edges e = edges_of(cam1, cam2, S, m);
    bool ok = chi_of(e.e1, m.w1) <= P.chi_sq && chi_of(e.e2, m.w2) <= P.chi_sq;
    if (cam1.model == 0) ok = ok && m.p1[2] > 0.0 && e.z1 > 0.0;
    if (cam2.model == 0) ok = ok && m.p2[2] > 0.0 && e.z2 > 0.0;
    return ok;
}

// rules 5 and 6: one active match added to the 36 sums: 28 of H's upper triangle by rows, 7 of b, the robust chi-square.
// pert[2 d] / pert[2 d + 1] are exp(+-Delta e_d) S. J is the lane's room for the 28 Jacobian entries, `stride` doubles apart: entry (edge e,
// row r, column d) at J[((2 e + r) * 7 + d) * stride]. The columns are a real loop (its body is two evaluations of both edges), which is
// why they pass through memory -- LDS on the device -- and not through registers.
S3_FN void accumulate(const Cam& cam1, const Cam& cam2, const State& S, const State* pert, const Match& m, const Params& P, double* J, int stride,
                      double (&acc)[36]) {
    const double k = 1.0 / (2.0 * kDelta);
#pragma unroll 1
    for (int d = 0; d < 7; ++d) {
        const Edges ep = edges_of(cam1, cam2, pert[2 * d], m), em = edges_of(cam1, cam2, pert[2 * d + 1], m);
        J[(0 * 7 + d) * stride] = k * (ep.e1[0] - em.e1[0]);
        J[(1 * 7 + d) * stride] = k * (ep.e1[1] - em.e1[1]);
        J[(2 * 7 + d) * stride] = k * (ep.e2[0] - em.e2[0]);
        J[(3 * 7 + d) * stride] = k * (ep.e2[1] - em.e2[1]);
    }
    const Edges e = edges_of(cam1, cam2, S, m);
    double r01, r11, r02, r12;
    huber(chi_of(e.e1, m.w1), P, r01, r11);
    huber(chi_of(e.e2, m.w2), P, r02, r12);
    const double W1 = r11 * m.w1, W2 = r12 * m.w2;
    int q = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        const double j10a = J[(0 * 7 + a) * stride], j11a = J[(1 * 7 + a) * stride], j20a = J[(2 * 7 + a) * stride], j21a = J[(3 * 7 + a) * stride];
#pragma unroll
        for (int b = a; b < 7; ++b, ++q) {
            const double j10b = J[(0 * 7 + b) * stride], j11b = J[(1 * 7 + b) * stride], j20b = J[(2 * 7 + b) * stride], j21b = J[(3 * 7 + b) * stride];
            acc[q] = acc[q] + (W1 * (j10a * j10b + j11a * j11b) + W2 * (j20a * j20b + j21a * j21b));
        }
        acc[28 + a] = acc[28 + a] + -(W1 * (j10a * e.e1[0] + j11a * e.e1[1]) + W2 * (j20a * e.e2[0] + j21a * e.e2[1]));
    }
    acc[35] = acc[35] + (r01 + r02);
}

// rule 7: (H + lambda I) dx = b by Cholesky in solve6's loop order, H as its upper triangle by rows; false when not positive definite
S3_FN bool solve7(const double (&Hu)[36], double lambda, double (&dx)[7]) {
    double H[7][7], L[7][7], y[7];
    {
        int q = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = a; b < 7; ++b, ++q) H[a][b] = H[b][a] = Hu[q];
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = H[i][j] + (i == j ? lambda : 0.0);
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            if (i == j) {
                ok = ok && s > 0;
                L[i][i] = ovs_dm::sqrt_d(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double s = Hu[28 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; ++k) s = s - L[k][i] * dx[k];
        dx[i] = s / L[i][i];
    }
    return ok;   // (a failed factorisation has run on through NaNs; its dx is not read)
}

S3_FN bool is_finite(double x) { return (ovs_dm::bits_of(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// Rules 7 and 8 for one problem of n matches. load(i) returns match i; `outlier` (n bytes) is both the working set (1 = not optimised)
// and, on return, the result's flags; `pert` is room for 14 states that every lane reads.
template <class X, class Load>
S3_FN void s3_optimize(X& x, const Cam& cam1, const Cam& cam2, int n, Load load, const State& S_in, const Params& P, uint8_t* outlier, State* pert,
                       Result& res) {
    State S = S_in;
    set_inverse(S);
    x.each([&](int lane) {
        for (int i = lane; i < n; i += 64) outlier[i] = 0;
    });
    x.sync();
#pragma unroll
    for (int k = 0; k < 8; ++k) res.info[k] = 0.0;
    int survivors = n, iters = kRound1Iters;
#pragma unroll 1
    for (int round = 0; round < 2; ++round) {
        State Serr = S;
        double lambda = 0.0, nu = 2.0, current_chi = 0.0;
        int it = 0, trials = 0;
#pragma unroll 1
        for (; it < iters;) {
            Serr = S;
            x.each([&](int lane) {
                if (lane < 14) {
                    double u[7];
#pragma unroll
                    for (int d = 0; d < 7; ++d) u[d] = (lane >> 1) == d ? ((lane & 1) ? -kDelta : kDelta) : 0.0;
                    exp_apply(u, P.fix_scale, S, pert[lane]);
                }
            });
            x.sync();
            double sums[36];
            x.template sum<36>([&](int lane, double(&acc)[36]) {
                for (int i = lane; i < n; i += 64)
                    if (!outlier[i]) accumulate(cam1, cam2, S, pert, load(i), P, x.jacobian(lane), X::kJacobianStride, acc);
            }, sums);
            x.sync();
            current_chi = sums[35];
            if (it == 0) {
                double md = 0.0;
                int q = 0;
#pragma unroll
                for (int j = 0; j < 7; q += 7 - j, ++j) {
                    const double a = ovs_dm::abs_d(sums[q]);
                    md = (a < md) ? md : a;
                }
                lambda = 1e-5 * md;
                nu = 2.0;
            }
            ++it;
            double rho = 0.0;
            int qmax = 0;
#pragma unroll 1
            do {
                double dx[7];
                const bool ok = solve7(sums, lambda, dx);
                State Sn = S;
                double temp_chi = kDblMax, scale = 0.0;
                if (ok) {
                    exp_apply(dx, P.fix_scale, S, Sn);
                    double c[1];
                    x.template sum<1>([&](int lane, double(&acc)[1]) {
                        for (int i = lane; i < n; i += 64)
                            if (!outlier[i]) acc[0] = acc[0] + robust_chi_of(cam1, cam2, Sn, load(i), P);
                    }, c);
                    temp_chi = c[0];
                    Serr = Sn;
#pragma unroll
                    for (int j = 0; j < 7; ++j) scale = scale + dx[j] * (lambda * dx[j] + sums[28 + j]);
                }
                rho = (current_chi - temp_chi) / (scale + 1e-3);
                if (rho > 0 && is_finite(temp_chi)) {
                    const double xx = 2.0 * rho - 1.0;
                    double alpha = 1.0 - (xx * xx) * xx;
                    alpha = (2.0 / 3.0 < alpha) ? 2.0 / 3.0 : alpha;
                    lambda = lambda * ((1.0 / 3.0 < alpha) ? alpha : 1.0 / 3.0);
                    nu = 2.0;
                    current_chi = temp_chi;
                    S = Sn;
                } else {
                    lambda = lambda * nu;
                    nu = nu * 2.0;
                }
                ++qmax;
                ++trials;
            } while (rho < 0 && qmax < kMaxTrials);
            if (qmax == kMaxTrials || rho == 0) break;
        }
        if (round == 0) {   // (compile-time indices: info stays in registers)
            res.info[0] = (double)it, res.info[1] = (double)trials, res.info[2] = current_chi;
        } else {
            res.info[4] = (double)it, res.info[5] = (double)trials, res.info[6] = current_chi;
        }
        res.info[7] = lambda;
        // rule 8: after round 1 at the state the errors were last computed at, after round 2 at the estimate; an outlier stays one
        State Sc;   // (selected entry by entry: a reference to one of two states would force both into memory)
        {
            const bool first = round == 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) Sc.R[k] = first ? Serr.R[k] : S.R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) Sc.t[k] = first ? Serr.t[k] : S.t[k], Sc.t21[k] = first ? Serr.t21[k] : S.t21[k];
            Sc.s = first ? Serr.s : S.s, Sc.s21 = first ? Serr.s21 : S.s21;
        }
        int cnt[1];
        x.count([&](int lane) {
            int c = 0;
            for (int i = lane; i < n; i += 64)
                if (!outlier[i]) {
                    const bool inl = is_inlier(cam1, cam2, Sc, load(i), P);
                    outlier[i] = inl ? 0 : 1;
                    c += inl ? 1 : 0;
                }
            return c;
        }, cnt);
        x.sync();
        const int before = survivors;
        survivors = cnt[0];
        if (round == 0) {
            res.info[3] = (double)(n - survivors);
            if (survivors < kMinSurvivors) {
                res.est = S_in;
                res.num_inliers = 0;
                return;
            }
            iters = survivors < before ? P.num_iter : kRound1Iters;
        }
    }
    res.est = S;
    res.num_inliers = survivors;
}

}   // namespace s3
