// triangulate_math.inc -- module::two_view_triangulator::triangulate with solve::triangulator::triangulate under it (DESIGN.md 3.12, rules
// T1 to T9) for ONE match over plain doubles, for the device (triangulate.hip) and for a plain host compiler alike: tests/test_triangulate_ref.py
// builds a stand-alone program from this file with g++ -ffp-contract=off and holds its bits to the sequential Python reference. A match is
// one lane's work, so there is no lane policy here. Everything is f64, every operation rounded on its own; float inputs are widened once by
// whoever fills a Match. No local array is indexed by a run-time value: on the device everything stays in registers.
// (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <stdint.h>

#include "../../include/ovs_detmath.h"
#include "jacobi_math.inc"
#include "sim3_opt_math.inc"

#if defined(__HIPCC__) || defined(__HIP__)
#define TRI_FN __host__ __device__ __forceinline__
#else
#define TRI_FN inline
#endif

namespace tri {

constexpr double kChiSqMono = (double)5.99146f, kChiSqStereo = (double)7.81473f;

// one side's camera: perspective (fx, fy, cx, cy) or equirectangular ((double)cols, (double)rows, -, -), as s3::Cam holds it, with the two
// stereo constants
struct Cam {
    double a, b, c, d, focal_x_baseline, true_baseline;
    int32_t model, pad;
};

// per problem: both cameras, both poses (rotation row-major, then translation) and both camera centres (rule T8)
struct Problem {
    Cam cam[2];
    double pose[2][12];
    double centre[2][3];
};

// one match as the rules read it; the float inputs already widened
struct Match {
    double b1[3], b2[3], kp1[2], kp2[2], x_right1, x_right2, depth1, depth2, sigma_sq1, sigma_sq2, scale_factor1, scale_factor2;
};

// per call: cos_rays_parallax_thr and (double)ratio_factor
struct Params {
    double cos_thr, ratio_factor;
};

struct Result {
    double pos_w[3];
    int status, method;
};

TRI_FN double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// rule T8's centre = -R^T t, once per problem (the host computes it when it stages a problem)
TRI_FN void set_centres(Problem& q) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int c = 0; c < 3; ++c) q.centre[s][c] = -dot3(q.pose[s][c], q.pose[s][3 + c], q.pose[s][6 + c], q.pose[s][9], q.pose[s][10], q.pose[s][11]);
}

// rule T4: the null vector of the two-view system by eight cyclic Jacobi sweeps on A^T A
TRI_FN void two_view(const double (&P1)[12], const double (&P2)[12], const double (&b1)[3], const double (&b2)[3], double (&pos_w)[3]) {
    double A[4][4], M[4][4], V[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // P[r][k]: k < 3 the rotation's row r, k = 3 the translation
        const double p10 = k < 3 ? P1[k] : P1[9], p11 = k < 3 ? P1[3 + k] : P1[10], p12 = k < 3 ? P1[6 + k] : P1[11];
        const double p20 = k < 3 ? P2[k] : P2[9], p21 = k < 3 ? P2[3 + k] : P2[10], p22 = k < 3 ? P2[6 + k] : P2[11];
        A[0][k] = b1[0] * p12 - b1[2] * p10;
        A[1][k] = b1[1] * p12 - b1[2] * p11;
        A[2][k] = b2[0] * p22 - b2[2] * p20;
        A[3][k] = b2[1] * p22 - b2[2] * p21;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) M[i][j] = ((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < r) M[r][c] = M[c][r];
            V[r][c] = r == c ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
        ovs_jacobi::jacobi_rotate<4, 0, 1>(M, V);
        ovs_jacobi::jacobi_rotate<4, 0, 2>(M, V);
        ovs_jacobi::jacobi_rotate<4, 0, 3>(M, V);
        ovs_jacobi::jacobi_rotate<4, 1, 2>(M, V);
        ovs_jacobi::jacobi_rotate<4, 1, 3>(M, V);
        ovs_jacobi::jacobi_rotate<4, 2, 3>(M, V);
    }
    double best = M[0][0], v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const bool take = M[i][i] < best;
        best = take ? M[i][i] : best;
        v0 = take ? V[0][i] : v0;
        v1 = take ? V[1][i] : v1;
        v2 = take ? V[2][i] : v2;
        v3 = take ? V[3][i] : v3;
    }
    pos_w[0] = v0 / v3, pos_w[1] = v1 / v3, pos_w[2] = v2 / v3;
}

// rule T5: the stereo observation of one side back-projected into the world
TRI_FN void back_project(const Cam& cam, const double (&P)[12], const double (&kp)[2], double depth, double (&pos_w)[3]) {
    const double x = (kp[0] - cam.c) * depth / cam.a - P[9];
    const double y = (kp[1] - cam.d) * depth / cam.b - P[10];
    const double z = depth - P[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) pos_w[c] = dot3(P[c], P[3 + c], P[6 + c], x, y, z);
}

// rule T6: true when the point lies in front of a perspective camera (a NaN does not)
TRI_FN bool depth_is_positive(const Cam& cam, const double (&P)[12], const double (&pos_w)[3]) {
    return cam.model != 0 || dot3(P[6], P[7], P[8], pos_w[0], pos_w[1], pos_w[2]) + P[11] > 0.0;
}

// rule T7: true when the reprojection error passes its chi-square gate (a NaN does not)
TRI_FN bool reprojection_is_good(const Cam& cam, const double (&P)[12], const double (&pos_w)[3], const double (&kp)[2], bool stereo, double x_right,
                                 double sigma_sq) {
    const double x = dot3(P[0], P[1], P[2], pos_w[0], pos_w[1], pos_w[2]) + P[9];
    const double y = dot3(P[3], P[4], P[5], pos_w[0], pos_w[1], pos_w[2]) + P[10];
    const double z = dot3(P[6], P[7], P[8], pos_w[0], pos_w[1], pos_w[2]) + P[11];
    s3::Cam pc;
    pc.a = cam.a, pc.b = cam.b, pc.c = cam.c, pc.d = cam.d, pc.model = cam.model, pc.pad = 0;
    double u, v;
    s3::project(pc, x, y, z, u, v);
    const double ex = u - kp[0], ey = v - kp[1];
    if (stereo) {
        const double ex_r = (u - cam.focal_x_baseline / z) - x_right;
        return ((ex * ex + ey * ey) + ex_r * ex_r) <= kChiSqStereo * sigma_sq;
    }
    return (ex * ex + ey * ey) <= kChiSqMono * sigma_sq;
}

// rules T1 to T9 for one match
TRI_FN Result triangulate(const Problem& q, const Match& m, const Params& prm) {
    Result r;
    r.pos_w[0] = r.pos_w[1] = r.pos_w[2] = 0.0;
    r.method = 0;
    const Cam &cam1 = q.cam[0], &cam2 = q.cam[1];
    const double(&P1)[12] = q.pose[0];
    const double(&P2)[12] = q.pose[1];
    // T1
    double ray1[3], ray2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ray1[c] = dot3(P1[c], P1[3 + c], P1[6 + c], m.b1[0], m.b1[1], m.b1[2]);
        ray2[c] = dot3(P2[c], P2[3 + c], P2[6 + c], m.b2[0], m.b2[1], m.b2[2]);
    }
    const double cos_rays = dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]);
    // T2
    const bool stereo1 = cam1.model == 0 && m.x_right1 >= 0.0, stereo2 = cam2.model == 0 && m.x_right2 >= 0.0;
    const double cs1 = stereo1 ? ovs_det_cos(2.0 * ovs_det_atan2(cam1.true_baseline / 2.0, m.depth1)) : 2.0;
    const double cs2 = stereo2 ? ovs_det_cos(2.0 * ovs_det_atan2(cam2.true_baseline / 2.0, m.depth2)) : 2.0;
    const double cos_stereo = cs2 < cs1 ? cs2 : cs1;
    // T3
    const bool any_stereo = stereo1 || stereo2;
    if (0.0 < cos_rays && ((!any_stereo && cos_rays < prm.cos_thr) || (any_stereo && cos_rays < cos_stereo))) {
        r.method = 1;
        two_view(P1, P2, m.b1, m.b2, r.pos_w);
    } else if (stereo1 && cs1 < cs2) {
        r.method = 2;
        back_project(cam1, P1, m.kp1, m.depth1, r.pos_w);
    } else if (stereo2 && cs2 < cs1) {
        r.method = 3;
        back_project(cam2, P2, m.kp2, m.depth2, r.pos_w);
    } else {
        r.status = 1;
        return r;
    }
    // T6 to T8: the first gate that fails names the status
    int status = 0;
    {
        const double dx1 = r.pos_w[0] - q.centre[0][0], dy1 = r.pos_w[1] - q.centre[0][1], dz1 = r.pos_w[2] - q.centre[0][2];
        const double dx2 = r.pos_w[0] - q.centre[1][0], dy2 = r.pos_w[1] - q.centre[1][1], dz2 = r.pos_w[2] - q.centre[1][2];
        const double d1 = ovs_dm::sqrt_d(dot3(dx1, dy1, dz1, dx1, dy1, dz1)), d2 = ovs_dm::sqrt_d(dot3(dx2, dy2, dz2, dx2, dy2, dz2));
        const double ratio_dists = d2 / d1, ratio_octave = m.scale_factor1 / m.scale_factor2;
        const bool scale_ok = d1 > 0.0 && d2 > 0.0 && ratio_octave <= ratio_dists * prm.ratio_factor && ratio_dists <= ratio_octave * prm.ratio_factor;
        status = scale_ok ? 0 : 6;
    }
    status = reprojection_is_good(cam2, P2, r.pos_w, m.kp2, stereo2, m.x_right2, m.sigma_sq2) ? status : 5;
    status = reprojection_is_good(cam1, P1, r.pos_w, m.kp1, stereo1, m.x_right1, m.sigma_sq1) ? status : 4;
    status = depth_is_positive(cam2, P2, r.pos_w) ? status : 3;
    status = depth_is_positive(cam1, P1, r.pos_w) ? status : 2;
    r.status = status;
    return r;
}

}   // namespace tri
