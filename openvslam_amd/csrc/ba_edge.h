// ba_edge.h -- the reprojection-edge model of local bundle adjustment, once (device only): quaternion -> R, the camera-frame point, the
// perspective (mono / stereo) or equirectangular residual, the Huber weight and the analytic Jacobians
// (expected: src/openvslam/optimize/g2o/se3/perspective_reproj_edge.{h,cc}, equirectangular_reproj_edge.{h,cc}, reproj_edge_wrapper.h;
// g2o RobustKernelHuber). Users: k_ba_linearize<D> (ba_linearize.hip), lin_pose_half, lin_landmark_wg and k_edge_chi2 (ba_graph.hip).
// The library is compiled with -ffp-contract=off: every product is individually rounded, in the CPU oracle's order, so the per-edge quantities
// are the oracle's bits. Every caller goes through these expressions; none restates them.
#pragma once
#include "ovs_common.h"

namespace ovs {

struct GEdge {   // mono and stereo observations in one record (ba_graph.hip: stereo iff index >= n_mono)
    int32_t pose, pt;
    double ox, oy, oxr, w;
};

// Jacobians are carried as [3][6] arrays; the third row is zero for a mono edge (never read: dot3 stops at two rows)
__device__ __forceinline__ double dot3(const double (&A)[3][6], int a, const double (&B)[3][6], int b, bool stereo) {
    double s = A[0][a] * B[0][b];
    s = s + A[1][a] * B[1][b];
    if (stereo) s = s + A[2][a] * B[2][b];
    return s;
}

// column a of J^T times the weighted residual r (a gradient term), rows in order
__device__ __forceinline__ double dot3r(const double (&J)[3][6], int a, const double (&r)[3], bool stereo) {
    double g = J[0][a] * r[0];
    g = g + J[1][a] * r[1];
    if (stereo) g = g + J[2][a] * r[2];
    return g;
}

// R of the 7-double pose record P = {t, q = (x, y, z, w)} and the landmark X in the camera frame
__device__ __forceinline__ void edge_cam_point(const double* __restrict__ P, const double* __restrict__ X, double (&R)[3][3], double& x, double& y,
                                               double& z) {
    const double qx = P[3], qy = P[4], qz = P[5], qw = P[6];
    const double tx2 = 2 * qx, ty2 = 2 * qy, tz2 = 2 * qz;
    const double twx = tx2 * qw, twy = ty2 * qw, twz = tz2 * qw;
    const double txx = tx2 * qx, txy = ty2 * qx, txz = tz2 * qx;
    const double tyy = ty2 * qy, tyz = tz2 * qy, tzz = tz2 * qz;
    R[0][0] = 1 - (tyy + tzz), R[0][1] = txy - twz, R[0][2] = txz + twy;
    R[1][0] = txy + twz, R[1][1] = 1 - (txx + tzz), R[1][2] = tyz - twx;
    R[2][0] = txz - twy, R[2][1] = tyz + twx, R[2][2] = 1 - (txx + tyy);
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    x = R[0][0] * X0 + R[0][1] * X1 + R[0][2] * X2 + P[0];
    y = R[1][0] * X0 + R[1][1] * X1 + R[1][2] * X2 + P[1];
    z = R[2][0] * X0 + R[2][1] * X1 + R[2][2] * X2 + P[2];
}

// perspective residual (third component u_r = u - bf / z for a stereo edge, else 0); returns its squared norm
__device__ __forceinline__ double edge_residual(double x, double y, double invz, const GEdge& ed, bool stereo, const ovs_ba_cam& cam, double bf,
                                                double (&er)[3]) {
    const double u = cam.fx * x * invz + cam.cx;
    er[0] = ed.ox - u;
    er[1] = ed.oy - (cam.fy * y * invz + cam.cy);
    er[2] = 0.0;
    double ss = er[0] * er[0] + er[1] * er[1];
    if (stereo) {
        er[2] = ed.oxr - (u - bf * invz);
        ss = ss + er[2] * er[2];
    }
    return ss;
}

// equirectangular residual (cam = {cols, rows, -, -}); L = |pos_c|; returns its squared norm
__device__ __forceinline__ double edge_residual_equirect(double x, double y, double z, const GEdge& ed, const ovs_ba_cam& cam, double& L,
                                                         double (&er)[3]) {
    const double kPi = 3.14159265358979323846;
    L = sqrt((x * x + y * y) + z * z);
    const double theta = ovs_det_atan2(x, z);
    const double phi = -ovs_det_asin(y / L);
    er[0] = ed.ox - cam.fx * (0.5 + theta / (2.0 * kPi));
    er[1] = ed.oy - cam.fy * (0.5 - phi / kPi);
    er[2] = 0.0;
    return er[0] * er[0] + er[1] * er[1];
}

// g2o RobustKernelHuber on c2 = w |e|^2: returns rho'(c2), rho0 = rho(c2)
__device__ __forceinline__ double edge_huber(double c2, double huber, double& rho0) {
    rho0 = c2;
    double rho1 = 1.0;
    const double dsqr = huber * huber;
    if (huber > 0 && c2 > dsqr) {
        const double sq = sqrt(c2);
        rho0 = 2 * sq * huber - dsqr;
        rho1 = huber / sq;
    }
    return rho1;
}

// residual, Jacobians, Huber weight of one perspective edge -- the operation order of the CPU oracle
__device__ __forceinline__ void edge_lin(const double* __restrict__ P, const double* __restrict__ X, const GEdge& ed, bool stereo,
                                         const ovs_ba_cam& cam, double bf, double huber, double (&Jl)[3][6], double (&Jp)[3][6], double (&r)[3],
                                         double& W, double& c2, double& rho0) {
    double R[3][3], x, y, z, er[3];
    edge_cam_point(P, X, R, x, y, z);
    const double invz = 1.0 / z, invz2 = invz * invz;
    const double ss = edge_residual(x, y, invz, ed, stereo, cam, bf, er);
    const double w = ed.w;
    c2 = w * ss;
    const double rho1 = edge_huber(c2, huber, rho0);
#pragma unroll
    for (int c = 0; c < 6; ++c) Jl[0][c] = Jl[1][c] = Jl[2][c] = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Jl[0][c] = -invz * (cam.fx * R[0][c] - cam.fx * x * invz * R[2][c]);
        Jl[1][c] = -invz * (cam.fy * R[1][c] - cam.fy * y * invz * R[2][c]);
        Jl[2][c] = stereo ? Jl[0][c] - bf * R[2][c] * invz2 : 0.0;
    }
    Jp[0][0] = x * y * invz2 * cam.fx;
    Jp[0][1] = -(1 + x * x * invz2) * cam.fx;
    Jp[0][2] = y * invz * cam.fx;
    Jp[0][3] = -invz * cam.fx;
    Jp[0][4] = 0;
    Jp[0][5] = x * invz2 * cam.fx;
    Jp[1][0] = (1 + y * y * invz2) * cam.fy;
    Jp[1][1] = -x * y * invz2 * cam.fy;
    Jp[1][2] = -x * invz * cam.fy;
    Jp[1][3] = 0;
    Jp[1][4] = -invz * cam.fy;
    Jp[1][5] = y * invz2 * cam.fy;
    if (stereo) {
        Jp[2][0] = Jp[0][0] - bf * y * invz2;
        Jp[2][1] = Jp[0][1] + bf * x * invz2;
        Jp[2][2] = Jp[0][2];
        Jp[2][3] = Jp[0][3];
        Jp[2][4] = 0;
        Jp[2][5] = Jp[0][5] - bf * invz2;
    } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) Jp[2][c] = 0.0;
    }
    W = rho1 * w;
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = -W * er[k];
}

// the equirectangular edge (model 1): mono edges only (rows 2 stay zero). equirectangular_reproj_edge::linearizeOplus: with dp the derivative of
// pos_c w.r.t. one state component,
//   d u = (cols / 2 pi) (z dp_x - x dp_z) / (x^2 + z^2),  d v = (rows / pi) (L dp_y - y dL) / (L sqrt(x^2 + z^2)),  dL = pos_c . dp / L,
// and J = -d(u, v). Columns: rotation (e_k x pos_c), translation (e_k), landmark (R's columns).
__device__ __forceinline__ void edge_lin_equirect(const double* __restrict__ P, const double* __restrict__ X, const GEdge& ed, const ovs_ba_cam& cam,
                                                  double huber, double (&Jl)[3][6], double (&Jp)[3][6], double (&r)[3], double& W, double& c2,
                                                  double& rho0) {
    double R[3][3], x, y, z, er[3], L;
    edge_cam_point(P, X, R, x, y, z);
    const double kPi = 3.14159265358979323846;
    const double cols = cam.fx, rows = cam.fy;
    const double ss = edge_residual_equirect(x, y, z, ed, cam, L, er);
    const double rxz = x * x + z * z;
    const double w = ed.w;
    c2 = w * ss;
    const double rho1 = edge_huber(c2, huber, rho0);
    const double a0 = -(cols / (2.0 * kPi)) * (1.0 / rxz);
    const double a1 = -(rows / kPi) * (1.0 / (L * sqrt(rxz)));
    auto col = [&](double dx, double dy, double dz, double& j0, double& j1) {
        const double dL = (1.0 / L) * ((x * dx + y * dy) + z * dz);
        j0 = a0 * (z * dx - x * dz);
        j1 = a1 * (L * dy - y * dL);
    };
#pragma unroll
    for (int c = 0; c < 6; ++c) Jl[0][c] = Jl[1][c] = Jl[2][c] = Jp[2][c] = 0.0;
    col(0.0, -z, y, Jp[0][0], Jp[1][0]);
    col(z, 0.0, -x, Jp[0][1], Jp[1][1]);
    col(-y, x, 0.0, Jp[0][2], Jp[1][2]);
    col(1.0, 0.0, 0.0, Jp[0][3], Jp[1][3]);
    col(0.0, 1.0, 0.0, Jp[0][4], Jp[1][4]);
    col(0.0, 0.0, 1.0, Jp[0][5], Jp[1][5]);
#pragma unroll
    for (int c = 0; c < 3; ++c) col(R[0][c], R[1][c], R[2][c], Jl[0][c], Jl[1][c]);
    W = rho1 * w;
    r[0] = -W * er[0];
    r[1] = -W * er[1];
    r[2] = 0.0;
}

}   // namespace ovs
