// jacobi_math.inc -- the cyclic Jacobi rotation on a symmetric matrix held in registers, for the device and for a plain host compiler alike:
// solve_internal.inc (Horn's quaternion form under Sim3, EPnP and the transform optimiser's callers) and triangulate_math.inc (the null vector
// of the two-view system) share it. The operations are those of jacobi_angle and jacobi_rotate below, every one rounded on its own (the units
// are built with -ffp-contract=off); sqrt and fabs are correctly rounded on both sides. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__HIP__)
#define OVS_JACOBI_FN __host__ __device__ __forceinline__
#else
#define OVS_JACOBI_FN inline
#endif

namespace ovs_jacobi {

// the rotation (c, s) that zeroes the off-diagonal entry apq != 0 of a symmetric matrix with the diagonal entries app, aqq
OVS_JACOBI_FN void jacobi_angle(double app, double aqq, double apq, double& c, double& s) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

// one Jacobi rotation on the pair (P, Q) of an N x N symmetric matrix held in registers: columns, then rows, then V
template <int N, int P, int Q>
OVS_JACOBI_FN void jacobi_rotate(double (&A)[N][N], double (&V)[N][N]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    double c, s;
    jacobi_angle(A[P][P], A[Q][Q], apq, c, s);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

}   // namespace ovs_jacobi
