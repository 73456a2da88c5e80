// solve_internal.inc -- what the RANSAC solvers of solve/ share on the device (sim3_solve.hip, pnp_solve.hip): the counter-based sampler's
// mixer, the cyclic Jacobi rotation and Horn's quaternion form of the absolute orientation. DESIGN.md 3.9 rule 2 fixes every operation;
// the units are built with -ffp-contract=off. (An .inc, not an .h: bench.py fingerprints every .h of this directory into the committed
// counters of the extractor and matcher stages, which include none of this.)
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one Jacobi rotation on the pair (P, Q) of an N x N symmetric matrix held in registers, the operations of
// essential_solver.h::compute_E_21: columns, then rows, then V
template <int N, int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[N][N], double (&V)[N][N]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
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

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// Horn's closed form with the scale left out: M[r][c] = sum over the centred pairs of b[r] * a[c]; R (row-major) is the rotation with
// a = R b in the least-squares sense. Eight cyclic sweeps over the 4 x 4 matrix, the eigenvector of the largest diagonal entry (lowest
// index on a tie; selects, not an indexed read), normalised.
__device__ __forceinline__ void horn_rotation(const double (&M)[3][3], double (&R)[9]) {
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[0][1] = M[1][2] - M[2][1];
    A[0][2] = M[2][0] - M[0][2];
    A[0][3] = M[0][1] - M[1][0];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[1][2] = M[0][1] + M[1][0];
    A[1][3] = M[2][0] + M[0][2];
    A[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    A[2][3] = M[1][2] + M[2][1];
    A[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < r) A[r][c] = A[c][r];
            V[r][c] = r == c ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
        jacobi_rotate<4, 0, 1>(A, V);
        jacobi_rotate<4, 0, 2>(A, V);
        jacobi_rotate<4, 0, 3>(A, V);
        jacobi_rotate<4, 1, 2>(A, V);
        jacobi_rotate<4, 1, 3>(A, V);
        jacobi_rotate<4, 2, 3>(A, V);
    }
    double best = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const bool take = A[i][i] > best;
        best = take ? A[i][i] : best;
        q0 = take ? V[0][i] : q0;
        q1 = take ? V[1][i] : q1;
        q2 = take ? V[2][i] : q2;
        q3 = take ? V[3][i] : q3;
    }
    const double nrm = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double w = q0 / nrm, x = q1 / nrm, y = q2 / nrm, z = q3 / nrm;
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

}   // namespace
