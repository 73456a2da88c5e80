// ba_linearize.hip -- B1-B3: reprojection residual, analytic 2x3 / 2x6 Jacobians and the normal-equation blocks of local
// bundle adjustment (expected: src/openvslam/optimize/g2o/se3/perspective_reproj_edge.{h,cc}, reproj_edge_wrapper.h; g2o
// BaseBinaryEdge::constructQuadraticForm, RobustKernelHuber, BlockSolver_6_3::buildSystem under
// optimize::local_bundle_adjuster::optimize).
//
// One lane per observation (edge), fp64, every product individually rounded (-ffp-contract=off) in the oracle's order, so the
// per-edge quantities (residual, Jacobians, Hpl block) are bit-identical to the CPU; only the SUMS differ by association:
//   * Hll / bl (3x3 + 3 per landmark): fp64 global atomics -- landmarks are scattered, contention is low;
//   * Hpp / bp (6x6 + 6 per keyframe): edges arrive grouped by keyframe, so a wave whose lanes share one pose reduces the 21
//     upper-triangle terms + 6 gradient terms with cross-lane shuffles and issues ONE atomic per term; mixed waves fall back
//     to per-lane atomics;
//   * Hpl (6x3 per edge) needs no reduction and is written once.
// Bandwidth/atomic-bound (20 MB per 100 k-edge linearisation, ~35 MFLOP): no LDS staging to gain. Across GPUs the edges are
// partitioned by keyframe and only the dense Hll|bl buffer needs a sum (RCCL all-reduce, host layer: openvslam_amd/ba.py).
#include <algorithm>
#include <type_traits>

#include "ba_edge.h"
#include "ba_internal.h"
#include "owned_internal.inc"

namespace ovs {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// D = 2: mono_perspective_reproj_edge (or, model 1, equirectangular_reproj_edge); D = 3: stereo_perspective_reproj_edge (third residual
// u_r = u - bf / z). The edge model is ba_edge.h's; "stereo" is D == 3, a constant the inlined model folds: a mono edge's third Jacobian row is
// never read.
template <int D>
struct EdgeOf;
template <>
struct EdgeOf<2> {
    typedef ovs_ba_edge type;
};
template <>
struct EdgeOf<3> {
    typedef ovs_ba_edge_stereo type;
};

constexpr int kEdgesPerThread = 2;   // 1, 2, 4 measured within 2 % of each other at 100 k edges: fabric-side fp64 atomics bound the kernel

template <int D>
__global__ __launch_bounds__(256) void k_ba_linearize(const double* __restrict__ poses, const uint8_t* __restrict__ pose_fixed,
                                                     int n_pose, const double* __restrict__ points, int n_pt,
                                                     const typename EdgeOf<D>::type* __restrict__ edges, int n_edge, ovs_ba_cam cam,
                                                     int model, double bf, double huber_delta, double* __restrict__ Hpp, double* __restrict__ bp,
                                                     double* __restrict__ Hll, double* __restrict__ bl, double* __restrict__ Hpl,
                                                     double* __restrict__ chi2) {
    // A workgroup takes kEdgesPerThread * 256 consecutive edges; lane l of wave w handles edges base + 64 (4 k + w) + l. Edges arrive
    // grouped by keyframe, so a wave usually sees ONE pose for all its iterations: its 21 + 6 pose-block terms are accumulated per lane
    // across the iterations and reduced across the wave once (the 27 fp64 wave reductions per 64 edges were a quarter of the kernel).
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    int acc_pose = -1;
    auto flush = [&]() {
        if (acc_pose < 0) return;
        double* hp = Hpp + 36 * (size_t)acc_pose;
        double* gp = bp + 6 * (size_t)acc_pose;
        int t = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) {
                const double sv = wave_sum_f64(acc[t]);
                acc[t++] = 0.0;
                if ((threadIdx.x & 63) == 0) {
                    atomicAdd(&hp[6 * a + b], sv);
                    if (b != a) atomicAdd(&hp[6 * b + a], sv);
                }
            }
            const double g = wave_sum_f64(acc[t]);
            acc[t++] = 0.0;
            if ((threadIdx.x & 63) == 0) atomicAdd(&gp[a], g);
        }
        acc_pose = -1;
    };
#pragma unroll 1
    for (int it = 0; it < kEdgesPerThread; ++it) {
    const int e = (blockIdx.x * kEdgesPerThread + it) * 256 + threadIdx.x;
    const bool valid = e < n_edge;
    int pose = -1, pt = 0;
    constexpr bool kStereo = D == 3;
    double Jl[3][6] = {}, Jp[3][6] = {};   // (padded to 6 columns so the landmark (3) and pose (6) blocks share dot3)
    double W = 0, r[3] = {}, c2 = 0, rho0 = 0;
    if (valid) {
        const typename EdgeOf<D>::type ed = edges[e];
        pose = ed.pose_idx;
        pt = ed.point_idx;
        GEdge ge{pose, pt, ed.obs_x, ed.obs_y, 0.0, ed.inv_sigma_sq};
        if constexpr (kStereo) ge.oxr = ed.obs_x_right;
        const double* P = poses + 7 * (size_t)pose;
        const double* X = points + 3 * (size_t)pt;
        // (model 1, mono only: cam.fx / cam.fy carry cols / rows)
        if (!kStereo && model == 1) edge_lin_equirect(P, X, ge, cam, huber_delta, Jl, Jp, r, W, c2, rho0);
        else edge_lin(P, X, ge, kStereo, cam, bf, huber_delta, Jl, Jp, r, W, c2, rho0);
        // landmark block: scattered fp64 atomics
        double* hl = Hll + 9 * (size_t)pt;
        double* gl = bl + 3 * (size_t)pt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) atomicAdd(&hl[3 * a + b], W * dot3(Jl, a, Jl, b, kStereo));
            atomicAdd(&gl[a], dot3r(Jl, a, r, kStereo));
        }
    }
    const bool free_pose = valid && !(pose_fixed && pose_fixed[pose]);
    if (valid) {   // blocks of fixed poses are zero (written here: no 14 MB memset in front of the kernel)
        double* hpl = Hpl + 18 * (size_t)e;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) hpl[3 * a + b] = free_pose ? W * dot3(Jp, a, Jl, b, kStereo) : 0.0;
    }
    // chi2: one atomic per wave
    {
        const double s0 = wave_sum_f64(valid ? c2 : 0.0), s1 = wave_sum_f64(valid ? rho0 : 0.0);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&chi2[0], s0);
            atomicAdd(&chi2[1], s1);
        }
    }
    auto grad = [&](int a) { return dot3r(Jp, a, r, kStereo); };
    // pose block
    const int p0 = __builtin_amdgcn_readfirstlane(pose);
    const bool uniform = __all(!valid || pose == p0) && p0 >= 0;
    if (uniform) {
        if (__any(free_pose)) {   // wave-uniform: all valid lanes share pose p0, hence the same fixed flag
            if (acc_pose != p0) flush();
            acc_pose = p0;
            if (free_pose) {
                int t = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
#pragma unroll
                    for (int b = a; b < 6; ++b) acc[t++] += W * dot3(Jp, a, Jp, b, kStereo);
                    acc[t++] += grad(a);
                }
            }
        }
    } else {
        flush();
        if (free_pose) {
            double* hp = Hpp + 36 * (size_t)pose;
            double* gp = bp + 6 * (size_t)pose;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int b = 0; b < 6; ++b) atomicAdd(&hp[6 * a + b], W * dot3(Jp, a, Jp, b, kStereo));
                atomicAdd(&gp[a], grad(a));
            }
        }
    }
    }   // edges of this thread
    flush();
}

// one launch instead of five hipMemsetAsync calls (each costs a launch: they were ~25 us of a 128 us linearisation call)
__global__ __launch_bounds__(256) void k_ba_zero(double* __restrict__ a, size_t na, double* __restrict__ b, size_t nb, double* __restrict__ c,
                                                size_t nc, double* __restrict__ d, size_t nd, double* __restrict__ e, size_t ne) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t k = i; k < na; k += stride) a[k] = 0.0;
    for (size_t k = i; k < nb; k += stride) b[k] = 0.0;
    for (size_t k = i; k < nc; k += stride) c[k] = 0.0;
    for (size_t k = i; k < nd; k += stride) d[k] = 0.0;
    for (size_t k = i; k < ne; k += stride) e[k] = 0.0;
}

}   // namespace ovs

using namespace ovs;

namespace {

template <class Edge>
constexpr int kResidualDim = std::is_same<Edge, ovs_ba_edge_stereo>::value ? 3 : 2;

// behind the three _dev entries: the argument check, the blocks zeroed unless the call accumulates, the launch
template <class Edge>
ovs_status linearize_on_device(int model, const double* d_poses, const uint8_t* d_pose_fixed, int32_t n_pose, const double* d_points, int32_t n_pt,
                               const Edge* d_edges, int32_t n_edge, const ovs_ba_cam* cam, double bf, double huber_delta, bool accumulate,
                               double* d_Hpp, double* d_bp, double* d_Hll, double* d_bl, double* d_Hpl, double* d_chi2, void* stream) {
    if (!d_poses || !d_points || !cam || !d_Hpp || !d_bp || !d_Hll || !d_bl || !d_Hpl || !d_chi2 || n_pose < 1 || n_pt < 1 || n_edge < 0 ||
        (n_edge > 0 && !d_edges))
        return OVS_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) {
        hipLaunchKernelGGL(k_ba_zero, dim3(128), dim3(256), 0, s, d_Hpp, (size_t)36 * n_pose, d_bp, (size_t)6 * n_pose, d_Hll, (size_t)9 * n_pt, d_bl,
                           (size_t)3 * n_pt, d_chi2, (size_t)2);
        OVS_HIP_TRY(hipGetLastError());
    }
    if (n_edge == 0) return OVS_OK;
    hipLaunchKernelGGL(k_ba_linearize<kResidualDim<Edge>>, dim3((n_edge + 256 * kEdgesPerThread - 1) / (256 * kEdgesPerThread)), dim3(256), 0, s, d_poses,
                       d_pose_fixed, n_pose, d_points, n_pt, d_edges, n_edge, *cam, model, bf, huber_delta, d_Hpp, d_bp, d_Hll, d_bl, d_Hpl, d_chi2);
    OVS_HIP_TRY(hipGetLastError());
    return OVS_OK;
}

// behind the three host-array entries: one allocation for the inputs, one for the blocks, blocking copies on the null stream
template <class Edge>
ovs_status linearize_from_host(int model, int32_t device, const double* poses, const uint8_t* pose_fixed, int32_t n_pose, const double* points,
                               int32_t n_pt, const Edge* edges, int32_t n_edge, const ovs_ba_cam* cam, double bf, double huber_delta, double* Hpp,
                               double* bp, double* Hll, double* bl, double* Hpl, double* chi2) {
    if (!poses || !points || !cam || !Hpp || !bp || !Hll || !bl || !Hpl || !chi2 || n_pose < 1 || n_pt < 1 || n_edge < 0 || (n_edge > 0 && !edges))
        return OVS_ERR_INVALID;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    const size_t np = (size_t)n_pose, npt = (size_t)n_pt, ne = (size_t)n_edge, ne1 = std::max<size_t>(ne, 1);
    ArenaLayout in, out;
    const size_t i_pose = in.place<double>(7 * np), i_pt = in.place<double>(3 * npt), i_e = in.place<Edge>(ne1), i_f = in.place<uint8_t>(np);
    const size_t o_Hpp = out.place<double>(36 * np), o_bp = out.place<double>(6 * np), o_Hll = out.place<double>(9 * npt),
                 o_bl = out.place<double>(3 * npt), o_Hpl = out.place<double>(18 * ne1), o_chi = out.place<double>(2);
    ovs::Owned tmp;
    unsigned char *d_in = nullptr, *d_out = nullptr;
    OVS_HIP_TRY(tmp.dev(&d_in, in.bytes()));
    OVS_HIP_TRY_RAW(tmp.dev(&d_out, out.bytes()));
    OVS_HIP_TRY_RAW(hipMemcpy(d_in + i_pose, poses, sizeof(double) * 7 * np, hipMemcpyHostToDevice));
    OVS_HIP_TRY_RAW(hipMemcpy(d_in + i_pt, points, sizeof(double) * 3 * npt, hipMemcpyHostToDevice));
    if (n_edge) OVS_HIP_TRY_RAW(hipMemcpy(d_in + i_e, edges, sizeof(Edge) * ne, hipMemcpyHostToDevice));
    if (pose_fixed) OVS_HIP_TRY_RAW(hipMemcpy(d_in + i_f, pose_fixed, np, hipMemcpyHostToDevice));
    const ovs_status st = linearize_on_device(model, ArenaLayout::at<double>(d_in, i_pose), pose_fixed ? d_in + i_f : nullptr, n_pose,
                                              ArenaLayout::at<double>(d_in, i_pt), n_pt, ArenaLayout::at<Edge>(d_in, i_e), n_edge, cam, bf, huber_delta, false,
                                              ArenaLayout::at<double>(d_out, o_Hpp), ArenaLayout::at<double>(d_out, o_bp), ArenaLayout::at<double>(d_out, o_Hll),
                                              ArenaLayout::at<double>(d_out, o_bl), ArenaLayout::at<double>(d_out, o_Hpl), ArenaLayout::at<double>(d_out, o_chi),
                                              nullptr);
    if (st != OVS_OK) return st;
    OVS_HIP_TRY_RAW(hipDeviceSynchronize());
    OVS_HIP_TRY_RAW(hipMemcpy(Hpp, d_out + o_Hpp, sizeof(double) * 36 * np, hipMemcpyDeviceToHost));
    OVS_HIP_TRY_RAW(hipMemcpy(bp, d_out + o_bp, sizeof(double) * 6 * np, hipMemcpyDeviceToHost));
    OVS_HIP_TRY_RAW(hipMemcpy(Hll, d_out + o_Hll, sizeof(double) * 9 * npt, hipMemcpyDeviceToHost));
    OVS_HIP_TRY_RAW(hipMemcpy(bl, d_out + o_bl, sizeof(double) * 3 * npt, hipMemcpyDeviceToHost));
    if (n_edge) OVS_HIP_TRY_RAW(hipMemcpy(Hpl, d_out + o_Hpl, sizeof(double) * 18 * ne, hipMemcpyDeviceToHost));
    OVS_HIP_TRY_RAW(hipMemcpy(chi2, d_out + o_chi, sizeof(double) * 2, hipMemcpyDeviceToHost));
    return OVS_OK;
}

}   // namespace

extern "C" {

ovs_status ovs_ba_linearize_dev(const double* d_poses, const uint8_t* d_pose_fixed, int32_t n_pose, const double* d_points,
                                int32_t n_pt, const ovs_ba_edge* d_edges, int32_t n_edge, const ovs_ba_cam* cam, double huber_delta,
                                double* d_Hpp, double* d_bp, double* d_Hll, double* d_bl, double* d_Hpl, double* d_chi2, void* stream) {
    return linearize_on_device(0, d_poses, d_pose_fixed, n_pose, d_points, n_pt, d_edges, n_edge, cam, 0.0, huber_delta, false, d_Hpp, d_bp, d_Hll,
                               d_bl, d_Hpl, d_chi2, stream);
}

ovs_status ovs_ba_linearize_equirect_dev(const double* d_poses, const uint8_t* d_pose_fixed, int32_t n_pose, const double* d_points,
                                         int32_t n_pt, const ovs_ba_edge* d_edges, int32_t n_edge, int32_t cols, int32_t rows,
                                         double huber_delta, double* d_Hpp, double* d_bp, double* d_Hll, double* d_bl, double* d_Hpl,
                                         double* d_chi2, void* stream) {
    if (cols < 1 || rows < 1) return OVS_ERR_INVALID;
    const ovs_ba_cam c = {(double)cols, (double)rows, 0.0, 0.0};   // the kernel reads cols / rows from fx / fy for model 1
    return linearize_on_device(1, d_poses, d_pose_fixed, n_pose, d_points, n_pt, d_edges, n_edge, &c, 0.0, huber_delta, false, d_Hpp, d_bp, d_Hll,
                               d_bl, d_Hpl, d_chi2, stream);
}

ovs_status ovs_ba_linearize_stereo_dev(const double* d_poses, const uint8_t* d_pose_fixed, int32_t n_pose, const double* d_points,
                                       int32_t n_pt, const ovs_ba_edge_stereo* d_edges, int32_t n_edge, const ovs_ba_cam* cam,
                                       double focal_x_baseline, double huber_delta, int32_t accumulate, double* d_Hpp, double* d_bp,
                                       double* d_Hll, double* d_bl, double* d_Hpl, double* d_chi2, void* stream) {
    return linearize_on_device(0, d_poses, d_pose_fixed, n_pose, d_points, n_pt, d_edges, n_edge, cam, focal_x_baseline, huber_delta, accumulate != 0,
                               d_Hpp, d_bp, d_Hll, d_bl, d_Hpl, d_chi2, stream);
}

ovs_status ovs_ba_linearize(int32_t device, const double* poses, const uint8_t* pose_fixed, int32_t n_pose, const double* points,
                            int32_t n_pt, const ovs_ba_edge* edges, int32_t n_edge, const ovs_ba_cam* cam, double huber_delta,
                            double* Hpp, double* bp, double* Hll, double* bl, double* Hpl, double* chi2) {
    return linearize_from_host(0, device, poses, pose_fixed, n_pose, points, n_pt, edges, n_edge, cam, 0.0, huber_delta, Hpp, bp, Hll, bl, Hpl, chi2);
}

ovs_status ovs_ba_linearize_equirect(int32_t device, const double* poses, const uint8_t* pose_fixed, int32_t n_pose, const double* points,
                                     int32_t n_pt, const ovs_ba_edge* edges, int32_t n_edge, int32_t cols, int32_t rows, double huber_delta,
                                     double* Hpp, double* bp, double* Hll, double* bl, double* Hpl, double* chi2) {
    if (cols < 1 || rows < 1) return OVS_ERR_INVALID;
    const ovs_ba_cam c = {(double)cols, (double)rows, 0.0, 0.0};
    return linearize_from_host(1, device, poses, pose_fixed, n_pose, points, n_pt, edges, n_edge, &c, 0.0, huber_delta, Hpp, bp, Hll, bl, Hpl, chi2);
}

ovs_status ovs_ba_linearize_stereo(int32_t device, const double* poses, const uint8_t* pose_fixed, int32_t n_pose, const double* points,
                                   int32_t n_pt, const ovs_ba_edge_stereo* edges, int32_t n_edge, const ovs_ba_cam* cam,
                                   double focal_x_baseline, double huber_delta, double* Hpp, double* bp, double* Hll, double* bl,
                                   double* Hpl, double* chi2) {
    return linearize_from_host(0, device, poses, pose_fixed, n_pose, points, n_pt, edges, n_edge, cam, focal_x_baseline, huber_delta, Hpp, bp, Hll, bl,
                               Hpl, chi2);
}

}   // extern "C"
