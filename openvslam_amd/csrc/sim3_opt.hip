// sim3_opt.hip -- optimize::transform_optimizer (expected: src/openvslam/optimize/transform_optimizer.{h,cc}): the Sim3 refinement over a batch
// of loop candidates (loop_detector runs it once per candidate after projection::match_by_Sim3_transform). Rules: DESIGN.md 3.11; the
// algebra is sim3_opt_math.inc, which a plain host compiler builds too.
//
// A problem is one (keyframe 1, keyframe 2) pair with n matches: p1 / p2 (the landmark in camera-1 / camera-2 coordinates), the two keypoints,
// their inv_level_sigma_sq, a camera per side and the initial Sim3_12. Everything is f64, every operation rounded on its own (the unit is
// built with -ffp-contract=off).
//
// k_sim3_optimize: one launch, grid = problems, one wavefront per workgroup and problem. Lane j owns the matches j, j + 64, ... and re-reads
// its 88 bytes per match on every pass. Lanes 0 .. 13 build the 14 perturbed states of rule 5 into LDS (2 KB); the edges read them as
// broadcasts. A lane's 28 Jacobian entries of a match pass through LDS too (14 KB, [entry][lane]: no bank conflicts), so that the seven
// columns are a loop and not seven copies of the two edge evaluations. The 36 sums of the normal equations end in a butterfly of
// x + shfl_xor(x, d), d = 32 .. 1: lane 0 holds rule 6's tree, and as IEEE addition commutes every lane holds the same bits. The 7 x 7
// Cholesky, the exponential and the Levenberg-Marquardt decisions are then computed by every lane for itself on compile-time indices:
// the values are wave-uniform, nothing is indexed dynamically, nothing goes to scratch. No atomics, no waiting between workgroups; every
// loop is bounded by num_iter and the ten trials of rule 7.
#include <cmath>
#include <cstring>

#include "ovs_common.h"
#include "solve_internal.inc"
#include "sim3_opt_math.inc"

namespace {

// the staged block of one call: solve_plan.inc
using splan::sim3opt::Layout;
using splan::sim3opt::layout_of;

// per problem in the result block
struct OptRec {
    double rot[9], trans[3], scale, info[8];
    int32_t num_inliers, pad;
};
static_assert(sizeof(OptRec) == 176, "OptRec is read by the host");

// sim3_opt_math.inc's 64 lanes as one wavefront
struct WaveLanes {
    static constexpr int kJacobianStride = 64;
    int lane;
    double* J;   // LDS [28][64]
    __device__ __forceinline__ double* jacobian(int l) { return J + l; }
    template <class F>
    __device__ __forceinline__ void each(F f) {
        f(lane);
    }
    template <int K, class F>
    __device__ __forceinline__ void sum(F f, double (&out)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = 0.0;
        f(lane, out);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int d = 32; d; d >>= 1) out[k] = out[k] + __shfl_xor(out[k], d);
    }
    template <class F>
    __device__ __forceinline__ void count(F f, int (&out)[1]) {
        int c = f(lane);
#pragma unroll
        for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
        out[0] = c;
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(64) void k_sim3_optimize(uint8_t* __restrict__ block, int P, int T, s3::Params prm, OptRec* __restrict__ out,
                                                      uint8_t* __restrict__ out_flags) {
    __shared__ s3::State pert[14];
    __shared__ double jac[28 * 64];
    const Layout lay = layout_of(P, T);
    const int p = blockIdx.x, lane = threadIdx.x;
    const auto [off, n] = problem_span(block, lay.offsets, p);
    const s3::Cam cam1 = reinterpret_cast<const s3::Cam*>(block + lay.cams)[2 * p], cam2 = reinterpret_cast<const s3::Cam*>(block + lay.cams)[2 * p + 1];
    const double* init = reinterpret_cast<const double*>(block + lay.init) + 13 * (size_t)p;
    const double* p1 = reinterpret_cast<const double*>(block + lay.p1) + 3 * (size_t)off;
    const double* p2 = reinterpret_cast<const double*>(block + lay.p2) + 3 * (size_t)off;
    const double* obs1 = reinterpret_cast<const double*>(block + lay.obs1) + 2 * (size_t)off;
    const double* obs2 = reinterpret_cast<const double*>(block + lay.obs2) + 2 * (size_t)off;
    const float* w1 = reinterpret_cast<const float*>(block + lay.w1) + off;
    const float* w2 = reinterpret_cast<const float*>(block + lay.w2) + off;
    uint8_t* work = block + lay.work + off;
    s3::State S;
#pragma unroll
    for (int k = 0; k < 9; ++k) S.R[k] = init[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) S.t[k] = init[9 + k];
    S.s = init[12];
    const auto load = [&](int i) {   // i < n
        s3::Match m;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            m.p1[x] = p1[3 * (size_t)i + x];
            m.p2[x] = p2[3 * (size_t)i + x];
        }
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            m.o1[x] = obs1[2 * (size_t)i + x];
            m.o2[x] = obs2[2 * (size_t)i + x];
        }
        m.w1 = (double)w1[i];
        m.w2 = (double)w2[i];
        return m;
    };
    WaveLanes x{lane, jac};
    s3::Result res;
    s3::s3_optimize(x, cam1, cam2, n, load, S, prm, work, pert, res);
    for (int i = lane; i < n; i += 64) out_flags[off + i] = work[i];   // a lane's own matches: written by itself
    if (lane == 0) {
        OptRec r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.rot[k] = res.est.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) r.trans[k] = res.est.t[k];
        r.scale = res.est.s;
#pragma unroll
        for (int k = 0; k < 8; ++k) r.info[k] = res.info[k];
        r.num_inliers = res.num_inliers;
        r.pad = 0;
        out[p] = r;
    }
}

}   // namespace

struct ovs_sim3opt : batch_handle {};

extern "C" {

ovs_status ovs_sim3opt_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_sim3opt** out) {
    return batch_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes, 0, 0, sizeof(OptRec), out, no_extra);
}

ovs_status ovs_sim3opt_destroy(ovs_sim3opt* s) { return batch_destroy(s); }

ovs_status ovs_sim3opt_optimize_batch(ovs_sim3opt* s, int32_t n_problems, const int32_t* offsets, const double* p1, const double* p2, const double* obs1,
                                      const double* obs2, const float* inv_sigma_sq_1, const float* inv_sigma_sq_2, const ovs_camera* cams_1,
                                      const ovs_camera* cams_2, const double* rot_12_in, const double* trans_12_in, const double* scale_12_in,
                                      int32_t fix_scale, float chi_sq, int32_t num_iter, int32_t* out_num_inliers, double* out_rot_12, double* out_trans_12,
                                      double* out_scale_12, uint8_t* out_outlier_flags, double* out_info) {
    const splan::sim3opt::Call call{s != nullptr, n_problems, offsets, p1, p2, obs1, obs2, inv_sigma_sq_1, inv_sigma_sq_2, cams_1, cams_2, rot_12_in,
                                    trans_12_in, scale_12_in, chi_sq, num_iter, out_num_inliers, out_rot_12, out_trans_12, out_scale_12, out_outlier_flags};
    const splan::Checked checked = splan::sim3opt::check(call, caps_of(s));
    const Layout lay = layout_of(n_problems, checked.T);
    s3::Params prm;   // (read only where the check accepted chi_sq)
    prm.fix_scale = fix_scale ? 1 : 0;
    prm.num_iter = num_iter;
    prm.chi_sq = (double)chi_sq;
    prm.delta = (double)std::sqrt(chi_sq);   // sqrtf: rule 4
    prm.delta_sq = prm.delta * prm.delta;
    const auto launch = [&](hipStream_t st, int32_t T) {
        hipLaunchKernelGGL(k_sim3_optimize, dim3(n_problems), dim3(64), 0, st, s->d_block, n_problems, T, prm, s->m_rec<OptRec>(), s->m_flags);
        OVS_HIP_TRY(hipGetLastError());
        return OVS_OK;
    };
    const auto collect = [&](int32_t T) {
        for (int32_t p = 0; p < n_problems; ++p) {
            const OptRec& r = s->h_rec<OptRec>()[p];
            out_num_inliers[p] = r.num_inliers;
            std::memcpy(out_rot_12 + 9 * (size_t)p, r.rot, sizeof(r.rot));
            std::memcpy(out_trans_12 + 3 * (size_t)p, r.trans, sizeof(r.trans));
            out_scale_12[p] = r.scale;
            if (out_info) std::memcpy(out_info + 8 * (size_t)p, r.info, sizeof(r.info));
        }
        if (T > 0) std::memcpy(out_outlier_flags, s->h_flags, (size_t)T);
    };
    return run_staged(s, checked, lay.bytes, [&] { splan::sim3opt::stage(call, lay, s->h_block); }, nothing_to_reserve, launch, collect);
}

}   // extern "C"
