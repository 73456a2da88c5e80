// triangulate.hip -- module::two_view_triangulator::triangulate (expected: src/openvslam/module/two_view_triangulator.{h,cc}, with
// solve::triangulator::triangulate of src/openvslam/solve/triangulator.h under it): the new landmarks of a keyframe, for every matched pair
// of every neighbour in one call (local_map_updater's create_new_landmarks runs it once per pair after robust::match_for_triangulation).
// Rules: DESIGN.md 3.12; the algebra is triangulate_math.inc, which a plain host compiler builds too.
//
// A problem is one (keyframe 1, keyframe 2) pair: a camera, a pose and a camera centre per side, and n matches. Everything is f64, every
// operation rounded on its own (the unit is built with -ffp-contract=off).
//
// k_triangulate: one launch, one lane per match over the whole batch, 64 lanes (one wavefront) per workgroup. The host (splan::triangulate of
// solve_plan.inc: argument errors, capacity, layout, staging, read-back) stages the match inputs as structure-of-arrays (a wavefront's
// loads are whole lines) with a per-match problem index. A wavefront's matches may belong to
// several problems: it walks the distinct ones among its lanes (at most 64, ascending: a bounded loop), the lanes copy each record of
// 44 doubles and two camera models into LDS once (a coalesced read of 368 bytes), and every lane then reads its own problem's record
// from LDS, a broadcast wherever lanes share it. No atomics, no waiting between workgroups, no scratch: the 4 x 4 matrices live in
// registers on compile-time indices.
#include <cmath>
#include <cstring>

#include "ovs_common.h"
#include "solve_internal.inc"
#include "triangulate_math.inc"

namespace {

constexpr int kLanes = 64;
constexpr int kProblemDoubles = sizeof(tri::Problem) / 8;

// the staged block of one call (structure-of-arrays; the kernel's outputs are its last sections): solve_plan.inc
using splan::triangulate::Layout;
using splan::triangulate::layout_of;

__global__ __launch_bounds__(kLanes) void k_triangulate(uint8_t* __restrict__ block, int P, int T, tri::Params prm) {
    __shared__ double records[kLanes * kProblemDoubles];
    const Layout lay = layout_of(P, T);
    const int lane = threadIdx.x;
    const int i = blockIdx.x * kLanes + lane;
    const bool live = i < T;
    const int my_problem = live ? reinterpret_cast<const int32_t*>(block + lay.pidx)[i] : -1;
    // the distinct problems of this wavefront's lanes, each record copied into LDS once
    int my_slot = 0;
    {
        unsigned long long remaining = __ballot(live);
        int slot = 0;
        while (remaining) {   // at most 64 rounds: every round retires at least its leader
            const int leader = __ffsll((long long)remaining) - 1;
            const int p = __shfl(my_problem, leader);
            const double* src = reinterpret_cast<const double*>(block + lay.problems) + (size_t)p * kProblemDoubles;
            if (lane < kProblemDoubles) records[slot * kProblemDoubles + lane] = src[lane];
            const bool mine = live && my_problem == p;
            my_slot = mine ? slot : my_slot;
            remaining &= ~__ballot(mine);
            ++slot;
        }
    }
    __syncthreads();
    if (!live) return;
    const tri::Problem& q = *reinterpret_cast<const tri::Problem*>(records + my_slot * kProblemDoubles);
    const double* b1 = reinterpret_cast<const double*>(block + lay.b1);
    const double* b2 = reinterpret_cast<const double*>(block + lay.b2);
    const float* f = reinterpret_cast<const float*>(block + lay.f32);
    const auto plane = [&](int k) { return (double)f[(size_t)k * lay.Te + (size_t)i]; };
    tri::Match m;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        m.b1[x] = b1[(size_t)x * T + i];
        m.b2[x] = b2[(size_t)x * T + i];
    }
    m.kp1[0] = plane(0), m.kp1[1] = plane(1), m.kp2[0] = plane(2), m.kp2[1] = plane(3);
    m.x_right1 = plane(4), m.x_right2 = plane(5), m.depth1 = plane(6), m.depth2 = plane(7);
    m.sigma_sq1 = plane(8), m.sigma_sq2 = plane(9), m.scale_factor1 = plane(10), m.scale_factor2 = plane(11);
    const tri::Result r = tri::triangulate(q, m, prm);
    double* pos = reinterpret_cast<double*>(block + lay.pos);
#pragma unroll
    for (int x = 0; x < 3; ++x) pos[(size_t)x * T + i] = r.pos_w[x];
    block[lay.status + i] = (uint8_t)r.status;
    block[lay.method + i] = (uint8_t)r.method;
}

}   // namespace

struct ovs_triangulate : batch_handle {};   // the results come back through the staged block: no records, no result block, no flags

extern "C" {

ovs_status ovs_triangulate_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_triangulate** out) {
    return batch_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes, 0, 0, 0, out, no_extra);
}

ovs_status ovs_triangulate_destroy(ovs_triangulate* s) { return batch_destroy(s); }

ovs_status ovs_triangulate_batch(ovs_triangulate* s, int32_t n_problems, const int32_t* offsets, const double* bearings_1, const double* bearings_2,
                                 const float* keypts_1, const float* keypts_2, const float* x_right_1, const float* x_right_2, const float* depths_1,
                                 const float* depths_2, const float* sigma_sq_1, const float* sigma_sq_2, const float* scale_factors_1,
                                 const float* scale_factors_2, const ovs_camera* cams_1, const ovs_camera* cams_2, const double* poses_cw_1,
                                 const double* poses_cw_2, double cos_rays_parallax_thr, float ratio_factor, double* out_pos_w, uint8_t* out_status,
                                 uint8_t* out_method, int32_t* out_num_accepted) {
    const splan::triangulate::Call call{s != nullptr, n_problems, offsets, bearings_1, bearings_2, keypts_1, keypts_2, x_right_1, x_right_2, depths_1,
                                        depths_2, sigma_sq_1, sigma_sq_2, scale_factors_1, scale_factors_2, cams_1, cams_2, poses_cw_1, poses_cw_2,
                                        cos_rays_parallax_thr, ratio_factor, out_pos_w, out_status, out_method, out_num_accepted};
    const splan::Checked checked = splan::triangulate::check(call, caps_of(s));
    const Layout lay = layout_of(n_problems, checked.T);
    tri::Params prm;
    prm.cos_thr = cos_rays_parallax_thr;
    prm.ratio_factor = (double)ratio_factor;
    const auto launch = [&](hipStream_t st, int32_t T) {
        if (T == 0) return OVS_OK;
        hipLaunchKernelGGL(k_triangulate, dim3((T + kLanes - 1) / kLanes), dim3(kLanes), 0, st, s->d_block, n_problems, T, prm);
        OVS_HIP_TRY(hipGetLastError());
        OVS_HIP_TRY(hipMemcpyAsync(s->h_block + lay.pos, s->d_block + lay.pos, lay.bytes - lay.pos, hipMemcpyDeviceToHost, st));
        return OVS_OK;
    };
    return run_staged(
        s, checked, lay.bytes, [&] { splan::triangulate::stage(call, lay, s->h_block); }, nothing_to_reserve, launch,
        [&](int32_t) { splan::triangulate::collect(call, lay, s->h_block); });
}

}   // extern "C"
