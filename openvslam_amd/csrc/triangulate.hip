// triangulate.hip -- module::two_view_triangulator::triangulate (expected: src/openvslam/module/two_view_triangulator.{h,cc}, with
// solve::triangulator::triangulate of src/openvslam/solve/triangulator.h under it): the new landmarks of a keyframe, for every matched pair
// of every neighbour in one call (local_map_updater's create_new_landmarks runs it once per pair after robust::match_for_triangulation).
// Rules: DESIGN.md 3.12; the algebra is triangulate_math.inc, which a plain host compiler builds too.
//
// A problem is one (keyframe 1, keyframe 2) pair: a camera, a pose and a camera centre per side, and n matches. Everything is f64, every
// operation rounded on its own (the unit is built with -ffp-contract=off).
//
// k_triangulate: one launch, one lane per match over the whole batch, 64 lanes (one wavefront) per workgroup. The host stages the match
// inputs as structure-of-arrays (a wavefront's loads are whole lines) with a per-match problem index. A wavefront's matches may belong to
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
static_assert(sizeof(tri::Cam) == 56 && sizeof(tri::Problem) == 352 && sizeof(tri::Problem) % 8 == 0, "tri::Problem is laid out in the staged block by the host");

// The staged block of one call, sections in this order: problems tri::Problem [P], b1 f64 [3][T], b2 f64 [3][T] (planes: x of every match, then
// y, then z), then planes of f32 [T'] each: kp1 x y, kp2 x y, x_right 1 2, depth 1 2, sigma_sq 1 2, scale_factor 1 2 (12 planes), the problem
// index i32 [T'], offsets i32 [P' + 1]; then what the kernel writes and the host copies back: pos f64 [3][T], status u8 [T], method u8 [T].
// T' = T rounded up to even, P' + 1 = P + 1 rounded up to even: every f64 section is 8-byte aligned.
struct Layout {
    size_t problems, b1, b2, f32, pidx, offsets, pos, status, method, bytes;
    size_t Te;
};
constexpr int kFloatPlanes = 12;
__host__ __device__ inline Layout layout_of(int P, int T) {
    Layout l;
    l.Te = ((size_t)T + 1) & ~(size_t)1;
    l.problems = 0;
    l.b1 = l.problems + sizeof(tri::Problem) * (size_t)P;
    l.b2 = l.b1 + 24 * (size_t)T;
    l.f32 = l.b2 + 24 * (size_t)T;
    l.pidx = l.f32 + 4 * kFloatPlanes * l.Te;
    l.offsets = l.pidx + 4 * l.Te;
    l.pos = l.offsets + 4 * ((((size_t)P + 1) + 1) & ~(size_t)1);
    l.status = l.pos + 24 * (size_t)T;
    l.method = l.status + (size_t)T;
    l.bytes = l.method + (size_t)T;
    return l;
}

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

// an ovs_camera as rule T2, T5 and T7 read it; false for what the ABI refuses
bool triangulation_camera_ok(const ovs_camera& c, tri::Cam* rec) {
    if (!camera_ok(c, rec)) return false;
    if (c.model == 0 && (c.fx == 0.0 || c.fy == 0.0)) return false;
    rec->focal_x_baseline = c.focal_x_baseline;
    rec->true_baseline = c.true_baseline;
    return true;
}

}   // namespace

struct ovs_triangulate : ransac_handle {};

extern "C" {

ovs_status ovs_triangulate_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_triangulate** out) {
    return ransac_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes, 0, 0, out, 8);
}

ovs_status ovs_triangulate_destroy(ovs_triangulate* s) { return ransac_destroy(s); }

ovs_status ovs_triangulate_batch(ovs_triangulate* s, int32_t n_problems, const int32_t* offsets, const double* bearings_1, const double* bearings_2,
                                 const float* keypts_1, const float* keypts_2, const float* x_right_1, const float* x_right_2, const float* depths_1,
                                 const float* depths_2, const float* sigma_sq_1, const float* sigma_sq_2, const float* scale_factors_1,
                                 const float* scale_factors_2, const ovs_camera* cams_1, const ovs_camera* cams_2, const double* poses_cw_1,
                                 const double* poses_cw_2, double cos_rays_parallax_thr, float ratio_factor, double* out_pos_w, uint8_t* out_status,
                                 uint8_t* out_method, int32_t* out_num_accepted) {
    if (!std::isfinite(cos_rays_parallax_thr) || !std::isfinite(ratio_factor)) return OVS_ERR_INVALID;
    tri::Params prm;
    prm.cos_thr = cos_rays_parallax_thr;
    prm.ratio_factor = (double)ratio_factor;
    Layout used{};
    const auto stage = [&](uint8_t* h_block, const Layout& lay, int32_t T) {
        used = lay;
        tri::Problem* problems = reinterpret_cast<tri::Problem*>(h_block + lay.problems);
        for (int32_t p = 0; p < n_problems; ++p) {
            tri::Problem& q = problems[p];
            if (!triangulation_camera_ok(cams_1[p], &q.cam[0]) || !triangulation_camera_ok(cams_2[p], &q.cam[1])) return OVS_ERR_INVALID;
            std::memcpy(q.pose[0], poses_cw_1 + 12 * (size_t)p, 96);
            std::memcpy(q.pose[1], poses_cw_2 + 12 * (size_t)p, 96);
            tri::set_centres(q);
        }
        if (T > 0) {
            double* b1 = reinterpret_cast<double*>(h_block + lay.b1);
            double* b2 = reinterpret_cast<double*>(h_block + lay.b2);
            float* f = reinterpret_cast<float*>(h_block + lay.f32);
            int32_t* pidx = reinterpret_cast<int32_t*>(h_block + lay.pidx);
            const auto fplane = [&](int k) { return f + (size_t)k * lay.Te; };
            for (int32_t i = 0; i < T; ++i) {
                for (int x = 0; x < 3; ++x) {
                    b1[(size_t)x * T + i] = bearings_1[3 * (size_t)i + x];
                    b2[(size_t)x * T + i] = bearings_2[3 * (size_t)i + x];
                }
                for (int x = 0; x < 2; ++x) {
                    fplane(x)[i] = keypts_1[2 * (size_t)i + x];
                    fplane(2 + x)[i] = keypts_2[2 * (size_t)i + x];
                }
            }
            std::memcpy(fplane(4), x_right_1, 4 * (size_t)T);
            std::memcpy(fplane(5), x_right_2, 4 * (size_t)T);
            std::memcpy(fplane(6), depths_1, 4 * (size_t)T);
            std::memcpy(fplane(7), depths_2, 4 * (size_t)T);
            std::memcpy(fplane(8), sigma_sq_1, 4 * (size_t)T);
            std::memcpy(fplane(9), sigma_sq_2, 4 * (size_t)T);
            std::memcpy(fplane(10), scale_factors_1, 4 * (size_t)T);
            std::memcpy(fplane(11), scale_factors_2, 4 * (size_t)T);
            for (int32_t p = 0; p < n_problems; ++p)
                for (int32_t i = offsets[p]; i < offsets[p + 1]; ++i) pidx[i] = p;
        }
        return OVS_OK;
    };
    const auto launch = [&](hipStream_t st, int32_t T) {
        if (T == 0) return OVS_OK;
        hipLaunchKernelGGL(k_triangulate, dim3((T + kLanes - 1) / kLanes), dim3(kLanes), 0, st, s->d_block, n_problems, T, prm);
        OVS_HIP_TRY(hipGetLastError());
        OVS_HIP_TRY(hipMemcpyAsync(s->h_block + used.pos, s->d_block + used.pos, used.bytes - used.pos, hipMemcpyDeviceToHost, st));
        return OVS_OK;
    };
    const auto collect = [&](int32_t T) {
        const double* pos = reinterpret_cast<const double*>(s->h_block + used.pos);
        const uint8_t* status = s->h_block + used.status;
        for (int32_t i = 0; i < T; ++i)
            for (int x = 0; x < 3; ++x) out_pos_w[3 * (size_t)i + x] = pos[(size_t)x * T + i];
        if (T > 0) {
            std::memcpy(out_status, status, (size_t)T);
            std::memcpy(out_method, s->h_block + used.method, (size_t)T);
        }
        for (int32_t p = 0; p < n_problems; ++p) {
            int32_t accepted = 0;
            for (int32_t i = offsets[p]; i < offsets[p + 1]; ++i) accepted += status[i] == 0 ? 1 : 0;
            out_num_accepted[p] = accepted;
        }
    };
    return run_staged(s, n_problems, offsets, {cams_1, cams_2, poses_cw_1, poses_cw_2, out_num_accepted},
                      {bearings_1, bearings_2, keypts_1, keypts_2, x_right_1, x_right_2, depths_1, depths_2, sigma_sq_1, sigma_sq_2, scale_factors_1,
                       scale_factors_2, out_status, out_method},
                      out_pos_w, layout_of, stage, [] { return OVS_OK; }, launch, collect);
}

}   // extern "C"
