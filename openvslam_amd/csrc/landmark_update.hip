// landmark_update.hip -- data::landmark::update_normal_and_depth and data::landmark::compute_descriptor (expected:
// src/openvslam/data/landmark.{h,cc}) for many landmarks in one call: local BA's write-back, local mapping after create_new_landmarks and
// after the fuse step, and the end of map_database::from_json. Rules: DESIGN.md 3.14 (L1 to L9); the algebra is landmark_math.inc, which a
// plain host compiler builds too.
//
// On the batch scaffold of solve_internal.inc: a "problem" is a landmark, its "matches" are its observations. What a call decides on the
// host (argument errors, capacity, the block's layout, staging, the two size lists, the read-back) is splan::landmarks of solve_plan.inc;
// this unit keeps the kernels and their launches. The staged block is structure-of-arrays. Observations name their keyframe by slot into a
// per-call table (camera centres, and in the _f form the device pointers of the resident keyframes' descriptors), staged once per call in
// a buffer of its own.
//
// k_landmark_geometry: a lane per landmark, 256 lanes per workgroup; the lane walks its observations in list order, which is what makes
//   the sum's bits the sequential reference's. The first kLdsCentres camera centres are copied into LDS once per workgroup, the others are
//   read through L2. No atomics, no scratch.
// k_landmark_descriptor<G>: G lanes per landmark, a wavefront per workgroup. Row i of the distance matrix belongs to lane i mod G; the
//   lane finds the median of its row by bisecting [0, 256] in nine counting passes (no sort), and the group's winner is the minimum of the
//   key {median | ordinal} over its lanes. G = 8 (eight landmarks per wavefront) serves landmarks of at most 8 descriptors and keeps a
//   row's distances in eight registers; G = 64 serves the others, rows strided over the lanes, the distances recomputed in every pass
//   from the group's descriptors in LDS (the first kLdsDescs64) or from memory (the others). The host sorts a call's landmarks into the
//   two lists once.
// k_landmark_gather (_f form): the descriptor section of the block filled on the device from the resident keyframes.
// The kernels are independent of each other (the gather precedes the descriptor kernels); a call enqueues what it needs and one copy down.
#include <cmath>
#include <cstring>

#include "frame_dev_internal.inc"
#include "landmark_math.inc"
#include "ovs_common.h"
#include "solve_internal.inc"

namespace {

constexpr int kGeoLanes = 256;
constexpr int kLdsCentres = 256;    // camera centres held in LDS (6 KiB); slots from here on are read from memory
constexpr int kLdsDescs64 = 128;    // descriptors of a G = 64 landmark held in LDS (4 KiB); the others are read from memory

// the staged block of one call (structure-of-arrays, every section 16-byte aligned; the kernels' outputs are its last sections): solve_plan.inc
using splan::landmarks::Layout;
using splan::landmarks::layout_of;

__global__ __launch_bounds__(kGeoLanes) void k_landmark_geometry(uint8_t* __restrict__ block, const double* __restrict__ centres, int P, int T, int K,
                                                                 float sf_last_level) {
    __shared__ double table[3 * kLdsCentres];
    const Layout lay = layout_of<false>(P, T);
    const int in_lds = K < kLdsCentres ? K : kLdsCentres;
    for (int i = threadIdx.x; i < 3 * in_lds; i += kGeoLanes) table[i] = centres[i];
    __syncthreads();
    const int p = blockIdx.x * kGeoLanes + threadIdx.x;
    if (p >= P) return;
    const Span span = problem_span(block, lay.offsets, p);
    if (span.n == 0) return;   // rule L1: the host leaves this landmark's outputs alone
    const auto centre = [&](int slot, double& cx, double& cy, double& cz) {
        const double* src = slot < kLdsCentres ? table + 3 * slot : centres + 3 * (size_t)slot;
        cx = src[0], cy = src[1], cz = src[2];
    };
    const double* pos = reinterpret_cast<const double*>(block + lay.pos);
    const double px = pos[p], py = pos[(size_t)P + p], pz = pos[2 * (size_t)P + p];
    const int32_t* obs_slot = reinterpret_cast<const int32_t*>(block + lay.obs_slot) + span.off;
    double sx = 0.0, sy = 0.0, sz = 0.0, cx, cy, cz;
#pragma unroll 1
    for (int k = 0; k < span.n; ++k) {
        centre(obs_slot[k], cx, cy, cz);
        lmk::add_ray(px, py, pz, cx, cy, cz, sx, sy, sz);
    }
    double* normal = reinterpret_cast<double*>(block + lay.normal);
    normal[p] = lmk::mean_of(sx, span.n);
    normal[(size_t)P + p] = lmk::mean_of(sy, span.n);
    normal[2 * (size_t)P + p] = lmk::mean_of(sz, span.n);
    centre(reinterpret_cast<const int32_t*>(block + lay.ref_slot)[p], cx, cy, cz);
    float min_valid, max_valid;
    lmk::valid_range(px, py, pz, cx, cy, cz, reinterpret_cast<const float*>(block + lay.sf_ref)[p], sf_last_level, min_valid, max_valid);
    float* range = reinterpret_cast<float*>(block + lay.range);
    range[p] = min_valid;
    range[(size_t)P + p] = max_valid;
}

// one thread per 32-bit word of an observation's descriptor: keyframe slot -> the resident keyframe's descriptors -> the keypoint's row
__global__ __launch_bounds__(256) void k_landmark_gather(uint8_t* __restrict__ block, const uint8_t* const* __restrict__ desc_of_slot, int P, int T) {
    const Layout lay = layout_of<false>(P, T);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t t = i >> 3, w = i & 7;
    if (t >= (size_t)T) return;
    const int slot = reinterpret_cast<const int32_t*>(block + lay.obs_slot)[t];
    const int kp = reinterpret_cast<const int32_t*>(block + lay.obs_kp)[t];
    reinterpret_cast<uint32_t*>(block + lay.desc)[i] = reinterpret_cast<const uint32_t*>(desc_of_slot[slot])[8 * (size_t)kp + w];
}

template <int G>
__global__ __launch_bounds__(64) void k_landmark_descriptor(uint8_t* __restrict__ block, int P, int T, int n_list) {
    constexpr int kGroups = 64 / G;
    constexpr int kLdsDescs = G == 8 ? 8 : kLdsDescs64;
    constexpr int kStride = 8 * kLdsDescs + (G == 8 ? 8 : 0);   // in words; the pad puts the eight groups of G = 8 on different banks
    __shared__ uint32_t lds[kGroups * kStride];
    const Layout lay = layout_of<false>(P, T);
    const int group = threadIdx.x / G, l = threadIdx.x % G;
    const int entry = blockIdx.x * kGroups + group;
    const bool live = entry < n_list;
    const int p = live ? reinterpret_cast<const int32_t*>(block + (G == 8 ? lay.list8 : lay.list64))[entry] : 0;
    const int off = reinterpret_cast<const int32_t*>(block + lay.offsets)[p];
    const int M = live ? reinterpret_cast<const int32_t*>(block + lay.n_used)[p] : 0;
    const int32_t* used = reinterpret_cast<const int32_t*>(block + lay.used) + off;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(block + lay.desc);
    uint32_t* mine_lds = lds + group * kStride;
    const int staged = M < kLdsDescs ? M : kLdsDescs;
    for (int i = l; i < 8 * staged; i += G) mine_lds[i] = words[8 * (size_t)used[i >> 3] + (i & 7)];
    __syncthreads();
    const auto load = [&](int j) {
        const uint32_t* src = j < kLdsDescs ? mine_lds + 8 * j : words + 8 * (size_t)used[j];
        lmk::Desc d;
#pragma unroll
        for (int k = 0; k < 8; ++k) d.w[k] = src[k];
        return d;
    };
    const int rank = lmk::median_rank(M);
    uint32_t best = lmk::kNoWinner;
#pragma unroll 1
    for (int i = l; i < M; i += G) {   // G = 8: at most one row per lane
        const lmk::Desc row = load(i);
        int median;
        if constexpr (G == 8) {
            int dist[8];   // compile-time indices only: registers
#pragma unroll
            for (int j = 0; j < 8; ++j) dist[j] = j < M ? lmk::hamming256(row, load(j)) : 257;
            median = lmk::kth_by_bisection(rank, [&](int v) {
                int c = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) c += dist[j] <= v ? 1 : 0;
                return c;
            });
        } else {
            median = lmk::kth_by_bisection(rank, [&](int v) {
                int c = 0;
#pragma unroll 1
                for (int j = 0; j < M; ++j) c += lmk::hamming256(row, load(j)) <= v ? 1 : 0;
                return c;
            });
        }
        const uint32_t key = lmk::winner_key(median, i);
        best = key < best ? key : best;
    }
#pragma unroll
    for (int m = G / 2; m > 0; m >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)best, m, G);
        best = other < best ? other : best;
    }
    if (M > 0 && l < 8) {
        const int t = used[lmk::winner_ordinal(best)];   // an index into the call's observations; off + its place in the landmark's list
        if (l == 0) reinterpret_cast<int32_t*>(block + lay.best)[p] = t;
        reinterpret_cast<uint32_t*>(block + lay.out_desc)[8 * (size_t)p + l] = words[8 * (size_t)t + l];
    }
}

}   // namespace

struct ovs_landmarks : batch_handle {   // the results come back through the staged block: no records, no result block, no flags
    int max_keyframes = 0;
    // the per-call keyframe table: camera centres f64 [K][3], then the descriptors' device pointers [K] (_f form), and its page-locked twin
    uint8_t *d_table = nullptr, *h_table = nullptr;
    const double* d_centres() const { return reinterpret_cast<const double*>(d_table); }
    const uint8_t* const* d_desc_of_slot(int32_t K) const { return reinterpret_cast<const uint8_t* const*>(d_table + splan::landmarks::table_ptrs_at(K)); }
};

namespace {

using splan::landmarks::Call;

ovs_status update_batch(ovs_landmarks* s, const Call& call) {
    const splan::Checked checked =
        splan::landmarks::check(call, [s] { return splan::Caps{s->max_problems, s->max_total_matches, s->max_keyframes, s->device}; });
    const int32_t P = call.n_landmarks, K = call.n_keyframes;
    const Layout lay = splan::landmarks::layout_for(call, checked.T);
    splan::landmarks::Lists lists{0, 0};
    const auto launch = [&](hipStream_t st, int32_t T) {
        if (T == 0) return OVS_OK;
        if (call.slots() && K > 0) OVS_HIP_TRY(hipMemcpyAsync(s->d_table, s->h_table, splan::landmarks::table_bytes(K), hipMemcpyHostToDevice, st));
        if (call.geo()) {
            hipLaunchKernelGGL(k_landmark_geometry, dim3((P + kGeoLanes - 1) / kGeoLanes), dim3(kGeoLanes), 0, st, s->d_block,
                               s->d_centres(), P, T, K, call.scale_factors[call.num_levels - 1]);
            OVS_HIP_TRY(hipGetLastError());
        }
        if (call.gathers()) {
            hipLaunchKernelGGL(k_landmark_gather, dim3((unsigned)((8 * (size_t)T + 255) / 256)), dim3(256), 0, st, s->d_block, s->d_desc_of_slot(K), P, T);
            OVS_HIP_TRY(hipGetLastError());
        }
        if (lists.n8 > 0) {
            hipLaunchKernelGGL(k_landmark_descriptor<8>, dim3((lists.n8 + 7) / 8), dim3(64), 0, st, s->d_block, P, T, lists.n8);
            OVS_HIP_TRY(hipGetLastError());
        }
        if (lists.n64 > 0) {
            hipLaunchKernelGGL(k_landmark_descriptor<64>, dim3(lists.n64), dim3(64), 0, st, s->d_block, P, T, lists.n64);
            OVS_HIP_TRY(hipGetLastError());
        }
        OVS_HIP_TRY(hipMemcpyAsync(s->h_block + lay.normal, s->d_block + lay.normal, lay.total - lay.normal, hipMemcpyDeviceToHost, st));
        return OVS_OK;
    };
    return run_staged(
        s, checked, lay.bytes, [&] { lists = splan::landmarks::stage(call, lay, s->h_block, s->h_table); }, nothing_to_reserve, launch,
        [&](int32_t) { splan::landmarks::collect(call, lay, s->h_block); });
}

// entry k of the _f form's keyframes as the plan reads it
splan::landmarks::KeyframeView keyframe_view(const void* keyfrms, int32_t k) {
    const ovs_frame_dev* f = static_cast<const ovs_frame_dev* const*>(keyfrms)[k];
    return f ? splan::landmarks::KeyframeView{f->device, f->n, f->d_desc} : splan::landmarks::KeyframeView{-1, 0, nullptr};
}

}   // namespace

extern "C" {

ovs_status ovs_landmarks_create(int32_t device, int32_t max_landmarks, int32_t max_total_observations, int32_t max_keyframes, ovs_landmarks** out) {
    if (!out) return OVS_ERR_INVALID;
    *out = nullptr;
    if (max_keyframes < 1) return OVS_ERR_INVALID;
    return batch_create(device, max_landmarks, max_total_observations, layout_of<true>(max_landmarks, max_total_observations).total, 0, 0, 0, out,
                        [&](ovs_landmarks* s) {
                            s->max_keyframes = max_keyframes;
                            const size_t table_bytes = splan::landmarks::table_bytes(max_keyframes);
                            if (s->res.dev(&s->d_table, table_bytes) != hipSuccess || s->res.pinned(&s->h_table, table_bytes) != hipSuccess) return OVS_ERR_HIP;
                            return OVS_OK;
                        });
}

ovs_status ovs_landmarks_destroy(ovs_landmarks* s) { return batch_destroy(s); }

ovs_status ovs_landmarks_update_batch(ovs_landmarks* s, int32_t what, int32_t n_landmarks, const int32_t* offsets, const double* pos_w,
                                      const int32_t* ref_keyfrm, const int32_t* ref_level, const int32_t* obs_keyfrm, const uint8_t* obs_desc,
                                      const uint8_t* obs_use, const double* cam_centers, int32_t n_keyframes, const float* scale_factors,
                                      int32_t num_levels, double* out_mean_normal, float* out_min_max_dist, int32_t* out_best_obs, uint8_t* out_desc,
                                      uint8_t* out_status) {
    return update_batch(s, Call{s != nullptr, what, n_landmarks, offsets, pos_w, ref_keyfrm, ref_level, obs_keyfrm, obs_desc, false, nullptr, nullptr, nullptr,
                                obs_use, cam_centers, n_keyframes, scale_factors, num_levels, out_mean_normal, out_min_max_dist, out_best_obs, out_desc,
                                out_status});
}

ovs_status ovs_landmarks_update_batch_f(ovs_landmarks* s, int32_t what, int32_t n_landmarks, const int32_t* offsets, const double* pos_w,
                                        const int32_t* ref_keyfrm, const int32_t* ref_level, const int32_t* obs_keyfrm,
                                        const ovs_frame_dev* const* keyfrms, const int32_t* obs_keypoint, const uint8_t* obs_use,
                                        const double* cam_centers, int32_t n_keyframes, const float* scale_factors, int32_t num_levels,
                                        double* out_mean_normal, float* out_min_max_dist, int32_t* out_best_obs, uint8_t* out_desc,
                                        uint8_t* out_status) {
    return update_batch(s, Call{s != nullptr, what, n_landmarks, offsets, pos_w, ref_keyfrm, ref_level, obs_keyfrm, nullptr, true, keyfrms, keyframe_view,
                                obs_keypoint, obs_use, cam_centers, n_keyframes, scale_factors, num_levels, out_mean_normal, out_min_max_dist, out_best_obs,
                                out_desc, out_status});
}

}   // extern "C"
