// landmark_update.hip -- data::landmark::update_normal_and_depth and data::landmark::compute_descriptor (expected:
// src/openvslam/data/landmark.{h,cc}) for many landmarks in one call: local BA's write-back, local mapping after create_new_landmarks and
// after the fuse step, and the end of map_database::from_json. Rules: DESIGN.md 3.14 (L1 to L9); the algebra is landmark_math.inc, which a
// plain host compiler builds too.
//
// On the batch scaffold of solve_internal.inc: a "problem" is a landmark, its "matches" are its observations. The staged block is
// structure-of-arrays. Observations name their keyframe by slot into a per-call table (camera centres, and in the _f form the device pointers
// of the resident keyframes' descriptors), staged once per call in a buffer of its own.
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
constexpr int kMaxObsPerLandmark = 1 << 22;   // the ordinal's share of the winner's key

__host__ __device__ inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// The staged block of one call, every section 16-byte aligned. Inputs: pos f64 [3][P] (planes), sf_ref f32 [P] (scale_factors[ref_level]),
// ref_slot i32 [P], offsets i32 [P + 1], obs_slot i32 [T], used i32 [T] (per landmark, from its offset on: the observations that take part in
// the descriptor, as indices into the call's observations), n_used i32 [P], list8 i32 [P], list64 i32 [P], obs_kp i32 [T] (_f form), desc
// u8 [T][32]. Then what the kernels write and the host copies back: normal f64 [3][P], range f32 [2][P], best i32 [P], out_desc u8 [P][32].
// `bytes` is what a call uploads: WITH_DESC = false ends it before the descriptors (a geometry-only call, or the _f form).
struct Layout {
    size_t pos, sf_ref, ref_slot, offsets, obs_slot, used, n_used, list8, list64, obs_kp, desc, normal, range, best, out_desc, total, bytes;
};
template <bool WITH_DESC>
__host__ __device__ inline Layout layout_of(int P, int T) {
    Layout l;
    const size_t p4 = al16(4 * (size_t)P), t4 = al16(4 * (size_t)T);
    l.pos = 0;
    l.sf_ref = l.pos + al16(24 * (size_t)P);
    l.ref_slot = l.sf_ref + p4;
    l.offsets = l.ref_slot + p4;
    l.obs_slot = l.offsets + al16(4 * ((size_t)P + 1));
    l.used = l.obs_slot + t4;
    l.n_used = l.used + t4;
    l.list8 = l.n_used + p4;
    l.list64 = l.list8 + p4;
    l.obs_kp = l.list64 + p4;
    l.desc = l.obs_kp + t4;
    l.normal = l.desc + 32 * (size_t)T;
    l.range = l.normal + al16(24 * (size_t)P);
    l.best = l.range + al16(8 * (size_t)P);
    l.out_desc = l.best + p4;
    l.total = l.out_desc + 32 * (size_t)P;
    l.bytes = WITH_DESC ? l.normal : l.desc;
    return l;
}

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

struct ovs_landmarks : ransac_handle {
    int max_keyframes = 0;
    // the per-call keyframe table: camera centres f64 [K][3], then the descriptors' device pointers [K] (_f form), and its page-locked twin
    uint8_t *d_table = nullptr, *h_table = nullptr;
};

namespace {

struct Inputs {
    int32_t what, n;
    const int32_t* offsets;
    const double* pos_w;
    const int32_t *ref_keyfrm, *ref_level, *obs_keyfrm;
    const uint8_t* obs_desc;
    bool resident;
    const ovs_frame_dev* const* keyfrms;
    const int32_t* obs_keypoint;
    const uint8_t* obs_use;
    const double* cam_centers;
    int32_t n_keyframes;
    const float* scale_factors;
    int32_t num_levels;
    double* out_mean_normal;
    float* out_min_max_dist;
    int32_t* out_best_obs;
    uint8_t *out_desc, *out_status;
};

ovs_status update_batch(ovs_landmarks* s, const Inputs& a) {
    if (!s || a.n < 0 || a.what < 1 || a.what > 3) return OVS_ERR_INVALID;
    if (a.n == 0) return OVS_OK;
    const bool geo = (a.what & 1) != 0, dsc = (a.what & 2) != 0;
    const int32_t P = a.n, K = a.n_keyframes;
    const bool slots = geo || (dsc && a.resident);   // whether obs_keyfrm and the keyframe table are read
    if (geo && (a.num_levels < 1 || a.num_levels > OVS_MAX_LEVELS)) return OVS_ERR_INVALID;
    if (slots && K < 0) return OVS_ERR_INVALID;
    const void* const unused = s;   // stands for an array this call does not read
    const auto when = [&](bool on, const void* q) { return on ? q : unused; };
    int32_t n8 = 0, n64 = 0;
    Layout used{};
    const size_t ptrs_at = 24 * (size_t)(K > 0 ? K : 0);
    const auto stage = [&](uint8_t* h_block, const Layout& lay, int32_t T) {
        used = lay;
        if (slots && K > s->max_keyframes) return OVS_ERR_CAPACITY;
        for (int32_t p = 0; p < P; ++p) {
            const int32_t count = a.offsets[p + 1] - a.offsets[p];
            if (count >= kMaxObsPerLandmark) return OVS_ERR_INVALID;
            if (geo && count > 0 && (a.ref_keyfrm[p] < 0 || a.ref_keyfrm[p] >= K || a.ref_level[p] < 0 || a.ref_level[p] >= a.num_levels)) return OVS_ERR_INVALID;
        }
        if (slots)
            for (int32_t t = 0; t < T; ++t)
                if (a.obs_keyfrm[t] < 0 || a.obs_keyfrm[t] >= K) return OVS_ERR_INVALID;
        if (dsc && a.resident) {
            const uint8_t** ptrs = reinterpret_cast<const uint8_t**>(s->h_table + ptrs_at);
            for (int32_t k = 0; k < K; ++k) {
                if (!a.keyfrms[k]) return OVS_ERR_INVALID;
                if (a.keyfrms[k]->device != s->device) return OVS_ERR_INVALID;
                ptrs[k] = a.keyfrms[k]->d_desc;
            }
            for (int32_t t = 0; t < T; ++t)
                if (a.obs_keypoint[t] < 0 || a.obs_keypoint[t] >= a.keyfrms[a.obs_keyfrm[t]]->n) return OVS_ERR_INVALID;
            if (T > 0) std::memcpy(h_block + lay.obs_kp, a.obs_keypoint, 4 * (size_t)T);
        }
        if (slots && T > 0) std::memcpy(h_block + lay.obs_slot, a.obs_keyfrm, 4 * (size_t)T);
        if (geo) {
            double* pos = reinterpret_cast<double*>(h_block + lay.pos);
            float* sf_ref = reinterpret_cast<float*>(h_block + lay.sf_ref);
            int32_t* ref_slot = reinterpret_cast<int32_t*>(h_block + lay.ref_slot);
            for (int32_t p = 0; p < P; ++p) {
                for (int x = 0; x < 3; ++x) pos[(size_t)x * P + p] = a.pos_w[3 * (size_t)p + x];
                const bool empty = a.offsets[p + 1] == a.offsets[p];
                sf_ref[p] = empty ? 0.0f : a.scale_factors[a.ref_level[p]];
                ref_slot[p] = empty ? 0 : a.ref_keyfrm[p];
            }
            if (K > 0) std::memcpy(s->h_table, a.cam_centers, 24 * (size_t)K);
        }
        if (dsc) {
            // the host plan: which observations take part (rule L6), and each landmark into the list of the kernel that serves its size
            int32_t* used_obs = reinterpret_cast<int32_t*>(h_block + lay.used);
            int32_t* n_used = reinterpret_cast<int32_t*>(h_block + lay.n_used);
            int32_t* list8 = reinterpret_cast<int32_t*>(h_block + lay.list8);
            int32_t* list64 = reinterpret_cast<int32_t*>(h_block + lay.list64);
            for (int32_t p = 0; p < P; ++p) {
                int32_t M = 0;
                for (int32_t t = a.offsets[p]; t < a.offsets[p + 1]; ++t)
                    if (!a.obs_use || a.obs_use[t]) used_obs[a.offsets[p] + M++] = t;
                n_used[p] = M;
                if (M > 8) list64[n64++] = p;
                else if (M > 0) list8[n8++] = p;
            }
            if (!a.resident && T > 0) std::memcpy(h_block + lay.desc, a.obs_desc, 32 * (size_t)T);
        }
        return OVS_OK;
    };
    const auto launch = [&](hipStream_t st, int32_t T) {
        if (T == 0) return OVS_OK;
        if (slots && K > 0) OVS_HIP_TRY(hipMemcpyAsync(s->d_table, s->h_table, ptrs_at + 8 * (size_t)K, hipMemcpyHostToDevice, st));
        if (geo) {
            hipLaunchKernelGGL(k_landmark_geometry, dim3((P + kGeoLanes - 1) / kGeoLanes), dim3(kGeoLanes), 0, st, s->d_block,
                               reinterpret_cast<const double*>(s->d_table), P, T, K, a.scale_factors[a.num_levels - 1]);
            OVS_HIP_TRY(hipGetLastError());
        }
        if (dsc && a.resident) {
            hipLaunchKernelGGL(k_landmark_gather, dim3((unsigned)((8 * (size_t)T + 255) / 256)), dim3(256), 0, st, s->d_block,
                               reinterpret_cast<const uint8_t* const*>(s->d_table + ptrs_at), P, T);
            OVS_HIP_TRY(hipGetLastError());
        }
        if (n8 > 0) {
            hipLaunchKernelGGL(k_landmark_descriptor<8>, dim3((n8 + 7) / 8), dim3(64), 0, st, s->d_block, P, T, n8);
            OVS_HIP_TRY(hipGetLastError());
        }
        if (n64 > 0) {
            hipLaunchKernelGGL(k_landmark_descriptor<64>, dim3(n64), dim3(64), 0, st, s->d_block, P, T, n64);
            OVS_HIP_TRY(hipGetLastError());
        }
        OVS_HIP_TRY(hipMemcpyAsync(s->h_block + used.normal, s->d_block + used.normal, used.total - used.normal, hipMemcpyDeviceToHost, st));
        return OVS_OK;
    };
    const auto collect = [&](int32_t) {
        const double* normal = reinterpret_cast<const double*>(s->h_block + used.normal);
        const float* range = reinterpret_cast<const float*>(s->h_block + used.range);
        const int32_t* best = reinterpret_cast<const int32_t*>(s->h_block + used.best);
        const int32_t* n_used = reinterpret_cast<const int32_t*>(s->h_block + used.n_used);
        for (int32_t p = 0; p < P; ++p) {
            const bool empty = a.offsets[p + 1] == a.offsets[p];
            a.out_status[p] = empty ? 1 : 0;
            if (geo && !empty) {
                for (int x = 0; x < 3; ++x) a.out_mean_normal[3 * (size_t)p + x] = normal[(size_t)x * P + p];
                a.out_min_max_dist[2 * (size_t)p] = range[p];
                a.out_min_max_dist[2 * (size_t)p + 1] = range[(size_t)P + p];
            }
            if (dsc && !empty) {
                if (n_used[p] == 0) {
                    a.out_best_obs[p] = -1;
                } else {
                    a.out_best_obs[p] = best[p] - a.offsets[p];
                    std::memcpy(a.out_desc + 32 * (size_t)p, s->h_block + used.out_desc + 32 * (size_t)p, 32);
                }
            }
        }
    };
    const std::initializer_list<const void*> required = {a.out_status,
                                                         when(geo, a.pos_w),
                                                         when(geo, a.ref_keyfrm),
                                                         when(geo, a.ref_level),
                                                         when(geo, a.cam_centers),
                                                         when(geo, a.scale_factors),
                                                         when(geo, a.out_mean_normal),
                                                         when(geo, a.out_min_max_dist),
                                                         when(dsc, a.out_best_obs),
                                                         when(dsc, a.out_desc),
                                                         when(dsc && a.resident, a.keyfrms)};
    const std::initializer_list<const void*> per_observation = {when(slots, a.obs_keyfrm), when(dsc && !a.resident, a.obs_desc),
                                                                when(dsc && a.resident, a.obs_keypoint)};
    if (dsc && !a.resident)
        return run_staged(s, P, a.offsets, required, per_observation, unused, layout_of<true>, stage, [] { return OVS_OK; }, launch, collect);
    return run_staged(s, P, a.offsets, required, per_observation, unused, layout_of<false>, stage, [] { return OVS_OK; }, launch, collect);
}

}   // namespace

extern "C" {

ovs_status ovs_landmarks_create(int32_t device, int32_t max_landmarks, int32_t max_total_observations, int32_t max_keyframes, ovs_landmarks** out) {
    if (!out) return OVS_ERR_INVALID;
    *out = nullptr;
    if (max_keyframes < 1) return OVS_ERR_INVALID;
    ovs_landmarks* s = nullptr;
    const ovs_status st = ransac_create(device, max_landmarks, max_total_observations, layout_of<true>(max_landmarks, max_total_observations).total, 0, 0, &s, 8);
    if (st != OVS_OK) return st;
    s->max_keyframes = max_keyframes;
    const size_t table_bytes = 32 * (size_t)max_keyframes;
    if (s->res.dev(&s->d_table, table_bytes) != hipSuccess || s->res.pinned(&s->h_table, table_bytes) != hipSuccess) {
        ransac_destroy(s);
        return OVS_ERR_HIP;
    }
    *out = s;
    return OVS_OK;
}

ovs_status ovs_landmarks_destroy(ovs_landmarks* s) { return ransac_destroy(s); }

ovs_status ovs_landmarks_update_batch(ovs_landmarks* s, int32_t what, int32_t n_landmarks, const int32_t* offsets, const double* pos_w,
                                      const int32_t* ref_keyfrm, const int32_t* ref_level, const int32_t* obs_keyfrm, const uint8_t* obs_desc,
                                      const uint8_t* obs_use, const double* cam_centers, int32_t n_keyframes, const float* scale_factors,
                                      int32_t num_levels, double* out_mean_normal, float* out_min_max_dist, int32_t* out_best_obs, uint8_t* out_desc,
                                      uint8_t* out_status) {
    return update_batch(s, Inputs{what, n_landmarks, offsets, pos_w, ref_keyfrm, ref_level, obs_keyfrm, obs_desc, false, nullptr, nullptr, obs_use,
                                  cam_centers, n_keyframes, scale_factors, num_levels, out_mean_normal, out_min_max_dist, out_best_obs, out_desc,
                                  out_status});
}

ovs_status ovs_landmarks_update_batch_f(ovs_landmarks* s, int32_t what, int32_t n_landmarks, const int32_t* offsets, const double* pos_w,
                                        const int32_t* ref_keyfrm, const int32_t* ref_level, const int32_t* obs_keyfrm,
                                        const ovs_frame_dev* const* keyfrms, const int32_t* obs_keypoint, const uint8_t* obs_use,
                                        const double* cam_centers, int32_t n_keyframes, const float* scale_factors, int32_t num_levels,
                                        double* out_mean_normal, float* out_min_max_dist, int32_t* out_best_obs, uint8_t* out_desc,
                                        uint8_t* out_status) {
    return update_batch(s, Inputs{what, n_landmarks, offsets, pos_w, ref_keyfrm, ref_level, obs_keyfrm, nullptr, true, keyfrms, obs_keypoint, obs_use,
                                  cam_centers, n_keyframes, scale_factors, num_levels, out_mean_normal, out_min_max_dist, out_best_obs, out_desc,
                                  out_status});
}

}   // extern "C"
