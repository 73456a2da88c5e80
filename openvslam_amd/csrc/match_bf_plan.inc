// match_bf_plan.inc -- everything the host side of the brute-force matcher (match_hamming.hip) decides with integers and one float: the constants
// the kernels share with it, near_threshold, the resolver's LDS layout and which form of k_bf_resolve a handle runs, the near stage's launch, the
// sizes of a handle's buffers and the argument checks of its entry points. Plain host C++, no HIP (the LDS layout alone is also device code, under
// hipcc): match_hamming.hip includes it, tests/match_bf_plan_host.cc builds it with the host compiler alone and tests/test_match_bf_plan.py holds it
// to a hand-written table. This is the one place these sizes, offsets and thresholds are computed. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/ovslam_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define OVS_BF_FN __host__ __device__ inline
#else
#define OVS_BF_FN inline
#endif

namespace ovs {

constexpr int kNearSplit = 4;         // waves per workgroup; each scans a quarter of the frame descriptors for the same 64 queries
constexpr int kNearSeg = 64;          // near-list capacity per (query, wave); beyond it: cooperative full scan, still exact
constexpr int kTopK = 8;              // sorted smallest keys kept per query for the resolver's fast path
constexpr int kNearQueries = 256;     // queries per workgroup of k_hamming_near (4 waves x 2 tiles of 32)
constexpr int kNearPopcQueries = 64;  // queries per workgroup of k_hamming_near_popc (the four waves share them)

constexpr size_t kBfLdsMax = 150 * 1024;      // dynamic LDS k_bf_resolve may ask for
constexpr size_t kBfLdsDefault = 64 * 1024;   // what a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize

// Largest distance that can still influence brute_force_match's accept/reject decision (see match_hamming.hip's header).
inline uint32_t near_threshold(float lowe_ratio) {
    uint32_t tau = 257;
    for (uint32_t s = 0; s <= 256; ++s) {
        const volatile float lhs = lowe_ratio * (float)s;   // one float multiply, as the device does (__fmul_rn)
        if (!(lhs < (float)OVS_HAMMING_DIST_THR_LOW)) { tau = s; break; }
    }
    // (a NaN ratio stops at s = 0: tau - 1 wraps to 2^32 - 1 and the clamp below answers 255, as for a ratio too small to ever stop rejecting)
    uint32_t thr = std::max<uint32_t>(OVS_HAMMING_DIST_THR_LOW, tau - 1);
    // a distance of 256 can never become best (strict '<' against the initial MAX_HAMMING_DIST) and as `second` equals "none"
    return std::min<uint32_t>(thr, OVS_MAX_HAMMING_DIST - 1);
}

// ---- resolver (k_bf_resolve) -------------------------------------------------------------------------------------------------
// Byte offsets of the sections of k_bf_resolve's dynamic LDS: mark u32[max_n1] | claimed u8[max_n1] | (on 16 bytes; the staged form only:)
// tops u32[max_n2][kTopK] | cnts u32[max_n2]. total: the end of cnts.
struct BfResolveLds {
    size_t mark, claimed, tops, cnts, total;
};
OVS_BF_FN BfResolveLds bf_resolve_lds(int max_n1, int max_n2) {
    BfResolveLds l;
    l.mark = 0;
    l.claimed = (size_t)max_n1 * 4;
    l.tops = ((size_t)max_n1 * 5 + 15) & ~(size_t)15;
    l.cnts = l.tops + (size_t)max_n2 * kTopK * 4;
    l.total = l.cnts + (size_t)max_n2 * 4;
    return l;
}

// Which k_bf_resolve a handle of these capacities runs: <true, 4> (four waves; every query's counts and top-8 staged in LDS) while the whole
// layout fits, else <false, 1> (one wave, mark and claimed only), refused when even that does not fit.
struct BfResolvePlan {
    bool refused;       // OVS_ERR_CAPACITY
    bool staged;
    int waves, block;   // 4 / 256 or 1 / 64
    size_t lds_bytes;
    bool raise_attr;    // beyond kBfLdsDefault: the attribute has to cover lds_bytes
};
inline BfResolvePlan bf_resolve_plan(int max_n1, int max_n2) {
    BfResolvePlan p{};
    const size_t one_wave = (size_t)max_n1 * 4 + (((size_t)max_n1 + 15) & ~(size_t)15);   // (16 bytes per started 16 flags: never below claimed's end)
    p.refused = one_wave > kBfLdsMax;
    if (p.refused) return p;
    const size_t staged = bf_resolve_lds(max_n1, max_n2).total;
    p.staged = staged <= kBfLdsMax;
    p.waves = p.staged ? 4 : 1;
    p.block = 64 * p.waves;
    p.lds_bytes = p.staged ? staged : one_wave;
    p.raise_attr = p.lds_bytes > kBfLdsDefault;
    return p;
}

// ---- near stage (k_hamming_near / k_hamming_near_popc) -------------------------------------------------------------------------
// One workgroup per (problem, chunk of queries); the grid is rounded up to the 8 XCDs for the kernels' XCD-major work order
struct BfNearLaunch {
    int chunks, total_wg, grid;
};
inline BfNearLaunch bf_near_launch(int max_n2, int batch, int near_path) {
    const int per_wg = near_path == OVS_NEAR_PATH_POPCOUNT ? kNearPopcQueries : kNearQueries;
    BfNearLaunch l;
    l.chunks = (max_n2 + per_wg - 1) / per_wg;
    l.total_wg = l.chunks * batch;
    l.grid = ((l.total_wg + 7) / 8) * 8;
    return l;
}

// ---- a handle's buffers ----------------------------------------------------------------------------------------------------------
struct BfCaps {
    int max_n1, max_n2, max_batch;
};
struct BfBuffers {
    size_t near_cnt, near_list, near_top;                                             // work buffers: per (problem, query)
    size_t desc_1, desc_2, valid, valid_1, n, pairs, count, best_idx, best, second;   // host-entry staging (one problem)
};
inline BfBuffers bf_buffer_bytes(const BfCaps& c) {
    const size_t B = (size_t)c.max_batch, n1 = (size_t)c.max_n1, n2 = (size_t)c.max_n2;
    BfBuffers b;
    b.near_cnt = sizeof(uint32_t) * B * n2 * kNearSplit;
    b.near_list = sizeof(uint32_t) * B * n2 * kNearSplit * kNearSeg;
    b.near_top = sizeof(uint32_t) * B * n2 * kTopK;
    b.desc_1 = n1 * 32;
    b.desc_2 = n2 * 32;
    b.valid = std::max(n1, n2);   // the keyframe side's mask in brute_force_match, the target side's (idx_1 buffers) in hamming_best2
    b.valid_1 = n1;
    b.n = sizeof(int32_t) * 2;
    b.pairs = sizeof(int32_t) * 2 * n2;
    b.count = sizeof(int32_t);
    b.best_idx = sizeof(int32_t) * n2;
    b.best = sizeof(uint16_t) * n2;
    b.second = sizeof(uint16_t) * n2;
    return b;
}

// ---- argument checks -------------------------------------------------------------------------------------------------------------
// Each returns what its entry point returns before it touches the device. OVS_OK with *run == false: the call is complete (nothing to match).
inline ovs_status bf_check_create(bool has_out, int32_t max_n1, int32_t max_n2, int32_t max_batch) {
    if (!has_out || max_n1 < 1 || max_n2 < 1 || max_batch < 1 || max_n1 > 65535 || max_n2 > 65535) return OVS_ERR_INVALID;
    return bf_resolve_plan(max_n1, max_n2).refused ? OVS_ERR_CAPACITY : OVS_OK;
}

// caps: nullptr without a handle. *n_out is zeroed once the handle, n_out and the three counts are accepted, as the entry point documents.
inline ovs_status bf_check_match(const BfCaps* caps, bool has_desc_1, int32_t n1, bool has_desc_2, int32_t n2, bool has_pairs, int32_t cap, int32_t* n_out,
                                 bool* run) {
    *run = false;
    if (!caps || !n_out || n1 < 0 || n2 < 0 || cap < 0) return OVS_ERR_INVALID;
    *n_out = 0;
    if (n1 == 0 || n2 == 0) return OVS_OK;
    if (!has_desc_1 || !has_desc_2 || (cap > 0 && !has_pairs)) return OVS_ERR_INVALID;
    if (n1 > caps->max_n1 || n2 > caps->max_n2) return OVS_ERR_CAPACITY;
    *run = true;
    return OVS_OK;
}

// all_set: the handle and the six required device pointers
inline ovs_status bf_check_batch_dev(const BfCaps* caps, bool all_set, uintptr_t desc_1, size_t stride_1, uintptr_t desc_2, size_t stride_2, int32_t batch,
                                     int32_t cap) {
    if (!caps || !all_set || batch < 1 || cap < 1) return OVS_ERR_INVALID;
    if (batch > caps->max_batch || stride_1 > (size_t)caps->max_n1 * 32 || stride_2 > (size_t)caps->max_n2 * 32) return OVS_ERR_CAPACITY;
    if ((desc_1 & 3) || (desc_2 & 3) || (stride_1 & 31) || (stride_2 & 31)) return OVS_ERR_ALIGN;
    return OVS_OK;
}

// queries ride in the idx_2 buffers, targets in the idx_1 buffers. has_out: best_idx, best and second
inline ovs_status bf_check_best2(const BfCaps* caps, bool has_q, int32_t nq, bool has_t, int32_t nt, bool has_out, bool* run) {
    *run = false;
    if (!caps || nq < 0 || nt < 0) return OVS_ERR_INVALID;
    if (nq == 0) return OVS_OK;
    if (!has_q || (nt > 0 && !has_t) || !has_out) return OVS_ERR_INVALID;
    if (nq > caps->max_n2 || nt > caps->max_n1) return OVS_ERR_CAPACITY;
    *run = true;
    return OVS_OK;
}

}   // namespace ovs
