// landmark_math.inc -- data::landmark::update_normal_and_depth and data::landmark::compute_descriptor (expected: src/openvslam/data/landmark.cc)
// as DESIGN.md 3.14 states them, rules L1 to L9, for the device (landmark_update.hip) and for a plain host compiler alike:
// tests/test_landmark_ref.py builds a stand-alone program from this file with g++ -ffp-contract=off and holds its bits to the sequential Python
// reference. The geometry is f64 (the range's last two steps f32), every operation rounded on its own. The pieces are written so that the
// device's lane policy (a lane per landmark for the geometry, a lane per row for the descriptor) calls the same expressions as the host's
// loops. No local array is indexed by a run-time value.
// (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define LMK_FN __host__ __device__ __forceinline__
#else
#define LMK_FN inline
#endif

namespace lmk {

// rule L2's norm form, also rule L4's
LMK_FN double norm3(double d0, double d1, double d2) { return sqrt((d0 * d0 + d1 * d1) + d2 * d2); }

// rule L2: one observation's step of the sequential sum. Three true divisions; a zero-length ray gives 0 / 0 (rule L5).
LMK_FN void add_ray(double px, double py, double pz, double cx, double cy, double cz, double& sx, double& sy, double& sz) {
    const double d0 = px - cx, d1 = py - cy, d2 = pz - cz;
    const double n = norm3(d0, d1, d2);
    sx = sx + d0 / n;
    sy = sy + d1 / n;
    sz = sz + d2 / n;
}

// rule L3
LMK_FN double mean_of(double sum, int count) { return sum / (double)count; }

// rule L4: the raw members max_valid_dist_ and min_valid_dist_
LMK_FN void valid_range(double px, double py, double pz, double cx, double cy, double cz, float sf_ref_level, float sf_last_level, float& min_valid,
                        float& max_valid) {
    const double dist = norm3(px - cx, py - cy, pz - cz);
    max_valid = (float)(dist * (double)sf_ref_level);
    min_valid = max_valid / sf_last_level;
}

LMK_FN int popcount32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// rule L7: a descriptor is eight 32-bit words
struct Desc {
    uint32_t w[8];
};
LMK_FN int hamming256(const Desc& a, const Desc& b) {
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) d += popcount32(a.w[k] ^ b.w[k]);
    return d;
}

// rule L8: the rank of the median in a row of M distances, floor(0.5 * (M - 1))
LMK_FN int median_rank(int M) { return (M - 1) >> 1; }

// rule L8 without a sort: the element of rank k of a row of values in [0, 256] is the smallest v with count(value <= v) > k. Nine counting
// passes halve [0, 256] down to it; count_le(v) is the caller's pass over the row.
template <class CountLe>
LMK_FN int kth_by_bisection(int k, CountLe count_le) {
    int lo = 0, hi = 256;
#pragma unroll 1
    for (int pass = 0; pass < 9; ++pass) {   // 257 values: 2^9 >= 257; a pass after lo == hi changes nothing
        const int mid = (lo + hi) >> 1;
        const bool enough = count_le(mid) > k;
        hi = enough ? mid : hi;
        lo = enough ? lo : mid + 1;
    }
    return lo;
}

// rule L9: strict-less, first-wins is the minimum of this key over the rows; a row that does not get below 256 never replaces ordinal 0
constexpr uint32_t kNoWinner = 0xFFFFFFFFu;
LMK_FN uint32_t winner_key(int median, int ordinal) { return median < 256 ? ((uint32_t)median << 22) | (uint32_t)ordinal : kNoWinner; }
LMK_FN int winner_ordinal(uint32_t key) { return key == kNoWinner ? 0 : (int)(key & 0x3FFFFFu); }

}   // namespace lmk
