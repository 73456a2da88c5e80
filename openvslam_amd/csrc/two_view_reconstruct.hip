// two_view_reconstruct.hip -- initialize::perspective's reconstruct_with_H / reconstruct_with_F (expected: src/openvslam/initialize/
// {base,perspective}.{h,cc}): the decomposition of the chosen model into 8 or 4 pose hypotheses, check_pose for each of them over every inlier
// match, and find_most_plausible_pose, for a batch of (reference frame, current frame) problems. It follows ovs_twoview_solve_batch in the
// monocular initialiser. Rules: DESIGN.md 3.15; the algebra is reconstruct_math.inc, which a plain host compiler builds too.
//
// A problem is one pair of frames with its chosen model (H_21 or F_21), its camera and n matches: the model's inlier flag, the two undistorted
// keypoints and the two bearings. Everything is f64 unless a rule says float, every operation rounded on its own (the unit is built with
// -ffp-contract=off).
//
// k_reconstruct_hypotheses: grid (8 hypotheses, problems), one wavefront per workgroup. Every lane derives the hypothesis for itself (a
// 3 x 3 decomposition in registers: short, the same in every lane); a hypothesis that does not exist (4 to 7 of an F, all of an H whose
// singular values are too close) leaves its record and exits. The lanes then walk the matches in rounds of 64: the gate chain of one match
// per lane, the count by ballot + popcount, the cosine's integer key into the handle's key buffer (the lane that wrote a key is the one that
// reads it again). The order statistic is a radix select over those keys, four bits at a time from the top: 8 counting passes of 16
// ballots a round, no sort and no rank count. One (count, parallax) record per hypothesis, nothing per match leaves the kernel.
// k_reconstruct_finish: one workgroup (one wavefront) per problem: find_most_plausible_pose over the eight records, then the winner's
// points and flags again with the same device function (the same bits, and no per-hypothesis point storage), written straight to
// page-locked memory. No atomics, no waiting between workgroups, no scratch.
#include <cmath>
#include <cstring>

#include "ovs_common.h"
#include "reconstruct_math.inc"
#include "solve_internal.inc"

namespace {

constexpr int kLanes = 64;
constexpr int kKeyDoublesPerMatch = rec::kMaxHypotheses / 2;   // a match's eight u32 keys, in the handle's records of doubles
constexpr int kInitialKeyMatches = 256;                        // the key buffer a handle is created with; it grows with a call's matches

// the staged block of one call: solve_plan.inc
using splan::reconstruct::Layout;
using splan::reconstruct::layout_of;

// per (problem, hypothesis) between the two kernels; count -1: there is no such hypothesis
struct HypRec {
    int32_t count;
    float parallax;
};

// per problem in the result block
struct ReconRec {
    double rot[9], trans[3];
    int32_t counts[rec::kMaxHypotheses];
    float parallax[rec::kMaxHypotheses];
    int32_t success, best;
};
static_assert(sizeof(ReconRec) == 168, "ReconRec is read by the host");

// a problem's matches in the staged block
struct Matches {
    const double *kp1, *kp2, *b1, *b2;
    const uint8_t* inlier;
};
__device__ __forceinline__ Matches matches_of(const uint8_t* __restrict__ block, const Layout& lay, int off) {
    Matches m;
    m.kp1 = reinterpret_cast<const double*>(block + lay.kp1) + 2 * (size_t)off;
    m.kp2 = reinterpret_cast<const double*>(block + lay.kp2) + 2 * (size_t)off;
    m.b1 = reinterpret_cast<const double*>(block + lay.b1) + 3 * (size_t)off;
    m.b2 = reinterpret_cast<const double*>(block + lay.b2) + 3 * (size_t)off;
    m.inlier = block + lay.inlier + off;
    return m;
}
__device__ __forceinline__ rec::Match load_match(const Matches& m, size_t j) {
    rec::Match x;
    x.kp1[0] = m.kp1[2 * j], x.kp1[1] = m.kp1[2 * j + 1];
    x.kp2[0] = m.kp2[2 * j], x.kp2[1] = m.kp2[2 * j + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) x.b1[c] = m.b1[3 * j + c], x.b2[c] = m.b2[3 * j + c];
    return x;
}

__global__ __launch_bounds__(kLanes) void k_reconstruct_hypotheses(const uint8_t* __restrict__ block, int P, int T, float thr_sq, uint32_t* keys,
                                                                   HypRec* __restrict__ hyp_recs) {
    const int h = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const Layout lay = layout_of(P, T);
    const rec::Problem q = reinterpret_cast<const rec::Problem*>(block + lay.problems)[p];
    HypRec* const out = hyp_recs + (size_t)p * rec::kMaxHypotheses + h;
    rec::Hyp hyp;
    if (!rec::hypothesis(q, h, hyp)) {
        if (lane == 0) *out = HypRec{-1, 0.0f};
        return;
    }
    const auto [off, n] = problem_span(block, lay.offsets, p);
    const Matches m = matches_of(block, lay, off);
    uint32_t* const my_keys = keys + (size_t)h * (size_t)T + (size_t)off;   // [8][T] of the call: this hypothesis's row, this problem's span
    int count = 0;
    for (int base = 0; base < n; base += kLanes) {
        const int i = base + lane;
        const bool in = i < n;
        const size_t j = in ? (size_t)i : 0;
        const rec::Point pt = rec::check_match(q, hyp, load_match(m, j), thr_sq);
        const bool ok = in && m.inlier[j] != 0 && pt.ok;
        if (in) my_keys[i] = ok ? rec::key_of(pt.cos) : rec::kKeyNone;
        count += __popcll(__ballot(ok));
    }
    float parallax = 0.0f;
    if (count > 0) {   // R10: the key of rank min(50, count - 1), four bits at a time from the top; kKeyNone is above every key a match left
        int rank = rec::parallax_rank(count);
        uint32_t prefix = 0;
#pragma unroll 1
        for (int shift = 28; shift >= 0; shift -= 4) {
            int digits[16];   // how many keys agree with the prefix above the digit and hold 0 .. 15 there: the same in every lane
#pragma unroll
            for (int d = 0; d < 16; ++d) digits[d] = 0;
            const uint32_t above = shift == 28 ? 0u : prefix >> (shift + 4);
            for (int base = 0; base < n; base += kLanes) {
                const int i = base + lane;
                const uint32_t key = my_keys[i < n ? i : 0];
                const bool agrees = i < n && (shift == 28 ? 0u : key >> (shift + 4)) == above;
                const uint32_t digit = (key >> shift) & 15u;
#pragma unroll
                for (int d = 0; d < 16; ++d) digits[d] += __popcll(__ballot(agrees && digit == (uint32_t)d));
            }
            bool found = false;
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                const bool here = !found && rank < digits[d];
                prefix = here ? prefix | ((uint32_t)d << shift) : prefix;
                rank = (found || here) ? rank : rank - digits[d];
                found = found || here;
            }
        }
        parallax = rec::parallax_deg(rec::float_of_key(prefix));
    }
    if (lane == 0) *out = HypRec{count, parallax};
}

__global__ __launch_bounds__(kLanes) void k_reconstruct_finish(const uint8_t* __restrict__ block, int P, int T, float thr_sq, float parallax_deg_thr,
                                                               int min_num_triangulated, const HypRec* __restrict__ hyp_recs,
                                                               ReconRec* __restrict__ out, double* __restrict__ out_pos, uint8_t* __restrict__ out_flags) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const Layout lay = layout_of(P, T);
    const rec::Problem q = reinterpret_cast<const rec::Problem*>(block + lay.problems)[p];
    const auto [off, n] = problem_span(block, lay.offsets, p);
    int32_t counts[rec::kMaxHypotheses];
    float parallax[rec::kMaxHypotheses];
    const int n_hyp = hyp_recs[(size_t)p * rec::kMaxHypotheses].count < 0 ? 0 : rec::hypotheses_of_model(q.model);
#pragma unroll
    for (int h = 0; h < rec::kMaxHypotheses; ++h) {
        const HypRec r = hyp_recs[(size_t)p * rec::kMaxHypotheses + h];
        counts[h] = r.count < 0 ? 0 : r.count;
        parallax[h] = r.parallax;
    }
    const int best = rec::most_plausible(counts, parallax, n_hyp, parallax_deg_thr, min_num_triangulated);
    rec::Hyp hyp;
#pragma unroll
    for (int k = 0; k < 9; ++k) hyp.R[k] = 0.0;
    hyp.t[0] = hyp.t[1] = hyp.t[2] = 0.0;
    double* const pos = out_pos + 3 * (size_t)off;
    uint8_t* const flags = out_flags + off;
    if (best < 0) {
        for (int i = lane; i < n; i += kLanes) {
            pos[3 * (size_t)i] = pos[3 * (size_t)i + 1] = pos[3 * (size_t)i + 2] = 0.0;
            flags[i] = 0;
        }
    } else {
        rec::hypothesis(q, best, hyp);
        const Matches m = matches_of(block, lay, off);
        for (int i = lane; i < n; i += kLanes) {
            const rec::Point pt = rec::check_match(q, hyp, load_match(m, (size_t)i), thr_sq);
            const bool ok = m.inlier[i] != 0 && pt.ok;
#pragma unroll
            for (int c = 0; c < 3; ++c) pos[3 * (size_t)i + c] = ok ? pt.pos[c] : 0.0;
            flags[i] = (ok && !pt.small) ? 1 : 0;
        }
    }
    if (lane == 0) {
        ReconRec& r = out[p];
#pragma unroll
        for (int k = 0; k < 9; ++k) r.rot[k] = hyp.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) r.trans[k] = hyp.t[k];
#pragma unroll
        for (int h = 0; h < rec::kMaxHypotheses; ++h) r.counts[h] = counts[h], r.parallax[h] = parallax[h];
        r.success = best < 0 ? 0 : 1;
        r.best = best;
    }
}

}   // namespace

struct ovs_reconstruct : batch_handle {                   // its records: a match's eight u32 keys
    HypRec* d_hyp = nullptr;                      // [problems][8] between the two kernels
    double *h_pos = nullptr, *m_pos = nullptr;    // the triangulated points, page-locked and mapped like the scaffold's flags
};

extern "C" {

ovs_status ovs_reconstruct_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_reconstruct** out) {
    return batch_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes,
                        (size_t)(max_total_matches < kInitialKeyMatches ? max_total_matches : kInitialKeyMatches), kKeyDoublesPerMatch, sizeof(ReconRec),
                        out, [&](ovs_reconstruct* s) {
                            OVS_HIP_TRY(s->res.dev(&s->d_hyp, sizeof(HypRec) * rec::kMaxHypotheses * (size_t)max_problems));
                            return mapped_block(s->res, &s->h_pos, &s->m_pos, 24 * (size_t)max_total_matches);
                        });
}

ovs_status ovs_reconstruct_destroy(ovs_reconstruct* s) { return batch_destroy(s); }

ovs_status ovs_reconstruct_batch(ovs_reconstruct* s, int32_t n_problems, const int32_t* offsets, const int32_t* models, const double* mats,
                                 const ovs_camera* cams, const uint8_t* inlier_flags, const double* keypts_ref, const double* keypts_cur,
                                 const double* bearings_ref, const double* bearings_cur, float reproj_err_thr, float parallax_deg_thr,
                                 int32_t min_num_triangulated, int32_t* out_success, int32_t* out_best, double* out_rot_ref_to_cur,
                                 double* out_trans_ref_to_cur, int32_t* out_counts, float* out_parallax_deg, double* out_triangulated_pts,
                                 uint8_t* out_is_triangulated) {
    const splan::reconstruct::Call call{s != nullptr, n_problems, offsets, models, mats, cams, inlier_flags, keypts_ref, keypts_cur, bearings_ref,
                                        bearings_cur, reproj_err_thr, parallax_deg_thr, out_success, out_best, out_rot_ref_to_cur, out_trans_ref_to_cur,
                                        out_counts, out_parallax_deg, out_triangulated_pts, out_is_triangulated};
    const splan::Checked checked = splan::reconstruct::check(call, caps_of(s));
    const Layout lay = layout_of(n_problems, checked.T);
    const float thr_sq = rec::threshold_sq(reproj_err_thr);
    const auto reserve = [&] { return s->reserve((size_t)checked.T) != OVS_OK ? OVS_ERR_HIP : OVS_OK; };
    const auto launch = [&](hipStream_t st, int32_t T) {
        hipLaunchKernelGGL(k_reconstruct_hypotheses, dim3(rec::kMaxHypotheses, n_problems), dim3(kLanes), 0, st, s->d_block, n_problems, T, thr_sq,
                           s->records_as<uint32_t>(), s->d_hyp);
        OVS_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_reconstruct_finish, dim3(n_problems), dim3(kLanes), 0, st, s->d_block, n_problems, T, thr_sq, parallax_deg_thr,
                           min_num_triangulated, s->d_hyp, s->m_rec<ReconRec>(), s->m_pos, s->m_flags);
        OVS_HIP_TRY(hipGetLastError());
        return OVS_OK;
    };
    const auto collect = [&](int32_t T) {
        for (int32_t p = 0; p < n_problems; ++p) {
            const ReconRec& r = s->h_rec<ReconRec>()[p];
            out_success[p] = r.success;
            out_best[p] = r.best;
            std::memcpy(out_rot_ref_to_cur + 9 * (size_t)p, r.rot, sizeof(r.rot));
            std::memcpy(out_trans_ref_to_cur + 3 * (size_t)p, r.trans, sizeof(r.trans));
            std::memcpy(out_counts + rec::kMaxHypotheses * (size_t)p, r.counts, sizeof(r.counts));
            std::memcpy(out_parallax_deg + rec::kMaxHypotheses * (size_t)p, r.parallax, sizeof(r.parallax));
        }
        if (T > 0) {
            std::memcpy(out_triangulated_pts, s->h_pos, 24 * (size_t)T);
            std::memcpy(out_is_triangulated, s->h_flags, (size_t)T);
        }
    };
    return run_staged(s, checked, lay.bytes, [&] { splan::reconstruct::stage(call, lay, s->h_block); }, reserve, launch, collect);
}

}   // extern "C"
