// essential_solve.hip -- solve::essential_solver (expected: src/openvslam/solve/essential_solver.{h,cc}): the bearing-vector eight-point RANSAC
// robust::match_frame_and_keyframe runs after its brute-force match, over a batch of (frame 1, frame 2) problems. Rules: DESIGN.md 3.16.
//
// A problem is one pair of frames with n matches: b1 / b2, the bearing of the match's keypoint in frame 1 / frame 2. Everything is f64,
// every operation rounded on its own (the unit is built with -ffp-contract=off). The algebra is essential_math.inc's, which a plain host
// compiler builds too (tests/essential_host.cc).
//
// One wavefront fits one model (fit_accumulate, the sweeps, fit_finish), the eight-match hypothesis and the refit over the winner's
// inliers alike, on the scaffold two_view_solve.hip shares (eight_point_internal.inc: the sums in rank order, the 9 x 9 eigenproblem in
// LDS, the null vector, the score walk, the score slots and their winner, the invalid form, the handle and the batch call). This unit's
// own: the row and the score term (essential_math.inc), the sweeps in the parallel ordering of rule E3 (jacobi_lds_rounds of
// solve_internal.inc): 9 rounds of four disjoint pairs per sweep, sixteen lanes per pair; and the rank-two step, which every lane computes
// for itself in registers on compile-time indices: nothing is indexed dynamically, nothing goes to scratch.
//
// k_essential_hypotheses: grid (hypotheses, problems), one wavefront per workgroup. After the fit the lanes walk the matches for the score;
// lane 0 saves E_21 and the score into the slot of (problem, h). No atomics at all, no waiting between workgroups.
// k_essential_finish: one workgroup (one wavefront) per problem: the scan of the score slots (rule E6), the winner's flags and its inliers
// compacted by rank (ballot + prefix popcount), rule E7's refit with the same device functions, the flags again and the result record.
#include <cmath>
#include <cstring>

#include "eight_point_internal.inc"
#include "essential_math.inc"
#include "ovs_common.h"

namespace {

constexpr int kSampleShare = 16;   // the counter share of a hypothesis (solve.essential_problem_seed: p << 24)

// the staged block of one call: solve_plan.inc
using splan::essential::Layout;
using splan::essential::layout_of;

// per problem in the result block
struct EssentialRec {
    double mat[9], score;
    int32_t valid, best_iter, num_inliers, pad;
};
static_assert(sizeof(EssentialRec) == 96, "EssentialRec is read by the host");

// rule E2: A^T A over the m matches idx[0 .. m) of a problem, in that order, into e.A, and the identity into e.V. idx may point into LDS
// or memory.
__device__ __forceinline__ void fit_accumulate(const double* __restrict__ b1, const double* __restrict__ b2, const int32_t* idx, int m, Eig& e, int lane) {
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
    for (int i = lane; i < m; i += 64) {
        const size_t j = (size_t)idx[i];
        double a[9];
        ess::row_of(b1 + 3 * j, b2 + 3 * j, a);
        int k = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int c = r; c < 9; ++c, ++k) acc[k] = acc[k] + a[r] * a[c];
    }
    store_sums(e, lane, acc);
}

// rules E3 (the choice of the vector) and E4 on the swept e: every lane returns the same E_21
__device__ __forceinline__ void fit_finish(const Eig& e, double (&E)[9]) {
    double Gm[9];
    const int best = null_column(e);
#pragma unroll
    for (int j = 0; j < 9; ++j) Gm[j] = e.V[j * 9 + best];
    ess::rank_two(Gm, E);
}

// rule E5 over the n matches of a problem by one wavefront, in the form of score_matches
__device__ __forceinline__ void score_wave(const double (&E)[9], const double* __restrict__ b1, const double* __restrict__ b2, int n, double thr, int lane,
                                           uint8_t* __restrict__ flags, int32_t* __restrict__ list, int& count, double& score) {
    score_matches(n, lane, flags, list, count, score, [&](size_t j, bool& inl) __attribute__((always_inline)) {
        double r2, r1;
        return ess::match_term(E, b1 + 3 * j, b2 + 3 * j, thr, inl, r2, r1);
    });
}

__global__ __launch_bounds__(64) void k_essential_hypotheses(const uint8_t* __restrict__ block, int P, int T, int max_iter, uint64_t seed, double thr,
                                                             double* __restrict__ wave_models) {
    __shared__ Eig e;
    __shared__ int32_t idx[8];   // the hypothesis's sample
    const int h = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const Layout lay = layout_of(P, T);
    const auto [off, n] = problem_span(block, lay.offsets, p);
    if (n < 8) return;   // rule E6: invalid, k_essential_finish says so
    const double* b1 = reinterpret_cast<const double*>(block + lay.b1) + 3 * (size_t)off;
    const double* b2 = reinterpret_cast<const double*>(block + lay.b2) + 3 * (size_t)off;
    if (lane == 0) {
        uint32_t i[8];
        sample_distinct<8, kSampleShare>(seed, (uint32_t)p, (uint32_t)h, (uint32_t)n, i);   // rule E1
#pragma unroll
        for (int k = 0; k < 8; ++k) idx[k] = (int32_t)i[k];
    }
    __syncthreads();
    double E[9], score;
    int count;
    fit_accumulate(b1, b2, idx, 8, e, lane);
    jacobi_lds_rounds<9, ess::kSweeps>(e.A, e.V, lane);
    fit_finish(e, E);
    score_wave(E, b1, b2, n, thr, lane, nullptr, nullptr, count, score);
    if (lane == 0) {
        double* slot = wave_models + slot_at(p, max_iter, h);
#pragma unroll
        for (int k = 0; k < 9; ++k) slot[k] = E[k];
        slot[9] = score;
    }
}

__global__ __launch_bounds__(64) void k_essential_finish(const uint8_t* __restrict__ block, int P, int T, int max_iter, int recompute, double thr,
                                                         const double* __restrict__ wave_models, int32_t* __restrict__ inlier_idx,
                                                         EssentialRec* __restrict__ out, uint8_t* __restrict__ out_flags) {
    __shared__ Eig e;
    const Layout lay = layout_of(P, T);
    const int p = blockIdx.x, lane = threadIdx.x;
    const auto [off, n] = problem_span(block, lay.offsets, p);
    const double* b1 = reinterpret_cast<const double*>(block + lay.b1) + 3 * (size_t)off;
    const double* b2 = reinterpret_cast<const double*>(block + lay.b2) + 3 * (size_t)off;
    int32_t* list = inlier_idx + off;
    uint8_t* flags = out_flags + off;
    bool valid = false;
    double E[9], score = 0.0;
    int count = 0, best_iter = -1;
    if (n >= 8) best_slot(wave_models + slot_at(p, max_iter, 0), max_iter, lane, best_iter);   // rule E6
    if (best_iter >= 0) {
        const double* md = wave_models + slot_at(p, max_iter, best_iter);   // the doubles the hypothesis kernel scored with
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = md[k];
        score_wave(E, b1, b2, n, thr, lane, flags, list, count, score);
        valid = score > 0.0 && count >= 8;
    }
    if (recompute && valid) {   // rule E7
        __syncthreads();        // the list is complete
        fit_accumulate(b1, b2, list, count, e, lane);
        jacobi_lds_rounds<9, ess::kSweeps>(e.A, e.V, lane);
        double E2[9];
        fit_finish(e, E2);
        if (all_finite(E2)) {
#pragma unroll
            for (int k = 0; k < 9; ++k) E[k] = E2[k];
            score_wave(E, b1, b2, n, thr, lane, flags, nullptr, count, score);
            valid = score > 0.0 && count >= 8;
        }
    }
    if (!valid) {   // rule E6
        invalid_form(flags, n, lane, E, score, count);
        best_iter = -1;
    }
    if (lane == 0) {
        EssentialRec* rec = out + p;
#pragma unroll
        for (int k = 0; k < 9; ++k) rec->mat[k] = E[k];
        rec->score = score;
        rec->valid = valid ? 1 : 0;
        rec->best_iter = best_iter;
        rec->num_inliers = count;
        rec->pad = 0;
    }
}

}   // namespace

struct ovs_essential : eight_point_handle {};

extern "C" {

ovs_status ovs_essential_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_essential** out) {
    return eight_point_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes, 1, sizeof(EssentialRec), out,
                              no_extra);
}

ovs_status ovs_essential_destroy(ovs_essential* s) { return batch_destroy(s); }

ovs_status ovs_essential_solve_batch(ovs_essential* s, int32_t n_problems, const int32_t* offsets, const double* bearings_1, const double* bearings_2,
                                     double residual_cos_thr, int32_t max_num_iter, int32_t recompute, uint64_t seed, double* out_E_21, double* out_scores,
                                     int32_t* out_valid, int32_t* out_best_iter, int32_t* out_num_inliers, uint8_t* out_inlier_flags) {
    const splan::essential::Call call{s != nullptr, n_problems, offsets, bearings_1, bearings_2, residual_cos_thr, max_num_iter, out_E_21,
                                      out_scores, out_valid, out_best_iter, out_num_inliers, out_inlier_flags};
    const splan::Checked checked = splan::essential::check(call, caps_of(s));
    const Layout lay = layout_of(n_problems, checked.T);
    const auto hypotheses = [&](hipStream_t st, int32_t T) {
        hipLaunchKernelGGL(k_essential_hypotheses, dim3(max_num_iter, n_problems), dim3(64), 0, st, s->d_block, n_problems, T, max_num_iter, seed,
                           residual_cos_thr, s->d_records);
    };
    const auto finish = [&](hipStream_t st, int32_t T) {
        hipLaunchKernelGGL(k_essential_finish, dim3(n_problems), dim3(64), 0, st, s->d_block, n_problems, T, max_num_iter, recompute ? 1 : 0,
                           residual_cos_thr, s->d_records, s->d_inlier_idx, s->m_rec<EssentialRec>(), s->m_flags);
    };
    const auto collect = [&](int32_t T) {
        for (int32_t p = 0; p < n_problems; ++p) {
            const EssentialRec& r = s->h_rec<EssentialRec>()[p];
            std::memcpy(out_E_21 + 9 * (size_t)p, r.mat, sizeof(r.mat));
            out_scores[p] = r.score;
            out_valid[p] = r.valid;
            out_best_iter[p] = r.best_iter;
            out_num_inliers[p] = r.num_inliers;
        }
        if (T > 0) std::memcpy(out_inlier_flags, s->h_flags, (size_t)T);
    };
    return run_slots(s, checked, lay.bytes, n_problems, 1, max_num_iter, [&] { splan::essential::stage(call, lay, s->h_block); }, hypotheses, finish,
                     collect);
}

}   // extern "C"
