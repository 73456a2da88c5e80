// essential_solve.hip -- solve::essential_solver (expected: src/openvslam/solve/essential_solver.{h,cc}): the bearing-vector eight-point RANSAC
// robust::match_frame_and_keyframe runs after its brute-force match, over a batch of (frame 1, frame 2) problems. Rules: DESIGN.md 3.16.
//
// A problem is one pair of frames with n matches: b1 / b2, the bearing of the match's keypoint in frame 1 / frame 2. Everything is f64,
// every operation rounded on its own (the unit is built with -ffp-contract=off). The algebra is essential_math.inc's, which a plain host
// compiler builds too (tests/essential_host.cc).
//
// One wavefront fits one model (fit_accumulate, the sweeps, fit_finish), the eight-match hypothesis and the refit over the winner's
// inliers alike, in the form of two_view_solve.hip: the sums over the matches (rule 6 of 3.10) give lane j the matches j, j + 64, ... in
// rank order and end in a butterfly of x + shfl_xor(x, d), d = 32 .. 1. The 9 x 9 eigenproblem lives in LDS (162 doubles) and is swept in
// the parallel ordering of rule E3 (jacobi_lds_rounds of solve_internal.inc): 9 rounds of four disjoint pairs per sweep, sixteen lanes per
// pair. The rank-two step every lane computes for itself in registers on compile-time indices: nothing is indexed dynamically, nothing
// goes to scratch.
//
// k_essential_hypotheses: grid (hypotheses, problems), one wavefront per workgroup. After the fit the lanes walk the matches for the score;
// lane 0 saves E_21 and the score into the slot of (problem, h). No atomics at all, no waiting between workgroups.
// k_essential_finish: one workgroup (one wavefront) per problem: the scan of the score slots (rule E6), the winner's flags and its inliers
// compacted by rank (ballot + prefix popcount), rule E7's refit with the same device functions, the flags again and the result record.
#include <cmath>
#include <cstring>

#include "essential_math.inc"
#include "ovs_common.h"
#include "solve_internal.inc"

namespace {

constexpr int kSlotDoubles = 10;   // per (problem, h): E_21 (9, row-major) and the score
constexpr int kSampleShare = 16;   // the counter share of a hypothesis (solve.essential_problem_seed: p << 24)

// The staged block of one call, sections in this order: b1 f64 [3 T], b2 f64 [3 T], offsets i32 [P + 1].
struct Layout {
    size_t b1, b2, offsets, bytes;
};
__host__ __device__ inline Layout layout_of(int P, int T) {
    Layout l;
    l.b1 = 0;
    l.b2 = l.b1 + 24 * (size_t)T;
    l.offsets = l.b2 + 24 * (size_t)T;
    l.bytes = l.offsets + 4 * ((size_t)P + 1);
    return l;
}

// per problem in the result block
struct EssentialRec {
    double mat[9], score;
    int32_t valid, best_iter, num_inliers, pad;
};
static_assert(sizeof(EssentialRec) == 96, "EssentialRec is read by the host");

// the 9 x 9 eigenproblem in LDS: the matrix and its vectors, row-major
struct Eig {
    double A[81], V[81];
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x = x + __shfl_xor(x, d);
    return x;
}

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
    __syncthreads();   // whoever read e before has left it
    int k = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = r; c < 9; ++c, ++k) {
            const double s = wave_sum(acc[k]);
            if (lane == 0) e.A[r * 9 + c] = e.A[c * 9 + r] = s;
        }
    for (int i = lane; i < 81; i += 64) e.V[i] = (i / 9 == i % 9) ? 1.0 : 0.0;
    __syncthreads();
}

// rules E3 (the choice of the vector) and E4 on the swept e: every lane returns the same E_21
__device__ __forceinline__ void fit_finish(const Eig& e, double (&E)[9]) {
    double Gm[9];
    int best = 0;   // the smallest diagonal entry, the lowest index on a tie
    double smallest = e.A[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const double d = e.A[i * 10];
        const bool take = d < smallest;
        smallest = take ? d : smallest;
        best = take ? i : best;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) Gm[j] = e.V[j * 9 + best];
    ess::rank_two(Gm, E);
}

// rule E5 over the n matches of a problem by one wavefront: count and score in every lane; flags (one byte per match) and list (the
// inliers by rank, in match order) are written where they are not null.
__device__ __forceinline__ void score_wave(const double (&E)[9], const double* __restrict__ b1, const double* __restrict__ b2, int n, double thr, int lane,
                                           uint8_t* __restrict__ flags, int32_t* __restrict__ list, int& count, double& score) {
    double part = 0.0;
    count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n;
        const size_t j = in ? (size_t)i : 0;
        bool inl;
        double r2, r1;
        const double term = ess::match_term(E, b1 + 3 * j, b2 + 3 * j, thr, inl, r2, r1);
        if (in) part = part + term;
        inl = in && inl;
        const unsigned long long mask = __ballot(inl);
        if (flags && in) flags[i] = inl ? 1 : 0;
        if (list && inl) list[count + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        count += __popcll(mask);
    }
    score = wave_sum(part);
}

// where the slot of (problem, h) starts in the models' buffer
__device__ __forceinline__ size_t slot_at(int p, int max_iter, int h) { return ((size_t)p * max_iter + h) * kSlotDoubles; }

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
    if (n >= 8) {
        // rule E6: the greatest score above 0.0, the lowest h on a tie; a NaN never wins
        const double* slots = wave_models + slot_at(p, max_iter, 0);
        double best = 0.0;
        for (int h = lane; h < max_iter; h += 64) {
            const double s = slots[(size_t)h * kSlotDoubles + 9];
            if (best < s) best = s, best_iter = h;
        }
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const double ob = __shfl_xor(best, d);
            const int oh = __shfl_xor(best_iter, d);
            const bool take = best < ob || (ob == best && oh >= 0 && oh < best_iter);
            best = take ? ob : best;
            best_iter = take ? oh : best_iter;
        }
    }
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
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) finite = finite && __builtin_isfinite(E2[k]);
        if (finite) {
#pragma unroll
            for (int k = 0; k < 9; ++k) E[k] = E2[k];
            score_wave(E, b1, b2, n, thr, lane, flags, nullptr, count, score);
            valid = score > 0.0 && count >= 8;
        }
    }
    if (!valid) {   // rule E6's invalid form
        for (int i = lane; i < n; i += 64) flags[i] = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = (k % 4 == 0) ? 1.0 : 0.0;
        score = 0.0;
        count = 0;
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

struct ovs_essential : ransac_handle {
    int32_t* d_inlier_idx = nullptr;   // [matches of the call] a winner's inliers by rank, per problem at its offset
    EssentialRec* h_rec() { return reinterpret_cast<EssentialRec*>(h_result); }
    EssentialRec* m_rec() { return reinterpret_cast<EssentialRec*>(m_result); }
};

extern "C" {

ovs_status ovs_essential_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_essential** out) {
    const ovs_status st = ransac_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes,
                                        (size_t)max_problems * 32,   // 32 iterations per problem without growing
                                        kSlotDoubles, out, sizeof(EssentialRec));
    if (st != OVS_OK) return st;
    std::unique_ptr<ovs_essential> owner(*out);
    *out = nullptr;
    OVS_HIP_TRY(owner->res.dev(&owner->d_inlier_idx, sizeof(int32_t) * (size_t)max_total_matches));
    *out = owner.release();
    return OVS_OK;
}

ovs_status ovs_essential_destroy(ovs_essential* s) { return ransac_destroy(s); }

ovs_status ovs_essential_solve_batch(ovs_essential* s, int32_t n_problems, const int32_t* offsets, const double* bearings_1, const double* bearings_2,
                                     double residual_cos_thr, int32_t max_num_iter, int32_t recompute, uint64_t seed, double* out_E_21, double* out_scores,
                                     int32_t* out_valid, int32_t* out_best_iter, int32_t* out_num_inliers, uint8_t* out_inlier_flags) {
    if (max_num_iter < 1 || max_num_iter > kMaxIter || !std::isfinite(residual_cos_thr) || !(residual_cos_thr > 0.0) || !(residual_cos_thr <= 1.0))
        return OVS_ERR_INVALID;
    const auto stage = [&](uint8_t* h_block, const Layout& lay, int32_t T) {
        if (T > 0) {
            std::memcpy(h_block + lay.b1, bearings_1, 24 * (size_t)T);
            std::memcpy(h_block + lay.b2, bearings_2, 24 * (size_t)T);
        }
        return OVS_OK;
    };
    const auto reserve = [&] { return s->reserve_models((size_t)n_problems * (size_t)max_num_iter) != OVS_OK ? OVS_ERR_HIP : OVS_OK; };
    const auto launch = [&](hipStream_t st, int32_t T) {
        hipLaunchKernelGGL(k_essential_hypotheses, dim3(max_num_iter, n_problems), dim3(64), 0, st, s->d_block, n_problems, T, max_num_iter, seed,
                           residual_cos_thr, s->d_wave_models);
        OVS_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_essential_finish, dim3(n_problems), dim3(64), 0, st, s->d_block, n_problems, T, max_num_iter, recompute ? 1 : 0,
                           residual_cos_thr, s->d_wave_models, s->d_inlier_idx, s->m_rec(), s->m_flags);
        OVS_HIP_TRY(hipGetLastError());
        return OVS_OK;
    };
    const auto collect = [&](int32_t T) {
        for (int32_t p = 0; p < n_problems; ++p) {
            const EssentialRec& r = s->h_rec()[p];
            std::memcpy(out_E_21 + 9 * (size_t)p, r.mat, sizeof(r.mat));
            out_scores[p] = r.score;
            out_valid[p] = r.valid;
            out_best_iter[p] = r.best_iter;
            out_num_inliers[p] = r.num_inliers;
        }
        if (T > 0) std::memcpy(out_inlier_flags, s->h_flags, (size_t)T);
    };
    return run_staged(s, n_problems, offsets, {out_E_21, out_scores, out_valid, out_best_iter, out_num_inliers}, {bearings_1, bearings_2}, out_inlier_flags,
                      layout_of, stage, reserve, launch, collect);
}

}   // extern "C"
