// eight_point_internal.inc -- the eight-point, score-slot RANSAC under two_view_solve.hip (DESIGN.md 3.13) and essential_solve.hip (3.16),
// on top of solve_internal.inc. One wavefront fits one model: A^T A summed in rank order into a 9 x 9 eigenproblem in LDS (the solver's
// loop over its rows, then store_sums), the solver's own sweeps, the vector of the smallest diagonal entry (null_column). The score is
// summed per lane with the inliers compacted by rank (score_matches); every (problem slot, hypothesis) owns a slot of kSlotDoubles, and the
// finish kernel scans a problem slot's slots for its winner (best_slot: the one statement of 3.13 rule 7 and 3.16 rule E6). A solver
// supplies its rows, its score term, its sweeps and everything between the null vector and the model. The one callable (score_matches'
// term) is a lambda on compile-time indices: nothing is indexed dynamically, nothing goes to scratch. The helpers' shapes are those that
// leave the kernels' instruction streams what they were (DESIGN.md 3.16 has the comparison). On the host: eight_point_handle, its create
// (batch_create with the inlier lists), and run_slots, the batch call of two launches. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include "solve_internal.inc"

namespace {

constexpr int kSlotDoubles = 10;   // per (problem slot, h): the matrix (9, row-major) and the score

// the 9 x 9 eigenproblem in LDS: the matrix and its vectors, row-major
struct Eig {
    double A[81], V[81];
};

// the second half of A^T A by one wavefront: acc holds the lane's 45 upper-triangle sums over its matches j, j + 64, ... in that order
// (the solver's own loop: its rows and their order of operations); their sum over the wavefront goes into e.A, the identity into e.V
__device__ __forceinline__ void store_sums(Eig& e, int lane, const double (&acc)[45]) {
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

// the null vector of the swept e is column null_column(e) of e.V: the smallest diagonal entry, the lowest index on a tie; the same in
// every lane
__device__ __forceinline__ int null_column(const Eig& e) {
    int best = 0;
    double smallest = e.A[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const double d = e.A[i * 10];
        const bool take = d < smallest;
        smallest = take ? d : smallest;
        best = take ? i : best;
    }
    return best;
}

// the score over the n matches of a problem by one wavefront: count and score in every lane; flags (one byte per match) and list (the
// inliers by rank, in match order) are written where they are not null. term(j, inlier) returns match j's term and says whether it is an
// inlier; a lane past the end evaluates match 0 and is masked out. The callers mark their lambda always_inline, as every helper here is.
template <class Term>
__device__ __forceinline__ void score_matches(int n, int lane, uint8_t* __restrict__ flags, int32_t* __restrict__ list, int& count, double& score,
                                              Term term) {
    double part = 0.0;
    count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n;
        bool inl;
        const double t = term(in ? (size_t)i : 0, inl);
        if (in) part = part + t;
        inl = in && inl;
        const unsigned long long mask = __ballot(inl);
        if (flags && in) flags[i] = inl ? 1 : 0;
        if (list && inl) list[count + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        count += __popcll(mask);
    }
    score = wave_sum(part);
}

// where the slot of (problem slot, h) starts in the models' buffer; the problem slot is p (essential) or 2 p + model (two-view)
__device__ __forceinline__ size_t slot_at(size_t problem_slot, int max_iter, int h) { return (problem_slot * max_iter + h) * kSlotDoubles; }

// the winner among a problem slot's max_iter slots: the greatest score above 0.0, the lowest h on a tie; a NaN never wins. -1: none.
__device__ __forceinline__ void best_slot(const double* __restrict__ slots, int max_iter, int lane, int& best_iter) {
    double best = 0.0;
    best_iter = -1;
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

// a refit replaces the winner only if every entry is finite
__device__ __forceinline__ bool all_finite(const double (&M)[9]) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) finite = finite && __builtin_isfinite(M[k]);
    return finite;
}

// the invalid form where there is no valid model: the problem's flags zeroed, the identity, no score, no inliers (and best_iter -1,
// which the caller sets)
__device__ __forceinline__ void invalid_form(uint8_t* __restrict__ flags, int n, int lane, double (&M)[9], double& score, int& count) {
    for (int i = lane; i < n; i += 64) flags[i] = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = (k % 4 == 0) ? 1.0 : 0.0;
    score = 0.0;
    count = 0;
}

// ---- the host side: the handle under ovs_twoview_* and ovs_essential_*
struct eight_point_handle : batch_handle {
    int32_t* d_inlier_idx = nullptr;   // [lists][matches of the call] a winner's inliers by rank, per problem slot at the problem's offset
};

// H: ovs_twoview (lists = 2: both models) or ovs_essential (1). `lists` x 32 iterations per problem fit without growing; extra(handle)
// acquires what the solver's handle adds to the lists.
template <class H, class Extra>
ovs_status eight_point_create(int32_t device, int32_t max_problems, int32_t max_total_matches, size_t block_bytes, int lists, size_t result_bytes,
                              H** out, Extra extra) {
    return batch_create(device, max_problems, max_total_matches, block_bytes, (size_t)max_problems * lists * 32, kSlotDoubles, result_bytes, out, [&](H* s) -> ovs_status {
        OVS_HIP_TRY(s->res.dev(&s->d_inlier_idx, sizeof(int32_t) * lists * (size_t)max_total_matches));
        return extra(s);
    });
}

// One solve_batch call of a slot solver: run_staged with room for n_problems x lists x max_num_iter slots and the two launches,
// hypotheses(stream, T) and finish(stream, T).
template <class Stage, class Hypotheses, class Finish, class Collect>
ovs_status run_slots(eight_point_handle* s, const splan::Checked& checked, size_t upload_bytes, int32_t n_problems, int lists, int32_t max_num_iter,
                     Stage stage, Hypotheses hypotheses, Finish finish, Collect collect) {
    return run_staged(
        s, checked, upload_bytes, stage,
        [&] { return s->reserve((size_t)n_problems * lists * (size_t)max_num_iter) != OVS_OK ? OVS_ERR_HIP : OVS_OK; },
        [&](hipStream_t stream, int32_t T) {
            hypotheses(stream, T);
            OVS_HIP_TRY(hipGetLastError());
            finish(stream, T);
            OVS_HIP_TRY(hipGetLastError());
            return OVS_OK;
        },
        collect);
}

}   // namespace
