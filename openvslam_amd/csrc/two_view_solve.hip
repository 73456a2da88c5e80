// two_view_solve.hip -- solve::homography_solver and solve::fundamental_solver (expected: src/openvslam/solve/{homography,fundamental}_solver.{h,cc}):
// the two RANSACs initialize::perspective::initialize runs on two host threads for every frame until the map exists, over a batch of
// (reference frame, current frame) problems, with upstream's choice between the two models. Rules: DESIGN.md 3.13.
//
// A problem is one pair of frames with n matches: x1 / x2, the undistorted keypoint of the reference / current frame. Everything is f64,
// every operation rounded on its own (the unit is built with -ffp-contract=off).
//
// One wavefront fits one model (fit_accumulate, the sweeps, fit_finish), the eight-match hypothesis and the refit over the winner's
// inliers alike, on the scaffold essential_solve.hip shares (eight_point_internal.inc: store_sums, null_column, score_matches, the
// score slots and best_slot, the invalid form, the handle and run_slots). The sums over the matches (rule 6 of 3.10) give lane j the
// matches j, j + 64, ... in rank order and end in wave_sum's butterfly of x + shfl_xor(x, d), d = 32 .. 1: lane 0 holds the rule's
// pairwise tree, and as IEEE addition commutes every lane holds the same bits. The 9 x 9 eigenproblem lives in LDS (162 doubles): the
// rotation's angle in every lane, its 9 column pairs, 9 row pairs and 9 vector pairs one per lane (jacobi_lds of solve_internal.inc,
// which pnp_solve.hip's 12 x 12 problem shares). What does not depend on the match (the 3 x 3 products, the rank-two step, the inverse)
// every lane computes for itself in registers on compile-time indices: nothing is indexed dynamically, nothing goes to scratch.
//
// k_twoview_hypotheses: grid (hypotheses, 2 models, problems), one wavefront per workgroup. Hypothesis h of a problem draws ONE sample for
// both models. After the fit the lanes walk the matches for the score; lane 0 saves the matrix and the score into the slot of
// (problem, model, h). No atomics at all, no waiting between workgroups. A masked-out model's workgroups return at once.
// k_twoview_finish: one workgroup (one wavefront) per problem: per model the scan of the score slots (rule 7), the winner's flags and its
// inliers compacted by rank (ballot + prefix popcount); rule 8's refits with the same device functions, the two 9 x 9 problems swept side
// by side (H's by lanes 0 .. 31, F's by lanes 32 .. 63: the sweeps are the long part and a matrix keeps 18 lanes busy); the flags again,
// both result records and rule 9's choice.
#include <cmath>
#include <cstring>

#include "eight_point_internal.inc"
#include "ovs_common.h"

namespace {

constexpr int kSweeps = 8;
constexpr int kSampleShare = 16;   // the counter share of a hypothesis (solve.two_view_problem_seed: p << 24)
constexpr double kChiH = 5.991, kChiF = 3.841, kScore = 5.991;

// the staged block of one call: solve_plan.inc
using splan::twoview::Layout;
using splan::twoview::layout_of;

// per problem in the result block: index 0 is H, 1 is F
struct TwoViewRec {
    double mat[2][9], score[2];
    int32_t valid[2], best_iter[2], num_inliers[2], selected, pad;
};
static_assert(sizeof(TwoViewRec) == 192, "TwoViewRec is read by the host");

// a 3 x 3 product, rows times columns by dot3, zeros multiplied like any value
__device__ __forceinline__ void mul3(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]);
}
__device__ __forceinline__ void transpose3(const double (&A)[9], double (&At)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) At[3 * r + c] = A[3 * c + r];
}

// rule 1: one side of a problem over its n matches, by one wavefront; every lane returns the same bits
struct Norm {
    double mean[2], dev[2], s[2];
};
__device__ __forceinline__ Norm normalise(const double* __restrict__ x, int n, int lane) {
    Norm N;
    const double fn = (double)n;
    double a0 = 0.0, a1 = 0.0;
    for (int i = lane; i < n; i += 64) {
        a0 = a0 + x[2 * (size_t)i];
        a1 = a1 + x[2 * (size_t)i + 1];
    }
    N.mean[0] = wave_sum(a0) / fn;
    N.mean[1] = wave_sum(a1) / fn;
    double d0 = 0.0, d1 = 0.0;
    for (int i = lane; i < n; i += 64) {
        d0 = d0 + fabs(x[2 * (size_t)i] - N.mean[0]);
        d1 = d1 + fabs(x[2 * (size_t)i + 1] - N.mean[1]);
    }
    N.dev[0] = wave_sum(d0) / fn;
    N.dev[1] = wave_sum(d1) / fn;
    N.s[0] = 1.0 / N.dev[0];
    N.s[1] = 1.0 / N.dev[1];
    return N;
}

// rule 3, first half: A^T A of the model (MODEL 0: H_21, 1: F_21) over the m matches idx[0 .. m) of a problem, in that order, under the
// problem's normalisation, into e.A, and the identity into e.V. idx may point into LDS or memory.
template <int MODEL>
__device__ __forceinline__ void fit_accumulate(const double* __restrict__ x1, const double* __restrict__ x2, const int32_t* idx, int m, const Norm& N1,
                                               const Norm& N2, Eig& e, int lane) {
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
    for (int i = lane; i < m; i += 64) {
        const size_t j = (size_t)idx[i];
        const double ax = (x1[2 * j] - N1.mean[0]) * N1.s[0], ay = (x1[2 * j + 1] - N1.mean[1]) * N1.s[1];
        const double bx = (x2[2 * j] - N2.mean[0]) * N2.s[0], by = (x2[2 * j + 1] - N2.mean[1]) * N2.s[1];
        if (MODEL == 0) {
            const double r1[9] = {0.0, 0.0, 0.0, -ax, -ay, -1.0, by * ax, by * ay, by};
            const double r2[9] = {ax, ay, 1.0, 0.0, 0.0, 0.0, -(bx * ax), -(bx * ay), -bx};
            int k = 0;
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
                for (int c = r; c < 9; ++c, ++k) acc[k] = acc[k] + (r1[r] * r1[c] + r2[r] * r2[c]);
        } else {
            const double r1[9] = {bx * ax, bx * ay, bx, by * ax, by * ay, by, ax, ay, 1.0};
            int k = 0;
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
                for (int c = r; c < 9; ++c, ++k) acc[k] = acc[k] + r1[r] * r1[c];
        }
    }
    store_sums(e, lane, acc);
}

// rules 3 (second half) to 5 on the swept e: the vector of the smallest diagonal entry as G, rank two for F, the denormalised model. Every
// lane returns the same M.
template <int MODEL>
__device__ __forceinline__ void fit_finish(const Eig& e, const Norm& N1, const Norm& N2, double (&M)[9]) {
    double Gm[9];
    const int best = null_column(e);
#pragma unroll
    for (int j = 0; j < 9; ++j) Gm[j] = e.V[j * 9 + best];
    const double T1[9] = {N1.s[0], 0.0, -(N1.mean[0] * N1.s[0]), 0.0, N1.s[1], -(N1.mean[1] * N1.s[1]), 0.0, 0.0, 1.0};
    double GT[9];
    if (MODEL == 0) {
        const double Tinv2[9] = {N2.dev[0], 0.0, N2.mean[0], 0.0, N2.dev[1], N2.mean[1], 0.0, 0.0, 1.0};
        mul3(Gm, T1, GT);
        mul3(Tinv2, GT, M);
    } else {
        // rule 4: the vector of the smallest eigenvalue of G^T G, projected out of G
        double Gt[9], GtG[9];
        transpose3(Gm, Gt);
        mul3(Gt, Gm, GtG);
        double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) A[r][c] = GtG[3 * r + c];
#pragma unroll 1
        for (int sweep = 0; sweep < kSweeps; ++sweep) {
            jacobi_rotate<3, 0, 1>(A, V);
            jacobi_rotate<3, 0, 2>(A, V);
            jacobi_rotate<3, 1, 2>(A, V);
        }
        double smallest = A[0][0], v3[3] = {V[0][0], V[1][0], V[2][0]};
#pragma unroll
        for (int i = 1; i < 3; ++i) {
            const bool take = A[i][i] < smallest;
            smallest = take ? A[i][i] : smallest;
#pragma unroll
            for (int j = 0; j < 3; ++j) v3[j] = take ? V[j][i] : v3[j];
        }
        double G2[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double w = dot3(Gm[3 * r], Gm[3 * r + 1], Gm[3 * r + 2], v3[0], v3[1], v3[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) G2[3 * r + c] = Gm[3 * r + c] - w * v3[c];
        }
        const double T2[9] = {N2.s[0], 0.0, -(N2.mean[0] * N2.s[0]), 0.0, N2.s[1], -(N2.mean[1] * N2.s[1]), 0.0, 0.0, 1.0};
        double T2t[9];
        transpose3(T2, T2t);
        mul3(G2, T1, GT);
        mul3(T2t, GT, M);
    }
}

// rule 6, one direction: the transfer of src by the homography Mh against dst; the epipolar line of src under Mf against dst
__device__ __forceinline__ double transfer_chi(const double (&Mh)[9], double sx, double sy, double dx, double dy, double inv_sigma_sq) {
    const double w = 1.0 / dot3(Mh[6], Mh[7], Mh[8], sx, sy, 1.0);
    const double u = dot3(Mh[0], Mh[1], Mh[2], sx, sy, 1.0) * w;
    const double v = dot3(Mh[3], Mh[4], Mh[5], sx, sy, 1.0) * w;
    const double du = dx - u, dv = dy - v;
    return (du * du + dv * dv) * inv_sigma_sq;
}
__device__ __forceinline__ double epipolar_chi(const double (&Mf)[9], double sx, double sy, double dx, double dy, double inv_sigma_sq) {
    const double l0 = dot3(Mf[0], Mf[1], Mf[2], sx, sy, 1.0);
    const double l1 = dot3(Mf[3], Mf[4], Mf[5], sx, sy, 1.0);
    const double l2 = dot3(Mf[6], Mf[7], Mf[8], sx, sy, 1.0);
    const double num = dot3(l0, l1, l2, dx, dy, 1.0);
    return (num * num / (l0 * l0 + l1 * l1)) * inv_sigma_sq;
}

// rule 6 over the n matches of a problem by one wavefront: count and score in every lane; flags (one byte per match) and list (the
// inliers by rank, in match order) are written where they are not null. A NaN fails "chi <= threshold".
template <int MODEL>
__device__ __forceinline__ void score_wave(const double (&M)[9], const double* __restrict__ x1, const double* __restrict__ x2, int n,
                                           double inv_sigma_sq, int lane, uint8_t* __restrict__ flags, int32_t* __restrict__ list, int& count,
                                           double& score) {
    double D1[9];   // direction 1's matrix: H_12 by cofactors (3.10 rule 2.2); direction 2's of F is the transpose
    if (MODEL == 0) {
        const double m00 = M[4] * M[8] - M[5] * M[7];
        const double m01 = M[5] * M[6] - M[3] * M[8];
        const double m02 = M[3] * M[7] - M[4] * M[6];
        const double det = (M[0] * m00 + M[1] * m01) + M[2] * m02;
        D1[0] = m00 / det;
        D1[1] = (M[2] * M[7] - M[1] * M[8]) / det;
        D1[2] = (M[1] * M[5] - M[2] * M[4]) / det;
        D1[3] = m01 / det;
        D1[4] = (M[0] * M[8] - M[2] * M[6]) / det;
        D1[5] = (M[2] * M[3] - M[0] * M[5]) / det;
        D1[6] = m02 / det;
        D1[7] = (M[1] * M[6] - M[0] * M[7]) / det;
        D1[8] = (M[0] * M[4] - M[1] * M[3]) / det;
    } else {
        transpose3(M, D1);
    }
    score_matches(n, lane, flags, list, count, score, [&](size_t j, bool& inl) __attribute__((always_inline)) {
        const double ax = x1[2 * j], ay = x1[2 * j + 1], bx = x2[2 * j], by = x2[2 * j + 1];
        double chi1, chi2;
        if (MODEL == 0) {
            chi1 = transfer_chi(D1, bx, by, ax, ay, inv_sigma_sq);
            chi2 = transfer_chi(M, ax, ay, bx, by, inv_sigma_sq);
        } else {
            chi1 = epipolar_chi(M, ax, ay, bx, by, inv_sigma_sq);
            chi2 = epipolar_chi(D1, bx, by, ax, ay, inv_sigma_sq);
        }
        const double thr = MODEL == 0 ? kChiH : kChiF;
        const bool pass1 = chi1 <= thr;
        inl = pass1 && chi2 <= thr;
        double term = 0.0;
        term = pass1 ? term + (kScore - chi1) : term;
        term = inl ? term + (kScore - chi2) : term;
        return term;
    });
}

template <int MODEL>
__device__ __forceinline__ void hypothesis(const double* __restrict__ x1, const double* __restrict__ x2, int n, double inv_sigma_sq, const int32_t* idx,
                                           Eig& e, int lane, double* __restrict__ slot) {
    const Norm N1 = normalise(x1, n, lane), N2 = normalise(x2, n, lane);
    double M[9], score;
    int count;
    fit_accumulate<MODEL>(x1, x2, idx, 8, N1, N2, e, lane);
    jacobi_lds<9, kSweeps>(e.A, e.V, lane);
    fit_finish<MODEL>(e, N1, N2, M);
    score_wave<MODEL>(M, x1, x2, n, inv_sigma_sq, lane, nullptr, nullptr, count, score);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) slot[k] = M[k];
        slot[9] = score;
    }
}

__global__ __launch_bounds__(64) void k_twoview_hypotheses(const uint8_t* __restrict__ block, int P, int T, int max_iter, int models, uint64_t seed,
                                                           double inv_sigma_sq, double* __restrict__ wave_models) {
    __shared__ Eig e;
    __shared__ int32_t idx[8];   // the hypothesis's sample
    const int h = blockIdx.x, model = blockIdx.y, p = blockIdx.z, lane = threadIdx.x;
    if (!((models >> model) & 1)) return;
    const Layout lay = layout_of(P, T);
    const auto [off, n] = problem_span(block, lay.offsets, p);
    if (n < 8) return;   // rule 7: invalid, k_twoview_finish says so
    const double* x1 = reinterpret_cast<const double*>(block + lay.x1) + 2 * (size_t)off;
    const double* x2 = reinterpret_cast<const double*>(block + lay.x2) + 2 * (size_t)off;
    if (lane == 0) {
        uint32_t i[8];
        sample_distinct<8, kSampleShare>(seed, (uint32_t)p, (uint32_t)h, (uint32_t)n, i);   // rule 2: one set for both models
#pragma unroll
        for (int k = 0; k < 8; ++k) idx[k] = (int32_t)i[k];
    }
    __syncthreads();
    double* slot = wave_models + slot_at((size_t)p * 2 + model, max_iter, h);
    if (model == 0)
        hypothesis<0>(x1, x2, n, inv_sigma_sq, idx, e, lane, slot);
    else
        hypothesis<1>(x1, x2, n, inv_sigma_sq, idx, e, lane, slot);
}

// a model's state in the finish kernel; the same in every lane
struct Model {
    bool valid;
    double M[9], score;
    int count, best_iter;
};

// rule 7 of one model by the problem's wavefront: the winner of the score slots, its flags, its inliers by rank in `list`, its validity
template <int MODEL>
__device__ __forceinline__ void winner_of(const double* __restrict__ x1, const double* __restrict__ x2, int n, int p, int max_iter, bool requested,
                                          double inv_sigma_sq, const double* __restrict__ wave_models, int32_t* __restrict__ list,
                                          uint8_t* __restrict__ flags, int lane, Model& w) {
    w.valid = false;
    w.score = 0.0;
    w.count = 0;
    w.best_iter = -1;
    if (!(requested && n >= 8)) return;
    const double* slots = wave_models + slot_at((size_t)p * 2 + MODEL, max_iter, 0);
    best_slot(slots, max_iter, lane, w.best_iter);
    if (w.best_iter < 0) return;
    const double* md = slots + (size_t)w.best_iter * kSlotDoubles;   // the doubles the hypothesis kernel scored with
#pragma unroll
    for (int k = 0; k < 9; ++k) w.M[k] = md[k];
    score_wave<MODEL>(w.M, x1, x2, n, inv_sigma_sq, lane, flags, list, w.count, w.score);
    w.valid = w.score > 0.0 && w.count >= 8;
}

// rule 8's second half: the swept e as the refit's model, which replaces the winner's if every entry is finite
template <int MODEL>
__device__ __forceinline__ void refit_of(const Eig& e, const Norm& N1, const Norm& N2, const double* __restrict__ x1, const double* __restrict__ x2, int n,
                                         double inv_sigma_sq, uint8_t* __restrict__ flags, int lane, Model& w) {
    double M2[9];
    fit_finish<MODEL>(e, N1, N2, M2);
    if (!all_finite(M2)) return;
#pragma unroll
    for (int k = 0; k < 9; ++k) w.M[k] = M2[k];
    score_wave<MODEL>(w.M, x1, x2, n, inv_sigma_sq, lane, flags, nullptr, w.count, w.score);
    w.valid = w.score > 0.0 && w.count >= 8;
}

// a model's half of the problem's record; rule 7's invalid form where it is not valid
template <int MODEL>
__device__ __forceinline__ void write_model(Model& w, int n, uint8_t* __restrict__ flags, int lane, TwoViewRec* __restrict__ rec) {
    if (!w.valid) {
        invalid_form(flags, n, lane, w.M, w.score, w.count);
        w.best_iter = -1;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) rec->mat[MODEL][k] = w.M[k];
        rec->score[MODEL] = w.score;
        rec->valid[MODEL] = w.valid ? 1 : 0;
        rec->best_iter[MODEL] = w.best_iter;
        rec->num_inliers[MODEL] = w.count;
    }
}

__global__ __launch_bounds__(64) void k_twoview_finish(const uint8_t* __restrict__ block, int P, int T, int max_iter, int models, int recompute,
                                                       double inv_sigma_sq, const double* __restrict__ wave_models, int32_t* __restrict__ inlier_idx,
                                                       TwoViewRec* __restrict__ out, uint8_t* __restrict__ out_flags_h, uint8_t* __restrict__ out_flags_f) {
    __shared__ Eig e[2];   // H's and F's refit
    const Layout lay = layout_of(P, T);
    const int p = blockIdx.x, lane = threadIdx.x;
    const auto [off, n] = problem_span(block, lay.offsets, p);
    const double* x1 = reinterpret_cast<const double*>(block + lay.x1) + 2 * (size_t)off;
    const double* x2 = reinterpret_cast<const double*>(block + lay.x2) + 2 * (size_t)off;
    int32_t *list_h = inlier_idx + off, *list_f = inlier_idx + T + off;   // the handle's list holds both models' halves
    uint8_t *flags_h = out_flags_h + off, *flags_f = out_flags_f + off;
    Model h, f;
    winner_of<0>(x1, x2, n, p, max_iter, (models & 1) != 0, inv_sigma_sq, wave_models, list_h, flags_h, lane, h);
    winner_of<1>(x1, x2, n, p, max_iter, (models & 2) != 0, inv_sigma_sq, wave_models, list_f, flags_f, lane, f);
    const bool refit_h = recompute && h.valid, refit_f = recompute && f.valid;
    if (refit_h || refit_f) {   // rule 8: the two 9 x 9 problems are swept side by side, H's by lanes 0 .. 31 and F's by lanes 32 .. 63
        __syncthreads();        // the lists are complete
        const Norm N1 = normalise(x1, n, lane), N2 = normalise(x2, n, lane);
        if (refit_h) fit_accumulate<0>(x1, x2, list_h, h.count, N1, N2, e[0], lane);
        if (refit_f) fit_accumulate<1>(x1, x2, list_f, f.count, N1, N2, e[1], lane);
        const bool mine = lane < 32 ? refit_h : refit_f;
        Eig& own = e[lane < 32 ? 0 : 1];
        if (!mine)   // a matrix of zeros is swept without a rotation
            for (int i = lane & 31; i < 81; i += 32) own.A[i] = 0.0;
        __syncthreads();
        jacobi_lds<9, kSweeps>(own.A, own.V, lane & 31);
        if (refit_h) refit_of<0>(e[0], N1, N2, x1, x2, n, inv_sigma_sq, flags_h, lane, h);
        if (refit_f) refit_of<1>(e[1], N1, N2, x1, x2, n, inv_sigma_sq, flags_f, lane, f);
    }
    write_model<0>(h, n, flags_h, lane, out + p);
    write_model<1>(f, n, flags_f, lane, out + p);
    if (lane == 0) {   // rule 9
        int selected;
        if (models == 3) {
            const double rel = h.score / (h.score + f.score);
            selected = (h.valid && 0.40 < rel) ? 1 : f.valid ? 2 : 0;
        } else {
            selected = models == 1 ? (h.valid ? 1 : 0) : (f.valid ? 2 : 0);
        }
        out[p].selected = selected;
        out[p].pad = 0;
    }
}

}   // namespace

struct ovs_twoview : eight_point_handle {                 // its d_inlier_idx: [2][matches of the call], H's half and F's
    uint8_t *h_flags_f = nullptr, *m_flags_f = nullptr;   // F's flags; the scaffold's h_flags / m_flags hold H's
};

extern "C" {

ovs_status ovs_twoview_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_twoview** out) {
    const auto flags_f = [&](ovs_twoview* s) { return mapped_block(s->res, &s->h_flags_f, &s->m_flags_f, (size_t)max_total_matches); };
    return eight_point_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes, 2, sizeof(TwoViewRec), out, flags_f);
}

ovs_status ovs_twoview_destroy(ovs_twoview* s) { return batch_destroy(s); }

ovs_status ovs_twoview_solve_batch(ovs_twoview* s, int32_t n_problems, const int32_t* offsets, const double* x1, const double* x2, double sigma,
                                   int32_t max_num_iter, int32_t recompute, uint64_t seed, int32_t models, double* out_H_21, double* out_F_21,
                                   double* out_scores, int32_t* out_valid, int32_t* out_best_iter, int32_t* out_num_inliers, int32_t* out_selected,
                                   uint8_t* out_inlier_flags_H, uint8_t* out_inlier_flags_F) {
    const splan::twoview::Call call{s != nullptr, n_problems, offsets, x1, x2, sigma, max_num_iter, models, out_H_21, out_F_21, out_scores, out_valid,
                                    out_best_iter, out_num_inliers, out_selected, out_inlier_flags_H, out_inlier_flags_F};
    const splan::Checked checked = splan::twoview::check(call, caps_of(s));
    const Layout lay = layout_of(n_problems, checked.T);
    const double inv_sigma_sq = 1.0 / (sigma * sigma);
    const auto hypotheses = [&](hipStream_t st, int32_t T) {
        hipLaunchKernelGGL(k_twoview_hypotheses, dim3(max_num_iter, 2, n_problems), dim3(64), 0, st, s->d_block, n_problems, T, max_num_iter, models, seed,
                           inv_sigma_sq, s->d_records);
    };
    const auto finish = [&](hipStream_t st, int32_t T) {
        hipLaunchKernelGGL(k_twoview_finish, dim3(n_problems), dim3(64), 0, st, s->d_block, n_problems, T, max_num_iter, models, recompute ? 1 : 0,
                           inv_sigma_sq, s->d_records, s->d_inlier_idx, s->m_rec<TwoViewRec>(), s->m_flags, s->m_flags_f);
    };
    const auto collect = [&](int32_t T) {
        for (int32_t p = 0; p < n_problems; ++p) {
            const TwoViewRec& r = s->h_rec<TwoViewRec>()[p];
            std::memcpy(out_H_21 + 9 * (size_t)p, r.mat[0], sizeof(r.mat[0]));
            std::memcpy(out_F_21 + 9 * (size_t)p, r.mat[1], sizeof(r.mat[1]));
            for (int m = 0; m < 2; ++m) {
                out_scores[2 * (size_t)p + m] = r.score[m];
                out_valid[2 * (size_t)p + m] = r.valid[m];
                out_best_iter[2 * (size_t)p + m] = r.best_iter[m];
                out_num_inliers[2 * (size_t)p + m] = r.num_inliers[m];
            }
            out_selected[p] = r.selected;
        }
        if (T > 0) {
            std::memcpy(out_inlier_flags_H, s->h_flags, (size_t)T);
            std::memcpy(out_inlier_flags_F, s->h_flags_f, (size_t)T);
        }
    };
    return run_slots(s, checked, lay.bytes, n_problems, 2, max_num_iter, [&] { splan::twoview::stage(call, lay, s->h_block); }, hypotheses, finish, collect);
}

}   // extern "C"
