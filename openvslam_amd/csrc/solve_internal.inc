// solve_internal.inc -- what the batch solvers share: the RANSACs of solve/ (sim3_solve.hip, pnp_solve.hip, and through
// eight_point_internal.inc two_view_solve.hip and essential_solve.hip), the Sim3 transform optimiser (sim3_opt.hip), the pose recovery
// (two_view_reconstruct.hip), the triangulator (triangulate.hip) and the landmark upkeep (landmark_update.hip). On the device: the
// counter-based sampler, the hypothesis key, the result record and its invalid form, the cyclic Jacobi rotation (jacobi_math.inc), its
// sweeps over a matrix in LDS, the wavefront's sum (wave_sum) and Horn's quaternion form of the absolute orientation. DESIGN.md 3.9 rule 2
// fixes every operation; the units are built with -ffp-contract=off. On the host: batch_handle (one staged block and its page-locked
// twin, a stream, grow-only records, and for the solvers that have them the mapped result and flags blocks), batch_create, and
// run_staged: what the solver's plan checked (solve_plan.inc holds every host decision of a call: errors, capacity, layout, staging,
// read-back), lock, stage, reserve, one upload, launch, synchronise, collect. run_batch is run_staged with the two launches, the keys and
// the result record of Sim3 and EPnP; the eight-point solvers' score-slot form of it is run_slots of eight_point_internal.inc; the
// one-launch solvers call run_staged themselves. (An .inc, not an .h: bench.py fingerprints every .h of this directory into the committed
// counters of the extractor and matcher stages, which include none of this.)
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>

#include <hip/hip_runtime.h>

#include "essential_math.inc"
#include "jacobi_math.inc"
#include "ovs_common.h"
#include "owned_internal.inc"
#include "solve_plan.inc"

namespace {

using splan::kMaxIter;   // h takes 20 bits of the sampler's counter

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// rule 1: K distinct indices below n (n >= K), no rejection loop. Draw k is below n - k and steps over the earlier indices in ascending
// order; `sorted` holds them by compare-exchange on compile-time indices (no local array is indexed dynamically: no scratch). STRIDE is the
// solver's share of the counter per hypothesis (4 for Sim3, 8 for EPnP: solve.problem_seed, solve.pnp_problem_seed).
template <int K, int STRIDE>
__device__ __forceinline__ void sample_distinct(uint64_t seed, uint32_t p, uint32_t h, uint32_t n, uint32_t (&idx)[K]) {
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    const uint64_t base = seed + G * (((((uint64_t)p) << 20) + h) * STRIDE + 1);
    uint32_t sorted[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint32_t v = (uint32_t)(mix64(base + G * k) % (n - k));
#pragma unroll
        for (int j = 0; j < k; ++j)
            if (v >= sorted[j]) ++v;
        idx[k] = v;
#pragma unroll
        for (int j = 0; j < k; ++j) {
            const uint32_t lo = min(sorted[j], v);
            v = max(sorted[j], v);
            sorted[j] = lo;
        }
        sorted[k] = v;
    }
}

// a hypothesis's key: the largest count wins an integer atomicMax, the lowest h on a tie; never 0 for a hypothesis
__device__ __forceinline__ unsigned long long hypothesis_key(int count, uint32_t h) {
    return ((unsigned long long)(uint32_t)count << 32) | (unsigned long long)(0xFFFFFFFFu - h);
}
__device__ __forceinline__ int key_count(unsigned long long key) { return (int)(key >> 32); }
__device__ __forceinline__ uint32_t key_iter(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }

// problem p's first match and number of matches, from the offsets section i32 [P + 1] of the staged block
struct Span {
    int off, n;
};
__device__ __forceinline__ Span problem_span(const uint8_t* __restrict__ block, size_t offsets_at, int p) {
    const int32_t* offsets = reinterpret_cast<const int32_t*>(block + offsets_at);
    const int off = offsets[p];
    return {off, offsets[p + 1] - off};
}

// per problem in the result block; a solver without a scale leaves it at 1.0
struct ResultRec {
    double rot[9], trans[3], scale;
    int32_t valid, best_iter, num_inliers, pad;
};
static_assert(sizeof(ResultRec) == 120, "ResultRec is read by the host");

// rule 4's invalid output, by the finish kernel's whole workgroup of `threads`: the problem's flags zeroed, the record by thread 0
__device__ __forceinline__ void write_invalid(uint8_t* __restrict__ flags, int n, int threads, ResultRec* __restrict__ out) {
    for (int i = threadIdx.x; i < n; i += threads) flags[i] = 0;
    if (threadIdx.x == 0) {
        ResultRec r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.rot[k] = (k % 4 == 0) ? 1.0 : 0.0;
        r.trans[0] = r.trans[1] = r.trans[2] = 0.0;
        r.scale = 1.0;
        r.valid = 0;
        r.best_iter = -1;
        r.num_inliers = 0;
        r.pad = 0;
        *out = r;
    }
}

// the cyclic Jacobi rotation (jacobi_math.inc: shared with triangulate_math.inc, which a plain host compiler builds too)
using ovs_jacobi::jacobi_angle;
using ovs_jacobi::jacobi_rotate;

// the cyclic Jacobi iteration by one wavefront on an N x N matrix A and its vectors V in LDS (row-major, N <= 16): row-major pair order,
// SWEEPS sweeps, the rotation of jacobi_rotate. Lane k < N rotates column pair k, then row pair k; lane 16 + k the vectors' pair k (which no entry of A
// depends on). `lane` is the lane's number among the 32 that share A and V: the halves of a wavefront may sweep two matrices side by side.
template <int N, int SWEEPS>
__device__ __forceinline__ void jacobi_lds(double* A, double* V, int lane) {
#pragma unroll 1
    for (int sweep = 0; sweep < SWEEPS; ++sweep)
#pragma unroll 1
        for (int p = 0; p < N - 1; ++p)
#pragma unroll 1
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                const bool rot = apq != 0.0;   // the same in every lane of one matrix
                double c = 1.0, s = 0.0;
                if (rot) jacobi_angle(A[p * N + p], A[q * N + q], apq, c, s);
                if (rot && lane < N) {
                    const double akp = A[lane * N + p], akq = A[lane * N + q];
                    A[lane * N + p] = c * akp - s * akq;
                    A[lane * N + q] = s * akp + c * akq;
                } else if (rot && lane >= 16 && lane < 16 + N) {
                    const int k = lane - 16;
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
                __syncthreads();
                if (rot && lane < N) {
                    const double apk = A[p * N + lane], aqk = A[q * N + lane];
                    A[p * N + lane] = c * apk - s * aqk;
                    A[q * N + lane] = s * apk + c * aqk;
                }
                __syncthreads();
            }
}

// the same iteration in the parallel ordering of DESIGN.md 3.16 rule E3 (essential_math.inc's round_pair): a sweep is N rounds of (N - 1) / 2
// disjoint pairs, so a round's rotations, its column updates and its row updates are each independent lane work: N dependent steps a sweep
// in place of N (N - 1) / 2. Sixteen lanes serve a pair, all computing its rotation from the matrix as the round finds it: lane i < N of the
// sixteen rotates row i of the pair's columns, then (after a barrier) column i of its rows; lanes N .. 15 rotate the vectors' rows
// 0 .. 15 - N beside the columns and the rest beside the rows. A pair whose entry is 0.0 does not rotate. Precondition: the 64 lanes are ONE
// wavefront. A round reads its pairs' three entries and then writes their columns with no barrier in between, which is right only because a
// wavefront's LDS operations execute in program order (jacobi_lds above rests on the same); a workgroup of several wavefronts sharing A
// would need a barrier after the reads.
template <int N, int SWEEPS>
__device__ __forceinline__ void jacobi_lds_rounds(double* A, double* V, int lane) {
    static_assert(N == ess::kRounds && (N - 1) / 2 == ess::kRoundPairs && 2 * (16 - N) >= N, "the lane layout is that of the 9 x 9 problem");
    const int k = (lane >> 4) + 1, i = lane & 15;
#pragma unroll 1
    for (int sweep = 0; sweep < SWEEPS; ++sweep)
#pragma unroll 1
        for (int r = 0; r < N; ++r) {
            int p, q;
            ess::round_pair(r, k, p, q);
            const double apq = A[p * N + q];
            const bool rot = apq != 0.0;   // the same in the sixteen lanes of a pair
            double c = 1.0, s = 0.0;
            if (rot) jacobi_angle(A[p * N + p], A[q * N + q], apq, c, s);
            if (rot) {
                double* M = i < N ? A + i * N : V + (i - N) * N;
                const double mp = M[p], mq = M[q];
                M[p] = c * mp - s * mq;
                M[q] = s * mp + c * mq;
            }
            __syncthreads();
            if (rot && i < N) {
                const double apk = A[p * N + i], aqk = A[q * N + i];
                A[p * N + i] = c * apk - s * aqk;
                A[q * N + i] = s * apk + c * aqk;
            } else if (rot && i < 3 * N - 16) {   // the vectors' rows 16 - N .. N - 1
                double* M = V + (i + 16 - 2 * N) * N;
                const double mp = M[p], mq = M[q];
                M[p] = c * mp - s * mq;
                M[q] = s * mp + c * mq;
            }
            __syncthreads();
        }
}

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// the tree of 3.10 rule 6 over a wavefront: lane 0's value is ((p0 + p32) + (p16 + p48)) + ... ; as IEEE addition commutes every lane
// ends with the same bits
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x = x + __shfl_xor(x, d);
    return x;
}

// Horn's closed form with the scale left out: M[r][c] = sum over the centred pairs of b[r] * a[c]; R (row-major) is the rotation with
// a = R b in the least-squares sense. Eight cyclic sweeps over the 4 x 4 matrix, the eigenvector of the largest diagonal entry (lowest
// index on a tie; selects, not an indexed read), normalised.
__device__ __forceinline__ void horn_rotation(const double (&M)[3][3], double (&R)[9]) {
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[0][1] = M[1][2] - M[2][1];
    A[0][2] = M[2][0] - M[0][2];
    A[0][3] = M[0][1] - M[1][0];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[1][2] = M[0][1] + M[1][0];
    A[1][3] = M[2][0] + M[0][2];
    A[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    A[2][3] = M[1][2] + M[2][1];
    A[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < r) A[r][c] = A[c][r];
            V[r][c] = r == c ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < 8; ++sweep) {
        jacobi_rotate<4, 0, 1>(A, V);
        jacobi_rotate<4, 0, 2>(A, V);
        jacobi_rotate<4, 0, 3>(A, V);
        jacobi_rotate<4, 1, 2>(A, V);
        jacobi_rotate<4, 1, 3>(A, V);
        jacobi_rotate<4, 2, 3>(A, V);
    }
    double best = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const bool take = A[i][i] > best;
        best = take ? A[i][i] : best;
        q0 = take ? V[0][i] : q0;
        q1 = take ? V[1][i] : q1;
        q2 = take ? V[2][i] : q2;
        q3 = take ? V[3][i] : q3;
    }
    const double nrm = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double w = q0 / nrm, x = q1 / nrm, y = q2 / nrm, z = q3 / nrm;
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// ---- the host side: one handle, one create and one batch call under the nine C-ABI families of solve_plan.inc
struct batch_handle {
    int device = 0;
    int max_problems = 0, max_total_matches = 0;   // fixed at create: a plan's check reads them without the lock
    std::mutex mu;
    ovs::Owned res;
    hipStream_t stream = nullptr;
    uint8_t *d_block = nullptr, *h_block = nullptr;   // the staged block (the solver's Layout) and its page-locked twin
    // device memory in records of record_doubles doubles, grow-only: a wave's best model per (problem, wave), a score slot per (problem slot,
    // hypothesis), a match's keys; what a call needs of it depends on its arguments
    double* d_records = nullptr;
    size_t records_cap = 0;
    int record_doubles = 0;
    // results, page-locked and mapped: the finish kernel writes them, the host reads them after the stream has drained. The result block is
    // the solver's record per problem; a solver whose results come back through the staged block has neither
    uint8_t *h_result = nullptr, *m_result = nullptr;
    uint8_t *h_flags = nullptr, *m_flags = nullptr;

    // the result block as the solver's record type, on the host and as the kernels address it
    template <class Rec>
    Rec* h_rec() { return reinterpret_cast<Rec*>(h_result); }
    template <class Rec>
    Rec* m_rec() { return reinterpret_cast<Rec*>(m_result); }
    // the records as the kernels' element type
    template <class T>
    T* records_as() { return reinterpret_cast<T*>(d_records); }

    // room for `records` records; the stream is idle: every call ends in a synchronise
    ovs_status reserve(size_t records) {
        if (records <= records_cap) return OVS_OK;
        records_cap = 0;
        if (d_records) OVS_HIP_TRY(res.drop(&d_records));
        OVS_HIP_TRY(res.dev(&d_records, sizeof(double) * record_doubles * records));
        records_cap = records;
        return OVS_OK;
    }
};

// a handle's limits for its plan's check, read when the check asks for them: after the argument errors that need no handle
inline auto caps_of(const batch_handle* s) {
    return [s] { return splan::Caps{s->max_problems, s->max_total_matches, 0, s->device}; };
}

// page-locked memory the kernels write through `*mapped`
template <class T>
ovs_status mapped_block(ovs::Owned& res, T** host, T** mapped, size_t bytes) {
    OVS_HIP_TRY(res.pinned(host, bytes, hipHostMallocMapped));
    OVS_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(mapped), *host, 0));
    return OVS_OK;
}

// The one create. H: the solver's handle. block_bytes: its Layout at full capacity; initial_records of record_doubles: the records that fit
// without growing; result_bytes: its record per problem in the mapped result block, 0 for a solver that reads its results from the staged
// block (it gets no result and no flags block); extra(handle) acquires what the solver's handle adds, under the same owner.
template <class H, class Extra>
ovs_status batch_create(int32_t device, int32_t max_problems, int32_t max_total_matches, size_t block_bytes, size_t initial_records, int record_doubles,
                        size_t result_bytes, H** out, Extra extra) {
    if (!out || max_problems < 1 || max_total_matches < 1) return OVS_ERR_INVALID;
    *out = nullptr;
    if (max_problems > 65535) return OVS_ERR_INVALID;   // a grid's y extent
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<H> owner(new H());
    H* const s = owner.get();
    s->device = device;
    s->max_problems = max_problems;
    s->max_total_matches = max_total_matches;
    s->record_doubles = record_doubles;
    OVS_HIP_TRY(s->res.stream(&s->stream));
    OVS_HIP_TRY(s->res.dev(&s->d_block, block_bytes));
    if (s->reserve(initial_records) != OVS_OK) return OVS_ERR_HIP;
    OVS_HIP_TRY(s->res.pinned(&s->h_block, block_bytes));
    if (result_bytes > 0) {
        if (mapped_block(s->res, &s->h_result, &s->m_result, result_bytes * (size_t)max_problems) != OVS_OK) return OVS_ERR_HIP;
        if (mapped_block(s->res, &s->h_flags, &s->m_flags, (size_t)max_total_matches) != OVS_OK) return OVS_ERR_HIP;
    }
    const ovs_status added = extra(s);
    if (added != OVS_OK) return added;
    *out = owner.release();
    return OVS_OK;
}
inline ovs_status no_extra(batch_handle*) { return OVS_OK; }

template <class H>
ovs_status batch_destroy(H* s) {
    if (!s) return OVS_ERR_INVALID;
    hipSetDevice(s->device);
    delete s;
    return OVS_OK;
}

// where a call's results go: the caller's arrays of the C ABI (scale: nullptr for a solver that has none)
struct BatchOut {
    int32_t *valid, *best_iter, *num_inliers;
    double *rot, *trans, *scale;
    uint8_t* flags;
};

// One batch call of any solver of this file's shape, whatever it launches. `checked`: what the solver's plan (solve_plan.inc: check) made of
// the call's arguments, capacity included, before anything is touched; upload_bytes: its Layout's bytes. stage() fills the page-locked block
// (the plan's stage); reserve() grows what the launch needs while the stream is idle; launch(stream, T) enqueues the solver's kernels
// behind the block's upload; collect(T) copies the results out after the stream has drained. No output is touched on any error.
template <class Stage, class Reserve, class Launch, class Collect>
ovs_status run_staged(batch_handle* s, const splan::Checked& checked, size_t upload_bytes, Stage stage, Reserve reserve, Launch launch, Collect collect) {
    if (!checked.run) return checked.status;
    std::lock_guard<std::mutex> lock(s->mu);
    stage();
    OVS_HIP_TRY(hipSetDevice(s->device));
    const ovs_status reserved = reserve();
    if (reserved != OVS_OK) return reserved;
    OVS_HIP_TRY(hipMemcpyAsync(s->d_block, s->h_block, upload_bytes, hipMemcpyHostToDevice, s->stream));
    const ovs_status launched = launch(s->stream, checked.T);
    if (launched != OVS_OK) return launched;
    OVS_HIP_TRY(hipStreamSynchronize(s->stream));
    collect(checked.T);
    return OVS_OK;
}
inline ovs_status nothing_to_reserve() { return OVS_OK; }

// One solve_batch call of a RANSAC solver: run_staged with the two launches, the keys and the result record both solvers have.
// hypotheses(stream, waves_per_problem, T) and finish(stream, waves_per_problem, T) launch the solver's two kernels.
template <class Stage, class Hypotheses, class Finish>
ovs_status run_batch(batch_handle* s, const splan::Checked& checked, size_t upload_bytes, int32_t n_problems, int32_t max_num_iter, int hyp_per_wave,
                     const BatchOut& o, Stage stage, Hypotheses hypotheses, Finish finish) {
    const int waves = checked.run ? (max_num_iter + hyp_per_wave - 1) / hyp_per_wave : 0;   // (a refused max_num_iter is not computed with)
    return run_staged(
        s, checked, upload_bytes, stage, [&] { return s->reserve((size_t)n_problems * (size_t)waves) != OVS_OK ? OVS_ERR_HIP : OVS_OK; },
        [&](hipStream_t stream, int32_t T) {
            hypotheses(stream, waves, T);
            OVS_HIP_TRY(hipGetLastError());
            finish(stream, waves, T);
            OVS_HIP_TRY(hipGetLastError());
            return OVS_OK;
        },
        [&](int32_t T) {
            for (int32_t p = 0; p < n_problems; ++p) {
                const ResultRec& r = s->h_rec<ResultRec>()[p];
                o.valid[p] = r.valid;
                o.best_iter[p] = r.best_iter;
                o.num_inliers[p] = r.num_inliers;
                std::memcpy(o.rot + 9 * (size_t)p, r.rot, sizeof(r.rot));
                std::memcpy(o.trans + 3 * (size_t)p, r.trans, sizeof(r.trans));
                if (o.scale) o.scale[p] = r.scale;
            }
            if (T > 0) std::memcpy(o.flags, s->h_flags, (size_t)T);
        });
}

}   // namespace
