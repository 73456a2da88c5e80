// ba_pcg_plan.inc -- everything the host side of the reduced camera system's conjugate-gradient solver (ba_pcg.hip, DESIGN.md 3.20 rule P7)
// decides with integers before a launch: the largest system a call accepts, the grids of the three kernels, the iteration cap, how the
// host deals the iterations into chunks, and the order and offsets of the arrays in the solver's arena. Plain host C++, no HIP: ba_pcg.hip
// includes it, tests/ba_pcg_host.cc builds it with the host compiler alone under the sanitizers. This is the one place these are computed.
// (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/ovslam_hip.h"

namespace pcgplan {

constexpr int kBlock = 6;               // unknowns per keyframe
constexpr int kMaxFree = 1024;          // free keyframes a call accepts: 6144 unknowns, a dense S of 302 MB; every index stays far below 2^31
constexpr int kFactorDoubles = 36;      // a diagonal block's Cholesky factor, row-major 6 x 6 (the lower triangle is written and read)
constexpr int kProductThreads = 64 * kBlock;   // k_pcg_product: a workgroup per block row, a wavefront per row of S
constexpr int kUpdateThreads = 256;     // k_pcg_init, k_pcg_update, k_pcg_finish: a lane per block
constexpr int kDefaultCheckEvery = 16;  // iterations queued between two looks at the done word

// One allocation, many arrays: offsets in placement order, each 256-byte aligned; an empty array still takes a byte.
struct Placer {
    size_t top = 0;
    size_t place(size_t elem_bytes, size_t count) {
        const size_t off = bytes();
        top = off + std::max<size_t>(elem_bytes * count, 1);
        return off;
    }
    size_t bytes() const { return (top + 255) & ~(size_t)255; }
};

struct Plan {
    int n, n_blocks;          // unknowns, blocks
    int max_iter;             // the cap in force (rule P4: 0 asked for means 12 per block)
    int check_every;          // the chunk in force
    int grid_product;         // workgroups of k_pcg_product: one per block
    int grid_update;          // workgroups of the lane-per-block kernels
    // the arena: the factors, the vectors (p twice: rule P6), the per-block terms of p.q and of r.z, the scalars and words
    size_t o_L, o_x, o_r, o_z, o_p0, o_p1, o_q, o_pq, o_rz, o_scal, o_words;
    size_t arena_bytes;
};

// device scalars (doubles at o_scal): dn by iteration parity, d0, and the info triple
constexpr int kScalDn0 = 0, kScalDn1 = 1, kScalD0 = 2, kScalInfo = 4, kScalDoubles = 16;
// device words (int32 at o_words)
constexpr int kWordDone = 0, kWordFailed = 1, kWords = 16;

// OVS_ERR_INVALID: n is no positive multiple of 6, a negative cap or chunk, a tolerance that is not in (0, 1) (a NaN included);
// OVS_ERR_CAPACITY: more than kMaxFree blocks. Nothing is allocated before this has passed.
inline ovs_status plan_of(int64_t n, double tol, int64_t max_iter, int64_t check_every, Plan* out) {
    if (n < kBlock || n % kBlock != 0 || max_iter < 0 || check_every < 0 || !(tol > 0.0 && tol < 1.0)) return OVS_ERR_INVALID;
    if (n / kBlock > kMaxFree) return OVS_ERR_CAPACITY;
    if (max_iter > (int64_t)1 << 24 || check_every > (int64_t)1 << 24) return OVS_ERR_INVALID;
    Plan p;
    p.n = (int)n;
    p.n_blocks = (int)(n / kBlock);
    p.max_iter = max_iter == 0 ? 12 * p.n_blocks : (int)max_iter;
    p.check_every = check_every == 0 ? kDefaultCheckEvery : (int)check_every;
    p.grid_product = p.n_blocks;
    p.grid_update = (p.n_blocks + kUpdateThreads - 1) / kUpdateThreads;
    Placer a;
    const size_t nb = (size_t)p.n_blocks, nn = (size_t)p.n;
    p.o_L = a.place(8, kFactorDoubles * nb);
    p.o_x = a.place(8, nn);
    p.o_r = a.place(8, nn);
    p.o_z = a.place(8, nn);
    p.o_p0 = a.place(8, nn);
    p.o_p1 = a.place(8, nn);
    p.o_q = a.place(8, nn);
    p.o_pq = a.place(8, nb);
    p.o_rz = a.place(8, nb);
    p.o_scal = a.place(8, kScalDoubles);
    p.o_words = a.place(4, kWords);
    p.arena_bytes = a.bytes();
    *out = p;
    return OVS_OK;
}

// the arena of the largest system: what a graph reserves once, whatever its size (0.6 MB)
inline size_t arena_bytes_max() {
    Plan p;
    (void)plan_of((int64_t)kBlock * kMaxFree, 0.5, 0, 0, &p);
    return p.arena_bytes;
}

// The host queues the passes k = first .. first + count - 1 of a chunk (pass k = the convergence test of iteration k, then iteration k), reads
// the done word and goes on. Pass max_iter only records that the cap was met. Returns the number of passes of the chunk that starts at
// `first` (0: nothing is left).
inline int chunk_passes(const Plan& p, int first) {
    const int last = p.max_iter;   // inclusive
    if (first > last) return 0;
    return std::min(p.check_every, last - first + 1);
}

}   // namespace pcgplan
