// ba_pcg.hip -- the reduced camera system of a GLOBAL bundle adjustment on the device: S x = g with S dense, symmetric, 6 n_free square, far
// beyond the 1024 unknowns ba_solve.hip's one-workgroup Cholesky stages. A block-Jacobi preconditioned conjugate gradient
// over all compute units, as plain launches on one stream:
//   k_pcg_init     a lane per block: the block's Cholesky factor (P1), x = 0, r = g, z = M^-1 r, the block's term of r.z
//   k_pcg_product  pass k, first half. A workgroup per block row, a wavefront per row of S. Every wavefront sums the blocks' terms of r.z
//                  for itself (P3) and takes the loop's decision from them (P4); the search direction p = z + beta p is formed on the fly
//                  from z and the previous p while the row of S streams by (P2), the block's owner stores its six entries into the OTHER
//                  of two p buffers, q's six entries and the block's term of p.q.
//   k_pcg_update   pass k, second half. A lane per block: every wavefront sums the terms of p.q for itself, alpha, x += alpha p,
//                  r -= alpha q, z = M^-1 r, the block's term of the next r.z.
//   k_pcg_finish   the solution replaces the right-hand side; FAILED goes into the caller's failure word.
// Two launches per iteration. No workgroup waits for another: what a launch reads was written by an earlier launch, and the words a launch
// both reads and writes (done, failed) are written with the one value every reader would have derived for itself. No atomics, no
// cooperative launch, no graph capture; the host queues pcgplan::chunk_passes passes, reads the done word and queues the next chunk, up to
// pass max_iter: the number of launches never depends on the data. S is only read.
#include <cstring>
#include <limits>
#include <vector>

#include "ba_internal.h"
#include "ba_pcg_internal.inc"
#include "ba_pcg_math.inc"
#include "ba_pcg_plan.inc"
#include "owned_internal.inc"

namespace ovs {

struct PcgDev {   // the arena's arrays as the kernels see them
    double *L, *x, *r, *z, *p[2], *q, *pq, *rz, *scal;
    int32_t* words;
};

// 3.10 rule 6 by one wavefront: lane j takes the items j, j + 64, ... from 0.0, then the butterfly (every lane ends with part[0]'s bits:
// at distance d lanes j and j ^ d add the same two values)
__device__ __forceinline__ double wave_tree_sum(const double* __restrict__ val, int n, int lane) {
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s = s + val[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    return s;
}

__global__ __launch_bounds__(pcgplan::kUpdateThreads) void k_pcg_init(const double* __restrict__ S, int pitch, const double* __restrict__ g, int nb,
                                                                     PcgDev d) {
    const int b = blockIdx.x * pcgplan::kUpdateThreads + threadIdx.x;
    if (b >= nb) return;
    double* const L = d.L + (size_t)pcgplan::kFactorDoubles * b;
    const bool ok = pcg::factor6(S, (size_t)pitch, b, L);
    double rb[6], zb[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        rb[c] = g[6 * b + c];
        d.x[6 * b + c] = 0.0;
        d.r[6 * b + c] = rb[c];
    }
    pcg::apply6(L, rb, zb);
#pragma unroll
    for (int c = 0; c < 6; ++c) d.z[6 * b + c] = zb[c];
    d.rz[b] = pcg::dot6(rb, zb);
    // a bad pivot: FAILED, and no pass does anything (every lane that finds one stores the same two values; the host cleared both words)
    if (!ok) {
        d.words[pcgplan::kWordFailed] = 1;
        d.words[pcgplan::kWordDone] = 1;
    }
}

__global__ __launch_bounds__(pcgplan::kProductThreads) void k_pcg_product(const double* __restrict__ S, int pitch, int n, int nb, int k, int max_iter,
                                                                         double tol, PcgDev d) {
    __shared__ double s_q[6];
    if (d.words[pcgplan::kWordDone]) return;   // (uniform over the grid in effect: see below)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x;
    const double dn = wave_tree_sum(d.rz, nb, lane);
    const double d0 = k == 0 ? dn : d.scal[pcgplan::kScalD0];
    if (!pcg::goes_on(dn, d0, tol, k, max_iter)) {
        // every wavefront of the grid finds the same; one records it. A workgroup that starts late may already read the done word as 1 above:
        // it would have come here.
        if (b == 0 && threadIdx.x == 0) {
            pcg::report(k, dn, d0, tol, d.scal + pcgplan::kScalInfo);
            d.words[pcgplan::kWordDone] = 1;
        }
        return;
    }
    const double beta = k == 0 ? 0.0 : dn / d.scal[pcgplan::kScalDn0 + ((k - 1) & 1)];
    const double* __restrict__ z = d.z;
    const double* __restrict__ p_old = d.p[(k & 1) ^ 1];
    const int row = 6 * b + w;
    const double* __restrict__ Srow = S + (size_t)row * pitch;
    double s = pcg::row_partial(Srow, n, lane, [&](int j) { return pcg::direction(k, z[j], beta, p_old[j]); });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    if (lane == 0) s_q[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double pb[6], qb[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            pb[c] = pcg::direction(k, z[6 * b + c], beta, p_old[6 * b + c]);
            qb[c] = s_q[c];
            d.p[k & 1][6 * b + c] = pb[c];
            d.q[6 * b + c] = qb[c];
        }
        d.pq[b] = pcg::dot6(pb, qb);
        if (b == 0) {
            d.scal[pcgplan::kScalDn0 + (k & 1)] = dn;
            if (k == 0) d.scal[pcgplan::kScalD0] = dn;
        }
    }
}

__global__ __launch_bounds__(pcgplan::kUpdateThreads) void k_pcg_update(int nb, int k, PcgDev d) {
    if (d.words[pcgplan::kWordDone]) return;   // set by this pass's k_pcg_product at the latest, or below with what every wavefront finds
    const int lane = threadIdx.x & 63, b = blockIdx.x * pcgplan::kUpdateThreads + threadIdx.x;
    const double pq = wave_tree_sum(d.pq, nb, lane);
    if (!pcg::curvature_ok(pq)) {
        if (b == 0) {
            d.words[pcgplan::kWordFailed] = 1;
            d.words[pcgplan::kWordDone] = 1;
        }
        return;
    }
    if (b >= nb) return;
    const double alpha = d.scal[pcgplan::kScalDn0 + (k & 1)] / pq;
    const double* __restrict__ p = d.p[k & 1];
    double rb[6], zb[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        d.x[6 * b + c] = d.x[6 * b + c] + alpha * p[6 * b + c];
        rb[c] = d.r[6 * b + c] - alpha * d.q[6 * b + c];
        d.r[6 * b + c] = rb[c];
    }
    pcg::apply6(d.L + (size_t)pcgplan::kFactorDoubles * b, rb, zb);
#pragma unroll
    for (int c = 0; c < 6; ++c) d.z[6 * b + c] = zb[c];
    d.rz[b] = pcg::dot6(rb, zb);   // (read by the NEXT launch only: k_pcg_product(k + 1))
}

__global__ __launch_bounds__(pcgplan::kUpdateThreads) void k_pcg_finish(int n, PcgDev d, double* __restrict__ rhs, int32_t* __restrict__ fail) {
    const int i = blockIdx.x * pcgplan::kUpdateThreads + threadIdx.x;
    if (i < n) rhs[i] = d.x[i];
    if (i == 0 && d.words[pcgplan::kWordFailed]) *fail = 2;   // (launch_dense_solve's value for "not positive definite")
}

static PcgDev carve(unsigned char* A, const pcgplan::Plan& P) {
    PcgDev d;
    d.L = ArenaLayout::at<double>(A, P.o_L);
    d.x = ArenaLayout::at<double>(A, P.o_x);
    d.r = ArenaLayout::at<double>(A, P.o_r);
    d.z = ArenaLayout::at<double>(A, P.o_z);
    d.p[0] = ArenaLayout::at<double>(A, P.o_p0);
    d.p[1] = ArenaLayout::at<double>(A, P.o_p1);
    d.q = ArenaLayout::at<double>(A, P.o_q);
    d.pq = ArenaLayout::at<double>(A, P.o_pq);
    d.rz = ArenaLayout::at<double>(A, P.o_rz);
    d.scal = ArenaLayout::at<double>(A, P.o_scal);
    d.words = ArenaLayout::at<int32_t>(A, P.o_words);
    return d;
}

int pcg_max_free() { return pcgplan::kMaxFree; }
size_t pcg_arena_bytes() { return pcgplan::arena_bytes_max(); }

// Contract as for launch_dense_solve: d_S is the system ba_graph_schur leaves (both triangles, `pitch` doubles per row, padding columns not
// read), the solution replaces d_rhs, FAILED (rule P5) ORs into *d_fail through k_pcg_finish's store of 2. S is only read: a failed solve
// leaves the system intact. d_arena: pcg_arena_bytes() of device memory; h_pin: page-locked, PcgHostBlock. Unlike launch_dense_solve the call
// WAITS for the stream every check_every passes (4 bytes come down) and once at the end (the three info doubles).
ovs_status launch_pcg_solve(const double* d_S, int pitch, double* d_rhs, int n, int32_t* d_fail, unsigned char* d_arena, PcgHostBlock* h_pin, double tol,
                            int max_iter, int check_every, hipStream_t s, PcgResult* out) {
    pcgplan::Plan P;
    const ovs_status ps = pcgplan::plan_of(n, tol, max_iter, check_every, &P);
    if (ps != OVS_OK) return ps;
    if (!d_S || !d_rhs || !d_fail || !d_arena || !h_pin || pitch < n) return OVS_ERR_INVALID;
    const PcgDev d = carve(d_arena, P);
    OVS_HIP_TRY(hipMemsetAsync(d.scal, 0, P.arena_bytes - P.o_scal, s));   // the scalars and, behind them, the words
    hipLaunchKernelGGL(k_pcg_init, dim3(P.grid_update), dim3(pcgplan::kUpdateThreads), 0, s, d_S, pitch, (const double*)d_rhs, P.n_blocks, d);
    OVS_LAUNCH_TRY("k_pcg_init");
    for (int first = 0;;) {
        const int count = pcgplan::chunk_passes(P, first);
        if (count == 0) break;
        for (int k = first; k < first + count; ++k) {
            hipLaunchKernelGGL(k_pcg_product, dim3(P.grid_product), dim3(pcgplan::kProductThreads), 0, s, d_S, pitch, P.n, P.n_blocks, k, P.max_iter, tol, d);
            OVS_LAUNCH_TRY("k_pcg_product");
            hipLaunchKernelGGL(k_pcg_update, dim3(P.grid_update), dim3(pcgplan::kUpdateThreads), 0, s, P.n_blocks, k, d);
            OVS_LAUNCH_TRY("k_pcg_update");
        }
        first += count;
        h_pin->done = 0;
        OVS_HIP_TRY(hipMemcpyAsync(&h_pin->done, d.words + pcgplan::kWordDone, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        OVS_HIP_TRY(hipStreamSynchronize(s));
        if (h_pin->done) break;
    }
    hipLaunchKernelGGL(k_pcg_finish, dim3((P.n + pcgplan::kUpdateThreads - 1) / pcgplan::kUpdateThreads), dim3(pcgplan::kUpdateThreads), 0, s, P.n, d, d_rhs,
                       d_fail);
    OVS_LAUNCH_TRY("k_pcg_finish");
    OVS_HIP_TRY(hipMemcpyAsync(h_pin->info, d.scal + pcgplan::kScalInfo, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipMemcpyAsync(&h_pin->failed, d.words + pcgplan::kWordFailed, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    if (out) {
        out->failed = h_pin->failed != 0;
        out->iterations = out->failed ? 0 : (int)h_pin->info[0];
        out->capped = !out->failed && h_pin->info[1] != 0.0;
        out->ratio = out->failed ? 0.0 : h_pin->info[2];
    }
    return OVS_OK;
}

}   // namespace ovs

extern "C" {

// the solver alone, on host arrays (a test entry, like ovs_ba_dense_solve). S: n x n row-major, both triangles. info: 3 doubles or null.
ovs_status ovs_ba_pcg_solve(int32_t device, const double* S, const double* rhs, int32_t n, double tol, int32_t max_iter, int32_t check_every, double* x,
                            double* info) {
    if (!S || !rhs || !x) return OVS_ERR_INVALID;
    pcgplan::Plan P;
    const ovs_status ps = pcgplan::plan_of(n, tol, max_iter, check_every, &P);   // (before the device and any allocation)
    if (ps != OVS_OK) return ps;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    const int pitch = ovs::dense_solve_pad(n);
    // the graph's layout: S with its row padding, then the right-hand side's row. What the kernels must not read -- the padding columns of
    // every row, the rows between n and pitch, the padding behind the right-hand side -- holds a quiet NaN, as it may in the real call (which
    // is why ba_graph_reset_system exists): one such value in a sum and no test of the solver's bits passes.
    std::vector<double> h((size_t)(pitch + 1) * pitch, std::numeric_limits<double>::quiet_NaN());
    for (int i = 0; i < n; ++i) std::memcpy(&h[(size_t)i * pitch], S + (size_t)i * n, sizeof(double) * n);
    std::memcpy(&h[(size_t)pitch * pitch], rhs, sizeof(double) * n);
    ovs::Owned tmp;
    double* d_sys = nullptr;
    unsigned char* d_arena = nullptr;
    ovs::PcgHostBlock* h_pin = nullptr;
    hipStream_t s = nullptr;
    const size_t bytes = sizeof(double) * h.size();
    OVS_HIP_TRY(tmp.dev(&d_sys, bytes + 256));
    OVS_HIP_TRY(tmp.dev(&d_arena, ovs::pcg_arena_bytes()));
    OVS_HIP_TRY(tmp.pinned(&h_pin, sizeof(ovs::PcgHostBlock)));
    OVS_HIP_TRY(tmp.stream(&s));
    int32_t* const d_fail = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(d_sys) + bytes);
    OVS_HIP_TRY(hipMemcpyAsync(d_sys, h.data(), bytes, hipMemcpyHostToDevice, s));
    OVS_HIP_TRY(hipMemsetAsync(d_fail, 0, 256, s));
    ovs::PcgResult res;
    const ovs_status st = ovs::launch_pcg_solve(d_sys, pitch, d_sys + (size_t)pitch * pitch, n, d_fail, d_arena, h_pin, tol, max_iter, check_every, s, &res);
    if (st != OVS_OK) {
        (void)hipStreamSynchronize(s);   // (h is read by the upload)
        return st;
    }
    int32_t h_fail = 0;
    OVS_HIP_TRY(hipMemcpyAsync(x, d_sys + (size_t)pitch * pitch, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipMemcpyAsync(&h_fail, d_fail, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    if (h_fail || res.failed) {
        ovs::set_last_error_text("ovs_ba_pcg_solve: a diagonal block is not positive definite, or p.q is not positive and finite");
        return OVS_ERR_INVALID;
    }
    if (info) {
        info[0] = res.iterations;
        info[1] = res.capped ? 1.0 : 0.0;
        info[2] = res.ratio;
    }
    return OVS_OK;
}

int32_t ovs_ba_pcg_max_free(void) { return pcgplan::kMaxFree; }

}   // extern "C"
