// pose_graph.hip -- optimize::graph_optimizer (expected: src/openvslam/optimize/graph_optimizer.{h,cc}): the Sim3 pose-graph optimisation over
// the essential graph after an accepted loop, and the landmark write-back. Rules: DESIGN.md 3.19 (G1 to G11); the algebra is
// pose_graph_math.inc, which a plain host compiler builds too; what the host decides with integers is pose_graph_plan.inc. Everything is f64,
// every operation rounded on its own (the unit is built with -ffp-contract=off).
//
// k_posegraph_optimize: ONE workgroup of 256 lanes (four wavefronts, one per SIMD, so a lane may take the whole register file's 512) runs the
// whole Levenberg-Marquardt: a lane per edge linearises in a strided loop (29 evaluations of log(M S_i S_j^-1), the perturbed states of its
// two vertices in registers), a lane per entry assembles the vertices' diagonal blocks and the edges' off-diagonal blocks, a lane per vertex
// runs the phases of the block-Jacobi PCG, and __syncthreads separates the phases. The blocks, the vectors and the trial copy of the
// vertices live in the handle's arena; LDS holds two doubles, the slots rule 6's sums are broadcast through. Such a sum is formed by
// wavefront 0 alone (lane j its items j, j + 64, ..., then the shfl_xor butterfly), so its order does not depend on the workgroup's size;
// every lane reads the same bits and takes the same Levenberg-Marquardt decisions for itself. No atomics, no waiting between workgroups;
// every loop is bounded by num_iter, the ten trials and pcg_max_iter.
// k_posegraph_correct: a grid over the landmarks, rule G10.
#include <cstring>
#include <memory>
#include <mutex>

#include "ovs_common.h"
#include "owned_internal.inc"
#include "pose_graph_math.inc"
#include "pose_graph_plan.inc"

namespace {

static_assert(pgplan::kStateBytes == 8 * pg::kStateDoubles && pgplan::kEdgeBytes == 8 * pg::kEdgeDoubles, "the plan sizes the kernels' records");

constexpr int kThreads = 256;

// pose_graph_math.inc's lanes as one workgroup
struct GroupLanes {
    static constexpr int kLanes = kThreads;
    double* slot;   // LDS [2]: a sum's broadcast, alternating, so that a sum may be written while the one before is still read
    int turn;
    template <class F>
    __device__ __forceinline__ void each(F f) {
        f((int)threadIdx.x);
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ double sum(int n, const double* val, const uint8_t* skip) {
        __syncthreads();
        if (threadIdx.x < 64) {
            double acc = 0.0;
            for (int i = threadIdx.x; i < n; i += 64)
                if (!skip || !skip[i]) acc = acc + val[i];
#pragma unroll
            for (int d = 32; d; d >>= 1) acc = acc + __shfl_xor(acc, d);
            if (threadIdx.x == 0) slot[turn] = acc;
        }
        __syncthreads();
        const double r = slot[turn];
        turn ^= 1;
        return r;
    }
};

__global__ __launch_bounds__(kThreads) void k_posegraph_optimize(pg::Problem P, pg::Params prm, double* info_out) {
    __shared__ double slot[2];
    GroupLanes x{slot, 0};
    double info[8];
    pg::pg_optimize(x, P, prm, info);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) info_out[k] = info[k];
    }
}

__global__ __launch_bounds__(256) void k_posegraph_correct(int n_l, const int32_t* __restrict__ lm_ref, const double* __restrict__ lm_pos,
                                                           const double* __restrict__ nc, const double* __restrict__ V,
                                                           double* __restrict__ out) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n_l) return;
    const int r = lm_ref[m];   // -1 or a vertex: the plan has refused anything else
    const double* p = lm_pos + 3 * (size_t)m;
    if (r < 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * (size_t)m + k] = p[k];
        return;
    }
    const pg::State Snc = pg::load_state(nc + (size_t)pg::kStateDoubles * r), Sopt = pg::load_state(V + (size_t)pg::kStateDoubles * r);
    double q[3];
    pg::correct_landmark(Snc, Sopt, p, q);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (size_t)m + k] = q[k];
}

// rot (9 per record), trans (3) and scale (1) as the kernels' 13-double records
void pack_states(double* dst, const double* rot, const double* trans, const double* scale, int32_t n) {
    for (int32_t k = 0; k < n; ++k) {
        std::memcpy(dst + 13 * (size_t)k, rot + 9 * (size_t)k, 72);
        std::memcpy(dst + 13 * (size_t)k + 9, trans + 3 * (size_t)k, 24);
        dst[13 * (size_t)k + 12] = scale[k];
    }
}

}   // namespace

struct ovs_posegraph {
    int device = 0;
    int32_t max_vertices = 0, max_edges = 0, max_landmarks = 0;
    std::mutex mu;
    ovs::Owned res;
    hipStream_t stream = nullptr;
    uint8_t *d_arena = nullptr, *h_image = nullptr;   // the arena and the page-locked twin of its uploaded part
    double* h_out = nullptr;                          // page-locked: the vertices (13 each), the landmarks (3 each), info (8)
};

extern "C" {

ovs_status ovs_posegraph_create(int32_t device, int32_t max_vertices, int32_t max_edges, int32_t max_landmarks, ovs_posegraph** out) {
    if (!out) return OVS_ERR_INVALID;
    *out = nullptr;
    if (!pgplan::create_ok(max_vertices, max_edges, max_landmarks)) return OVS_ERR_INVALID;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<ovs_posegraph> owner(new ovs_posegraph());
    ovs_posegraph* const s = owner.get();
    s->device = device;
    s->max_vertices = max_vertices, s->max_edges = max_edges, s->max_landmarks = max_landmarks;
    const pgplan::Arena a = pgplan::arena_of(max_vertices, max_edges, max_landmarks);
    OVS_HIP_TRY(s->res.stream(&s->stream));
    OVS_HIP_TRY(s->res.dev(&s->d_arena, a.arena_bytes));
    OVS_HIP_TRY(s->res.pinned(&s->h_image, a.upload_bytes));
    OVS_HIP_TRY(s->res.pinned(&s->h_out, 8 * (13 * (size_t)max_vertices + 3 * (size_t)max_landmarks + 8)));
    *out = owner.release();
    return OVS_OK;
}

ovs_status ovs_posegraph_destroy(ovs_posegraph* s) {
    if (!s) return OVS_ERR_INVALID;
    hipSetDevice(s->device);
    delete s;
    return OVS_OK;
}

ovs_status ovs_posegraph_optimize(ovs_posegraph* s, int32_t n_vertices, const double* rot_in, const double* trans_in, const double* scale_in,
                                  const uint8_t* fixed, const double* nc_rot, const double* nc_trans, const double* nc_scale, int32_t n_edges,
                                  const int32_t* edge_ij, const double* edge_rot, const double* edge_trans, const double* edge_scale,
                                  int32_t fix_scale, int32_t num_iter, int32_t pcg_max_iter, int32_t n_landmarks, const int32_t* lm_ref_vertex,
                                  const double* lm_pos_in, double* out_rot, double* out_trans, double* out_scale, double* out_lm_pos,
                                  double* out_info) {
    // every caller-side error is decided here, before the device is touched
    if (!s) return OVS_ERR_INVALID;
    const pgplan::Call c{n_vertices, rot_in,    trans_in,   scale_in,   fixed,     nc_rot,   nc_trans,     nc_scale,    n_edges,
                         edge_ij,    edge_rot,  edge_trans, edge_scale, fix_scale, num_iter, pcg_max_iter, n_landmarks, lm_ref_vertex,
                         lm_pos_in,  out_rot,   out_trans,  out_scale,  out_lm_pos, out_info};
    const ovs_status checked = pgplan::check_call(c, s->max_vertices, s->max_edges, s->max_landmarks);
    if (checked != OVS_OK) return checked;
    std::lock_guard<std::mutex> lock(s->mu);
    const pgplan::Arena a = pgplan::arena_of(n_vertices, n_edges, n_landmarks);
    uint8_t* const h = s->h_image;
    if (n_vertices > 0) std::memcpy(h + a.o_fixed, fixed, (size_t)n_vertices);
    if (n_edges > 0) std::memcpy(h + a.o_edge_ij, edge_ij, 8 * (size_t)n_edges);
    const int32_t n_free = pgplan::build_incidence(n_vertices, n_edges, edge_ij, fixed, reinterpret_cast<int32_t*>(h + a.o_inc_row),
                                                   reinterpret_cast<int32_t*>(h + a.o_inc));
    pack_states(reinterpret_cast<double*>(h + a.o_V), rot_in, trans_in, scale_in, n_vertices);
    pack_states(reinterpret_cast<double*>(h + a.o_nc), nc_rot, nc_trans, nc_scale, n_vertices);
    pack_states(reinterpret_cast<double*>(h + a.o_meas), edge_rot, edge_trans, edge_scale, n_edges);
    if (n_landmarks > 0) {
        std::memcpy(h + a.o_lm_ref, lm_ref_vertex, 4 * (size_t)n_landmarks);
        std::memcpy(h + a.o_lm_pos, lm_pos_in, 24 * (size_t)n_landmarks);
    }
    uint8_t* const d = s->d_arena;
    const auto dd = [&](size_t off) { return reinterpret_cast<double*>(d + off); };
    pg::Problem P;
    P.n_v = n_vertices, P.n_e = n_edges, P.n_free = n_free;
    P.fixed = d + a.o_fixed;
    P.edge_ij = reinterpret_cast<const int32_t*>(d + a.o_edge_ij);
    P.meas = dd(a.o_meas);
    P.inc_row = reinterpret_cast<const int32_t*>(d + a.o_inc_row);
    P.inc = reinterpret_cast<const int32_t*>(d + a.o_inc);
    P.V = dd(a.o_V), P.Vt = dd(a.o_Vt), P.edge = dd(a.o_edge), P.chi_e = dd(a.o_chi_e), P.Hd = dd(a.o_Hd), P.Lf = dd(a.o_Lf);
    P.g = dd(a.o_g), P.x = dd(a.o_x), P.r = dd(a.o_r), P.z = dd(a.o_z), P.p = dd(a.o_p), P.q = dd(a.o_q), P.val = dd(a.o_val);
    pg::Params prm;
    prm.fix_scale = fix_scale ? 1 : 0, prm.num_iter = num_iter, prm.pcg_max_iter = pcg_max_iter;
    double* const h_V = s->h_out;
    double* const h_lm = h_V + 13 * (size_t)n_vertices;
    double* const h_info = h_lm + 3 * (size_t)n_landmarks;
    OVS_HIP_TRY(hipSetDevice(s->device));
    OVS_HIP_TRY(hipMemcpyAsync(d, h, a.upload_bytes, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_posegraph_optimize, dim3(1), dim3(kThreads), 0, s->stream, P, prm, dd(a.o_info));
    OVS_HIP_TRY(hipGetLastError());
    if (n_landmarks > 0) {
        hipLaunchKernelGGL(k_posegraph_correct, dim3((n_landmarks + 255) / 256), dim3(256), 0, s->stream, n_landmarks,
                           reinterpret_cast<const int32_t*>(d + a.o_lm_ref), dd(a.o_lm_pos), dd(a.o_nc), dd(a.o_V), dd(a.o_lm_out));
        OVS_HIP_TRY(hipGetLastError());
        OVS_HIP_TRY(hipMemcpyAsync(h_lm, d + a.o_lm_out, 24 * (size_t)n_landmarks, hipMemcpyDeviceToHost, s->stream));
    }
    if (n_vertices > 0) OVS_HIP_TRY(hipMemcpyAsync(h_V, d + a.o_V, 104 * (size_t)n_vertices, hipMemcpyDeviceToHost, s->stream));
    OVS_HIP_TRY(hipMemcpyAsync(h_info, d + a.o_info, 64, hipMemcpyDeviceToHost, s->stream));
    OVS_HIP_TRY(hipStreamSynchronize(s->stream));
    for (int32_t v = 0; v < n_vertices; ++v) {
        std::memcpy(out_rot + 9 * (size_t)v, h_V + 13 * (size_t)v, 72);
        std::memcpy(out_trans + 3 * (size_t)v, h_V + 13 * (size_t)v + 9, 24);
        out_scale[v] = h_V[13 * (size_t)v + 12];
    }
    if (n_landmarks > 0) std::memcpy(out_lm_pos, h_lm, 24 * (size_t)n_landmarks);
    if (out_info) std::memcpy(out_info, h_info, 64);
    return OVS_OK;
}

}   // extern "C"
