// pose_graph_plan.inc -- everything the host side of the pose-graph optimiser (pose_graph.hip) decides with integers before a launch:
// the caller-side errors of ovs_posegraph_optimize (DESIGN.md 3.19), the incidence CSR of rule G7 and the order and offsets of the arrays
// in the handle's arena. Plain host C++, no HIP: pose_graph.hip includes it, tests/posegraph_plan_host.cc builds it with the host compiler
// alone under the sanitizers. This is the one place these are computed. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/ovslam_hip.h"

namespace pgplan {

constexpr size_t kStateBytes = 13 * 8;    // a Sim3 as the kernels read it: R (9), t (3), s
constexpr size_t kEdgeBytes = 154 * 8;    // e (7), J_i (49), J_j (49), A_ij (49): pg::kEdgeDoubles

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

// First what the host stages and uploads as one block, then what only the kernels touch.
struct Arena {
    size_t o_fixed, o_edge_ij, o_inc_row, o_inc, o_lm_ref, o_V, o_nc, o_meas, o_lm_pos;
    size_t upload_bytes;
    size_t o_Vt, o_edge, o_chi_e, o_Hd, o_Lf, o_g, o_x, o_r, o_z, o_p, o_q, o_val, o_lm_out, o_info;
    size_t arena_bytes;
};

inline Arena arena_of(int n_v, int n_e, int n_l) {
    const size_t nv = (size_t)n_v, ne = (size_t)n_e, nl = (size_t)n_l;
    Arena a;
    Placer p;
    a.o_fixed = p.place(1, nv);
    a.o_edge_ij = p.place(4, 2 * ne);
    a.o_inc_row = p.place(4, nv + 1);
    a.o_inc = p.place(4, 2 * ne);
    a.o_lm_ref = p.place(4, nl);
    a.o_V = p.place(kStateBytes, nv);
    a.o_nc = p.place(kStateBytes, nv);
    a.o_meas = p.place(kStateBytes, ne);
    a.o_lm_pos = p.place(24, nl);
    a.upload_bytes = p.bytes();
    a.o_Vt = p.place(kStateBytes, nv);
    a.o_edge = p.place(kEdgeBytes, ne);
    a.o_chi_e = p.place(8, ne);
    a.o_Hd = p.place(8 * 49, nv);
    a.o_Lf = p.place(8 * 49, nv);
    a.o_g = p.place(8 * 7, nv);
    a.o_x = p.place(8 * 7, nv);
    a.o_r = p.place(8 * 7, nv);
    a.o_z = p.place(8 * 7, nv);
    a.o_p = p.place(8 * 7, nv);
    a.o_q = p.place(8 * 7, nv);
    a.o_val = p.place(8, nv);
    a.o_lm_out = p.place(24, nl);
    a.o_info = p.place(8, 8);
    a.arena_bytes = p.bytes();
    return a;
}

inline bool create_ok(int32_t max_vertices, int32_t max_edges, int32_t max_landmarks) {
    return max_vertices >= 1 && max_edges >= 0 && max_landmarks >= 0 && max_vertices <= (1 << 24) && max_edges <= (1 << 24) &&
           max_landmarks <= (1 << 26);   // every index the kernels form stays far below 2^31
}

// One call's arguments as the C ABI receives them (the handle aside)
struct Call {
    int32_t n_vertices;
    const double *rot_in, *trans_in, *scale_in;
    const uint8_t* fixed;
    const double *nc_rot, *nc_trans, *nc_scale;
    int32_t n_edges;
    const int32_t* edge_ij;
    const double *edge_rot, *edge_trans, *edge_scale;
    int32_t fix_scale, num_iter, pcg_max_iter;
    int32_t n_landmarks;
    const int32_t* lm_ref_vertex;
    const double* lm_pos_in;
    double *out_rot, *out_trans, *out_scale, *out_lm_pos, *out_info;
};

// OVS_ERR_INVALID as the header lists it, then OVS_ERR_CAPACITY; OVS_OK when the call may be staged
inline ovs_status check_call(const Call& c, int32_t max_vertices, int32_t max_edges, int32_t max_landmarks) {
    if (c.n_vertices < 0 || c.n_edges < 0 || c.n_landmarks < 0 || c.num_iter < 1 || c.pcg_max_iter < 0) return OVS_ERR_INVALID;
    if (c.n_vertices > 0 && (!c.rot_in || !c.trans_in || !c.scale_in || !c.fixed || !c.nc_rot || !c.nc_trans || !c.nc_scale || !c.out_rot ||
                             !c.out_trans || !c.out_scale))
        return OVS_ERR_INVALID;
    if (c.n_edges > 0 && (!c.edge_ij || !c.edge_rot || !c.edge_trans || !c.edge_scale)) return OVS_ERR_INVALID;
    if (c.n_landmarks > 0 && (!c.lm_ref_vertex || !c.lm_pos_in || !c.out_lm_pos)) return OVS_ERR_INVALID;
    for (int32_t v = 0; v < c.n_vertices; ++v)
        if (c.fixed[v] > 1) return OVS_ERR_INVALID;
    for (int32_t e = 0; e < c.n_edges; ++e) {
        const int32_t i = c.edge_ij[2 * (size_t)e], j = c.edge_ij[2 * (size_t)e + 1];
        if (i < 0 || j < 0 || i >= c.n_vertices || j >= c.n_vertices || i == j) return OVS_ERR_INVALID;
    }
    for (int32_t m = 0; m < c.n_landmarks; ++m)
        if (c.lm_ref_vertex[m] < -1 || c.lm_ref_vertex[m] >= c.n_vertices) return OVS_ERR_INVALID;
    if (c.n_vertices > max_vertices || c.n_edges > max_edges || c.n_landmarks > max_landmarks) return OVS_ERR_CAPACITY;
    return OVS_OK;
}

// Rule G7's incidence lists by a counting sort: vertex v owns inc[inc_row[v] .. inc_row[v + 1]), each entry 2 * edge + side (side 0: v is
// the edge's i), in ascending edge index. inc_row has n_v + 1 entries, inc 2 n_e. edge_ij has passed check_call. Returns the free vertices.
inline int32_t build_incidence(int32_t n_v, int32_t n_e, const int32_t* edge_ij, const uint8_t* fixed, int32_t* inc_row, int32_t* inc) {
    for (int32_t v = 0; v <= n_v; ++v) inc_row[v] = 0;
    for (int32_t k = 0; k < 2 * n_e; ++k) ++inc_row[edge_ij[k] + 1];
    for (int32_t v = 0; v < n_v; ++v) inc_row[v + 1] += inc_row[v];
    for (int32_t k = 0; k < 2 * n_e; ++k) {   // k = 2 * edge + side ascends, so every list does; inc_row[v] ends one list further on
        const int32_t v = edge_ij[k];
        inc[inc_row[v]++] = k;
    }
    for (int32_t v = n_v; v > 0; --v) inc_row[v] = inc_row[v - 1];
    inc_row[0] = 0;
    int32_t n_free = 0;
    for (int32_t v = 0; v < n_v; ++v) n_free += fixed[v] ? 0 : 1;
    return n_free;
}

}   // namespace pgplan
