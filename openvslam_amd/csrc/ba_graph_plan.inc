// ba_graph_plan.inc -- everything the host side of the local-BA graph (ba_graph.hip: graph_create, solver_workspace_create) decides with integers:
// the order and offsets of the arrays in the graph arena and in the solver arena, which prefix of the graph arena is uploaded and which part of
// it early, the free keyframes' slots, the two counting sorts that index the edges by landmark and by keyframe, k_linearize2's landmark runs and
// keyframe chunks, the pair table, k_schur_l's work order and the bound of the pair lists. Plain host C++, no HIP: ba_graph.hip includes it,
// tests/ba_graph_plan_host.cc builds it with the host compiler alone and tests/test_ba_graph_plan.py holds it to a hand-written table.
// This is the one place these sizes, offsets and partitions are computed. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/ovslam_hip.h"

namespace ovs {

constexpr int kPoseChunk = 512;   // entries of pose_edges per chunk (k_linearize2: two keyframe workgroups, one entry per thread)
constexpr int kLmSlots = 256;     // edges per landmark workgroup
constexpr int kLmPerWg = 256;     // landmarks per landmark workgroup: one lane per landmark finishes the workgroup's scalars
constexpr int kXcds = 8;          // k_schur_l's work order deals rows of the pair table to the XCDs (workgroup w runs on XCD w % 8)

// The edge record as the host fills it. ba_edge.h's GEdge is the same record for the kernels (a HIP header: ba_graph.hip asserts size and offsets).
struct EdgeRec {
    int32_t pose, pt;
    double ox, oy, oxr, w;
};

// One allocation, many arrays: offsets in placement order, each 256-byte aligned; an empty array still takes a byte, so no two share an offset.
struct Placer {
    size_t top = 0;
    size_t place(size_t elem_bytes, size_t count) {
        const size_t off = bytes();
        top = off + std::max<size_t>(elem_bytes * count, 1);
        return off;
    }
    size_t bytes() const { return (top + 255) & ~(size_t)255; }   // where the next array would start = the size to allocate
};

// ---- the graph arena ---------------------------------------------------------------------------------------------------------
// One layout for the page-locked host image and the device arena. First the arrays the host fills, uploaded as they are: the edge records go up
// early (they are final after pass 1), the rest when the partitions are done. Behind them, on the device, what the kernels write; in the image,
// only the word the duplicate check's verdict comes down to.
struct GraphArena {
    // uploaded
    size_t o_edges, o_lm_start, o_lm_edges, o_lm_nmono, o_pose_start, o_pose_edges, o_fixed, o_active, o_slot_of_pose, o_pose_pt, o_pair_ab, o_slot_pose,
        o_wg_pair, o_lm_wg_first, o_chunk_kf, o_chunk_start;
    // device only
    size_t o_lm_of_slot, o_dup, o_lm_tmp, o_pose_part, o_ledges;
    size_t early_bytes;    // the edge records: they end where lm_start begins
    size_t upload_bytes;   // what the device reads before writing it ends here
    size_t o_dup_host;     // image only: the duplicate check's verdict
    size_t image_bytes, arena_bytes;
    size_t max_chunks;     // an upper bound of the keyframe chunks (the partition needs the counting sorts): n_edge / kPoseChunk + n_pose
    int n_pairs;           // n_free (n_free + 1) / 2
    int wg_pair_cap;       // wg_pair_capacity(n_free); wg_pair has kXcds times as many entries
};

// pairs one XCD's sequence of k_schur_l's work order can take: a fair share, the longest row, and one
inline int wg_pair_capacity(int n_free) { return n_free * (n_free + 1) / 2 / kXcds + n_free + 1; }

inline GraphArena graph_arena_of(int n_pose, int n_pt, int n_edge, int n_free) {
    GraphArena a;
    const size_t ne = (size_t)n_edge, np = (size_t)n_pose, nl = (size_t)n_pt, nf = (size_t)n_free;
    a.n_pairs = n_free * (n_free + 1) / 2;
    a.wg_pair_cap = wg_pair_capacity(n_free);
    a.max_chunks = ne / kPoseChunk + np;
    Placer p;
    a.o_edges = p.place(sizeof(EdgeRec), ne);
    a.o_lm_start = p.place(4, nl + 1);
    a.o_lm_edges = p.place(4, ne);
    a.o_lm_nmono = p.place(4, nl);
    a.o_pose_start = p.place(4, np + 1);
    a.o_pose_edges = p.place(4, ne);
    a.o_fixed = p.place(1, np);
    a.o_active = p.place(1, ne);
    a.o_slot_of_pose = p.place(4, np);
    a.o_pose_pt = p.place(4, ne);
    a.o_pair_ab = p.place(4, 2 * (size_t)a.n_pairs);
    a.o_slot_pose = p.place(4, nf);
    a.o_wg_pair = p.place(4, (size_t)kXcds * (size_t)a.wg_pair_cap);
    a.o_lm_wg_first = p.place(4, nl + 1);
    a.o_chunk_kf = p.place(4, a.max_chunks);
    a.o_chunk_start = p.place(4, np + 1);
    a.early_bytes = a.o_lm_start;
    a.upload_bytes = p.bytes();
    Placer host = p;
    a.o_dup_host = host.place(8, 1);
    a.image_bytes = host.bytes();
    a.o_lm_of_slot = p.place(4, ne);
    a.o_dup = p.place(8, 1);
    a.o_lm_tmp = p.place(8, 4 * nl);
    a.o_pose_part = p.place(8, 27 * 2 * a.max_chunks);   // k_linearize2: one sum of the 21 + 6 pose-block terms per HALF chunk
    a.o_ledges = p.place(sizeof(EdgeRec), ne);
    a.arena_bytes = p.bytes();
    return a;
}

// ---- the solver arena --------------------------------------------------------------------------------------------------------
constexpr size_t kPairListCap = (size_t)1 << 28;   // entries; the lists' offsets are 32-bit and their storage is sized by the bound
constexpr size_t kScalDoubles = 32, kFailWords = 64;
// ba_optimize.hip's TrialBlock takes d_scal and both failure words in one download: the words lie 256 bytes behind d_scal
static_assert(kScalDoubles * sizeof(double) == 256 && kFailWords * sizeof(int32_t) == 256, "d_scal and d_fail are one 256-byte unit each");

struct SolverArena {
    size_t o_hinv, o_y, o_s, o_dxp, o_scal, o_fail, o_edge_of, o_pl_cnt, o_pl_off, o_pl_ent;
    size_t arena_bytes;
    size_t n_lists;      // four per pair
    size_t ff_bytes;     // the 0xff memset from o_edge_of: the table (-1 = no edge) and its padding up to pl_cnt
    bool pl_ok;          // pl_bound (GraphPartition) is within kPairListCap. Beyond it (2 GB; e.g. hundreds of keyframes that all observe the
                         // same landmarks) the lists are not built, pl_ent takes one entry and k_schur scans per trial instead
};

// solve_doubles: the padded reduced camera system's storage (ba_solve.hip: dense_solve_doubles(6 max(n_free, 1)))
inline SolverArena solver_arena_of(int n_pose, int n_pt, int n_edge, int n_free, int n_pairs, size_t pl_bound, size_t solve_doubles) {
    SolverArena a;
    const size_t ne = (size_t)std::max(n_edge, 1), np = (size_t)n_pose, nl = (size_t)n_pt;
    a.n_lists = 4 * (size_t)std::max(n_pairs, 0);
    a.pl_ok = pl_bound <= kPairListCap;
    Placer p;
    a.o_hinv = p.place(8, 9 * nl);
    a.o_y = p.place(8, 18 * ne);
    a.o_s = p.place(8, solve_doubles + 6 * np);   // the padded system | a copy of bp
    a.o_dxp = p.place(8, 6 * np);
    a.o_scal = p.place(8, kScalDoubles);
    a.o_fail = p.place(4, kFailWords);
    a.o_edge_of = p.place(4, (size_t)std::max(n_free, 1) * nl);
    a.o_pl_cnt = p.place(4, a.n_lists + 1);
    a.o_pl_off = p.place(4, a.n_lists + 1);
    a.o_pl_ent = p.place(8, a.pl_ok ? std::max<size_t>(pl_bound, 1) : 1);
    a.arena_bytes = p.bytes();
    a.ff_bytes = a.o_pl_cnt - a.o_edge_of;
    return a;
}

// ---- free keyframes ----------------------------------------------------------------------------------------------------------
// slot[k]: keyframe k's block of the reduced system or -1 (fixed); slot_pose[s]: the keyframe of block s. pose_fixed: null = none is fixed.
// Returns n_free.
inline int assign_slots(const uint8_t* pose_fixed, int n_pose, int32_t* slot, int32_t* slot_pose) {
    int n_free = 0;
    for (int k = 0; k < n_pose; ++k) {
        const bool fixed = pose_fixed && pose_fixed[k];
        slot[k] = fixed ? -1 : n_free;
        if (!fixed) slot_pose[n_free++] = k;
    }
    return n_free;
}

// ---- the edge index ----------------------------------------------------------------------------------------------------------
// Two counting sorts, ascending edge index inside every landmark and every keyframe (mono edges have the lower indices, so "mono first" is
// free), in four passes over the edges: the histograms and the range check ride on the record fill (pass 1), pose_pt on the scatter (pass 2);
// the device writes the landmark of every slot and looks for duplicates (k_edges_by_slot, k_dup_check). Two functions because the records are
// final after pass 1: the caller starts their upload between the two.

// Fills edges, edge_pose, edge_pt [n_mono + n_stereo], the counts lm_start[j + 1], pose_start[k + 1] and lm_nmono[j]. Returns the first edge
// (stereo edges count from n_mono) whose keyframe or landmark index is out of range, where it stops, or -1.
inline int index_pass1(const ovs_ba_edge* mono, int n_mono, const ovs_ba_edge_stereo* stereo, int n_stereo, int n_pose, int n_pt, EdgeRec* edges,
                       int32_t* edge_pose, int32_t* edge_pt, int32_t* lm_start, int32_t* lm_nmono, int32_t* pose_start) {
    std::memset(lm_start, 0, sizeof(int32_t) * ((size_t)n_pt + 1));
    std::memset(lm_nmono, 0, sizeof(int32_t) * (size_t)n_pt);
    std::memset(pose_start, 0, sizeof(int32_t) * ((size_t)n_pose + 1));
    for (int i = 0; i < n_mono; ++i) {
        const int32_t kp = mono[i].pose_idx, pt = mono[i].point_idx;
        if ((uint32_t)kp >= (uint32_t)n_pose || (uint32_t)pt >= (uint32_t)n_pt) return i;
        edges[i] = EdgeRec{kp, pt, mono[i].obs_x, mono[i].obs_y, 0.0, mono[i].inv_sigma_sq};
        edge_pose[i] = kp;
        edge_pt[i] = pt;
        ++lm_start[(size_t)pt + 1];
        ++lm_nmono[pt];
        ++pose_start[(size_t)kp + 1];
    }
    for (int i = 0; i < n_stereo; ++i) {
        const int32_t kp = stereo[i].pose_idx, pt = stereo[i].point_idx;
        if ((uint32_t)kp >= (uint32_t)n_pose || (uint32_t)pt >= (uint32_t)n_pt) return n_mono + i;
        const size_t e = (size_t)n_mono + (size_t)i;
        edges[e] = EdgeRec{kp, pt, stereo[i].obs_x, stereo[i].obs_y, stereo[i].obs_x_right, stereo[i].inv_sigma_sq};
        edge_pose[e] = kp;
        edge_pt[e] = pt;
        ++lm_start[(size_t)pt + 1];
        ++pose_start[(size_t)kp + 1];
    }
    return -1;
}

// The counts become starts (lm_start [n_pt + 1], pose_start [n_pose + 1]); every edge goes to its landmark's and its keyframe's list, and
// pose_pt gets the landmark of every entry of pose_edges. lm_cursor [n_pt] and pose_cursor [n_pose] are scratch.
inline void index_pass2(const int32_t* edge_pose, const int32_t* edge_pt, int n_edge, int n_pose, int n_pt, int32_t* lm_start, int32_t* pose_start,
                        int32_t* lm_cursor, int32_t* pose_cursor, int32_t* lm_edges, int32_t* pose_edges, int32_t* pose_pt) {
    for (int j = 0; j < n_pt; ++j) lm_start[(size_t)j + 1] += lm_start[j];
    for (int k = 0; k < n_pose; ++k) pose_start[(size_t)k + 1] += pose_start[k];
    std::memcpy(lm_cursor, lm_start, sizeof(int32_t) * (size_t)n_pt);
    std::memcpy(pose_cursor, pose_start, sizeof(int32_t) * (size_t)n_pose);
    for (int e = 0; e < n_edge; ++e) {
        const int32_t pt = edge_pt[e];
        lm_edges[(size_t)lm_cursor[pt]++] = e;
        const int32_t at = pose_cursor[edge_pose[e]]++;
        pose_edges[(size_t)at] = e;
        pose_pt[(size_t)at] = pt;
    }
}

// ---- k_linearize2's work partition ---------------------------------------------------------------------------------------------
struct GraphPartition {
    int n_lm_wg = 0;       // landmark workgroups (also k_trial_update's)
    int n_chunks = 0;      // keyframe chunks: two workgroups each
    int n_pair_wg = 0;     // k_schur_l's pair workgroups: kXcds times the longest XCD sequence
    size_t pl_bound = 0;   // entries the pair lists (k_pair_lists) can have together: the sum over the landmarks of n (n + 1) / 2, n = its edges
};

// Landmark side: runs of whole landmarks with at most kLmSlots edges and kLmPerWg landmarks; a landmark with more edges is a run of its own.
// wg_first [n_pt + 1 at most; n_lm_wg + 1 written]: the first landmark of every run, then n_pt.
inline void partition_landmarks(const int32_t* lm_start, int n_pt, int32_t* wg_first, GraphPartition& part) {
    int n_wg = 0, first = 0;
    size_t pl_bound = 0;
    for (int j = 0; j < n_pt; ++j) {
        const size_t nj = (size_t)(lm_start[(size_t)j + 1] - lm_start[j]);
        pl_bound += nj * (nj + 1) / 2;
        if (j > first && (lm_start[(size_t)j + 1] - lm_start[first] > kLmSlots || j - first >= kLmPerWg)) {   // j does not fit: it opens the next run
            wg_first[n_wg++] = first;
            first = j;
        }
    }
    wg_first[n_wg++] = first;
    wg_first[n_wg] = n_pt;
    part.n_lm_wg = n_wg;
    part.pl_bound = pl_bound;
}

// Keyframe side: chunks of kPoseChunk entries of a keyframe's edge list. chunk_kf [n_chunks <= GraphArena::max_chunks]: the keyframe of every
// chunk; chunk_start [n_pose + 1]: the first chunk of every keyframe.
inline void partition_chunks(const int32_t* pose_start, int n_pose, int32_t* chunk_kf, int32_t* chunk_start, GraphPartition& part) {
    int n_ch = 0;
    for (int k = 0; k < n_pose; ++k) {
        chunk_start[k] = n_ch;
        for (int i = pose_start[k]; i < pose_start[(size_t)k + 1]; i += kPoseChunk) chunk_kf[n_ch++] = k;
    }
    chunk_start[n_pose] = n_ch;
    part.n_chunks = n_ch;
}

// ---- the reduced system's blocks ---------------------------------------------------------------------------------------------
// The blocks (a, b), a <= b in slot order, a-major: a row (a, a .. n_free - 1) stays together (k_schur_l hands contiguous runs of pairs to one
// XCD) and starts with its longest list, the diagonal pair's (all of a's landmarks). "All diagonal pairs first" was measured: no change.
inline void pair_table(int n_free, int32_t* pair_ab) {   // [2 n_pairs]
    int p = 0;
    for (int a = 0; a < n_free; ++a)
        for (int b = a; b < n_free; ++b) {
            pair_ab[(size_t)2 * p] = a;
            pair_ab[(size_t)2 * p + 1] = b;
            ++p;
        }
}

// k_schur_l's work order. Rows are dealt to the XCDs in serpentine order (rows 0 .. 7 to XCDs 0 .. 7, rows 8 .. 15 to XCDs 7 .. 0, ...: row a
// has n_free - a pairs, so the eight sums come out within a row's length of each other); XCD x's i-th pair is workgroup 8 i + x, -1 = no pair.
// wg_pair [kXcds * GraphArena::wg_pair_cap], all of it written. n_free = 0: nothing is written.
inline void pair_work_order(int n_free, int32_t* wg_pair, GraphPartition& part) {
    part.n_pair_wg = 0;
    if (n_free <= 0) return;
    const int cap = wg_pair_capacity(n_free);
    for (int i = 0; i < kXcds * cap; ++i) wg_pair[i] = -1;
    int fill[kXcds] = {};
    int first = 0;   // index of pair (a, a)
    for (int a = 0; a < n_free; ++a) {
        const int x = ((a >> 3) & 1) ? 7 - (a & 7) : (a & 7);
        for (int b = a; b < n_free; ++b) wg_pair[(size_t)kXcds * fill[x]++ + x] = first + (b - a);
        first += n_free - a;
    }
    part.n_pair_wg = kXcds * *std::max_element(fill, fill + kXcds);
}

}   // namespace ovs
