// match_window_plan.inc -- everything the host side of the window matchers (match_window.hip) and of the resident frame handle (frame_dev.hip)
// decides with integers and a few doubles: the launch plans of k_grid_assign and k_list_resolve, the dead-candidate thresholds, the pose helpers,
// the frame arena's layout, and the staging arena -- the arithmetic of the Stager, the argument structs it fills, every matcher's staging list,
// the capacity ovs_wmatcher_create gives the arena and what each entry point needs of it. Plain host C++, no HIP: the two units include it,
// tests/match_window_plan_host.cc builds it with the host compiler alone and tests/test_match_window_plan.py holds it to a hand-written table.
// This is the one place these sizes, thresholds and offsets are computed. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/ovslam_hip.h"

namespace ovs {

// ---- grid (data::assign_keypoints_to_grid) ---------------------------------------------------------------------------------
struct GridP {
    float min_x, min_y;
    float inv_w, inv_h;
    int32_t cols, rows;
};

constexpr int kMaxGridCells = 16384;
constexpr int kGridItemsLds = 8192;   // keypoints up to which k_grid_assign builds and sorts the member lists in LDS

inline GridP make_gridp(const ovs_grid_params& p) {
    GridP g;
    g.min_x = p.min_x;
    g.min_y = p.min_y;
    g.inv_w = (float)((double)p.cols / (double)(p.max_x - p.min_x));   // camera::base: double division, float member
    g.inv_h = (float)((double)p.rows / (double)(p.max_y - p.min_y));
    g.cols = p.cols;
    g.rows = p.rows;
    return g;
}

inline bool grid_params_ok(const ovs_grid_params* gp) {
    return gp && gp->cols >= 1 && gp->rows >= 1 && gp->cols * gp->rows <= kMaxGridCells && gp->max_x > gp->min_x && gp->max_y > gp->min_y;
}

// k_grid_assign over n keypoints and nc cells: one workgroup; histogram and cell starts in LDS, the member lists too when they fit
struct GridLaunch {
    int items_in_lds;
    size_t lds_bytes;
    bool raise_attr;   // beyond the 64 KiB a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize
};
inline GridLaunch grid_launch_plan(int n, int nc) {
    GridLaunch l;
    l.items_in_lds = (n <= kGridItemsLds && (size_t)(2 * nc + 1 + n) * sizeof(int32_t) <= 144 * 1024) ? 1 : 0;
    l.lds_bytes = (size_t)(2 * nc + 1 + (l.items_in_lds ? n : 0)) * sizeof(int32_t);
    l.raise_attr = l.lds_bytes > 64 * 1024;
    return l;
}

// ---- resolver (k_list_resolve) ---------------------------------------------------------------------------------------------
constexpr int kMarkSize = 4096;   // hashed stamp table of the resolver (collisions only cost an extra round)

// stamp table, angle histogram, thr / owner per target, match / accepted per query
inline size_t resolve_lds_bytes(int n_q, int n_t) {
    return (size_t)kMarkSize * 4 + 32 * 4 + (size_t)2 * 2 * ((n_t + 1) & ~1) + (size_t)2 * 2 * ((n_q + 1) & ~1);
}

struct ResolveLaunch {
    bool ok;              // false: the fixed part alone exceeds 150 KiB (OVS_ERR_CAPACITY)
    int offsets_in_lds;
    size_t lds_bytes;
    uint32_t key_pool;    // LDS words left for a copy of the key CSR
    int width;            // 0 / 1 / 2: k_list_resolve<RULE, 1 / 4 / 8>
};
inline ResolveLaunch resolve_plan(int n_q, int n_t, int wide_from) {
    ResolveLaunch l{};
    size_t fixed = resolve_lds_bytes(n_q, n_t);
    l.ok = fixed <= 150 * 1024;
    if (!l.ok) return l;
    // the queries' list bounds are staged in LDS too unless the problem is so large that they would take the room of everything else
    const size_t off_bytes = (size_t)4 * ((n_q + 4) & ~3);
    l.offsets_in_lds = fixed + off_bytes <= (size_t)120 * 1024 ? 1 : 0;
    if (l.offsets_in_lds) fixed += off_bytes;
    // the rest of the allocation (96 KiB, or 24 KiB beyond the fixed part for the largest problems) holds a copy of the key CSR when it
    // fits (checked on the device: the size is only known there)
    l.lds_bytes = std::min((size_t)150 * 1024, std::max((size_t)96 * 1024, fixed + (size_t)24 * 1024));
    l.key_pool = (uint32_t)((l.lds_bytes - fixed) / 4);
    // 1 / 4 / 8 waves (64 / 256 / 512 queries per round) by problem size: up to 256, up to wide_from, beyond
    // (wide_from: Tuning::resolve_wide_from, 1024; 2048 until the commit rule changed: tracked frame, 2008 queries: 0.158 -> 0.147 ms, area 0.123 -> 0.094)
    l.width = n_q > wide_from ? 2 : (n_q > 256 ? 1 : 0);
    return l;
}

// WinArgs::dead_from for a rule that accepts iff best <= thr and (ratio rules) !(fl(second * ratio) < best): the smallest distance d > thr with
// fl(d * ratio) >= thr -- from there on a candidate can neither be an accepted best nor make the ratio test fail (the float product is monotone
// in d, and "no second at all" counts as distance 256, which then accepts too). 257: nothing is dead; 0 would switch the filter off.
inline uint32_t dead_from_ratio(uint32_t thr, float ratio) {
    if (!(ratio > 0.0f)) return 257u;
    for (uint32_t d = thr + 1u; d <= 256u; ++d)
        if ((float)d * ratio >= (float)thr) return d;
    return 257u;
}
inline uint32_t dead_from_thr(uint32_t thr) { return thr + 1u; }   // rules without a ratio test: best <= thr or nothing

// ---- pose helpers ------------------------------------------------------------------------------------------------------------
// camera centre -R^T t of the pose P = [R | t] (9 + 3 doubles, row-major R)
inline void camera_centre(const double* P, double* cc) {
    cc[0] = -((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]);
    cc[1] = -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]);
    cc[2] = -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11]);
}
// Sim3_cw = [s R | t'] -> scale s = |first row of sR|, rot_cw = sR / s, trans_cw = t' / s, camera centre -R^T t (upstream decomposes the
// 4x4 the same way in fuse::detect_duplication / projection::match_by_Sim3_transform)
inline void decompose_sim3(const double* S, double* P, double* cc) {
    const double sc = std::sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]);
    for (int i = 0; i < 9; ++i) P[i] = S[i] / sc;
    for (int i = 0; i < 3; ++i) P[9 + i] = S[9 + i] / sc;
    camera_centre(P, cc);
}
// projection::match_keyframes_mutually, the Sim3 in both directions: S12 = [s_12 R_12 | t_12] takes keyframe-2 coordinates to keyframe 1;
// S21 = [R_12^T / s_12 | -(R_12^T / s_12) t_12] back
inline void sim3_both_ways(double s_12, const double* rot_12, const double* trans_12, double* S12, double* S21) {
    for (int i = 0; i < 9; ++i) S12[i] = s_12 * rot_12[i];
    for (int i = 0; i < 3; ++i) S12[9 + i] = trans_12[i];
    const double inv_s = 1.0 / s_12;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S21[3 * r + c] = inv_s * rot_12[3 * c + r];
    for (int r = 0; r < 3; ++r) S21[9 + r] = -((S21[3 * r] * trans_12[0] + S21[3 * r + 1] * trans_12[1]) + S21[3 * r + 2] * trans_12[2]);
}
// the per-level tables the kernels index up to OVS_MAX_LEVELS: `src` (nullptr: none) for the levels in use, `fill` beyond
inline void pad_levels(float* dst, const float* src, int num_levels, float fill) {
    for (int l = 0; l < OVS_MAX_LEVELS; ++l) dst[l] = (src && l < num_levels) ? src[l] : fill;
}
// match_current_and_last_frames (stereo / RGBD only): trans_wc = -rot_cw^T trans_cw; trans_lc = rot_lw trans_wc + trans_lw; its z against the baseline
inline void motion_direction(const ovs_camera* cam, const double* pose_cw_curr, const double* pose_cw_last, int* forward, int* backward) {
    double twc[3];
    camera_centre(pose_cw_curr, twc);
    const double* Rl = pose_cw_last;
    const double tlc_z = ((Rl[6] * twc[0] + Rl[7] * twc[1]) + Rl[8] * twc[2]) + pose_cw_last[11];
    *forward = cam->setup == 0 ? 0 : (tlc_z > cam->true_baseline);
    *backward = cam->setup == 0 ? 0 : (-tlc_z > cam->true_baseline);
}

// ---- frame arena (ovs_frame_dev_create) ------------------------------------------------------------------------------------
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// One device block per resident frame: keypoints | descriptors | stereo_x_right | cell of keypoint | grid items | cell starts, each on a 256-byte
// boundary and sized for the frame's capacity class (4096 keypoints: pooled arenas fit the next frame).
struct FrameArena {
    int cap;
    size_t o_kps, o_desc, o_xr, o_cellof, o_items, o_start, arena_bytes;
};
inline FrameArena frame_arena_of(int n) {
    FrameArena a;
    a.cap = std::max((n + 4095) & ~4095, 4096);
    const size_t C = (size_t)a.cap;
    a.o_kps = 0;
    a.o_desc = al256(a.o_kps + sizeof(ovs_keypoint) * C);
    a.o_xr = al256(a.o_desc + 32 * C);
    a.o_cellof = al256(a.o_xr + 4 * C);
    a.o_items = al256(a.o_cellof + 4 * C);
    a.o_start = al256(a.o_items + 4 * C);
    a.arena_bytes = al256(a.o_start + sizeof(int32_t) * (kMaxGridCells + 1));
    return a;
}
// the three uploaded arrays keep their arena offsets in the pinned staging buffer, so ONE copy of [0, end of the last array) uploads them
inline size_t frame_upload_bytes(const FrameArena& a, int n, bool stereo) {
    return n ? (stereo ? a.o_xr + 4 * (size_t)n : a.o_desc + 32 * (size_t)n) : 0;
}
// what the per-thread pinned buffer is (re)allocated at: the upload, and no less than a stereo frame of four capacity classes
inline size_t frame_stage_bytes(const FrameArena& a, size_t up_bytes) { return std::max(up_bytes, al256(a.o_xr + 4 * (size_t)4096 * 4)); }

// ---- the kernels' argument structs ---------------------------------------------------------------------------------------------
struct WinArgs {
    // targets: the frame whose grid is searched
    const ovs_keypoint* t_kps;
    const uint8_t* t_desc;
    const uint8_t* t_occupied;   // projection: keypoint already holds a landmark with observations (NULL = none)
    const float* t_x_right;      // projection: frm.stereo_x_right_ (NULL = monocular)
    const int32_t* cell_start;
    const int32_t* items;
    GridP gp;
    // queries
    int n_q;
    const float* q_xy;           // projection: reproj_in_tracking_; area: prev_matched_pts
    const float* q_x_right;      // projection: x_right_in_tracking_
    const int32_t* q_level;      // projection: scale_level_in_tracking_
    const uint8_t* q_valid;      // projection: is_observable_in_tracking_ && !will_be_erased()
    const ovs_keypoint* q_kps;   // area: frame-1 undistorted keypoints
    const float* q_radius;       // generic: search radius, level window (filled by k_reproject_queries)
    const int32_t* q_minl;
    const int32_t* q_maxl;
    const uint8_t* q_desc;
    float margin;
    float sf[OVS_MAX_LEVELS];
    int mode;
    // Candidates whose Hamming distance can neither win (d > the rule's acceptance threshold) nor make a ratio test fail (fl(d * ratio) >= that
    // threshold) are left out of the lists altogether: every candidate with d >= dead_from (0: no filter; set per rule by dead_from_*() above).
    // The sequential rule decides the same with or without them (a dropped best is a reject either way, a dropped second accepts either way, and
    // so does every later second), but the resolver's rounds are bounded by the chains of queries sharing LIVE candidates and its lists only fit
    // LDS when they are short: with a 100-px margin (BASELINE config 0) a query has ~110 candidates of which ~1 is alive.
    uint32_t dead_from;
};

// camera::perspective / camera::equirectangular ::reproject_to_image in double precision, one rounding per operation (the library
// is built with -ffp-contract=off), same operation order as the oracle.
struct CamP {
    int32_t model, setup;
    double fx, fy, cx, cy, fxb;
    int32_t cols, rows;
    float min_x, min_y, max_x, max_y;
    double P[12];   // rot_cw row-major, trans_cw
};

// fuse::replace_duplication, candidate search: landmarks are independent (the write-back that follows is host-side graph surgery)
struct FuseArgs {
    const ovs_keypoint* t_kps;
    const uint8_t* t_desc;
    const float* t_x_right;
    const int32_t* cell_start;
    const int32_t* items;
    GridP gp;
    CamP cam;
    double cc[3];                 // camera centre
    const double* lm_pos_w;
    const float* lm_dist;         // (min, max) valid distance
    const double* lm_normal;
    const uint8_t* lm_desc;
    const uint8_t* lm_valid;
    int m, num_levels;
    float log_scale_factor, margin;
    float sf[OVS_MAX_LEVELS], ils[OVS_MAX_LEVELS];
    int variant;                  // kFuseReplace / kFuseDetect / kFuseMutual
    uint32_t max_dist;            // acceptance threshold on the best Hamming distance
    double P1[12];                // kFuseMutual: pose of the landmark's own keyframe (pos_1 = R_1w X + t_1w, then cam.P = [s R_21 | t_21])
};

// tracking_module::search_local_landmarks, the visibility pass (k_observe_landmarks, DESIGN.md 3.17 rules V1 - V6): frame::can_observe for every
// local landmark. It writes the queries the kModeProjection lists read (q_xy, q_x_right, q_level; observable doubles as their q_valid) and the
// caller's per-landmark outputs.
struct ObserveArgs {
    CamP cam;
    double cc[3];                 // camera centre
    const double* lm_pos_w;
    const float* lm_dist;         // RAW (min_valid_dist_, max_valid_dist_)
    const double* lm_normal;
    const uint8_t* lm_search;     // V1: tested iff != 0 (nullptr: every landmark)
    int m, num_levels;
    float log_scale_factor;
    float* q_xy;                  // [2 m] (float)reproj
    float* q_x_right;             // [m]
    int32_t* q_level;             // [m]
    uint8_t* observable;          // [m]
    double* reproj;               // [2 m] or nullptr
    int32_t* assigned;            // nullptr, or [m] set to -1 (a call without keypoints runs no resolver that would write them)
    int32_t* num_observable;      // zero on entry
};

// bow_tree: queries = the keyframe's feature-vector entries in walk order; the list of a query is its node's frame bucket
struct BowArgs {
    const uint8_t* kf_desc;
    const uint8_t* kf_valid;
    const int32_t* kf_node_ids;
    const int32_t* kf_node_start;
    const int32_t* kf_items;
    int kf_nodes, n_q;           // n_q = kf_node_start[kf_nodes]
    const uint8_t* frm_desc;
    const uint8_t* frm_valid;    // match_keyframes: the target keypoint must hold a live landmark too (NULL = all)
    // robust::match_for_triangulation (tri != 0): pair filters d <= THR_LOW, epipole proximity, epipolar constraint; candidates are
    // listed in REVERSE bucket order because upstream lets a later equal distance replace an earlier one
    int tri;
    uint32_t dead_from;   // as WinArgs::dead_from (bow rule; the triangulation filter d <= THR_LOW is part of its pair test)
    const ovs_keypoint* kf_kps;  // octave of keypoint 1 (threshold scale)
    const float* kf_x_right;
    const float* frm_x_right;
    const double* kf_bearings;
    const double* frm_bearings;
    double E[9], epipole[3];
    float sf[OVS_MAX_LEVELS];
    const int32_t* frm_node_ids;
    const int32_t* frm_node_start;
    const int32_t* frm_items;
    int frm_nodes;
};

struct ResolveArgs {
    const uint32_t* offsets;   // n_q + 1
    const uint32_t* keys;
    int n_q, n_t;
    float lowe_ratio;
    int check_orientation;
    int angle_keep_rule;   // ovs_match_set_variant(OVS_MATCH_VARIANT_ANGLE_KEEP_RULE): filled in by launch_resolve
    int angle_tie_order;   // ovs_match_set_variant(OVS_MATCH_VARIANT_ANGLE_TIE_ORDER): 0 equal sizes -> lower bin first, 1 higher bin first
    const ovs_keypoint* q_kps;    // area: frame-1 keypoints (angle); bow: keyframe keypoints (angle), indexed through q_items
    const int32_t* q_items;       // bow: query -> keyframe keypoint index (NULL: identity)
    const ovs_keypoint* t_kps;    // area / bow: target keypoints (angle, pt)
    float* prev_matched_xy;       // area: updated for the final matches
    int32_t* assigned;            // projection / area: [n_q] target or -1; bow: [n_t] keyframe keypoint index or -1
    uint32_t key_pool;            // LDS words available for a copy of the key CSR
    int offsets_in_lds;           // the list bounds are staged in LDS (room for n_q + 1 words before the key pool)
    uint32_t best_only_thr;       // BestOnly: accept iff best <= this (match_current_and_last_frames: THR_HIGH)
    int bow_by_query;             // bow (match_keyframes): output [n_out_q] indexed by q_items[q] = target or -1
    int n_out_q;
    int32_t* num_matches;
};

// ---- staging -------------------------------------------------------------------------------------------------------------------
// Per-call staging of host arrays: every array of ONE call is copied into the context's pinned buffer, each on a 256-byte boundary, and goes up
// with ONE copy into the device arena of the same layout (match_window.hip's Stager adds that copy). This is the arithmetic: where an array
// lands, the device address that is, and whether the arena overflowed. Without a host buffer the writer only counts (stage_need_* below).
struct StagePlacement {
    size_t off, bytes;
    const void* src;   // nullptr: reserved, not copied
};
struct StageWriter {
    unsigned char* h;   // pinned host buffer (nullptr: count only)
    unsigned char* d;   // device arena (nullptr: no addresses)
    size_t cap;
    size_t used = 0;
    bool overflow = false;
    StagePlacement* trace = nullptr;   // the host test's record of every placement
    int placed = 0;
    StageWriter(unsigned char* h_, unsigned char* d_, size_t cap_) : h(h_), d(d_), cap(cap_) {}
    unsigned char* place(const void* src, size_t bytes) {
        const size_t off = al256(used);
        if (off + bytes > cap) {
            overflow = true;
            return nullptr;
        }
        if (src && h) std::memcpy(h + off, src, bytes);
        used = off + bytes;
        if (trace) trace[placed] = StagePlacement{off, bytes, src};
        ++placed;
        return d ? d + off : nullptr;
    }
    template <typename T>
    const T* put(const T* src, size_t count) {   // nullptr in -> nullptr out
        return src ? reinterpret_cast<const T*>(place(src, sizeof(T) * count)) : nullptr;
    }
    template <typename T>
    T* reserve(size_t count) {   // device-only scratch in the same arena (filled by a kernel)
        return reinterpret_cast<T*>(place(nullptr, sizeof(T) * count));
    }
};

// One SIDE of a call -- the keypoints that are searched through the grid (the target of a windowed matcher), or either side of a BoW matcher:
// host arrays, staged per call, or a frame / keyframe RESIDENT in HBM (ovs_frame_dev: uploaded and indexed once, when the handle was
// created). Keyframes are the long-lived, immutable objects of the map: mapping_module matches every new keyframe against ~20 covisible
// ones (fuse::replace_duplication), loop closing against more; with the handle none of those calls moves keypoints or descriptors.
struct TargetRef {
    const ovs_keypoint* kps;
    const uint8_t* desc;
    const float* x_right;
    const double* bearings;
    const int32_t* cell_start;   // nullptr: staged, not indexed yet (index_target)
    const int32_t* items;
    GridP gp;
};
// the one place that decides resident or uploaded (`resident`: the handle's arrays, or nullptr); a staged side travels with the Stager's flush.
// bearings: the handle's when it carries them (ovs_frame_dev_attach_bearings), else the caller's
inline TargetRef stage_target(StageWriter& stg, const TargetRef* resident, const ovs_keypoint* kps, const uint8_t* desc, const float* x_right,
                              const double* bearings, int n) {
    TargetRef t{};
    if (resident) {
        t = *resident;
        if (!t.bearings) t.bearings = stg.put(bearings, (size_t)3 * n);
        return t;
    }
    t.kps = stg.put(kps, (size_t)n);
    t.desc = stg.put(desc, (size_t)32 * n);
    t.x_right = stg.put(x_right, (size_t)n);
    t.bearings = stg.put(bearings, (size_t)3 * n);
    return t;
}

// projection::match_frame_and_landmarks: the frame's occupied flags and the landmark side (lm_x_right: nullptr for a monocular frame)
struct LandmarkQueries {
    const uint8_t* occupied;
    const float *xy, *x_right;
    const int32_t* level;
    const uint8_t *valid, *desc;
};
inline LandmarkQueries stage_landmark_queries(StageWriter& stg, const uint8_t* occupied, int n, const float* lm_xy, const float* lm_x_right,
                                              const int32_t* lm_level, const uint8_t* lm_valid, const uint8_t* lm_desc, int m) {
    LandmarkQueries q{};
    q.occupied = stg.put(occupied, (size_t)n);
    q.xy = stg.put(lm_xy, (size_t)2 * m);
    q.x_right = stg.put(lm_x_right, (size_t)m);
    q.level = stg.put(lm_level, (size_t)m);
    q.valid = stg.put(lm_valid, (size_t)m);
    q.desc = stg.put(lm_desc, (size_t)32 * m);
    return q;
}

// tracking_module::search_local_landmarks: the frame's occupied flags, the local landmarks as the map holds them, and the queries
// k_observe_landmarks makes of them (reproj only when the caller asks for it; observable and assigned live in the context's result block)
struct LocalLandmarks {
    const uint8_t* occupied;
    const double *pos, *normal;
    const float* dist;
    const uint8_t *desc, *search;
    float *xy, *x_right;
    int32_t* level;
    double* reproj;
};
inline LocalLandmarks stage_local_landmarks(StageWriter& stg, const uint8_t* occupied, int n, const double* lm_pos_w, const float* lm_dist_min_max,
                                            const double* lm_normal, const uint8_t* lm_desc, const uint8_t* lm_search, int m, bool want_reproj) {
    LocalLandmarks q{};
    q.occupied = stg.put(occupied, (size_t)n);
    q.pos = stg.put(lm_pos_w, (size_t)3 * m);
    q.dist = stg.put(lm_dist_min_max, (size_t)2 * m);
    q.normal = stg.put(lm_normal, (size_t)3 * m);
    q.desc = stg.put(lm_desc, (size_t)32 * m);
    q.search = stg.put(lm_search, (size_t)m);
    q.xy = stg.reserve<float>((size_t)2 * m);
    q.x_right = stg.reserve<float>((size_t)m);
    q.level = stg.reserve<int32_t>((size_t)m);
    q.reproj = want_reproj ? stg.reserve<double>((size_t)2 * m) : nullptr;
    return q;
}
// the result block of a search_local_landmarks call: 8 words of flags and counts, assigned[m], then observable[m] -- one copy down
inline size_t search_result_bytes(int m) { return sizeof(int32_t) * (8 + (size_t)m) + (size_t)m; }

// what k_reproject_queries writes per query, in the staging arena
struct QueryScratch {
    const uint8_t* valid_in;   // the caller's flags (nullptr: every query), read ...
    uint8_t* valid;            // ... and written in place: same index, read-then-write by one lane
    float *xy, *x_right, *radius;
    int32_t *minl, *maxl;
};
inline QueryScratch reserve_queries(StageWriter& stg, const uint8_t* valid, int n) {
    QueryScratch q{};
    q.valid = valid ? const_cast<uint8_t*>(stg.put(valid, (size_t)n)) : stg.reserve<uint8_t>((size_t)n);
    q.valid_in = valid ? q.valid : nullptr;
    q.xy = stg.reserve<float>((size_t)2 * n);
    q.x_right = stg.reserve<float>((size_t)n);
    q.radius = stg.reserve<float>((size_t)n);
    q.minl = stg.reserve<int32_t>((size_t)n);
    q.maxl = stg.reserve<int32_t>((size_t)n);
    return q;
}
// the three reprojecting matchers (match_current_and_last_frames, match_frame_and_keyframe, match_by_Sim3_transform): the target's occupied
// flags, the query side each of them has a part of (nullptr: not this matcher's), the padded scale factors and the queries' scratch
struct ReprojectedQueries {
    const uint8_t* occupied;
    const ovs_keypoint* kps;
    const double* pos;
    const float* dist;
    const double* normal;
    const uint8_t* desc;
    const float* scale;
    QueryScratch q;
};
inline ReprojectedQueries stage_reprojected_queries(StageWriter& stg, const uint8_t* occupied, int n_t, const ovs_keypoint* q_kps, const double* q_pos_w,
                                                    const float* q_dist_min_max, const double* q_normal, const uint8_t* q_desc, const float* sf16,
                                                    const uint8_t* q_valid, int n_q) {
    ReprojectedQueries r{};
    r.occupied = stg.put(occupied, (size_t)n_t);
    r.kps = stg.put(q_kps, (size_t)n_q);
    r.pos = stg.put(q_pos_w, (size_t)3 * n_q);
    r.dist = stg.put(q_dist_min_max, (size_t)2 * n_q);
    r.normal = stg.put(q_normal, (size_t)3 * n_q);
    r.desc = stg.put(q_desc, (size_t)32 * n_q);
    r.scale = stg.put(sf16, (size_t)OVS_MAX_LEVELS);
    r.q = reserve_queries(stg, q_valid, n_q);
    return r;
}

// the landmark side of a k_fuse_best launch
inline void stage_fuse_landmarks(StageWriter& stg, FuseArgs& a, const double* lm_pos_w, const double* lm_normal, const float* lm_dist_min_max,
                                 const uint8_t* lm_desc, const uint8_t* lm_valid, int m) {
    a.m = m;
    a.lm_pos_w = stg.put(lm_pos_w, (size_t)3 * m);
    a.lm_normal = stg.put(lm_normal, (size_t)3 * m);
    a.lm_dist = stg.put(lm_dist_min_max, (size_t)2 * m);
    a.lm_desc = stg.put(lm_desc, (size_t)32 * m);
    a.lm_valid = stg.put(lm_valid, (size_t)m);
}

// one side of a BoW matcher beyond its keypoints: the flags and the feature vector (node CSR: ids | start | items)
struct BowSide {
    const uint8_t* valid;
    const int32_t *node_ids, *node_start, *items;
};
inline BowSide stage_bow_side(StageWriter& stg, const uint8_t* valid, int n, const int32_t* node_ids, const int32_t* node_start, const int32_t* items,
                              int nodes, int n_items) {
    BowSide b{};
    b.valid = stg.put(valid, (size_t)n);
    b.node_ids = stg.put(node_ids, (size_t)nodes);
    b.node_start = stg.put(node_start, (size_t)nodes + 1);
    b.items = stg.put(items, (size_t)n_items);
    return b;
}

// The staging arena holds every array of ONE call, each aligned to 256 bytes, so it is sized for the entry point that stages the most with
// n == max_targets (T) and m == max_queries (Q). Which one that is depends on T : Q, hence three sums (every other entry point stages a subset of
// the first): the host form of projection::match_frame_and_keyframe (with the stereo_x_right that match_current_and_last_frames adds),
// the host form of robust::match_for_triangulation, and the host form of projection::match_keyframes_mutually (n1, n2 <= min(T, Q)).
// (tracking_module::search_local_landmarks stages no query keypoints, radius or level window but the search flags and the double reprojection:
// 121 bytes per query against the first sum's 141, in 13 placements against its 15.)
// tests/test_match_window_plan.py proves stage_need_* <= stage_capacity.
inline size_t stage_capacity(size_t T, size_t Q) {
    const size_t N = std::min(T, Q);
    const size_t cap_window = T * (sizeof(ovs_keypoint)    // target keypoints
                                   + 32                    // target descriptors
                                   + sizeof(float)         // target stereo_x_right
                                   + 1)                    // occupied flags
                              + Q * (sizeof(ovs_keypoint)  // query keypoints
                                     + 3 * sizeof(double)  // world positions
                                     + 3 * sizeof(double)  // mean normals (match_by_Sim3_transform, fuse; those stage no query keypoints: slack)
                                     + 2 * sizeof(float)   // valid distance range
                                     + 32                  // landmark descriptors
                                     + 1                   // valid flags
                                     + 2 * sizeof(float)   // k_reproject_queries: reprojection
                                     + sizeof(float)       //   x_right
                                     + sizeof(float)       //   search radius
                                     + 2 * sizeof(int32_t))   //   level window
                              + sizeof(float) * OVS_MAX_LEVELS   // padded scale factors
                              + 15 * 256;
    const size_t cap_bow = (T + Q) * (sizeof(ovs_keypoint)    // keypoints of either side
                                      + 32                    // descriptors
                                      + 1                     // valid / has-no-landmark flags
                                      + sizeof(float)         // stereo_x_right
                                      + 3 * sizeof(double))   // bearings
                           + sizeof(int32_t) * (4 * (T + Q) + 16)   // the two feature vectors: ids | start | items (<= 3 n + 1 each with no empty node)
                           + 16 * 256;
    const size_t cap_mutual = 2 * N * (sizeof(ovs_keypoint)    // keypoints of either keyframe
                                       + 32                    // descriptors
                                       + 3 * sizeof(double)    // landmark positions
                                       + 2 * sizeof(float)     // valid distance range
                                       + 32                    // landmark descriptors
                                       + 1                     // valid flags
                                       + sizeof(int32_t))      // the one-way result
                              + 14 * 256;
    return std::max(cap_window, std::max(cap_bow, cap_mutual));
}

// ---- each entry point's staging list (match_window.hip's *_impl call these; stage_need_* runs them over a counting writer) ----
struct AreaStaged {
    float* prev;   // prev_matched_pts are read AND updated by the resolver: first in the arena (offset 0), they come back with their own copy
    TargetRef f1, f2;
};
inline AreaStaged stage_area(StageWriter& stg, float* prev_matched_xy, const TargetRef* res_1, const ovs_keypoint* kps_1, const uint8_t* desc_1, int n1,
                             const TargetRef* res_2, const ovs_keypoint* kps_2, const uint8_t* desc_2, int n2) {
    AreaStaged a{};
    a.prev = const_cast<float*>(stg.put(prev_matched_xy, (size_t)2 * n1));
    a.f1 = stage_target(stg, res_1, kps_1, desc_1, nullptr, nullptr, n1);
    a.f2 = stage_target(stg, res_2, kps_2, desc_2, nullptr, nullptr, n2);
    return a;
}
// projection::match_keyframes_mutually: both directions in one arena (a21: the landmarks of keyframe 1 against the keypoints of keyframe 2)
struct MutualStaged {
    int32_t *d_2_in_1, *d_1_in_2;   // the one-way results
    TargetRef t1, t2;
};
inline MutualStaged stage_mutual(StageWriter& stg, FuseArgs& a21, FuseArgs& a12, const TargetRef* res_1, const ovs_keypoint* kps_1, const uint8_t* desc_1,
                                 int n1, const double* lm_pos_w_1, const float* lm_dist_1, const uint8_t* lm_desc_1, const uint8_t* lm_valid_1,
                                 const TargetRef* res_2, const ovs_keypoint* kps_2, const uint8_t* desc_2, int n2, const double* lm_pos_w_2,
                                 const float* lm_dist_2, const uint8_t* lm_desc_2, const uint8_t* lm_valid_2) {
    MutualStaged m{};
    stage_fuse_landmarks(stg, a21, lm_pos_w_1, nullptr, lm_dist_1, lm_desc_1, lm_valid_1, n1);
    stage_fuse_landmarks(stg, a12, lm_pos_w_2, nullptr, lm_dist_2, lm_desc_2, lm_valid_2, n2);
    m.d_2_in_1 = stg.reserve<int32_t>((size_t)n1);
    m.d_1_in_2 = stg.reserve<int32_t>((size_t)n2);
    m.t1 = stage_target(stg, res_1, kps_1, desc_1, nullptr, nullptr, n1);
    m.t2 = stage_target(stg, res_2, kps_2, desc_2, nullptr, nullptr, n2);
    return m;
}
// the three BoW matchers: both sides' keypoints (x_right and bearings: match_for_triangulation), then both sides' flags and feature vectors
struct BowStaged {
    TargetRef kf, frm;
    BowSide kf_fv, frm_fv;
};
inline BowStaged stage_bow(StageWriter& stg, const TargetRef* res_kf, const ovs_keypoint* kf_kps, const uint8_t* kf_desc, const float* kf_x_right,
                           const double* kf_bearings, const uint8_t* kf_valid, int n_kf, const int32_t* kf_node_ids, const int32_t* kf_node_start,
                           const int32_t* kf_items, int kf_nodes, int nq, const TargetRef* res_frm, const ovs_keypoint* frm_kps, const uint8_t* frm_desc,
                           const float* frm_x_right, const double* frm_bearings, const uint8_t* frm_valid, int n_frm, const int32_t* frm_node_ids,
                           const int32_t* frm_node_start, const int32_t* frm_items, int frm_nodes, int nfi) {
    BowStaged b{};
    b.kf = stage_target(stg, res_kf, kf_kps, kf_desc, kf_x_right, kf_bearings, n_kf);
    b.frm = stage_target(stg, res_frm, frm_kps, frm_desc, frm_x_right, frm_bearings, n_frm);
    b.kf_fv = stage_bow_side(stg, kf_valid, n_kf, kf_node_ids, kf_node_start, kf_items, kf_nodes, nq);
    b.frm_fv = stage_bow_side(stg, frm_valid, n_frm, frm_node_ids, frm_node_start, frm_items, frm_nodes, nfi);
    return b;
}

// ---- what an entry point needs of the arena -----------------------------------------------------------------------------------
// stage_need_<entry>: the entry point's own staging functions above, in the order its *_impl calls them, with n targets and m queries and every
// optional array present; returns the bytes used. resident: the _f twin (a handle with stereo_x_right and, for the triangulation matcher,
// bearings). Over a StageCount this is the need that stage_capacity has to cover; the host test also runs them over a real buffer.
struct StageSources {   // one address per element type: real arrays in the host test, never-read addresses when counting
    const ovs_keypoint* kps;
    const uint8_t* u8;
    const float* f32;
    const double* f64;
    const int32_t* i32;
};
struct StageCount {   // a writer without a host buffer and sources it therefore never reads
    StageWriter w{nullptr, nullptr, ~(size_t)0 >> 1};
    StageSources s{reinterpret_cast<const ovs_keypoint*>(256), reinterpret_cast<const uint8_t*>(256), reinterpret_cast<const float*>(256),
                   reinterpret_cast<const double*>(256), reinterpret_cast<const int32_t*>(256)};
};
inline const TargetRef* stage_need_handle(const StageSources& s, bool resident, bool bearings, TargetRef* r) {
    *r = TargetRef{s.kps, s.u8, s.f32, bearings ? s.f64 : nullptr, s.i32, s.i32, GridP{}};
    return resident ? r : nullptr;
}

inline size_t stage_need_grid(StageWriter& stg, const StageSources& s, int n) {
    (void)stg.put(s.kps, (size_t)n);
    return stg.used;
}
inline size_t stage_need_frame_and_landmarks(StageWriter& stg, const StageSources& s, int n, int m, bool resident) {
    TargetRef r;
    (void)stage_target(stg, stage_need_handle(s, resident, false, &r), s.kps, s.u8, s.f32, nullptr, n);
    (void)stage_landmark_queries(stg, s.u8, n, s.f32, s.f32, s.i32, s.u8, s.u8, m);
    return stg.used;
}
inline size_t stage_need_search_local(StageWriter& stg, const StageSources& s, int n, int m, bool resident) {
    TargetRef r;
    (void)stage_target(stg, stage_need_handle(s, resident, false, &r), s.kps, s.u8, s.f32, nullptr, n);
    (void)stage_local_landmarks(stg, s.u8, n, s.f64, s.f32, s.f64, s.u8, s.u8, m, true);
    return stg.used;
}
inline size_t stage_need_area(StageWriter& stg, const StageSources& s, int n, int m, bool resident) {   // n2 = n targets, n1 = m queries
    TargetRef r;
    const TargetRef* h = stage_need_handle(s, resident, false, &r);
    (void)stage_area(stg, const_cast<float*>(s.f32), h, s.kps, s.u8, m, h, s.kps, s.u8, n);
    return stg.used;
}
inline size_t stage_need_current_and_last(StageWriter& stg, const StageSources& s, int n, int m, bool resident) {
    TargetRef r;
    (void)stage_target(stg, stage_need_handle(s, resident, false, &r), s.kps, s.u8, s.f32, nullptr, n);
    (void)stage_reprojected_queries(stg, s.u8, n, s.kps, s.f64, nullptr, nullptr, s.u8, s.f32, s.u8, m);
    return stg.used;
}
inline size_t stage_need_frame_and_keyframe(StageWriter& stg, const StageSources& s, int n, int m, bool resident) {
    TargetRef r;
    (void)stage_reprojected_queries(stg, s.u8, n, s.kps, s.f64, s.f32, nullptr, s.u8, s.f32, s.u8, m);
    (void)stage_target(stg, stage_need_handle(s, resident, false, &r), s.kps, s.u8, nullptr, nullptr, n);
    return stg.used;
}
inline size_t stage_need_sim3_transform(StageWriter& stg, const StageSources& s, int n, int m, bool resident) {
    TargetRef r;
    (void)stage_reprojected_queries(stg, s.u8, n, nullptr, s.f64, s.f32, s.f64, s.u8, s.f32, s.u8, m);
    (void)stage_target(stg, stage_need_handle(s, resident, false, &r), s.kps, s.u8, nullptr, nullptr, n);
    return stg.used;
}
inline size_t stage_need_fuse(StageWriter& stg, const StageSources& s, int n, int m, bool resident) {   // replace_duplication; detect_ stages no x_right
    TargetRef r;
    FuseArgs a{};
    stage_fuse_landmarks(stg, a, s.f64, s.f64, s.f32, s.u8, s.u8, m);
    (void)stage_target(stg, stage_need_handle(s, resident, false, &r), s.kps, s.u8, s.f32, nullptr, n);
    return stg.used;
}
inline size_t stage_need_mutual(StageWriter& stg, const StageSources& s, int n1, int n2, bool resident) {
    TargetRef r;
    FuseArgs a21{}, a12{};
    const TargetRef* h = stage_need_handle(s, resident, false, &r);
    (void)stage_mutual(stg, a21, a12, h, s.kps, s.u8, n1, s.f64, s.f32, s.u8, s.u8, h, s.kps, s.u8, n2, s.f64, s.f32, s.u8, s.u8);
    return stg.used;
}
// n_frm = n targets, n_kf = m queries, the two feature vectors' sizes; tri: robust::match_for_triangulation (x_right and bearings of either side)
inline size_t stage_need_bow(StageWriter& stg, const StageSources& s, int n, int m, int kf_nodes, int nq, int frm_nodes, int nfi, bool tri, bool resident) {
    TargetRef r;
    const TargetRef* h = stage_need_handle(s, resident, tri, &r);
    const float* xr = tri ? s.f32 : nullptr;
    const double* br = tri ? s.f64 : nullptr;
    (void)stage_bow(stg, h, s.kps, s.u8, xr, br, s.u8, m, s.i32, s.i32, s.i32, kf_nodes, nq, h, s.kps, s.u8, xr, br, s.u8, n, s.i32, s.i32, s.i32, frm_nodes, nfi);
    return stg.used;
}

}   // namespace ovs
