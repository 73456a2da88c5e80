// solve_plan.inc -- everything the nine batch calls on the scaffold of solve_internal.inc decide on the host: ovs_sim3_*, ovs_pnp_*,
// ovs_sim3opt_*, ovs_twoview_*, ovs_essential_*, ovs_reconstruct_*, ovs_triangulate_* and both forms of ovs_landmarks_*. Per family: the
// Layout of the staged block (the kernels recompute it from (P, T), so layout_of is __host__ __device__ under hipcc), a Call holding the
// ABI's arguments, check (the argument errors in the ABI's order, then capacity, then what staging used to refuse halfway), stage (the
// copies into the page-locked block at the layout's offsets) and, where results come back through the block, collect. Plain C++, no HIP
// header: the units include it, tests/solve_plan_host.cc builds it with the host compiler alone, also under the sanitizers. This is the
// one place these are computed. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

#include "../../include/ovslam_hip.h"
#include "reconstruct_math.inc"
#include "sim3_opt_math.inc"
#include "triangulate_math.inc"

#if defined(__HIPCC__) || defined(__HIP__)
#define SPLAN_FN __host__ __device__ inline
#else
#define SPLAN_FN inline
#endif

namespace splan {

constexpr int kMaxIter = 1 << 20;   // h takes 20 bits of the sampler's counter

// what a check decides: the status, the call's matches and whether there is anything to run (OVS_OK without it: no problems)
struct Checked {
    ovs_status status;
    int32_t T;
    bool run;
};
constexpr Checked refused(ovs_status st) { return Checked{st, 0, false}; }

inline bool all_set(std::initializer_list<const void*> pointers) {
    for (const void* q : pointers)
        if (!q) return false;
    return true;
}

// a handle's limits, fixed at its create. A check takes them as a callable and asks once, after every argument error: the errors that need no
// handle are decided without reading one (a caller's stale handle is not touched for them).
struct Caps {
    int32_t max_problems, max_total_matches, max_keyframes, device;   // the last two: the landmark handle's
};

// The check every call starts with (a solver's scalar checks may precede it). `required`: the pointers every call needs are set;
// `per_match`: so are the arrays needed once there is a match, the per-match outputs among them. Nothing is truncated. `read`: where to
// leave the handle's limits for a check that goes on.
template <class CapsOf>
Checked check_common(bool handle, int32_t n_problems, const int32_t* offsets, bool required, bool per_match, CapsOf caps_of, Caps* read = nullptr) {
    if (!handle || n_problems < 0) return refused(OVS_ERR_INVALID);
    if (n_problems == 0) return Checked{OVS_OK, 0, false};
    if (!offsets || !required) return refused(OVS_ERR_INVALID);
    if (offsets[0] != 0) return refused(OVS_ERR_INVALID);
    for (int32_t p = 0; p < n_problems; ++p)
        if (offsets[p + 1] < offsets[p]) return refused(OVS_ERR_INVALID);
    const int32_t T = offsets[n_problems];
    if (T > 0 && !per_match) return refused(OVS_ERR_INVALID);
    const Caps caps = caps_of();
    if (read) *read = caps;
    if (n_problems > caps.max_problems || T > caps.max_total_matches) return refused(OVS_ERR_CAPACITY);
    return Checked{OVS_OK, T, true};
}

// what run_batch puts before it: the two RANSAC scalars
inline bool ransac_scalars_ok(int32_t max_num_iter, int32_t min_num_inliers) {
    return max_num_iter >= 1 && max_num_iter <= kMaxIter && min_num_inliers >= 0;
}

inline void stage_offsets(uint8_t* h_block, size_t at, const int32_t* offsets, int32_t n_problems) {
    std::memcpy(h_block + at, offsets, 4 * ((size_t)n_problems + 1));
}

// an ovs_camera as the kernels read it (Rec: a, b, c, d, model, pad): perspective (fx, fy, cx, cy) or equirectangular ((double)cols,
// (double)rows, -, -); false for an unknown model or intrinsics a kernel cannot use
template <class Rec>
bool camera_ok(const ovs_camera& c, Rec* rec) {
    rec->pad = 0;
    rec->model = c.model;
    if (c.model == 0) {
        if (!std::isfinite(c.fx) || !std::isfinite(c.fy) || !std::isfinite(c.cx) || !std::isfinite(c.cy)) return false;
        rec->a = c.fx, rec->b = c.fy, rec->c = c.cx, rec->d = c.cy;
        return true;
    }
    if (c.model == 1) {
        if (c.cols < 1 || c.rows < 1) return false;
        rec->a = (double)c.cols, rec->b = (double)c.rows, rec->c = 0.0, rec->d = 0.0;
        return true;
    }
    return false;
}

// both sides' cameras of every problem are ones camera_ok accepts
template <class Rec>
bool cameras_ok(const ovs_camera* cams_1, const ovs_camera* cams_2, int32_t n_problems) {
    Rec rec;
    for (int32_t p = 0; p < n_problems; ++p)
        if (!camera_ok(cams_1[p], &rec) || !camera_ok(cams_2[p], &rec)) return false;
    return true;
}

// ---- ovs_sim3_solve_batch (sim3_solve.hip)
namespace sim3 {

// one side's camera as the kernels read it: perspective (fx, fy, cx, cy) or equirectangular ((double)cols, (double)rows, -, -)
struct CamRec {
    double a, b, c, d;
    int32_t model, pad;
};
static_assert(sizeof(CamRec) == 40, "CamRec is laid out in the staged block by the host");

// The staged block of one call, sections in this order (each a multiple of 8 bytes but the last): keys u64 [P] (zero), cameras CamRec [2 P]
// (side 1 then side 2 of a problem), p1 f64 [3 T], p2 f64 [3 T], thr1 f32 [T'], thr2 f32 [T'], offsets i32 [P + 1]; T' = T rounded up to even.
struct Layout {
    size_t keys, cams, p1, p2, thr1, thr2, offsets, bytes;
};
SPLAN_FN Layout layout_of(int P, int T) {
    const size_t Te = ((size_t)T + 1) & ~(size_t)1;
    Layout l;
    l.keys = 0;
    l.cams = l.keys + 8 * (size_t)P;
    l.p1 = l.cams + sizeof(CamRec) * 2 * (size_t)P;
    l.p2 = l.p1 + 24 * (size_t)T;
    l.thr1 = l.p2 + 24 * (size_t)T;
    l.thr2 = l.thr1 + 4 * Te;
    l.offsets = l.thr2 + 4 * Te;
    l.bytes = l.offsets + 4 * ((size_t)P + 1);
    return l;
}

struct Call {
    bool handle;
    int32_t n_problems;
    const int32_t* offsets;
    const double *p1, *p2;
    const float *thr1, *thr2;
    const ovs_camera *cams_1, *cams_2;
    int32_t min_num_inliers, max_num_iter;
    const int32_t *out_valid, *out_best_iter, *out_num_inliers;
    const double *out_rot, *out_trans, *out_scale;
    const uint8_t* out_flags;
};

template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (!ransac_scalars_ok(c.max_num_iter, c.min_num_inliers)) return refused(OVS_ERR_INVALID);
    const Checked k = check_common(c.handle, c.n_problems, c.offsets,
                                   all_set({c.out_valid, c.out_best_iter, c.out_num_inliers, c.out_rot, c.out_trans, c.out_scale, c.cams_1, c.cams_2}),
                                   all_set({c.p1, c.p2, c.thr1, c.thr2, c.out_flags}), caps_of);
    if (k.run && !cameras_ok<CamRec>(c.cams_1, c.cams_2, c.n_problems)) return refused(OVS_ERR_INVALID);
    return k;
}

inline void stage(const Call& c, const Layout& lay, uint8_t* h_block) {
    const size_t T = (size_t)c.offsets[c.n_problems];
    std::memset(h_block + lay.keys, 0, 8 * (size_t)c.n_problems);
    CamRec* cams = reinterpret_cast<CamRec*>(h_block + lay.cams);
    for (int32_t p = 0; p < c.n_problems; ++p) {
        camera_ok(c.cams_1[p], &cams[2 * p]);
        camera_ok(c.cams_2[p], &cams[2 * p + 1]);
    }
    if (T > 0) {
        std::memcpy(h_block + lay.p1, c.p1, 24 * T);
        std::memcpy(h_block + lay.p2, c.p2, 24 * T);
        std::memcpy(h_block + lay.thr1, c.thr1, 4 * T);
        std::memcpy(h_block + lay.thr2, c.thr2, 4 * T);
    }
    stage_offsets(h_block, lay.offsets, c.offsets, c.n_problems);
}

}   // namespace sim3

// ---- ovs_pnp_solve_batch (pnp_solve.hip)
namespace pnp {

// The staged block of one call, sections in this order: keys u64 [P] (zero), bearings f64 [3 T], pos_w f64 [3 T], max_cos_error f64 [T],
// offsets i32 [P + 1].
struct Layout {
    size_t keys, bearings, pos_w, max_cos, offsets, bytes;
};
SPLAN_FN Layout layout_of(int P, int T) {
    Layout l;
    l.keys = 0;
    l.bearings = l.keys + 8 * (size_t)P;
    l.pos_w = l.bearings + 24 * (size_t)T;
    l.max_cos = l.pos_w + 24 * (size_t)T;
    l.offsets = l.max_cos + 8 * (size_t)T;
    l.bytes = l.offsets + 4 * ((size_t)P + 1);
    return l;
}

struct Call {
    bool handle;
    int32_t n_problems;
    const int32_t* offsets;
    const double *bearings, *pos_w, *max_cos_errors;
    int32_t min_num_inliers, max_num_iter;
    const int32_t *out_valid, *out_best_iter, *out_num_inliers;
    const double *out_rot, *out_trans;
    const uint8_t* out_flags;
};

template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (!ransac_scalars_ok(c.max_num_iter, c.min_num_inliers)) return refused(OVS_ERR_INVALID);
    return check_common(c.handle, c.n_problems, c.offsets, all_set({c.out_valid, c.out_best_iter, c.out_num_inliers, c.out_rot, c.out_trans}),
                        all_set({c.bearings, c.pos_w, c.max_cos_errors, c.out_flags}), caps_of);
}

inline void stage(const Call& c, const Layout& lay, uint8_t* h_block) {
    const size_t T = (size_t)c.offsets[c.n_problems];
    std::memset(h_block + lay.keys, 0, 8 * (size_t)c.n_problems);
    if (T > 0) {
        std::memcpy(h_block + lay.bearings, c.bearings, 24 * T);
        std::memcpy(h_block + lay.pos_w, c.pos_w, 24 * T);
        std::memcpy(h_block + lay.max_cos, c.max_cos_errors, 8 * T);
    }
    stage_offsets(h_block, lay.offsets, c.offsets, c.n_problems);
}

}   // namespace pnp

// ---- ovs_sim3opt_optimize_batch (sim3_opt.hip)
namespace sim3opt {

static_assert(sizeof(s3::Cam) == 40, "s3::Cam is laid out in the staged block by the host");

// The staged block of one call, sections in this order (each a multiple of 8 bytes but the last two): cameras s3::Cam [2 P] (side 1 then
// side 2 of a problem), init f64 [13 P] (R12, t12, s12), p1 f64 [3 T], p2 f64 [3 T], obs1 f64 [2 T], obs2 f64 [2 T], w1 f32 [T'], w2 f32 [T'],
// offsets i32 [P + 1], work u8 [T] (the kernel's outlier flags; nothing is staged there); T' = T rounded up to even.
struct Layout {
    size_t cams, init, p1, p2, obs1, obs2, w1, w2, offsets, work, bytes;
};
SPLAN_FN Layout layout_of(int P, int T) {
    const size_t Te = ((size_t)T + 1) & ~(size_t)1;
    Layout l;
    l.cams = 0;
    l.init = l.cams + sizeof(s3::Cam) * 2 * (size_t)P;
    l.p1 = l.init + 8 * 13 * (size_t)P;
    l.p2 = l.p1 + 24 * (size_t)T;
    l.obs1 = l.p2 + 24 * (size_t)T;
    l.obs2 = l.obs1 + 16 * (size_t)T;
    l.w1 = l.obs2 + 16 * (size_t)T;
    l.w2 = l.w1 + 4 * Te;
    l.offsets = l.w2 + 4 * Te;
    l.work = l.offsets + 4 * ((size_t)P + 1);
    l.bytes = l.work + (size_t)T;
    return l;
}

struct Call {
    bool handle;
    int32_t n_problems;
    const int32_t* offsets;
    const double *p1, *p2, *obs1, *obs2;
    const float *inv_sigma_sq_1, *inv_sigma_sq_2;
    const ovs_camera *cams_1, *cams_2;
    const double *rot_12_in, *trans_12_in, *scale_12_in;
    float chi_sq;
    int32_t num_iter;
    const int32_t* out_num_inliers;
    const double *out_rot, *out_trans, *out_scale;
    const uint8_t* out_flags;
};

template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (!(c.chi_sq > 0.0f) || !std::isfinite(c.chi_sq) || c.num_iter < 1) return refused(OVS_ERR_INVALID);
    const Checked k = check_common(
        c.handle, c.n_problems, c.offsets,
        all_set({c.cams_1, c.cams_2, c.rot_12_in, c.trans_12_in, c.scale_12_in, c.out_num_inliers, c.out_rot, c.out_trans, c.out_scale}),
        all_set({c.p1, c.p2, c.obs1, c.obs2, c.inv_sigma_sq_1, c.inv_sigma_sq_2, c.out_flags}), caps_of);
    if (k.run && !cameras_ok<s3::Cam>(c.cams_1, c.cams_2, c.n_problems)) return refused(OVS_ERR_INVALID);
    return k;
}

inline void stage(const Call& c, const Layout& lay, uint8_t* h_block) {
    const size_t T = (size_t)c.offsets[c.n_problems];
    s3::Cam* cams = reinterpret_cast<s3::Cam*>(h_block + lay.cams);
    double* init = reinterpret_cast<double*>(h_block + lay.init);
    for (int32_t p = 0; p < c.n_problems; ++p) {
        camera_ok(c.cams_1[p], &cams[2 * p]);
        camera_ok(c.cams_2[p], &cams[2 * p + 1]);
        std::memcpy(init + 13 * (size_t)p, c.rot_12_in + 9 * (size_t)p, 72);
        std::memcpy(init + 13 * (size_t)p + 9, c.trans_12_in + 3 * (size_t)p, 24);
        init[13 * (size_t)p + 12] = c.scale_12_in[p];
    }
    if (T > 0) {
        std::memcpy(h_block + lay.p1, c.p1, 24 * T);
        std::memcpy(h_block + lay.p2, c.p2, 24 * T);
        std::memcpy(h_block + lay.obs1, c.obs1, 16 * T);
        std::memcpy(h_block + lay.obs2, c.obs2, 16 * T);
        std::memcpy(h_block + lay.w1, c.inv_sigma_sq_1, 4 * T);
        std::memcpy(h_block + lay.w2, c.inv_sigma_sq_2, 4 * T);
        std::memset(h_block + lay.work, 0, T);
    }
    stage_offsets(h_block, lay.offsets, c.offsets, c.n_problems);
}

}   // namespace sim3opt

// ---- ovs_twoview_solve_batch (two_view_solve.hip)
namespace twoview {

// The staged block of one call, sections in this order: x1 f64 [2 T], x2 f64 [2 T], offsets i32 [P + 1].
struct Layout {
    size_t x1, x2, offsets, bytes;
};
SPLAN_FN Layout layout_of(int P, int T) {
    Layout l;
    l.x1 = 0;
    l.x2 = l.x1 + 16 * (size_t)T;
    l.offsets = l.x2 + 16 * (size_t)T;
    l.bytes = l.offsets + 4 * ((size_t)P + 1);
    return l;
}

struct Call {
    bool handle;
    int32_t n_problems;
    const int32_t* offsets;
    const double *x1, *x2;
    double sigma;
    int32_t max_num_iter, models;
    const double *out_H_21, *out_F_21, *out_scores;
    const int32_t *out_valid, *out_best_iter, *out_num_inliers, *out_selected;
    const uint8_t *out_flags_H, *out_flags_F;
};

template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (c.max_num_iter < 1 || c.max_num_iter > kMaxIter || c.models < 1 || c.models > 3 || !(c.sigma > 0.0) || !std::isfinite(c.sigma))
        return refused(OVS_ERR_INVALID);
    return check_common(c.handle, c.n_problems, c.offsets,
                        all_set({c.out_H_21, c.out_F_21, c.out_scores, c.out_valid, c.out_best_iter, c.out_num_inliers, c.out_selected}),
                        all_set({c.x1, c.x2, c.out_flags_F, c.out_flags_H}), caps_of);
}

inline void stage(const Call& c, const Layout& lay, uint8_t* h_block) {
    const size_t T = (size_t)c.offsets[c.n_problems];
    if (T > 0) {
        std::memcpy(h_block + lay.x1, c.x1, 16 * T);
        std::memcpy(h_block + lay.x2, c.x2, 16 * T);
    }
    stage_offsets(h_block, lay.offsets, c.offsets, c.n_problems);
}

}   // namespace twoview

// ---- ovs_essential_solve_batch (essential_solve.hip)
namespace essential {

// The staged block of one call, sections in this order: b1 f64 [3 T], b2 f64 [3 T], offsets i32 [P + 1].
struct Layout {
    size_t b1, b2, offsets, bytes;
};
SPLAN_FN Layout layout_of(int P, int T) {
    Layout l;
    l.b1 = 0;
    l.b2 = l.b1 + 24 * (size_t)T;
    l.offsets = l.b2 + 24 * (size_t)T;
    l.bytes = l.offsets + 4 * ((size_t)P + 1);
    return l;
}

struct Call {
    bool handle;
    int32_t n_problems;
    const int32_t* offsets;
    const double *bearings_1, *bearings_2;
    double residual_cos_thr;
    int32_t max_num_iter;
    const double *out_E_21, *out_scores;
    const int32_t *out_valid, *out_best_iter, *out_num_inliers;
    const uint8_t* out_flags;
};

template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (c.max_num_iter < 1 || c.max_num_iter > kMaxIter || !std::isfinite(c.residual_cos_thr) || !(c.residual_cos_thr > 0.0) ||
        !(c.residual_cos_thr <= 1.0))
        return refused(OVS_ERR_INVALID);
    return check_common(c.handle, c.n_problems, c.offsets, all_set({c.out_E_21, c.out_scores, c.out_valid, c.out_best_iter, c.out_num_inliers}),
                        all_set({c.bearings_1, c.bearings_2, c.out_flags}), caps_of);
}

inline void stage(const Call& c, const Layout& lay, uint8_t* h_block) {
    const size_t T = (size_t)c.offsets[c.n_problems];
    if (T > 0) {
        std::memcpy(h_block + lay.b1, c.bearings_1, 24 * T);
        std::memcpy(h_block + lay.b2, c.bearings_2, 24 * T);
    }
    stage_offsets(h_block, lay.offsets, c.offsets, c.n_problems);
}

}   // namespace essential

// ---- ovs_reconstruct_batch (two_view_reconstruct.hip)
namespace reconstruct {

static_assert(sizeof(rec::Problem) == 112, "rec::Problem is laid out in the staged block by the host");

// The staged block of one call, sections in this order: problems rec::Problem [P], kp_ref f64 [2 T], kp_cur f64 [2 T], b_ref f64 [3 T],
// b_cur f64 [3 T], offsets i32 [P + 1], inlier u8 [T].
struct Layout {
    size_t problems, kp1, kp2, b1, b2, offsets, inlier, bytes;
};
SPLAN_FN Layout layout_of(int P, int T) {
    Layout l;
    l.problems = 0;
    l.kp1 = l.problems + sizeof(rec::Problem) * (size_t)P;
    l.kp2 = l.kp1 + 16 * (size_t)T;
    l.b1 = l.kp2 + 16 * (size_t)T;
    l.b2 = l.b1 + 24 * (size_t)T;
    l.offsets = l.b2 + 24 * (size_t)T;
    l.inlier = l.offsets + 4 * ((size_t)P + 1);
    l.bytes = l.inlier + (size_t)T;
    return l;
}

struct Call {
    bool handle;
    int32_t n_problems;
    const int32_t *offsets, *models;
    const double* mats;
    const ovs_camera* cams;
    const uint8_t* inlier_flags;
    const double *keypts_ref, *keypts_cur, *bearings_ref, *bearings_cur;
    float reproj_err_thr, parallax_deg_thr;
    const int32_t *out_success, *out_best;
    const double *out_rot, *out_trans;
    const int32_t* out_counts;
    const float* out_parallax_deg;
    const double* out_triangulated_pts;
    const uint8_t* out_is_triangulated;
};

template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (!(c.reproj_err_thr > 0.0f) || !std::isfinite(c.reproj_err_thr) || !(c.parallax_deg_thr > 0.0f) || !std::isfinite(c.parallax_deg_thr))
        return refused(OVS_ERR_INVALID);
    const Checked k = check_common(
        c.handle, c.n_problems, c.offsets,
        all_set({c.models, c.mats, c.cams, c.out_success, c.out_best, c.out_rot, c.out_trans, c.out_counts, c.out_parallax_deg}),
        all_set({c.inlier_flags, c.keypts_ref, c.keypts_cur, c.bearings_ref, c.bearings_cur, c.out_triangulated_pts, c.out_is_triangulated}),
        caps_of);
    if (!k.run) return k;
    for (int32_t p = 0; p < c.n_problems; ++p) {
        const ovs_camera& cam = c.cams[p];
        if (c.models[p] < 1 || c.models[p] > 2 || cam.model != 0) return refused(OVS_ERR_INVALID);
        if (!std::isfinite(cam.fx) || !std::isfinite(cam.fy) || !std::isfinite(cam.cx) || !std::isfinite(cam.cy) || cam.fx == 0.0 || cam.fy == 0.0)
            return refused(OVS_ERR_INVALID);
    }
    return k;
}

inline void stage(const Call& c, const Layout& lay, uint8_t* h_block) {
    const size_t T = (size_t)c.offsets[c.n_problems];
    rec::Problem* problems = reinterpret_cast<rec::Problem*>(h_block + lay.problems);
    for (int32_t p = 0; p < c.n_problems; ++p) {
        const ovs_camera& cam = c.cams[p];
        rec::Problem& q = problems[p];
        std::memcpy(q.mat, c.mats + 9 * (size_t)p, sizeof(q.mat));
        q.fx = cam.fx, q.fy = cam.fy, q.cx = cam.cx, q.cy = cam.cy;
        q.model = c.models[p];
        q.pad = 0;
    }
    if (T > 0) {
        std::memcpy(h_block + lay.kp1, c.keypts_ref, 16 * T);
        std::memcpy(h_block + lay.kp2, c.keypts_cur, 16 * T);
        std::memcpy(h_block + lay.b1, c.bearings_ref, 24 * T);
        std::memcpy(h_block + lay.b2, c.bearings_cur, 24 * T);
        std::memcpy(h_block + lay.inlier, c.inlier_flags, T);
    }
    stage_offsets(h_block, lay.offsets, c.offsets, c.n_problems);
}

}   // namespace reconstruct

// ---- ovs_triangulate_batch (triangulate.hip)
namespace triangulate {

static_assert(sizeof(tri::Cam) == 56 && sizeof(tri::Problem) == 352 && sizeof(tri::Problem) % 8 == 0,
              "tri::Problem is laid out in the staged block by the host");

// The staged block of one call, sections in this order: problems tri::Problem [P], b1 f64 [3][T], b2 f64 [3][T] (planes: x of every match, then
// y, then z), then planes of f32 [T'] each: kp1 x y, kp2 x y, x_right 1 2, depth 1 2, sigma_sq 1 2, scale_factor 1 2 (12 planes), the problem
// index i32 [T'], offsets i32 [P' + 1]; then what the kernel writes and the host copies back: pos f64 [3][T], status u8 [T], method u8 [T].
// T' = T rounded up to even, P' + 1 = P + 1 rounded up to even: every f64 section is 8-byte aligned.
struct Layout {
    size_t problems, b1, b2, f32, pidx, offsets, pos, status, method, bytes;
    size_t Te;
};
constexpr int kFloatPlanes = 12;
SPLAN_FN Layout layout_of(int P, int T) {
    Layout l;
    l.Te = ((size_t)T + 1) & ~(size_t)1;
    l.problems = 0;
    l.b1 = l.problems + sizeof(tri::Problem) * (size_t)P;
    l.b2 = l.b1 + 24 * (size_t)T;
    l.f32 = l.b2 + 24 * (size_t)T;
    l.pidx = l.f32 + 4 * kFloatPlanes * l.Te;
    l.offsets = l.pidx + 4 * l.Te;
    l.pos = l.offsets + 4 * ((((size_t)P + 1) + 1) & ~(size_t)1);
    l.status = l.pos + 24 * (size_t)T;
    l.method = l.status + (size_t)T;
    l.bytes = l.method + (size_t)T;
    return l;
}

// an ovs_camera as rule T2, T5 and T7 read it; false for what the ABI refuses
inline bool triangulation_camera_ok(const ovs_camera& c, tri::Cam* rec) {
    if (!camera_ok(c, rec)) return false;
    if (c.model == 0 && (c.fx == 0.0 || c.fy == 0.0)) return false;
    rec->focal_x_baseline = c.focal_x_baseline;
    rec->true_baseline = c.true_baseline;
    return true;
}

struct Call {
    bool handle;
    int32_t n_problems;
    const int32_t* offsets;
    const double *bearings_1, *bearings_2;
    const float *keypts_1, *keypts_2, *x_right_1, *x_right_2, *depths_1, *depths_2, *sigma_sq_1, *sigma_sq_2, *scale_factors_1, *scale_factors_2;
    const ovs_camera *cams_1, *cams_2;
    const double *poses_cw_1, *poses_cw_2;
    double cos_rays_parallax_thr;
    float ratio_factor;
    double* out_pos_w;
    uint8_t *out_status, *out_method;
    int32_t* out_num_accepted;
};

template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (!std::isfinite(c.cos_rays_parallax_thr) || !std::isfinite(c.ratio_factor)) return refused(OVS_ERR_INVALID);
    const Checked k = check_common(c.handle, c.n_problems, c.offsets, all_set({c.cams_1, c.cams_2, c.poses_cw_1, c.poses_cw_2, c.out_num_accepted}),
                                   all_set({c.bearings_1, c.bearings_2, c.keypts_1, c.keypts_2, c.x_right_1, c.x_right_2, c.depths_1, c.depths_2,
                                            c.sigma_sq_1, c.sigma_sq_2, c.scale_factors_1, c.scale_factors_2, c.out_status, c.out_method, c.out_pos_w}),
                                   caps_of);
    if (!k.run) return k;
    tri::Cam cam;
    for (int32_t p = 0; p < c.n_problems; ++p)
        if (!triangulation_camera_ok(c.cams_1[p], &cam) || !triangulation_camera_ok(c.cams_2[p], &cam)) return refused(OVS_ERR_INVALID);
    return k;
}

inline void stage(const Call& c, const Layout& lay, uint8_t* h_block) {
    const int32_t T = c.offsets[c.n_problems];
    tri::Problem* problems = reinterpret_cast<tri::Problem*>(h_block + lay.problems);
    for (int32_t p = 0; p < c.n_problems; ++p) {
        tri::Problem& q = problems[p];
        triangulation_camera_ok(c.cams_1[p], &q.cam[0]);
        triangulation_camera_ok(c.cams_2[p], &q.cam[1]);
        std::memcpy(q.pose[0], c.poses_cw_1 + 12 * (size_t)p, 96);
        std::memcpy(q.pose[1], c.poses_cw_2 + 12 * (size_t)p, 96);
        tri::set_centres(q);
    }
    if (T > 0) {
        double* b1 = reinterpret_cast<double*>(h_block + lay.b1);
        double* b2 = reinterpret_cast<double*>(h_block + lay.b2);
        float* f = reinterpret_cast<float*>(h_block + lay.f32);
        int32_t* pidx = reinterpret_cast<int32_t*>(h_block + lay.pidx);
        const auto fplane = [&](int k) { return f + (size_t)k * lay.Te; };
        for (int32_t i = 0; i < T; ++i) {
            for (int x = 0; x < 3; ++x) {
                b1[(size_t)x * T + i] = c.bearings_1[3 * (size_t)i + x];
                b2[(size_t)x * T + i] = c.bearings_2[3 * (size_t)i + x];
            }
            for (int x = 0; x < 2; ++x) {
                fplane(x)[i] = c.keypts_1[2 * (size_t)i + x];
                fplane(2 + x)[i] = c.keypts_2[2 * (size_t)i + x];
            }
        }
        std::memcpy(fplane(4), c.x_right_1, 4 * (size_t)T);
        std::memcpy(fplane(5), c.x_right_2, 4 * (size_t)T);
        std::memcpy(fplane(6), c.depths_1, 4 * (size_t)T);
        std::memcpy(fplane(7), c.depths_2, 4 * (size_t)T);
        std::memcpy(fplane(8), c.sigma_sq_1, 4 * (size_t)T);
        std::memcpy(fplane(9), c.sigma_sq_2, 4 * (size_t)T);
        std::memcpy(fplane(10), c.scale_factors_1, 4 * (size_t)T);
        std::memcpy(fplane(11), c.scale_factors_2, 4 * (size_t)T);
        for (int32_t p = 0; p < c.n_problems; ++p)
            for (int32_t i = c.offsets[p]; i < c.offsets[p + 1]; ++i) pidx[i] = p;
    }
    stage_offsets(h_block, lay.offsets, c.offsets, c.n_problems);
}

// the sections the kernel wrote, copied back into h_block, to the caller's arrays
inline void collect(const Call& c, const Layout& lay, const uint8_t* h_block) {
    const int32_t T = c.offsets[c.n_problems];
    const double* pos = reinterpret_cast<const double*>(h_block + lay.pos);
    const uint8_t* status = h_block + lay.status;
    for (int32_t i = 0; i < T; ++i)
        for (int x = 0; x < 3; ++x) c.out_pos_w[3 * (size_t)i + x] = pos[(size_t)x * T + i];
    if (T > 0) {
        std::memcpy(c.out_status, status, (size_t)T);
        std::memcpy(c.out_method, h_block + lay.method, (size_t)T);
    }
    for (int32_t p = 0; p < c.n_problems; ++p) {
        int32_t accepted = 0;
        for (int32_t i = c.offsets[p]; i < c.offsets[p + 1]; ++i) accepted += status[i] == 0 ? 1 : 0;
        c.out_num_accepted[p] = accepted;
    }
}

}   // namespace triangulate

// ---- ovs_landmarks_update_batch and ovs_landmarks_update_batch_f (landmark_update.hip): a "problem" is a landmark, its "matches" are its
// observations
namespace landmarks {

constexpr int kMaxObsPerLandmark = 1 << 22;   // the ordinal's share of the winner's key

SPLAN_FN size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// The staged block of one call, every section 16-byte aligned. Inputs: pos f64 [3][P] (planes), sf_ref f32 [P] (scale_factors[ref_level]),
// ref_slot i32 [P], offsets i32 [P + 1], obs_slot i32 [T], used i32 [T] (per landmark, from its offset on: the observations that take part in
// the descriptor, as indices into the call's observations), n_used i32 [P], list8 i32 [P], list64 i32 [P], obs_kp i32 [T] (_f form), desc
// u8 [T][32]. Then what the kernels write and the host copies back: normal f64 [3][P], range f32 [2][P], best i32 [P], out_desc u8 [P][32].
// `bytes` is what a call uploads: WITH_DESC = false ends it before the descriptors (a geometry-only call, or the _f form).
struct Layout {
    size_t pos, sf_ref, ref_slot, offsets, obs_slot, used, n_used, list8, list64, obs_kp, desc, normal, range, best, out_desc, total, bytes;
};
template <bool WITH_DESC>
SPLAN_FN Layout layout_of(int P, int T) {
    Layout l;
    const size_t p4 = al16(4 * (size_t)P), t4 = al16(4 * (size_t)T);
    l.pos = 0;
    l.sf_ref = l.pos + al16(24 * (size_t)P);
    l.ref_slot = l.sf_ref + p4;
    l.offsets = l.ref_slot + p4;
    l.obs_slot = l.offsets + al16(4 * ((size_t)P + 1));
    l.used = l.obs_slot + t4;
    l.n_used = l.used + t4;
    l.list8 = l.n_used + p4;
    l.list64 = l.list8 + p4;
    l.obs_kp = l.list64 + p4;
    l.desc = l.obs_kp + t4;
    l.normal = l.desc + 32 * (size_t)T;
    l.range = l.normal + al16(24 * (size_t)P);
    l.best = l.range + al16(8 * (size_t)P);
    l.out_desc = l.best + p4;
    l.total = l.out_desc + 32 * (size_t)P;
    l.bytes = WITH_DESC ? l.normal : l.desc;
    return l;
}

// The per-call keyframe table, a buffer of its own: camera centres f64 [K][3], then (_f form) the descriptors' device pointers [K].
inline size_t table_ptrs_at(int32_t K) { return 24 * (size_t)(K > 0 ? K : 0); }
inline size_t table_bytes(int32_t K) { return table_ptrs_at(K) + 8 * (size_t)(K > 0 ? K : 0); }

// a resident keyframe as the _f form reads it; device -1: the caller's entry is null
struct KeyframeView {
    int32_t device, n;
    const uint8_t* d_desc;
};

struct Call {
    bool handle;
    int32_t what, n_landmarks;
    const int32_t* offsets;
    const double* pos_w;
    const int32_t *ref_keyfrm, *ref_level, *obs_keyfrm;
    const uint8_t* obs_desc;
    bool resident;                                                // the _f form
    const void* keyfrms;                                          // the _f form's array of keyframes, read through `keyframe` only
    KeyframeView (*keyframe)(const void* keyfrms, int32_t k);
    const int32_t* obs_keypoint;
    const uint8_t* obs_use;
    const double* cam_centers;
    int32_t n_keyframes;
    const float* scale_factors;
    int32_t num_levels;
    double* out_mean_normal;
    float* out_min_max_dist;
    int32_t* out_best_obs;
    uint8_t *out_desc, *out_status;

    bool geo() const { return (what & 1) != 0; }
    bool dsc() const { return (what & 2) != 0; }
    bool gathers() const { return dsc() && resident; }           // the descriptors come from the resident keyframes
    bool slots() const { return geo() || gathers(); }             // whether obs_keyfrm and the keyframe table are read
    bool uploads_desc() const { return dsc() && !resident; }
};

inline Layout layout_for(const Call& c, int32_t T) {
    return c.uploads_desc() ? layout_of<true>(c.n_landmarks, T) : layout_of<false>(c.n_landmarks, T);
}

// An array the call's `what` / form does not read may be null.
template <class CapsOf>
Checked check(const Call& c, CapsOf caps_of) {
    if (!c.handle || c.n_landmarks < 0 || c.what < 1 || c.what > 3) return refused(OVS_ERR_INVALID);
    if (c.n_landmarks == 0) return Checked{OVS_OK, 0, false};
    const bool geo = c.geo(), dsc = c.dsc(), gathers = c.gathers(), slots = c.slots();
    const int32_t P = c.n_landmarks, K = c.n_keyframes;
    if (geo && (c.num_levels < 1 || c.num_levels > OVS_MAX_LEVELS)) return refused(OVS_ERR_INVALID);
    if (slots && K < 0) return refused(OVS_ERR_INVALID);
    const bool required = c.out_status &&
                          (!geo || all_set({c.pos_w, c.ref_keyfrm, c.ref_level, c.cam_centers, c.scale_factors, c.out_mean_normal, c.out_min_max_dist})) &&
                          (!dsc || all_set({c.out_best_obs, c.out_desc})) && (!gathers || c.keyfrms);
    const bool per_observation = (!slots || c.obs_keyfrm) && (!c.uploads_desc() || c.obs_desc) && (!gathers || c.obs_keypoint);
    Caps caps{};
    const Checked k = check_common(true, P, c.offsets, required, per_observation, caps_of, &caps);
    if (!k.run) return k;
    if (slots && K > caps.max_keyframes) return refused(OVS_ERR_CAPACITY);
    for (int32_t p = 0; p < P; ++p) {
        const int32_t count = c.offsets[p + 1] - c.offsets[p];
        if (count >= kMaxObsPerLandmark) return refused(OVS_ERR_INVALID);
        if (geo && count > 0 && (c.ref_keyfrm[p] < 0 || c.ref_keyfrm[p] >= K || c.ref_level[p] < 0 || c.ref_level[p] >= c.num_levels))
            return refused(OVS_ERR_INVALID);
    }
    if (slots)
        for (int32_t t = 0; t < k.T; ++t)
            if (c.obs_keyfrm[t] < 0 || c.obs_keyfrm[t] >= K) return refused(OVS_ERR_INVALID);
    if (gathers) {
        for (int32_t i = 0; i < K; ++i)
            if (c.keyframe(c.keyfrms, i).device != caps.device) return refused(OVS_ERR_INVALID);   // a null entry too
        for (int32_t t = 0; t < k.T; ++t)
            if (c.obs_keypoint[t] < 0 || c.obs_keypoint[t] >= c.keyframe(c.keyfrms, c.obs_keyfrm[t]).n) return refused(OVS_ERR_INVALID);
    }
    return k;
}

// how many landmarks each descriptor kernel serves
struct Lists {
    int32_t n8, n64;
};

inline Lists stage(const Call& c, const Layout& lay, uint8_t* h_block, uint8_t* h_table) {
    const int32_t P = c.n_landmarks, K = c.n_keyframes, T = c.offsets[P];
    Lists lists{0, 0};
    if (c.gathers()) {
        const uint8_t** ptrs = reinterpret_cast<const uint8_t**>(h_table + table_ptrs_at(K));
        for (int32_t k = 0; k < K; ++k) ptrs[k] = c.keyframe(c.keyfrms, k).d_desc;
        if (T > 0) std::memcpy(h_block + lay.obs_kp, c.obs_keypoint, 4 * (size_t)T);
    }
    if (c.slots() && T > 0) std::memcpy(h_block + lay.obs_slot, c.obs_keyfrm, 4 * (size_t)T);
    if (c.geo()) {
        double* pos = reinterpret_cast<double*>(h_block + lay.pos);
        float* sf_ref = reinterpret_cast<float*>(h_block + lay.sf_ref);
        int32_t* ref_slot = reinterpret_cast<int32_t*>(h_block + lay.ref_slot);
        for (int32_t p = 0; p < P; ++p) {
            for (int x = 0; x < 3; ++x) pos[(size_t)x * P + p] = c.pos_w[3 * (size_t)p + x];
            const bool empty = c.offsets[p + 1] == c.offsets[p];
            sf_ref[p] = empty ? 0.0f : c.scale_factors[c.ref_level[p]];
            ref_slot[p] = empty ? 0 : c.ref_keyfrm[p];
        }
        if (K > 0) std::memcpy(h_table, c.cam_centers, 24 * (size_t)K);
    }
    if (c.dsc()) {
        // which observations take part (rule L6), and each landmark into the list of the kernel that serves its size
        int32_t* used_obs = reinterpret_cast<int32_t*>(h_block + lay.used);
        int32_t* n_used = reinterpret_cast<int32_t*>(h_block + lay.n_used);
        int32_t* list8 = reinterpret_cast<int32_t*>(h_block + lay.list8);
        int32_t* list64 = reinterpret_cast<int32_t*>(h_block + lay.list64);
        for (int32_t p = 0; p < P; ++p) {
            int32_t M = 0;
            for (int32_t t = c.offsets[p]; t < c.offsets[p + 1]; ++t)
                if (!c.obs_use || c.obs_use[t]) used_obs[c.offsets[p] + M++] = t;
            n_used[p] = M;
            if (M > 8) list64[lists.n64++] = p;
            else if (M > 0) list8[lists.n8++] = p;
        }
        if (c.uploads_desc() && T > 0) std::memcpy(h_block + lay.desc, c.obs_desc, 32 * (size_t)T);
    }
    stage_offsets(h_block, lay.offsets, c.offsets, P);
    return lists;
}

// the sections the kernels wrote, copied back into h_block, to the caller's arrays; n_used is the host's own
inline void collect(const Call& c, const Layout& lay, const uint8_t* h_block) {
    const int32_t P = c.n_landmarks;
    const double* normal = reinterpret_cast<const double*>(h_block + lay.normal);
    const float* range = reinterpret_cast<const float*>(h_block + lay.range);
    const int32_t* best = reinterpret_cast<const int32_t*>(h_block + lay.best);
    const int32_t* n_used = reinterpret_cast<const int32_t*>(h_block + lay.n_used);
    for (int32_t p = 0; p < P; ++p) {
        const bool empty = c.offsets[p + 1] == c.offsets[p];
        c.out_status[p] = empty ? 1 : 0;
        if (c.geo() && !empty) {
            for (int x = 0; x < 3; ++x) c.out_mean_normal[3 * (size_t)p + x] = normal[(size_t)x * P + p];
            c.out_min_max_dist[2 * (size_t)p] = range[p];
            c.out_min_max_dist[2 * (size_t)p + 1] = range[(size_t)P + p];
        }
        if (c.dsc() && !empty) {
            if (n_used[p] == 0) {
                c.out_best_obs[p] = -1;
            } else {
                c.out_best_obs[p] = best[p] - c.offsets[p];
                std::memcpy(c.out_desc + 32 * (size_t)p, h_block + lay.out_desc + 32 * (size_t)p, 32);
            }
        }
    }
}

}   // namespace landmarks

}   // namespace splan
