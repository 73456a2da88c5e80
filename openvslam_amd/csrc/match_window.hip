// match_window.hip -- D1 + M3 + M5 + M7: the grid candidate generator and the windowed matchers built on it
// (expected: src/openvslam/data/common.{h,cc}; src/openvslam/match/{projection,area,bow_tree}.{h,cc}, angle_checker.h).
//
// These are small, latency-bound problems (a 3840x1920 frame with 4000 keypoints and 10 000 landmarks is ~3 Hamming distances
// per landmark); what the device buys is that extract -> grid -> match never leaves HBM. Three stages, all exact:
//   1. k_grid_assign   assign_keypoints_to_grid as a CSR (cell id = cx*rows + cy, members ascending = upstream's push_back order):
//                      one workgroup, LDS histogram + scan + fill + per-cell sort.
//   2. k_window_*/k_bow_*  get_keypoints_in_cell + compute_descriptor_distance_32 for every query (one lane per query, count pass,
//                      scan, fill pass): a CSR of keys  d << 20 | octave << 16 | target  in UPSTREAM'S ENUMERATION ORDER
//                      (cells x-major, then y, then members), because strict `<` keeps the first minimum.
//   3. k_list_resolve  upstream's loops are sequential -- a query sees the targets earlier queries claimed (M3, M7) or the
//                      distance they were matched at (M5). A workgroup replays them 64 * NW queries per round: every pending thread
//                      evaluates against the current state and stamps every live candidate of its list; a thread is affected if a
//                      LOWER thread stamped the best / second candidate its decision rests on; every unaffected thread commits (the
//                      rule is spelled out at the kernel). State per target is ONE number, thr[t]: a candidate at distance d is
//                      alive iff d < thr[t] (256 = free, 0 = claimed, M5: the distance it is currently matched at), and thr only
//                      ever decreases, so a decision that rests on (best, second) can only be changed by a lower thread taking
//                      one of those two.
//      The rotation-histogram check (match::angle_checker, 30 bins, keep the 3 fullest) runs in the same kernel.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "frame_dev_internal.inc"      // ovs_frame_dev, launch_grid_assign
#include "match_window_plan.inc"       // every size, threshold and offset the host side decides; the kernels' argument structs
#include "ovs_common.h"
#include "owned_internal.inc"

namespace ovs {

constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t hamming256_g(const uint32_t (&a)[8], const uint32_t* __restrict__ b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d = __builtin_popcount(a[i] ^ b[i]) + d;
    return d;
}

// ---- 1. D1 assign_keypoints_to_grid ---------------------------------------------------------------------------------
// Round 6: the scan of the cell histogram by wave shuffles (two barriers; the 1024-wide Hillis-Steele loop had twenty) and, when the keypoints fit
// (items_in_lds: n <= kGridItemsLds), the member lists built and sorted in LDS and written once, coalesced -- the per-cell insertion sort used to walk
// `items` in global memory, a chain of dependent round trips per cell: 17 -> ~8 us per 2000-keypoint frame, once per tracked frame.
__global__ __launch_bounds__(1024) void k_grid_assign(const ovs_keypoint* __restrict__ kps, int n, GridP gp, int32_t* __restrict__ cell_of,
                                                     int32_t* __restrict__ cell_start, int32_t* __restrict__ items, int items_in_lds) {
    extern __shared__ int32_t s_grid[];
    const int nc = gp.cols * gp.rows;
    int32_t* cnt = s_grid;            // [nc] histogram, then fill cursor
    int32_t* start = s_grid + nc;     // [nc + 1]
    int32_t* const lit = items_in_lds ? s_grid + 2 * nc + 1 : items;   // [n] the member lists while they are built and sorted
    __shared__ int32_t s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int c = tid; c < nc; c += 1024) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        // get_cell_indices: cvRound((pt - min) * inv_cell)
        const int cx = __float2int_rn(__fmul_rn(__fsub_rn(kps[i].x, gp.min_x), gp.inv_w));
        const int cy = __float2int_rn(__fmul_rn(__fsub_rn(kps[i].y, gp.min_y), gp.inv_h));
        int c = -1;
        if (0 <= cx && cx < gp.cols && 0 <= cy && cy < gp.rows) {
            c = cx * gp.rows + cy;
            atomicAdd(&cnt[c], 1);
        }
        cell_of[i] = c;
    }
    __syncthreads();
    // exclusive scan: thread t owns cells [t*per, t*per + per)
    const int per = (nc + 1023) / 1024;
    int local = 0;
    for (int k = 0; k < per; ++k) {
        const int c = tid * per + k;
        if (c < nc) local += cnt[c];
    }
    int incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int run = incl - local, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int t = s_w[w];
        run += w < wv ? t : 0;
        total += t;
    }
    for (int k = 0; k < per; ++k) {
        const int c = tid * per + k;
        if (c < nc) {
            start[c] = run;
            run += cnt[c];
        }
    }
    if (tid == 0) start[nc] = total;
    __syncthreads();
    for (int c = tid; c <= nc; c += 1024) {
        cell_start[c] = start[c];
        if (c < nc) cnt[c] = start[c];
    }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int c = cell_of[i];   // (this thread's own store above)
        if (c >= 0) lit[atomicAdd(&cnt[c], 1)] = i;
    }
    __syncthreads();   // also makes this workgroup's global writes visible to itself
    // members in ascending keypoint index (upstream pushes them in keypoint order)
    for (int c = tid; c < nc; c += 1024) {
        const int b = start[c], e = start[c + 1];
        for (int i = b + 1; i < e; ++i) {
            const int v = lit[i];
            int j = i - 1;
            while (j >= b && lit[j] > v) {
                lit[j + 1] = lit[j];
                --j;
            }
            lit[j + 1] = v;
        }
    }
    if (items_in_lds) {
        __syncthreads();
        for (int i = tid; i < total; i += 1024) items[i] = lit[i];
    }
}

// ---- 2. candidate lists ---------------------------------------------------------------------------------------------------
enum { kModeProjection = 0, kModeArea = 1, kModeGeneric = 2 };

// One WAVE per query: the lanes take the cells of the query's window (a 100-px margin covers ~340 of the 64 x 48 cells -- a single
// lane walking them was ~0.7 ms of dependent loads per pass), count their members that pass the filters, and an exclusive scan over
// the lanes places every cell's members at their position in UPSTREAM'S ORDER (cells x-major, then y, then members).
template <bool FILL>
__global__ __launch_bounds__(256) void k_window_lists(WinArgs a, uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                     uint32_t* __restrict__ keys, uint32_t key_cap, uint32_t* __restrict__ overflow) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.n_q) return;   // wave-uniform
    bool valid = !a.q_valid || a.q_valid[q];
    float r;
    int minl, maxl;
    if (a.mode == kModeProjection) {
        const int lvl = valid ? a.q_level[q] : 0;
        r = __fmul_rn(a.margin, a.sf[lvl]);
        minl = lvl - 1;
        maxl = lvl;
    } else if (a.mode == kModeGeneric) {
        r = a.q_radius[q];
        minl = a.q_minl[q];
        maxl = a.q_maxl[q];
    } else {
        const int lvl = a.q_kps[q].octave;
        if (0 < lvl) valid = false;   // "only level-0 keypoints"
        r = a.margin;
        minl = maxl = lvl;
    }
    uint32_t total = 0;
    if (valid) {
        const uint32_t base = FILL ? offsets[q] : 0u;
        const float ref_x = a.q_xy[2 * q], ref_y = a.q_xy[2 * q + 1];
        const float q_xr = (a.mode != kModeArea && a.t_x_right) ? a.q_x_right[q] : 0.0f;
        uint32_t qd[8];
        if (FILL || a.dead_from) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(a.q_desc + (size_t)q * 32);
#pragma unroll
            for (int i = 0; i < 8; ++i) qd[i] = src[i];
        }
        const GridP& g = a.gp;
        // get_keypoints_in_cell
        const int min_cx = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(ref_x, g.min_x), r), g.inv_w)));
        const int max_cx = min(g.cols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(ref_x, g.min_x), r), g.inv_w)));
        const int min_cy = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(ref_y, g.min_y), r), g.inv_h)));
        const int max_cy = min(g.rows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(ref_y, g.min_y), r), g.inv_h)));
        if (min_cx < g.cols && max_cx >= 0 && min_cy < g.rows && max_cy >= 0) {
            const bool check_level = (0 < minl) || (0 <= maxl);
            const int ncy = max_cy - min_cy + 1, ncell = (max_cx - min_cx + 1) * ncy;
            auto passes = [&](int idx, const ovs_keypoint& kp) -> bool {
                if (check_level && (kp.octave < minl || (0 <= maxl && maxl < kp.octave))) return false;
                if (!(fabsf(__fsub_rn(kp.x, ref_x)) < r && fabsf(__fsub_rn(kp.y, ref_y)) < r)) return false;
                if (a.mode != kModeArea) {
                    if (a.t_occupied && a.t_occupied[idx]) return false;
                    if (a.t_x_right) {
                        const float xr = a.t_x_right[idx];
                        if (0 < xr && r < fabsf(__fsub_rn(q_xr, xr))) return false;
                    }
                }
                return true;
            };
            for (int c0 = 0; c0 < ncell; c0 += 64) {
                const int ci = c0 + lane;
                int b = 0, e = 0;
                if (ci < ncell) {
                    const int cxo = ci / ncy;
                    const int c = (min_cx + cxo) * g.rows + min_cy + (ci - cxo * ncy);
                    b = a.cell_start[c];
                    e = a.cell_start[c + 1];
                }
                uint32_t n_pass = 0;
                for (int k = b; k < e; ++k) {
                    const int idx = a.items[k];
                    bool ok = passes(idx, a.t_kps[idx]);
                    if (ok && a.dead_from) ok = hamming256_g(qd, reinterpret_cast<const uint32_t*>(a.t_desc + (size_t)idx * 32)) < a.dead_from;
                    n_pass += ok ? 1u : 0u;
                }
                uint32_t incl = n_pass;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t t = __shfl_up(incl, off);
                    if (lane >= off) incl += t;
                }
                if (FILL && n_pass) {
                    uint32_t pos = base + total + (incl - n_pass);
                    for (int k = b; k < e; ++k) {
                        const int idx = a.items[k];
                        const ovs_keypoint kp = a.t_kps[idx];
                        if (!passes(idx, kp)) continue;
                        const uint32_t d = hamming256_g(qd, reinterpret_cast<const uint32_t*>(a.t_desc + (size_t)idx * 32));
                        if (a.dead_from && !(d < a.dead_from)) continue;
                        if (pos < key_cap) keys[pos] = (d << 20) | ((uint32_t)(kp.octave & 15) << 16) | (uint32_t)idx;
                        else *overflow = 1u;
                        ++pos;
                    }
                }
                total += __shfl(incl, 63);
            }
        }
    }
    if (!FILL && lane == 0) counts[q] = total;
}

// camera::perspective / camera::equirectangular ::reproject_to_image (CamP: match_window_plan.inc)
__device__ __forceinline__ bool reproject_to_image(const CamP& c, const double* __restrict__ X, double& u, double& v, float& x_right) {
    const double pcx = (c.P[0] * X[0] + c.P[1] * X[1]) + c.P[2] * X[2] + c.P[9];
    const double pcy = (c.P[3] * X[0] + c.P[4] * X[1]) + c.P[5] * X[2] + c.P[10];
    const double pcz = (c.P[6] * X[0] + c.P[7] * X[1]) + c.P[8] * X[2] + c.P[11];
    if (c.model == 0) {
        if (pcz <= 0.0) return false;
        const double z_inv = 1.0 / pcz;
        u = c.fx * pcx * z_inv + c.cx;
        v = c.fy * pcy * z_inv + c.cy;
        x_right = (float)(u - c.fxb * z_inv);
        if (u < c.min_x || u > c.max_x) return false;
        if (v < c.min_y || v > c.max_y) return false;
        return true;
    }
    const double norm = sqrt((pcx * pcx + pcy * pcy) + pcz * pcz);
    const double bx = pcx / norm, by = pcy / norm, bz = pcz / norm;
    const double latitude = -ovs_det_asin(by);
    const double longitude = ovs_det_atan2(bx, bz);
    u = c.cols * (0.5 + longitude / (2.0 * 3.14159265358979323846));
    v = c.rows * (0.5 - latitude / 3.14159265358979323846);
    x_right = -1.0f;
    return true;
}

// match_current_and_last_frames: one lane per last-frame keypoint -> query (reprojection, radius, level window, validity)
__global__ __launch_bounds__(256) void k_reproject_queries(CamP cam, const ovs_keypoint* __restrict__ last_kps,
                                                          const double* __restrict__ pos_w, const uint8_t* __restrict__ last_valid, int n,
                                                          float margin, const float* __restrict__ sf_dev, int num_levels, int forward,
                                                          int backward, const float* __restrict__ dist_min_max, double ccx, double ccy,
                                                          double ccz, float log_scale_factor, float* __restrict__ q_xy,
                                                          float* __restrict__ q_x_right, float* __restrict__ q_radius,
                                                          int32_t* __restrict__ q_minl, int32_t* __restrict__ q_maxl,
                                                          uint8_t* __restrict__ q_valid, const double* __restrict__ normals = nullptr,
                                                          int level_up = 1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool valid = !last_valid || last_valid[i];
    double u = 0, v = 0;
    float xr = -1.0f;
    const double* X = pos_w + 3 * (size_t)i;
    if (valid) valid = reproject_to_image(cam, X, u, v, xr);
    int lvl, minl, maxl;
    if (dist_min_max) {
        // match_frame_and_keyframe: valid distance range, level from the distance (landmark::predict_scale_level), window [pred-1, pred+1]
        const double dx = X[0] - ccx, dy = X[1] - ccy, dz = X[2] - ccz;
        const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
        // landmark::get_min_valid_distance() = 0.7 * min_valid_dist_, get_max_valid_distance() = 1.3 * max_valid_dist_ (double product
        // returned as float) gate the range; predict_scale_level uses the RAW max_valid_dist_
        const float dmin = dist_min_max[2 * i], dmax = dist_min_max[2 * i + 1];
        if (dist < (double)(float)(0.7 * (double)dmin) || (double)(float)(1.3 * (double)dmax) < dist) valid = false;
        if (normals) {   // match_by_Sim3_transform: viewing-angle gate against the landmark's mean normal
            const double* nrm = normals + 3 * (size_t)i;
            if ((dx * nrm[0] + dy * nrm[1]) + dz * nrm[2] < 0.5 * dist) valid = false;
        }
        lvl = valid ? (int)ceilf(__fdiv_rn(ovs_det_logf(__fdiv_rn(dmax, (float)dist)), log_scale_factor)) : 0;
        if (lvl < 0) lvl = 0;
        else if (num_levels <= lvl) lvl = num_levels - 1;
        minl = lvl - 1;
        maxl = lvl + level_up;
    } else {
        lvl = last_kps[i].octave;
        minl = forward ? lvl : (backward ? 0 : lvl - 1);
        maxl = forward ? num_levels - 1 : (backward ? lvl : lvl + 1);
    }
    q_xy[2 * i] = (float)u;
    q_xy[2 * i + 1] = (float)v;
    q_x_right[i] = xr;
    q_radius[i] = __fmul_rn(margin, sf_dev[lvl]);
    q_minl[i] = minl;
    q_maxl[i] = maxl;
    q_valid[i] = valid ? 1 : 0;
}

// tracking_module::search_local_landmarks, the visibility pass: frame::can_observe(lm, 0.5, ...) of every local landmark, one lane per landmark
// (ObserveArgs: match_window_plan.inc; rules V1 - V6 of DESIGN.md 3.17). The kModeProjection lists and the ratio resolver follow on the same stream
// and read what this writes: q_xy / q_x_right / q_level, and observable as their q_valid.
__global__ __launch_bounds__(256) void k_observe_landmarks(ObserveArgs a) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    bool obs = false;
    double u = 0.0, v = 0.0;
    float xr = -1.0f;
    int lvl = 0;
    if (l < a.m && (!a.lm_search || a.lm_search[l])) {   // V1
        const double* X = a.lm_pos_w + 3 * (size_t)l;
        obs = reproject_to_image(a.cam, X, u, v, xr);   // V2
        if (obs) {
            const double dx = X[0] - a.cc[0], dy = X[1] - a.cc[1], dz = X[2] - a.cc[2];
            const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
            // V3: landmark::is_inside_in_orb_scale through the getters (0.7 / 1.3 of the raw members, double product returned as float)
            const float dmin = a.lm_dist[2 * l], dmax = a.lm_dist[2 * l + 1];
            if (dist < (double)(float)(0.7 * (double)dmin) || (double)(float)(1.3 * (double)dmax) < dist) obs = false;
            // V4: upstream's dot / dist < 0.5 in the product form (0.5 * dist is exact, and a quotient below one half cannot round up to it)
            const double* nrm = a.lm_normal + 3 * (size_t)l;
            if ((dx * nrm[0] + dy * nrm[1]) + dz * nrm[2] < 0.5 * dist) obs = false;
            if (obs) {   // V5: landmark::predict_scale_level on the raw max_valid_dist_
                lvl = (int)ceilf(__fdiv_rn(ovs_det_logf(__fdiv_rn(dmax, (float)dist)), a.log_scale_factor));
                if (lvl < 0) lvl = 0;
                else if (a.num_levels <= lvl) lvl = a.num_levels - 1;
            }
        }
    }
    if (!obs) {   // V6 (a landmark the image bounds rejected has been projected)
        u = v = 0.0;
        xr = -1.0f;
        lvl = 0;
    }
    if (l < a.m) {
        a.q_xy[2 * l] = (float)u;
        a.q_xy[2 * l + 1] = (float)v;
        a.q_x_right[l] = xr;
        a.q_level[l] = lvl;
        a.observable[l] = obs ? 1 : 0;
        if (a.reproj) {
            a.reproj[2 * l] = u;
            a.reproj[2 * l + 1] = v;
        }
        if (a.assigned) a.assigned[l] = -1;
    }
    const unsigned long long any = __ballot(obs);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(a.num_observable, (int32_t)__popcll(any));
}

// fuse::replace_duplication, candidate search (FuseArgs: match_window_plan.inc).
// kFuseReplace: fuse::replace_duplication (chi-square gate); kFuseDetect: fuse::detect_duplication (no chi-square gate);
// kFuseMutual: one direction of projection::match_keyframes_mutually (no viewing-angle gate, distance = |pos in the other keyframe|)
enum { kFuseReplace = 0, kFuseDetect = 1, kFuseMutual = 2 };

// Round 6: kFuseLanes lanes per landmark. One lane per landmark walked its (up to nine) grid cells one after the other -- cell bounds, item,
// keypoint record, descriptor: four dependent loads per candidate, 2000 landmarks on eight workgroups, 35 us of latency. Now lane `sub` of a
// landmark takes the cells whose ordinal in upstream's enumeration (cx outer, cy inner) is sub, sub + 16, ...; the winner is the minimum of
// {distance : 16 | cell ordinal : 24 | position in the cell : 24} over the sixteen lanes, i.e. the smallest distance and among equal distances
// the first candidate upstream's loop meets (its `d < best` is strict): the same index. The per-landmark prelude is computed by all sixteen.
constexpr int kFuseLanes = 16;
__global__ __launch_bounds__(256) void k_fuse_best(FuseArgs a, int32_t* __restrict__ best_out, int32_t* __restrict__ num_fused) {
    const int gl = blockIdx.x * 256 + threadIdx.x;
    const int l = gl / kFuseLanes, sub = gl % kFuseLanes;
    unsigned long long key = ~0ull;
    int best_idx = -1;
    do {
        if (l >= a.m) break;
        if (a.lm_valid && !a.lm_valid[l]) break;
        const double* Xw = a.lm_pos_w + 3 * (size_t)l;
        // (held by value: a pointer that is either the global position or a local array put that array, 32 bytes, in scratch memory)
        double X[3] = {Xw[0], Xw[1], Xw[2]};
        if (a.variant == kFuseMutual) {
            const double x0 = (a.P1[0] * X[0] + a.P1[1] * X[1]) + a.P1[2] * X[2] + a.P1[9];
            const double x1 = (a.P1[3] * X[0] + a.P1[4] * X[1]) + a.P1[5] * X[2] + a.P1[10];
            const double x2 = (a.P1[6] * X[0] + a.P1[7] * X[1]) + a.P1[8] * X[2] + a.P1[11];
            X[0] = x0;
            X[1] = x1;
            X[2] = x2;
        }
        double u, v;
        float x_right;
        if (!reproject_to_image(a.cam, X, u, v, x_right)) break;
        double dx, dy, dz;
        if (a.variant == kFuseMutual) {   // pos_2 = s R_21 pos_1 + t_21 (the same expression reproject_to_image evaluates)
            dx = (a.cam.P[0] * X[0] + a.cam.P[1] * X[1]) + a.cam.P[2] * X[2] + a.cam.P[9];
            dy = (a.cam.P[3] * X[0] + a.cam.P[4] * X[1]) + a.cam.P[5] * X[2] + a.cam.P[10];
            dz = (a.cam.P[6] * X[0] + a.cam.P[7] * X[1]) + a.cam.P[8] * X[2] + a.cam.P[11];
        } else {
            dx = X[0] - a.cc[0];
            dy = X[1] - a.cc[1];
            dz = X[2] - a.cc[2];
        }
        const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
        const float dmin = a.lm_dist[2 * l], dmax = a.lm_dist[2 * l + 1];   // raw min_valid_dist_ / max_valid_dist_
        if (dist < (double)(float)(0.7 * (double)dmin) || (double)(float)(1.3 * (double)dmax) < dist) break;
        if (a.variant != kFuseMutual) {
            const double* nrm = a.lm_normal + 3 * (size_t)l;
            if ((dx * nrm[0] + dy * nrm[1]) + dz * nrm[2] < 0.5 * dist) break;
        }
        const float ratio = __fdiv_rn(dmax, (float)dist);
        int pred = (int)ceilf(__fdiv_rn(ovs_det_logf(ratio), a.log_scale_factor));
        if (pred < 0) pred = 0;
        else if (a.num_levels <= pred) pred = a.num_levels - 1;
        const float r = __fmul_rn(a.margin, a.sf[pred]);
        const float ref_x = (float)u, ref_y = (float)v;
        const GridP& g = a.gp;
        const int min_cx = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(ref_x, g.min_x), r), g.inv_w)));
        const int max_cx = min(g.cols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(ref_x, g.min_x), r), g.inv_w)));
        const int min_cy = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(ref_y, g.min_y), r), g.inv_h)));
        const int max_cy = min(g.rows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(ref_y, g.min_y), r), g.inv_h)));
        if (!(min_cx < g.cols && max_cx >= 0 && min_cy < g.rows && max_cy >= 0)) break;
        uint32_t qd[8];
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.lm_desc + (size_t)l * 32);
#pragma unroll
        for (int i = 0; i < 8; ++i) qd[i] = src[i];
        const int ny = max_cy - min_cy + 1, n_cells = (max_cx - min_cx + 1) * ny;
        for (int ord = sub; ord < n_cells; ord += kFuseLanes) {
            {
                const int ox = ord / ny;
                const int cx = min_cx + ox, cy = min_cy + (ord - ox * ny);
                const int c = cx * g.rows + cy;
                const int k0 = a.cell_start[c], e = a.cell_start[c + 1];
                for (int k = k0; k < e; ++k) {
                    const int idx = a.items[k];
                    const ovs_keypoint kp = a.t_kps[idx];
                    if (!(fabsf(__fsub_rn(kp.x, ref_x)) < r && fabsf(__fsub_rn(kp.y, ref_y)) < r)) continue;
                    const int level = kp.octave;
                    if (level < pred - 1 || pred < level) continue;
                    if (a.variant == kFuseReplace) {
                        const double ex = u - (double)kp.x, ey = v - (double)kp.y;
                        const float xr = a.t_x_right ? a.t_x_right[idx] : -1.0f;
                        if (xr >= 0) {
                            const double exr = (double)x_right - (double)xr;
                            const double e2 = (ex * ex + ey * ey) + exr * exr;
                            if ((double)7.81473f < e2 * (double)a.ils[level]) continue;
                        } else {
                            const double e2 = ex * ex + ey * ey;
                            if ((double)5.99146f < e2 * (double)a.ils[level]) continue;
                        }
                    }
                    const uint32_t d = hamming256_g(qd, reinterpret_cast<const uint32_t*>(a.t_desc + (size_t)idx * 32));
                    const unsigned long long cand = ((unsigned long long)d << 48) | ((unsigned long long)(ord & 0xffffff) << 24) | (unsigned long long)((uint32_t)(k - k0) & 0xffffffu);
                    if (cand < key) {   // (within a lane the keys grow with the enumeration: this is upstream's strict `d < best`)
                        key = cand;
                        best_idx = idx;
                    }
                }
            }
        }
    } while (false);
#pragma unroll
    for (int off = kFuseLanes / 2; off > 0; off >>= 1) {   // (xor partners stay inside the landmark's aligned group of sixteen lanes)
        const unsigned long long ok = __shfl_xor(key, off);
        const int oi = __shfl_xor(best_idx, off);
        if (ok < key) {
            key = ok;
            best_idx = oi;
        }
    }
    const int32_t result = (key != ~0ull && (uint32_t)(key >> 48) <= a.max_dist) ? best_idx : -1;
    if (sub == 0 && l < a.m) best_out[l] = result;
    const unsigned long long any = __ballot(sub == 0 && l < a.m && result >= 0);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(num_fused, (int32_t)__popcll(any));
}

// projection::match_keyframes_mutually, last step: keep idx_1 -> idx_2 only if idx_2 -> idx_1 came back
__global__ __launch_bounds__(256) void k_cross_check(const int32_t* __restrict__ m_2_in_1, const int32_t* __restrict__ m_1_in_2, int n1, int n2,
                                                     int32_t* __restrict__ out, int32_t* __restrict__ num) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int32_t r = -1;
    if (i < n1) {
        const int32_t j = m_2_in_1[i];
        if (j >= 0 && j < n2 && m_1_in_2[j] == i) r = j;
        out[i] = r;
    }
    const unsigned long long any = __ballot(r >= 0);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(num, (int32_t)__popcll(any));
}

// bow_tree (BowArgs: match_window_plan.inc)
template <bool FILL>
__global__ __launch_bounds__(256) void k_bow_lists(BowArgs a, uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                  uint32_t* __restrict__ keys, uint32_t key_cap, uint32_t* __restrict__ overflow) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= a.n_q) return;
    const int kf_idx = a.kf_items[q];
    uint32_t n = 0;
    if (!a.kf_valid || a.kf_valid[kf_idx]) {
        // node of this entry: last node whose start <= q
        int lo = 0, hi = a.kf_nodes - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.kf_node_start[mid] <= q) lo = mid;
            else hi = mid - 1;
        }
        const int node = a.kf_node_ids[lo];
        int l2 = 0, h2 = a.frm_nodes;   // lower_bound
        while (l2 < h2) {
            const int mid = (l2 + h2) >> 1;
            if (a.frm_node_ids[mid] < node) l2 = mid + 1;
            else h2 = mid;
        }
        if (l2 < a.frm_nodes && a.frm_node_ids[l2] == node) {
            const int b = a.frm_node_start[l2], e = a.frm_node_start[l2 + 1];
            if (a.tri) {
                uint32_t qd[8];
                const uint32_t* src = reinterpret_cast<const uint32_t*>(a.kf_desc + (size_t)kf_idx * 32);
#pragma unroll
                for (int i = 0; i < 8; ++i) qd[i] = src[i];
                const bool stereo_1 = a.kf_x_right && 0 <= a.kf_x_right[kf_idx];
                const double* b1 = a.kf_bearings + 3 * (size_t)kf_idx;
                const double thr = (0.2 * 3.14159265358979323846 / 180.0) * (double)a.sf[a.kf_kps[kf_idx].octave];
                uint32_t pos = FILL ? offsets[q] : 0u;
                for (int k = e - 1; k >= b; --k) {
                    const int idx = a.frm_items[k];
                    if (a.frm_valid && !a.frm_valid[idx]) continue;
                    const uint32_t d = hamming256_g(qd, reinterpret_cast<const uint32_t*>(a.frm_desc + (size_t)idx * 32));
                    if ((uint32_t)OVS_HAMMING_DIST_THR_LOW < d) continue;
                    const double* b2 = a.frm_bearings + 3 * (size_t)idx;
                    if (!stereo_1 && !(a.frm_x_right && 0 <= a.frm_x_right[idx])) {
                        const double cos_dist = (a.epipole[0] * b2[0] + a.epipole[1] * b2[1]) + a.epipole[2] * b2[2];
                        if (0.99862953475 < cos_dist) continue;
                    }
                    const double ex = (a.E[0] * b2[0] + a.E[1] * b2[1]) + a.E[2] * b2[2], ey = (a.E[3] * b2[0] + a.E[4] * b2[1]) + a.E[5] * b2[2],
                                 ez = (a.E[6] * b2[0] + a.E[7] * b2[1]) + a.E[8] * b2[2];
                    const double nrm = sqrt((ex * ex + ey * ey) + ez * ez);
                    const double cos_residual = ((ex * b1[0] + ey * b1[1]) + ez * b1[2]) / nrm;
                    const double residual_rad = 3.14159265358979323846 / 2.0 - fabs(ovs_det_acos(cos_residual));
                    if (!(residual_rad < thr)) continue;
                    if (FILL) {
                        if (pos < key_cap) keys[pos] = (d << 20) | (uint32_t)idx;
                        else *overflow = 1u;
                        ++pos;
                    }
                    ++n;
                }
            } else {
            uint32_t qd[8];
            if (FILL || a.dead_from) {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(a.kf_desc + (size_t)kf_idx * 32);
#pragma unroll
                for (int i = 0; i < 8; ++i) qd[i] = src[i];
            }
            if (!a.frm_valid && !a.dead_from) n = (uint32_t)(e - b);
            else
                for (int k = b; k < e; ++k) {
                    const int idx = a.frm_items[k];
                    bool ok = !a.frm_valid || a.frm_valid[idx];
                    if (ok && a.dead_from) ok = hamming256_g(qd, reinterpret_cast<const uint32_t*>(a.frm_desc + (size_t)idx * 32)) < a.dead_from;
                    n += ok ? 1u : 0u;
                }
            if (FILL) {
                uint32_t pos = offsets[q];
                for (int k = b; k < e; ++k) {
                    const int idx = a.frm_items[k];
                    if (a.frm_valid && !a.frm_valid[idx]) continue;
                    const uint32_t d = hamming256_g(qd, reinterpret_cast<const uint32_t*>(a.frm_desc + (size_t)idx * 32));
                    if (a.dead_from && !(d < a.dead_from)) continue;
                    if (pos < key_cap) keys[pos] = (d << 20) | (uint32_t)idx;
                    else *overflow = 1u;
                    ++pos;
                }
            }
            }
        }
    }
    if (!FILL) counts[q] = n;
}

// exclusive scan of counts[n] into offsets[n + 1] (one workgroup; n <= 65535)
__global__ __launch_bounds__(1024) void k_scan_counts(const uint32_t* __restrict__ counts, int n, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    uint32_t local = 0;
    for (int k = 0; k < per; ++k) {
        const int i = tid * per + k;
        if (i < n) local += counts[i];
    }
    s_part[tid] = local;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = tid >= off ? s_part[tid - off] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - local;
    for (int k = 0; k < per; ++k) {
        const int i = tid * per + k;
        if (i < n) {
            offsets[i] = run;
            run += counts[i];
        }
    }
    if (tid == 1023) offsets[n] = s_part[1023];
}

// ---- 3. sequential-claim resolver ---------------------------------------------------------------------------------------
enum { kRuleProjection = 0, kRuleArea = 1, kRuleBow = 2, kRuleBestOnly = 3, kRuleTriang = 4 };   // Triang = BestOnly accept, Bow output

template <int RULE>
__device__ __forceinline__ bool rule_accepts(uint32_t best, uint32_t second, float ratio, uint32_t best_only_thr) {
    if (best == kNone) return false;
    const uint32_t bd = best >> 20;
    const uint32_t sd = second == kNone ? (uint32_t)OVS_MAX_HAMMING_DIST : (second >> 20);
    if (RULE == kRuleBestOnly || RULE == kRuleTriang) return bd <= best_only_thr;   // match_current_and_last_frames / match_frame_and_keyframe: no ratio test
    if (RULE == kRuleProjection) {
        if (bd > (uint32_t)OVS_HAMMING_DIST_THR_HIGH) return false;
        const int bl = (int)((best >> 16) & 15u), sl = second == kNone ? -1 : (int)((second >> 16) & 15u);
        return !(bl == sl && (float)bd > __fmul_rn(ratio, (float)sd));
    }
    if (bd > (uint32_t)OVS_HAMMING_DIST_THR_LOW) return false;
    return !(__fmul_rn((float)sd, ratio) < (float)bd);   // area: second * ratio < best; bow: ratio * second < best (same product)
}

// NW waves replay 64 * NW queries per round. A pending query evaluates (best, second) against the current claims and stamps EVERY live
// candidate of its list with its thread index (LDS atomicMin, epoch-tagged). It is AFFECTED if a lower thread of the round stamped its best
// (or, where the rule has a ratio test, its second): some earlier, still undecided query has that target in its list, so it could still
// claim it -- or could still come to look at it, which is why the stamps cover all live candidates and not just the claimable ones: an
// early commit must not change what an earlier query sees when it evaluates again. An unaffected query is final whatever the others do
// (candidate sets only shrink), so EVERY unaffected query of the round commits -- round 2 committed only the ones below the first affected
// thread, and one cluster of neighbours sharing a target held the whole batch back (~6 rounds per 256 tracked-frame queries). The lowest
// pending query is never affected, so each round makes progress; the number of rounds is the longest chain of queries sharing candidates.
// tests/test_resolver_rule.py is the executable statement of this rule against the sequential loops (and of why the stamps must cover
// every live candidate). With NW > 1 the waves meet at two LDS-only workgroup barriers per round.
template <int RULE, int NW>
__global__ __launch_bounds__(64 * NW) void k_list_resolve(ResolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_res[];
    typedef __attribute__((address_space(3))) volatile uint32_t lds_u32;
    typedef __attribute__((address_space(3))) volatile uint16_t lds_u16;
    constexpr int T = 64 * NW;
    __shared__ uint32_t s_first[NW], s_any[NW], s_keep[4], s_keep_cnt[4];
    lds_u32* mark = (lds_u32*)s_res;                                        // [kMarkSize]
    lds_u32* hist = mark + kMarkSize;                                       // [32]
    lds_u16* thr = (lds_u16*)(hist + 32);                                   // [n_t]  alive(d, t) <=> d < thr[t]
    lds_u16* owner = thr + ((a.n_t + 1) & ~1);                              // [n_t]  area: query currently matched to t
    lds_u16* match = owner + ((a.n_t + 1) & ~1);                            // [n_q]  target of query (0xFFFF none)
    lds_u16* accepted = match + ((a.n_q + 1) & ~1);                         // [n_q]  target at acceptance time (orientation entries)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto wg_barrier = [&]() {
        if (NW == 1) {
            __builtin_amdgcn_wave_barrier();
        } else {   // orders LDS traffic only: the key loads of the global path need not drain
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        }
    };
    const uint32_t max_d = (RULE == kRuleBestOnly || RULE == kRuleTriang) ? a.best_only_thr : (RULE == kRuleProjection ? OVS_HAMMING_DIST_THR_HIGH : OVS_HAMMING_DIST_THR_LOW);
    for (int i = tid; i < a.n_t; i += T) {
        thr[i] = (uint16_t)OVS_MAX_HAMMING_DIST;
        owner[i] = 0xFFFFu;
    }
    for (int i = tid; i < a.n_q; i += T) {
        match[i] = 0xFFFFu;
        accepted[i] = 0xFFFFu;
    }
    for (int i = tid; i < kMarkSize; i += T) mark[i] = ~0u;
    if (tid < 32) hist[tid] = 0;
    // the candidate CSR is one contiguous array: when it fits the rest of the LDS allocation it is copied there once (coalesced
    // 16-byte loads), and the rounds below never touch HBM
    // the queries' list bounds, staged once (coalesced): every batch of the loop below used to start with two dependent global loads
    lds_u32* s_off = (lds_u32*)(accepted + ((a.n_q + 1) & ~1));             // [n_q + 1] (if offsets_in_lds)
    lds_u32* s_keys = s_off + (a.offsets_in_lds ? ((a.n_q + 4) & ~3) : 0);
    if (a.offsets_in_lds)
        for (int i = tid; i <= a.n_q; i += T) s_off[i] = a.offsets[i];
    const uint32_t n_keys = a.offsets[a.n_q];
    const bool keys_in_lds = n_keys <= a.key_pool;
    if (keys_in_lds) {
        const uint32_t n4 = n_keys >> 2;
        const uint4* src4 = reinterpret_cast<const uint4*>(a.keys);
        for (uint32_t i = tid; i < n4; i += T) {
            const uint4 v = src4[i];
            s_keys[4 * i] = v.x;
            s_keys[4 * i + 1] = v.y;
            s_keys[4 * i + 2] = v.z;
            s_keys[4 * i + 3] = v.w;
        }
        for (uint32_t i = 4 * n4 + tid; i < n_keys; i += T) s_keys[i] = a.keys[i];
    }
    wg_barrier();
    uint32_t epoch = 0;

    for (int q0 = 0; q0 < a.n_q; q0 += T) {
        const int q = q0 + tid;
        uint32_t lb = 0, le = 0;
        if (q < a.n_q) {
            lb = a.offsets_in_lds ? (uint32_t)s_off[q] : a.offsets[q];
            le = a.offsets_in_lds ? (uint32_t)s_off[q + 1] : a.offsets[q + 1];
        }
        bool pending = le > lb;
        for (;;) {
            // ---- any query of the batch still undecided? (the barrier also publishes the previous round's commits)
            {
                const unsigned long long pb = __ballot(pending);
                if (NW == 1) {
                    if (!pb) break;
                } else {
                    if (lane == 0) s_any[wv] = pb != 0ull;
                    wg_barrier();
                    uint32_t any = 0;
#pragma unroll
                    for (int w = 0; w < NW; ++w) any |= s_any[w];
                    if (!any) break;
                }
            }
            uint32_t best = kNone, second = kNone;
            bool acc = false;
            ++epoch;
            const uint32_t tag = (0x3FFFFFu - epoch) << 10;   // newer rounds carry smaller tags: atomicMin overrides stale stamps; low 10 bits: thread
            asm volatile("" ::: "memory");   // thr[] committed in the previous round must be re-read
            if (pending) {
                uint32_t bd = OVS_MAX_HAMMING_DIST, sd = OVS_MAX_HAMMING_DIST;
                // eight keys and their eight thr[] values are fetched as independent batches (one load round trip per batch instead of
                // one per entry: that latency is the whole cost); keys come from LDS when the CSR was staged
                const __attribute__((address_space(3))) uint16_t* thr_nv = (const __attribute__((address_space(3))) uint16_t*)thr;
                // (the staged keys never change: read them through a plain pointer too, or each of the eight reads waits for the one before)
                const __attribute__((address_space(3))) uint32_t* keys_nv = (const __attribute__((address_space(3))) uint32_t*)s_keys;
                // UNCONDITIONAL loads (indices clamped into the list, results masked afterwards): a load under a per-lane condition gets its own
                // branch and its own wait, i.e. eight serialised round trips for the keys and eight for thr[] (seen in the ISA)
                const uint32_t last = le - 1u;   // (pending => le > lb)
                for (uint32_t k0 = lb; k0 < le; k0 += 8) {
                    uint32_t e8[8], t8[8];
                    if (keys_in_lds) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) e8[u] = keys_nv[min(k0 + u, last)];
                    } else {
#pragma unroll
                        for (int u = 0; u < 8; ++u) e8[u] = a.keys[min(k0 + u, last)];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) e8[u] = k0 + u < le ? e8[u] : kNone;
#pragma unroll
                    for (int u = 0; u < 8; ++u) t8[u] = (uint32_t)thr_nv[e8[u] != kNone ? (e8[u] & 0xFFFFu) : 0u];
#pragma unroll
                    for (int u = 0; u < 8; ++u) t8[u] = e8[u] != kNone ? t8[u] : 0u;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const uint32_t e = e8[u], d = e >> 20;
                        if (e == kNone || !(d < t8[u])) continue;   // claimed / matched at a distance <= ours
                        // every live candidate, whatever its distance: a later query must neither rest on a target this one may still
                        // claim nor claim a target this one may still come to look at
                        __hip_atomic_fetch_min((__attribute__((address_space(3))) uint32_t*)&mark[(e & 0xFFFFu) & (kMarkSize - 1)],
                                               tag | (uint32_t)tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (d < bd) {
                            second = best;
                            sd = bd;
                            best = e;
                            bd = d;
                        } else if (d < sd) {
                            second = e;
                            sd = d;
                        }
                    }
                }
                acc = rule_accepts<RULE>(best, second, a.lowe_ratio, a.best_only_thr);
            }
            wg_barrier();
            bool affected = false;
            if (pending && best != kNone && (best >> 20) <= max_d) {   // a best beyond the threshold is a final reject (it can only grow)
                const uint32_t m1 = mark[(best & 0xFFFFu) & (kMarkSize - 1)];
                affected = (m1 & ~0x3FFu) == tag && (m1 & 0x3FFu) < (uint32_t)tid;
                if (RULE != kRuleBestOnly && RULE != kRuleTriang && second != kNone) {   // (no ratio test: the decision rests on `best` alone)
                    const uint32_t m2 = mark[(second & 0xFFFFu) & (kMarkSize - 1)];
                    affected |= (m2 & ~0x3FFu) == tag && (m2 & 0x3FFu) < (uint32_t)tid;
                }
            }
            if (pending && !affected && acc) {
                const uint32_t t = best & 0xFFFFu;
                if (RULE == kRuleArea) {
                    const uint32_t prev = owner[t];
                    if (prev != 0xFFFFu) match[prev] = 0xFFFFu;   // the earlier owner loses the target
                    owner[t] = (uint16_t)q;
                    thr[t] = (uint16_t)(best >> 20);
                } else {
                    thr[t] = 0;
                }
                match[q] = (uint16_t)t;
                accepted[q] = (uint16_t)t;
            }
            if (!affected) pending = false;
            if (NW == 1) __builtin_amdgcn_wave_barrier();   // NW > 1: the barrier at the top of the loop publishes the commits
        }
    }
    wg_barrier();
    // ---- match::angle_checker: bin = cvRound(delta / 30) over every ACCEPTED query (a later-stolen match keeps its entry)
    if (RULE != kRuleProjection && a.check_orientation) {
        for (int q = tid; q < a.n_q; q += T) {
            const uint32_t t = accepted[q];
            if (t == 0xFFFFu) continue;
            const int qi = a.q_items ? a.q_items[q] : q;
            float delta = __fsub_rn(a.q_kps[qi].angle, a.t_kps[t].angle);
            if (delta < 0.0f) delta = __fadd_rn(delta, 360.0f);
            if (360.0f <= delta) delta = __fsub_rn(delta, 360.0f);
            int bin = __float2int_rn(__fmul_rn(delta, 1.0f / 30));
            if (bin == 30) bin = 0;
            __hip_atomic_fetch_add((__attribute__((address_space(3))) uint32_t*)&hist[bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            accepted[q] = (uint16_t)(0x8000u | (uint32_t)bin);   // reuse the slot: bin of this entry
        }
        wg_barrier();
        // the three fullest bins, equal sizes -> lower bin first (ORACLE_SPEC rule 17); wave 0 picks them
        if (wv == 0) {
            const uint32_t h = lane < 30 ? (uint32_t)hist[lane] : 0u;
            // larger count first; equal counts: the lower bin (rule 17 as fixed) or, in the variant, the higher bin -- upstream std::sort's on the
            // sizes, which leaves the order of equal bins to the library
            const uint32_t tie_key = a.angle_tie_order ? (uint32_t)(lane + 1) : (uint32_t)(31 - lane);
            uint32_t key = lane < 30 ? ((h << 8) | tie_key) : 0u;
            for (int k = 0; k < 3; ++k) {
                uint32_t m = key;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t o = __shfl_xor(m, off);
                    m = o > m ? o : m;
                }
                if (lane == 0) {
                    s_keep[k] = a.angle_tie_order ? (m & 0xFFu) - 1u : (uint32_t)(31 - (int)(m & 0xFFu));
                    s_keep_cnt[k] = m >> 8;
                }
                if (key == m) key = 0u;
            }
            // rule 17's alternative (ORB-SLAM2's ComputeThreeMaxima): a second bin below 0.1 x the fullest drops out and takes the third with it,
            // a third bin below that alone (bin 99 matches nothing)
            if (a.angle_keep_rule && lane == 0) {
                const float max1 = (float)s_keep_cnt[0];
                if ((float)s_keep_cnt[1] < __fmul_rn(0.1f, max1)) s_keep[1] = s_keep[2] = 99u;
                else if ((float)s_keep_cnt[2] < __fmul_rn(0.1f, max1)) s_keep[2] = 99u;
            }
        }
        wg_barrier();
        const int keep0 = (int)s_keep[0], keep1 = (int)s_keep[1], keep2 = (int)s_keep[2];
        for (int q = tid; q < a.n_q; q += T) {
            const uint32_t v = accepted[q];
            if (!(v & 0x8000u) || v == 0xFFFFu) continue;
            const int bin = (int)(v & 0xFFu);
            if (bin != keep0 && bin != keep1 && bin != keep2) match[q] = 0xFFFFu;
        }
        wg_barrier();
    }
    // ---- outputs
    uint32_t total = 0;
    constexpr bool kBowOut = RULE == kRuleBow || RULE == kRuleTriang;
    if (kBowOut) {
        const int n_clear = a.bow_by_query ? a.n_out_q : a.n_t;
        for (int t = tid; t < n_clear; t += T) a.assigned[t] = -1;
        __threadfence_block();
        __syncthreads();   // global writes above must land before the scattered ones below
    }
    for (int q0 = 0; q0 < a.n_q; q0 += T) {
        const int q = q0 + tid;
        uint32_t t = 0xFFFFu;
        if (q < a.n_q) t = match[q];
        if (q < a.n_q) {
            if (kBowOut) {
                if (t != 0xFFFFu) {
                    const int qi = a.q_items ? a.q_items[q] : q;
                    if (a.bow_by_query) a.assigned[qi] = (int32_t)t;
                    else a.assigned[t] = qi;
                }
            } else {
                a.assigned[q] = t == 0xFFFFu ? -1 : (int32_t)t;
                if (RULE == kRuleArea && t != 0xFFFFu) {
                    a.prev_matched_xy[2 * q] = a.t_kps[t].x;
                    a.prev_matched_xy[2 * q + 1] = a.t_kps[t].y;
                }
            }
        }
        total += (uint32_t)__popcll(__ballot(t != 0xFFFFu));
    }
    if (NW == 1) {
        if (lane == 0) *a.num_matches = (int32_t)total;
    } else {
        if (lane == 0) s_first[wv] = total;
        wg_barrier();
        if (tid == 0) {
            uint32_t sum = 0;
            for (int w = 0; w < NW; ++w) sum += s_first[w];
            *a.num_matches = (int32_t)sum;
        }
    }
}

}   // namespace ovs

using namespace ovs;

// ovs_match_set_variant(OVS_MATCH_VARIANT_ANGLE_KEEP_RULE, 0 | 1): process-wide, read at every resolver launch
static std::atomic<int> g_angle_keep_rule{0};
static std::atomic<int> g_angle_tie_order{0};   // OVS_MATCH_VARIANT_ANGLE_TIE_ORDER
static std::atomic<int> g_bf_frame_mask{0};     // OVS_MATCH_VARIANT_BF_FRAME_MASK (read by the class shim of robust::brute_force_match)

struct ovs_wmatcher {
    int device = 0;
    int max_t = 0, max_q = 0;
    uint32_t max_entries = 0;
    ovs::Owned res;
    hipStream_t stream = nullptr;
    // grid of a target frame that is uploaded per call (a resident frame carries its own)
    int32_t* d_cell_of = nullptr;
    int32_t* d_cell_start = nullptr;
    int32_t* d_items = nullptr;
    GridP gp{};
    // candidate lists
    uint32_t* d_counts = nullptr;
    uint32_t* d_offsets = nullptr;
    uint32_t* d_keys = nullptr;
    uint32_t* d_overflow = nullptr;
    bool overflow_dirty = true;        // the overflow word may be non-zero (build_lists clears it then)
    int32_t* d_assigned = nullptr;      // max(max_q, max_t)
    int32_t* d_num = nullptr;
    // d_overflow | d_num[4] | pad | d_assigned are ONE block: a call's results come down with one copy (fetch_results)
    uint32_t* d_res_block = nullptr;
    int32_t* h_res = nullptr;           // pinned mirror of the result block
    // every per-call host array goes through one pinned buffer into one device arena with one copy up (Stager)
    unsigned char* h_stage = nullptr;   // pinned
    unsigned char* d_stage = nullptr;
    size_t stage_cap = 0;
};

// k_grid_assign over `n` device keypoints (frame_dev_internal.inc: the resident frame handle indexes its keypoints with it too)
hipError_t ovs::launch_grid_assign(const ovs_keypoint* d_kps, int n, const GridP& g, int32_t* cell_of, int32_t* cell_start, int32_t* items, hipStream_t s) {
    const GridLaunch l = grid_launch_plan(n, g.cols * g.rows);
    if (l.raise_attr) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_grid_assign), hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_grid_assign, dim3(1), dim3(1024), l.lds_bytes, s, d_kps, n, g, cell_of, cell_start, items, l.items_in_lds);
    return hipGetLastError();
}

namespace {

template <int RULE>
ovs_status launch_resolve(const ResolveArgs& ra_in, hipStream_t s) {
    ResolveArgs ra = ra_in;
    ra.angle_keep_rule = g_angle_keep_rule.load(std::memory_order_relaxed);
    ra.angle_tie_order = g_angle_tie_order.load(std::memory_order_relaxed);
    const ResolveLaunch l = resolve_plan(ra.n_q, ra.n_t, tuning().resolve_wide_from);
    if (!l.ok) return OVS_ERR_CAPACITY;
    ra.offsets_in_lds = l.offsets_in_lds;
    ra.key_pool = l.key_pool;
    {
        static LdsAttrCache configured[3];   // per (RULE: this instantiation, width), per device
        const void* fn = l.width == 2 ? reinterpret_cast<const void*>(k_list_resolve<RULE, 8>)
                                      : (l.width == 1 ? reinterpret_cast<const void*>(k_list_resolve<RULE, 4>) : reinterpret_cast<const void*>(k_list_resolve<RULE, 1>));
        OVS_HIP_TRY(ensure_dynamic_lds(fn, l.lds_bytes, configured[l.width]));
    }
    if (l.width == 2)
        hipLaunchKernelGGL((k_list_resolve<RULE, 8>), dim3(1), dim3(512), l.lds_bytes, s, ra);
    else if (l.width == 1)
        hipLaunchKernelGGL((k_list_resolve<RULE, 4>), dim3(1), dim3(256), l.lds_bytes, s, ra);
    else
        hipLaunchKernelGGL((k_list_resolve<RULE, 1>), dim3(1), dim3(64), l.lds_bytes, s, ra);
    OVS_HIP_TRY(hipGetLastError());
    return OVS_OK;
}

// the context's own grid over device keypoints
ovs_status grid_assign(ovs_wmatcher* w, const ovs_grid_params* gp, const ovs_keypoint* d_kps, int n, hipStream_t s) {
    if (!grid_params_ok(gp)) return OVS_ERR_INVALID;
    if (n > w->max_t) return OVS_ERR_CAPACITY;
    w->gp = make_gridp(*gp);
    OVS_HIP_TRY(launch_grid_assign(d_kps, n, w->gp, w->d_cell_of, w->d_cell_start, w->d_items, s));
    return OVS_OK;
}

// per-call staging of host arrays: StageWriter (match_window_plan.inc) places them in the context's pinned buffer, ONE copy up for all of them
struct Stager : StageWriter {
    explicit Stager(ovs_wmatcher* w) : StageWriter(w->h_stage, w->d_stage, w->stage_cap) {}
    ovs_status flush(hipStream_t s) {   // behind the call's last put / reserve
        if (overflow) return OVS_ERR_CAPACITY;
        flushed_on = s;
        flushed = true;
        if (used) OVS_HIP_TRY(hipMemcpyAsync(d, h, used, hipMemcpyHostToDevice, s));
        return OVS_OK;
    }
    // A call returns with its stream idle, on EVERY path: the next call (or the shim's immediate retry) memcpy's into the same pinned buffer, and
    // a frame arena may go back to the pool -- neither may happen while a copy or a kernel of a failed call is still in flight. After a
    // successful call the stream is already idle (fetch_results synchronised it) and this costs a microsecond.
    hipStream_t flushed_on = nullptr;
    bool flushed = false;
    ~Stager() {
        if (flushed) (void)hipStreamSynchronize(flushed_on);
    }
};

// A side of a call that is a resident frame / keyframe: checked against the context, then its arrays as stage_target (match_window_plan.inc) takes
// them (the callers pass `res ? &r : nullptr` on). Nothing to do for a side that comes as host arrays.
ovs_status resident_side(const ovs_wmatcher* w, const ovs_frame_dev* res, int n, TargetRef* r) {
    if (!res) return OVS_OK;
    if (res->device != w->device || res->n != n) return OVS_ERR_INVALID;
    *r = TargetRef{res->d_kps, res->d_desc, res->has_stereo ? res->d_x_right : nullptr, res->d_bearings, res->d_cell_start, res->d_items, res->gp};
    return OVS_OK;
}
// behind the flush: the grid of a staged target (a resident one brings its own)
ovs_status index_target(ovs_wmatcher* w, const ovs_grid_params* gp, int n, TargetRef* t, hipStream_t s) {
    if (t->cell_start) return OVS_OK;
    const ovs_status st = grid_assign(w, gp, t->kps, n, s);
    if (st != OVS_OK) return st;
    t->cell_start = w->d_cell_start;
    t->items = w->d_items;
    t->gp = w->gp;
    return OVS_OK;
}

template <typename ARGS, typename KCOUNT, typename KFILL>
ovs_status build_lists(ovs_wmatcher* w, const ARGS& args, int n_q, KCOUNT kcount, KFILL kfill, hipStream_t s, int q_per_block = 4) {
    if (n_q > w->max_q) return OVS_ERR_CAPACITY;
    // the overflow word is zero between calls unless a call ended without having read it as zero (a failed call, an overflow): only then is it cleared
    // here (round 6: the clearing was a fill kernel and a launch gap in front of every list build).
    // (Also tried: the counting launch's last workgroup scanning the counts instead of the one-workgroup k_scan_counts launch -- the device-scope
    // release every workgroup needs before it takes its ticket is an L2 write-back on this multi-XCD part: +20 us per call, dropped.)
    if (w->overflow_dirty) OVS_HIP_TRY(hipMemsetAsync(w->d_overflow, 0, sizeof(uint32_t), s));
    w->overflow_dirty = true;
    const dim3 grid((n_q + q_per_block - 1) / q_per_block);
    hipLaunchKernelGGL(kcount, grid, dim3(256), 0, s, args, w->d_counts, (const uint32_t*)w->d_offsets, w->d_keys, w->max_entries, w->d_overflow);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, (const uint32_t*)w->d_counts, n_q, w->d_offsets);
    hipLaunchKernelGGL(kfill, grid, dim3(256), 0, s, args, w->d_counts, (const uint32_t*)w->d_offsets, w->d_keys, w->max_entries, w->d_overflow);
    OVS_HIP_TRY(hipGetLastError());
    return OVS_OK;
}

// what every resolver launch reads from the context: the lists build_lists wrote, the result block as output
ResolveArgs resolve_args(const ovs_wmatcher* w, int n_q, int n_t) {
    ResolveArgs ra{};
    ra.offsets = w->d_offsets;
    ra.keys = w->d_keys;
    ra.n_q = n_q;
    ra.n_t = n_t;
    ra.assigned = w->d_assigned;
    ra.num_matches = w->d_num;
    return ra;
}

// results: overflow flag, counts and `n_out` assignments in one copy
ovs_status fetch_results(ovs_wmatcher* w, int n_out, int32_t* assigned, int32_t* num_matches, hipStream_t s, bool check_overflow = true) {
    OVS_HIP_TRY(hipMemcpyAsync(w->h_res, w->d_res_block, sizeof(int32_t) * (8 + (size_t)n_out), hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(assigned, w->h_res + 8, sizeof(int32_t) * (size_t)n_out);
    *num_matches = w->h_res[1];
    if (check_overflow && w->h_res[0] == 0) w->overflow_dirty = false;   // read as zero behind every kernel of the call: still zero for the next one
    return (check_overflow && w->h_res[0]) ? OVS_ERR_CAPACITY : OVS_OK;   // (k_fuse_best and k_cross_check write no overflow flag: the word may be stale)
}

void fill_cam(CamP& cp, const ovs_camera* cam, const ovs_grid_params* gp, const double* P) {
    cp.model = cam->model;
    cp.setup = cam->setup;
    cp.fx = cam->fx;
    cp.fy = cam->fy;
    cp.cx = cam->cx;
    cp.cy = cam->cy;
    cp.fxb = cam->focal_x_baseline;
    cp.cols = cam->cols;
    cp.rows = cam->rows;
    cp.min_x = gp->min_x;
    cp.min_y = gp->min_y;
    cp.max_x = gp->max_x;
    cp.max_y = gp->max_y;
    std::memcpy(cp.P, P, sizeof(double) * 12);
}
// robust::match_for_triangulation: "valid" for the bow kernels = the keypoint has NO landmark yet
std::vector<uint8_t> no_landmark_mask(const uint8_t* has_lm, int n) {
    std::vector<uint8_t> v((size_t)std::max(n, 1), 1);
    if (has_lm)
        for (int i = 0; i < n; ++i) v[i] = has_lm[i] ? 0 : 1;
    return v;
}

// kModeGeneric: reprojected queries with their own radius and level window against a target's grid
WinArgs generic_window_args(const TargetRef& t, bool stereo, const uint8_t* d_occupied, const QueryScratch& q, const uint8_t* d_q_desc, int n_q, float margin,
                            uint32_t dead_from) {
    WinArgs a{};
    a.t_kps = t.kps;
    a.t_desc = t.desc;
    a.t_occupied = d_occupied;
    a.t_x_right = stereo ? t.x_right : nullptr;
    a.cell_start = t.cell_start;
    a.items = t.items;
    a.gp = t.gp;
    a.n_q = n_q;
    a.q_xy = q.xy;
    a.q_x_right = q.x_right;
    a.q_valid = q.valid;
    a.q_radius = q.radius;
    a.q_minl = q.minl;
    a.q_maxl = q.maxl;
    a.q_desc = d_q_desc;
    a.margin = margin;
    a.mode = kModeGeneric;
    a.dead_from = dead_from;
    return a;
}
// lists and the best-only resolver over reprojected queries, results down: the tail of the three kModeGeneric matchers
ovs_status generic_match(ovs_wmatcher* w, const WinArgs& a, int n_t, const ovs_keypoint* d_query_kps, int check_orientation, uint32_t thr, int32_t* assigned,
                         int32_t* num_matches, hipStream_t s) {
    ovs_status st = build_lists(w, a, a.n_q, k_window_lists<false>, k_window_lists<true>, s);
    if (st != OVS_OK) return st;
    ResolveArgs ra = resolve_args(w, a.n_q, n_t);
    ra.check_orientation = check_orientation;
    ra.q_kps = d_query_kps;
    ra.t_kps = a.t_kps;
    ra.best_only_thr = thr;
    st = launch_resolve<kRuleBestOnly>(ra, s);
    if (st != OVS_OK) return st;
    return fetch_results(w, a.n_q, assigned, num_matches, s);
}

// projection::match_frame_and_landmarks on device arrays: lists and resolver into the given device outputs
ovs_status frame_and_landmarks_on_device(ovs_wmatcher* w, const TargetRef& t, const uint8_t* d_occupied, int n, const float* d_lm_xy, const float* d_lm_x_right,
                                         const int32_t* d_lm_level, const uint8_t* d_lm_desc, const uint8_t* d_lm_valid, int m, const float* scale_factors,
                                         int num_levels, float margin, float lowe_ratio, int32_t* d_assigned, int32_t* d_num_matches, hipStream_t s) {
    WinArgs a{};
    a.t_kps = t.kps;
    a.t_desc = t.desc;
    a.t_occupied = d_occupied;
    a.t_x_right = t.x_right;
    a.cell_start = t.cell_start;
    a.items = t.items;
    a.gp = t.gp;
    a.n_q = m;
    a.q_xy = d_lm_xy;
    a.q_x_right = d_lm_x_right;
    a.q_level = d_lm_level;
    a.q_valid = d_lm_valid;
    a.q_desc = d_lm_desc;
    a.margin = margin;
    pad_levels(a.sf, scale_factors, num_levels, 1.0f);
    a.mode = kModeProjection;
    a.dead_from = dead_from_ratio(OVS_HAMMING_DIST_THR_HIGH, lowe_ratio);
    const ovs_status st = build_lists(w, a, m, k_window_lists<false>, k_window_lists<true>, s);
    if (st != OVS_OK) return st;
    ResolveArgs ra = resolve_args(w, m, n);
    ra.lowe_ratio = lowe_ratio;
    ra.assigned = d_assigned;
    ra.num_matches = d_num_matches;
    return launch_resolve<kRuleProjection>(ra, s);
}

// area::match_in_consistent_area on device arrays; d_prev_matched_xy is read AND updated by the resolver
ovs_status area_on_device(ovs_wmatcher* w, const ovs_keypoint* d_kps_1, const uint8_t* d_desc_1, int n1, const TargetRef& t2, int n2, float* d_prev_matched_xy,
                          int32_t* d_matched_2_in_1, int margin, float lowe_ratio, int check_orientation, int32_t* d_num_matches, hipStream_t s) {
    WinArgs a{};
    a.t_kps = t2.kps;
    a.t_desc = t2.desc;
    a.cell_start = t2.cell_start;
    a.items = t2.items;
    a.gp = t2.gp;
    a.n_q = n1;
    a.q_xy = d_prev_matched_xy;
    a.q_kps = d_kps_1;
    a.q_desc = d_desc_1;
    a.margin = (float)margin;
    a.mode = kModeArea;
    a.dead_from = dead_from_ratio(OVS_HAMMING_DIST_THR_LOW, lowe_ratio);
    const ovs_status st = build_lists(w, a, n1, k_window_lists<false>, k_window_lists<true>, s);
    if (st != OVS_OK) return st;
    ResolveArgs ra = resolve_args(w, n1, n2);
    ra.lowe_ratio = lowe_ratio;
    ra.check_orientation = check_orientation;
    ra.q_kps = d_kps_1;
    ra.t_kps = t2.kps;
    ra.prev_matched_xy = d_prev_matched_xy;
    ra.assigned = d_matched_2_in_1;
    ra.num_matches = d_num_matches;
    return launch_resolve<kRuleArea>(ra, s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// One implementation per matcher. Each serves the host-array entry point and its resident twin (_f): `res` is the frame / keyframe handle
// of the twin (then the host arrays of that side are nullptr and gp is the handle's), or nullptr. A frame's matcher-side data --
// undistorted keypoints, descriptors, stereo_x_right and the keypoint grid -- is uploaded and indexed ONCE per handle; what travels per call
// is what changes per call: the landmark side and the flags, through the Stager (one copy up), and the result block (one copy down).
// ---------------------------------------------------------------------------------------------------------------------------

ovs_status projection_match_frame_and_landmarks_impl(ovs_wmatcher* w, const ovs_frame_dev* res, const ovs_grid_params* gp, const ovs_keypoint* kps,
                                                     const uint8_t* desc, const float* stereo_x_right, const uint8_t* occupied, int32_t n, const float* lm_xy,
                                                     const float* lm_x_right, const int32_t* lm_level, const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m,
                                                     const float* scale_factors, int32_t num_levels, float margin, float lowe_ratio, int32_t* assigned,
                                                     int32_t* num_matches) {
    if (!w || !num_matches || n < 0 || m < 0 || !scale_factors || num_levels < 1 || num_levels > OVS_MAX_LEVELS) return OVS_ERR_INVALID;
    *num_matches = 0;
    if (m == 0) return OVS_OK;
    if (!assigned) return OVS_ERR_INVALID;
    if (n == 0) {
        for (int i = 0; i < m; ++i) assigned[i] = -1;
        return OVS_OK;
    }
    const bool stereo = res ? res->has_stereo : stereo_x_right != nullptr;
    if ((!res && (!kps || !desc)) || !lm_xy || !lm_level || !lm_desc || (stereo && !lm_x_right)) return OVS_ERR_INVALID;
    Stager stg(w);
    TargetRef r;
    ovs_status st = resident_side(w, res, n, &r);
    if (st != OVS_OK) return st;
    TargetRef tg = stage_target(stg, res ? &r : nullptr, kps, desc, stereo_x_right, nullptr, n);
    if (n > w->max_t || m > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    const LandmarkQueries q = stage_landmark_queries(stg, occupied, n, lm_xy, stereo ? lm_x_right : nullptr, lm_level, lm_valid, lm_desc, m);
    if ((st = stg.flush(s)) != OVS_OK || (st = index_target(w, gp, n, &tg, s)) != OVS_OK) return st;
    st = frame_and_landmarks_on_device(w, tg, q.occupied, n, q.xy, q.x_right, q.level, q.desc, q.valid, m, scale_factors, num_levels, margin, lowe_ratio,
                                       w->d_assigned, w->d_num, s);
    if (st != OVS_OK) return st;
    return fetch_results(w, m, assigned, num_matches, s);
}

// tracking_module::search_local_landmarks on device arrays: k_observe_landmarks, then (with keypoints to match against) the lists and the resolver
// of projection::match_frame_and_landmarks on what it wrote -- one stream, no host step in between. d_num_observable and d_num_matches are written
// on every path; without keypoints the kernel also sets every assigned to -1.
ovs_status search_local_on_device(ovs_wmatcher* w, const CamP& cp, const double* cc, const TargetRef& t, const uint8_t* d_occupied, int n, const double* d_lm_pos_w,
                                  const float* d_lm_dist, const double* d_lm_normal, const uint8_t* d_lm_desc, const uint8_t* d_lm_search, int m,
                                  const float* scale_factors, int num_levels, float log_scale_factor, float margin, float lowe_ratio, float* d_xy,
                                  float* d_x_right, int32_t* d_level, uint8_t* d_observable, double* d_reproj, int32_t* d_assigned, int32_t* d_num_observable,
                                  int32_t* d_num_matches, hipStream_t s) {
    ObserveArgs a{};
    a.cam = cp;
    std::memcpy(a.cc, cc, sizeof(a.cc));
    a.lm_pos_w = d_lm_pos_w;
    a.lm_dist = d_lm_dist;
    a.lm_normal = d_lm_normal;
    a.lm_search = d_lm_search;
    a.m = m;
    a.num_levels = num_levels;
    a.log_scale_factor = log_scale_factor;
    a.q_xy = d_xy;
    a.q_x_right = d_x_right;
    a.q_level = d_level;
    a.observable = d_observable;
    a.reproj = d_reproj;
    a.assigned = n == 0 ? d_assigned : nullptr;
    a.num_observable = d_num_observable;
    OVS_HIP_TRY(hipMemsetAsync(d_num_observable, 0, sizeof(int32_t), s));
    if (n == 0) OVS_HIP_TRY(hipMemsetAsync(d_num_matches, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_observe_landmarks, dim3((m + 255) / 256), dim3(256), 0, s, a);
    OVS_HIP_TRY(hipGetLastError());
    if (n == 0) return OVS_OK;   // upstream: `if (!found_proj_candidate) return;` -- and no keypoint can take a landmark
    return frame_and_landmarks_on_device(w, t, d_occupied, n, d_xy, d_x_right, d_level, d_lm_desc, d_observable, m, scale_factors, num_levels, margin, lowe_ratio,
                                         d_assigned, d_num_matches, s);
}

ovs_status tracking_search_local_landmarks_impl(ovs_wmatcher* w, const ovs_frame_dev* res, const ovs_camera* cam, const ovs_grid_params* gp,
                                                const ovs_keypoint* kps, const uint8_t* desc, const float* stereo_x_right, const uint8_t* occupied, int32_t n,
                                                const double* pose_cw, const double* lm_pos_w, const float* lm_dist_min_max, const double* lm_normal,
                                                const uint8_t* lm_desc, const uint8_t* lm_search, int32_t m, const float* scale_factors, int32_t num_levels,
                                                float log_scale_factor, float margin, float lowe_ratio, uint8_t* observable, double* reproj, float* x_right,
                                                int32_t* level, int32_t* assigned, int32_t* num_observable, int32_t* num_matches) {
    if (!w || !cam || !gp || !num_observable || !num_matches || n < 0 || m < 0 || !pose_cw || !scale_factors || num_levels < 1 ||
        num_levels > OVS_MAX_LEVELS || (cam->model != 0 && cam->model != 1))
        return OVS_ERR_INVALID;
    *num_observable = *num_matches = 0;
    if (m == 0) return OVS_OK;
    if (!observable || !assigned || !lm_pos_w || !lm_dist_min_max || !lm_normal || !lm_desc || (n > 0 && !res && (!kps || !desc))) return OVS_ERR_INVALID;
    if (n > w->max_t || m > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    CamP cp{};
    fill_cam(cp, cam, gp, pose_cw);
    double cc[3];
    camera_centre(pose_cw, cc);
    Stager stg(w);
    TargetRef r;
    ovs_status st = resident_side(w, res, n, &r);
    if (st != OVS_OK) return st;
    TargetRef tg = stage_target(stg, res ? &r : nullptr, kps, desc, stereo_x_right, nullptr, n);
    const LocalLandmarks q = stage_local_landmarks(stg, occupied, n, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc, lm_search, m, reproj != nullptr);
    if ((st = stg.flush(s)) != OVS_OK) return st;
    if (n > 0 && (st = index_target(w, gp, n, &tg, s)) != OVS_OK) return st;
    uint8_t* const d_observable = reinterpret_cast<uint8_t*>(w->d_assigned + m);   // behind assigned[m]: the result block comes down with one copy
    st = search_local_on_device(w, cp, cc, tg, q.occupied, n, q.pos, q.dist, q.normal, q.desc, q.search, m, scale_factors, num_levels, log_scale_factor, margin,
                                lowe_ratio, q.xy, q.x_right, q.level, d_observable, q.reproj, w->d_assigned, w->d_num + 1, w->d_num, s);
    if (st != OVS_OK) return st;
    // the optional outputs come down only when asked for, through the pinned buffer at their arena offsets (the copy up is behind us on this stream)
    auto mirror = [&](const void* d_ptr) { return w->h_stage + (reinterpret_cast<const unsigned char*>(d_ptr) - w->d_stage); };
    if (reproj) OVS_HIP_TRY(hipMemcpyAsync(mirror(q.reproj), q.reproj, sizeof(double) * 2 * (size_t)m, hipMemcpyDeviceToHost, s));
    if (x_right) OVS_HIP_TRY(hipMemcpyAsync(mirror(q.x_right), q.x_right, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, s));
    if (level) OVS_HIP_TRY(hipMemcpyAsync(mirror(q.level), q.level, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipMemcpyAsync(w->h_res, w->d_res_block, search_result_bytes(m), hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    if (n > 0) {   // (without keypoints no list was built: the overflow word is whatever the last call left)
        if (w->h_res[0]) return OVS_ERR_CAPACITY;
        w->overflow_dirty = false;
    }
    std::memcpy(assigned, w->h_res + 8, sizeof(int32_t) * (size_t)m);
    std::memcpy(observable, w->h_res + 8 + m, (size_t)m);
    *num_matches = w->h_res[1];
    *num_observable = w->h_res[2];
    if (reproj) std::memcpy(reproj, mirror(q.reproj), sizeof(double) * 2 * (size_t)m);
    if (x_right) std::memcpy(x_right, mirror(q.x_right), sizeof(float) * (size_t)m);
    if (level) std::memcpy(level, mirror(q.level), sizeof(int32_t) * (size_t)m);
    return OVS_OK;
}

ovs_status area_match_in_consistent_area_impl(ovs_wmatcher* w, const ovs_frame_dev* res_1, const ovs_frame_dev* res_2, const ovs_grid_params* gp,
                                              const ovs_keypoint* kps_1, const uint8_t* desc_1, int32_t n1, const ovs_keypoint* kps_2, const uint8_t* desc_2,
                                              int32_t n2, float* prev_matched_xy, int32_t* matched_2_in_1, int32_t margin, float lowe_ratio,
                                              int32_t check_orientation, int32_t* num_matches) {
    if (!w || !num_matches || n1 < 0 || n2 < 0) return OVS_ERR_INVALID;
    *num_matches = 0;
    if (n1 == 0) return OVS_OK;
    if ((!res_1 && (!kps_1 || !desc_1)) || !prev_matched_xy || !matched_2_in_1) return OVS_ERR_INVALID;
    if (n2 == 0) {
        for (int i = 0; i < n1; ++i) matched_2_in_1[i] = -1;
        return OVS_OK;
    }
    if (!res_2 && (!kps_2 || !desc_2)) return OVS_ERR_INVALID;
    Stager stg(w);
    TargetRef r1, r2;
    ovs_status st = resident_side(w, res_1, n1, &r1);
    if (st == OVS_OK) st = resident_side(w, res_2, n2, &r2);
    if (st != OVS_OK) return st;
    AreaStaged a = stage_area(stg, prev_matched_xy, res_1 ? &r1 : nullptr, kps_1, desc_1, n1, res_2 ? &r2 : nullptr, kps_2, desc_2, n2);
    if (n2 > w->max_t || n1 > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    if ((st = stg.flush(s)) != OVS_OK || (st = index_target(w, gp, n2, &a.f2, s)) != OVS_OK) return st;
    st = area_on_device(w, a.f1.kps, a.f1.desc, n1, a.f2, n2, a.prev, w->d_assigned, margin, lowe_ratio, check_orientation, w->d_num, s);
    if (st != OVS_OK) return st;
    OVS_HIP_TRY(hipMemcpyAsync(w->h_stage, a.prev, sizeof(float) * 2 * (size_t)n1, hipMemcpyDeviceToHost, s));
    st = fetch_results(w, n1, matched_2_in_1, num_matches, s);
    if (st != OVS_ERR_HIP) std::memcpy(prev_matched_xy, w->h_stage, sizeof(float) * 2 * (size_t)n1);   // only behind fetch_results' synchronisation
    return st;
}

ovs_status projection_match_current_and_last_frames_impl(ovs_wmatcher* w, const ovs_frame_dev* res, const ovs_camera* cam, const ovs_grid_params* gp,
                                                         const ovs_keypoint* curr_kps, const uint8_t* curr_desc, const float* curr_stereo_x_right,
                                                         const uint8_t* curr_occupied, int32_t n_curr, const double* pose_cw_curr, const ovs_keypoint* last_kps,
                                                         const double* last_pos_w, const uint8_t* last_lm_desc, const uint8_t* last_valid, int32_t n_last,
                                                         const double* pose_cw_last, const float* scale_factors, int32_t num_levels, float margin,
                                                         int32_t check_orientation, int32_t* assigned, int32_t* num_matches) {
    if (!w || !cam || !gp || !num_matches || n_curr < 0 || n_last < 0 || !pose_cw_curr || !pose_cw_last || !scale_factors || num_levels < 1 ||
        num_levels > OVS_MAX_LEVELS || (cam->model != 0 && cam->model != 1))
        return OVS_ERR_INVALID;
    *num_matches = 0;
    if (n_last == 0) return OVS_OK;
    if (!assigned) return OVS_ERR_INVALID;
    for (int i = 0; i < n_last; ++i) assigned[i] = -1;
    if (n_curr == 0) return OVS_OK;
    if ((!res && (!curr_kps || !curr_desc)) || !last_kps || !last_pos_w || !last_lm_desc) return OVS_ERR_INVALID;
    Stager stg(w);
    TargetRef r;
    ovs_status st = resident_side(w, res, n_curr, &r);
    if (st != OVS_OK) return st;
    TargetRef tg = stage_target(stg, res ? &r : nullptr, curr_kps, curr_desc, curr_stereo_x_right, nullptr, n_curr);
    if (n_curr > w->max_t || n_last > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    int forward, backward;
    motion_direction(cam, pose_cw_curr, pose_cw_last, &forward, &backward);
    CamP cp{};
    fill_cam(cp, cam, gp, pose_cw_curr);
    float sf16[OVS_MAX_LEVELS];
    pad_levels(sf16, scale_factors, num_levels, 1.0f);
    const ReprojectedQueries rq = stage_reprojected_queries(stg, curr_occupied, n_curr, last_kps, last_pos_w, nullptr, nullptr, last_lm_desc, sf16, last_valid, n_last);
    const QueryScratch& q = rq.q;
    if ((st = stg.flush(s)) != OVS_OK || (st = index_target(w, gp, n_curr, &tg, s)) != OVS_OK) return st;
    hipLaunchKernelGGL(k_reproject_queries, dim3((n_last + 255) / 256), dim3(256), 0, s, cp, rq.kps, rq.pos, q.valid_in, n_last, margin, rq.scale, num_levels, forward,
                       backward, (const float*)nullptr, 0.0, 0.0, 0.0, 0.0f, q.xy, q.x_right, q.radius, q.minl, q.maxl, q.valid);
    OVS_HIP_TRY(hipGetLastError());
    const WinArgs a = generic_window_args(tg, true, rq.occupied, q, rq.desc, n_last, margin, dead_from_thr(OVS_HAMMING_DIST_THR_HIGH));
    return generic_match(w, a, n_curr, rq.kps, check_orientation, OVS_HAMMING_DIST_THR_HIGH, assigned, num_matches, s);
}

ovs_status projection_match_frame_and_keyframe_impl(ovs_wmatcher* w, const ovs_frame_dev* res, const ovs_camera* cam, const ovs_grid_params* gp,
                                                    const ovs_keypoint* curr_kps, const uint8_t* curr_desc, const uint8_t* curr_occupied, int32_t n_curr,
                                                    const double* pose_cw_curr, const ovs_keypoint* kf_kps, const double* kf_pos_w, const float* kf_dist_min_max,
                                                    const uint8_t* kf_lm_desc, const uint8_t* kf_valid, int32_t n_kf, const float* scale_factors,
                                                    int32_t num_levels, float log_scale_factor, float margin, uint32_t hamm_dist_thr, int32_t check_orientation,
                                                    int32_t* assigned, int32_t* num_matches) {
    if (!w || !cam || !gp || !num_matches || n_curr < 0 || n_kf < 0 || !pose_cw_curr || !scale_factors || num_levels < 1 ||
        num_levels > OVS_MAX_LEVELS || (cam->model != 0 && cam->model != 1))
        return OVS_ERR_INVALID;
    *num_matches = 0;
    if (n_kf == 0) return OVS_OK;
    if (!assigned) return OVS_ERR_INVALID;
    for (int i = 0; i < n_kf; ++i) assigned[i] = -1;
    if (n_curr == 0) return OVS_OK;
    if ((!res && (!curr_kps || !curr_desc)) || !kf_kps || !kf_pos_w || !kf_dist_min_max || !kf_lm_desc) return OVS_ERR_INVALID;
    if (n_curr > w->max_t || n_kf > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    CamP cp{};
    fill_cam(cp, cam, gp, pose_cw_curr);
    double cc[3];
    camera_centre(pose_cw_curr, cc);
    float sf16[OVS_MAX_LEVELS];
    pad_levels(sf16, scale_factors, num_levels, 1.0f);
    Stager stg(w);
    TargetRef r;
    ovs_status st = resident_side(w, res, n_curr, &r);
    if (st != OVS_OK) return st;
    const ReprojectedQueries rq = stage_reprojected_queries(stg, curr_occupied, n_curr, kf_kps, kf_pos_w, kf_dist_min_max, nullptr, kf_lm_desc, sf16, kf_valid, n_kf);
    const QueryScratch& q = rq.q;
    TargetRef tg = stage_target(stg, res ? &r : nullptr, curr_kps, curr_desc, nullptr, nullptr, n_curr);
    if ((st = stg.flush(s)) != OVS_OK || (st = index_target(w, gp, n_curr, &tg, s)) != OVS_OK) return st;
    hipLaunchKernelGGL(k_reproject_queries, dim3((n_kf + 255) / 256), dim3(256), 0, s, cp, rq.kps, rq.pos, q.valid_in, n_kf, margin, rq.scale, num_levels, 0, 0,
                       rq.dist, cc[0], cc[1], cc[2], log_scale_factor, q.xy, q.x_right, q.radius, q.minl, q.maxl, q.valid);
    OVS_HIP_TRY(hipGetLastError());
    const WinArgs a = generic_window_args(tg, false, rq.occupied, q, rq.desc, n_kf, margin, dead_from_thr(hamm_dist_thr));
    return generic_match(w, a, n_curr, rq.kps, check_orientation, hamm_dist_thr, assigned, num_matches, s);
}

ovs_status projection_match_by_sim3_transform_impl(ovs_wmatcher* w, const ovs_frame_dev* res, const ovs_camera* cam, const ovs_grid_params* gp,
                                                   const ovs_keypoint* kps, const uint8_t* desc, const uint8_t* occupied, int32_t n, const double* sim3_cw,
                                                   const double* lm_pos_w, const float* lm_dist_min_max, const double* lm_normal, const uint8_t* lm_desc,
                                                   const uint8_t* lm_valid, int32_t m, const float* scale_factors, int32_t num_levels, float log_scale_factor,
                                                   float margin, int32_t* assigned, int32_t* num_matches) {
    if (!w || !cam || !gp || !num_matches || n < 0 || m < 0 || !sim3_cw || !scale_factors || num_levels < 1 || num_levels > OVS_MAX_LEVELS ||
        (cam->model != 0 && cam->model != 1))
        return OVS_ERR_INVALID;
    *num_matches = 0;
    if (m == 0) return OVS_OK;
    if (!assigned) return OVS_ERR_INVALID;
    for (int i = 0; i < m; ++i) assigned[i] = -1;
    if (n == 0) return OVS_OK;
    if ((!res && (!kps || !desc)) || !lm_pos_w || !lm_dist_min_max || !lm_normal || !lm_desc) return OVS_ERR_INVALID;
    if (n > w->max_t || m > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    CamP cp{};
    double P[12], cc[3];
    decompose_sim3(sim3_cw, P, cc);
    fill_cam(cp, cam, gp, P);
    float sf16[OVS_MAX_LEVELS];
    pad_levels(sf16, scale_factors, num_levels, 1.0f);
    Stager stg(w);
    TargetRef r;
    ovs_status st = resident_side(w, res, n, &r);
    if (st != OVS_OK) return st;
    const ReprojectedQueries rq = stage_reprojected_queries(stg, occupied, n, nullptr, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc, sf16, lm_valid, m);
    const QueryScratch& q = rq.q;
    TargetRef tg = stage_target(stg, res ? &r : nullptr, kps, desc, nullptr, nullptr, n);
    if ((st = stg.flush(s)) != OVS_OK || (st = index_target(w, gp, n, &tg, s)) != OVS_OK) return st;
    hipLaunchKernelGGL(k_reproject_queries, dim3((m + 255) / 256), dim3(256), 0, s, cp, rq.kps, rq.pos, q.valid_in, m, margin, rq.scale, num_levels, 0, 0, rq.dist,
                       cc[0], cc[1], cc[2], log_scale_factor, q.xy, q.x_right, q.radius, q.minl, q.maxl, q.valid, rq.normal, 0);
    OVS_HIP_TRY(hipGetLastError());
    const WinArgs a = generic_window_args(tg, false, rq.occupied, q, rq.desc, m, margin, dead_from_thr(OVS_HAMMING_DIST_THR_LOW));
    return generic_match(w, a, n, nullptr, 0, OVS_HAMMING_DIST_THR_LOW, assigned, num_matches, s);
}

// k_fuse_best of `a.m` landmarks against an indexed target
ovs_status launch_fuse_best(FuseArgs& a, const TargetRef& t, bool stereo, int32_t* d_best, int32_t* d_num, hipStream_t s) {
    a.t_kps = t.kps;
    a.t_desc = t.desc;
    a.t_x_right = stereo ? t.x_right : nullptr;
    a.cell_start = t.cell_start;
    a.items = t.items;
    a.gp = t.gp;
    hipLaunchKernelGGL(k_fuse_best, dim3((unsigned)(((size_t)a.m * kFuseLanes + 255) / 256)), dim3(256), 0, s, a, d_best, d_num);
    OVS_HIP_TRY(hipGetLastError());
    return OVS_OK;
}

// fuse::replace_duplication (kFuseReplace: pose_cw, chi-square gate with inv_level_sigma_sq, stereo) and fuse::detect_duplication (kFuseDetect: `pose` is
// Sim3_cw, no inv_level_sigma_sq, monocular)
ovs_status fuse_duplication_impl(ovs_wmatcher* w, const ovs_frame_dev* res, int variant, const ovs_camera* cam, const ovs_grid_params* gp, const ovs_keypoint* kps,
                                 const uint8_t* desc, const float* stereo_x_right, int32_t n, const double* pose, const double* lm_pos_w,
                                 const float* lm_dist_min_max, const double* lm_normal, const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m,
                                 const float* scale_factors, const float* inv_level_sigma_sq, int32_t num_levels, float log_scale_factor, float margin,
                                 int32_t* best_idx, int32_t* num_found) {
    const bool replace = variant == kFuseReplace;
    if (!w || !cam || !gp || !num_found || n < 0 || m < 0 || !pose || !scale_factors || (replace && !inv_level_sigma_sq) || num_levels < 1 ||
        num_levels > OVS_MAX_LEVELS || (cam->model != 0 && cam->model != 1))
        return OVS_ERR_INVALID;
    *num_found = 0;
    if (m == 0) return OVS_OK;
    if (!best_idx) return OVS_ERR_INVALID;
    for (int i = 0; i < m; ++i) best_idx[i] = -1;
    if (n == 0) return OVS_OK;
    if ((!res && (!kps || !desc)) || !lm_pos_w || !lm_dist_min_max || !lm_normal || !lm_desc) return OVS_ERR_INVALID;
    if (n > w->max_t || m > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    FuseArgs a{};
    if (replace) {
        fill_cam(a.cam, cam, gp, pose);
        camera_centre(pose, a.cc);
    } else {
        double P[12];
        decompose_sim3(pose, P, a.cc);
        fill_cam(a.cam, cam, gp, P);
    }
    pad_levels(a.sf, scale_factors, num_levels, 1.0f);
    pad_levels(a.ils, replace ? inv_level_sigma_sq : nullptr, num_levels, 1.0f);
    a.num_levels = num_levels;
    a.log_scale_factor = log_scale_factor;
    a.margin = margin;
    a.variant = variant;
    a.max_dist = OVS_HAMMING_DIST_THR_LOW;
    Stager stg(w);
    TargetRef r;
    ovs_status st = resident_side(w, res, n, &r);
    if (st != OVS_OK) return st;
    stage_fuse_landmarks(stg, a, lm_pos_w, lm_normal, lm_dist_min_max, lm_desc, lm_valid, m);
    TargetRef tg = stage_target(stg, res ? &r : nullptr, kps, desc, stereo_x_right, nullptr, n);
    if ((st = stg.flush(s)) != OVS_OK || (st = index_target(w, gp, n, &tg, s)) != OVS_OK) return st;
    OVS_HIP_TRY(hipMemsetAsync(w->d_num, 0, sizeof(int32_t), s));
    st = launch_fuse_best(a, tg, replace, w->d_assigned, w->d_num, s);
    if (st != OVS_OK) return st;
    return fetch_results(w, m, best_idx, num_found, s, false);
}

ovs_status projection_match_keyframes_mutually_impl(ovs_wmatcher* w, const ovs_frame_dev* res_1, const ovs_frame_dev* res_2, const ovs_camera* cam_1,
                                                    const ovs_grid_params* gp_1, const ovs_keypoint* kps_1, const uint8_t* desc_1, int32_t n1,
                                                    const double* pose_cw_1, const double* lm_pos_w_1, const float* lm_dist_1, const uint8_t* lm_desc_1,
                                                    const uint8_t* lm_valid_1, const ovs_camera* cam_2, const ovs_grid_params* gp_2, const ovs_keypoint* kps_2,
                                                    const uint8_t* desc_2, int32_t n2, const double* pose_cw_2, const double* lm_pos_w_2, const float* lm_dist_2,
                                                    const uint8_t* lm_desc_2, const uint8_t* lm_valid_2, double s_12, const double* rot_12, const double* trans_12,
                                                    const float* scale_factors, int32_t num_levels, float log_scale_factor, float margin, int32_t* matched_2_in_1,
                                                    int32_t* num_matches) {
    if (!w || !cam_1 || !cam_2 || !gp_1 || !gp_2 || !num_matches || n1 < 0 || n2 < 0 || !pose_cw_1 || !pose_cw_2 || !rot_12 || !trans_12 ||
        !scale_factors || num_levels < 1 || num_levels > OVS_MAX_LEVELS || (cam_1->model != 0 && cam_1->model != 1) ||
        (cam_2->model != 0 && cam_2->model != 1) || !(s_12 > 0.0))
        return OVS_ERR_INVALID;
    *num_matches = 0;
    if (n1 == 0) return OVS_OK;
    if (!matched_2_in_1) return OVS_ERR_INVALID;
    for (int i = 0; i < n1; ++i) matched_2_in_1[i] = -1;
    if (n2 == 0) return OVS_OK;
    if ((!res_1 && (!kps_1 || !desc_1)) || !lm_pos_w_1 || !lm_dist_1 || !lm_desc_1 || (!res_2 && (!kps_2 || !desc_2)) || !lm_pos_w_2 || !lm_dist_2 || !lm_desc_2)
        return OVS_ERR_INVALID;
    const int nmax = std::max(n1, n2);
    if (nmax > w->max_t || nmax > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    double S12[12], S21[12];
    sim3_both_ways(s_12, rot_12, trans_12, S12, S21);
    // two one-way searches, then the cross check. a21: the landmarks of keyframe 1 (pose 1, then S21) against the keypoints of keyframe 2; a12: the reverse
    FuseArgs a21{}, a12{};
    fill_cam(a21.cam, cam_2, gp_2, S21);
    fill_cam(a12.cam, cam_1, gp_1, S12);
    std::memcpy(a21.P1, pose_cw_1, sizeof(double) * 12);
    std::memcpy(a12.P1, pose_cw_2, sizeof(double) * 12);
    for (FuseArgs* a : {&a21, &a12}) {
        pad_levels(a->sf, scale_factors, num_levels, 1.0f);
        pad_levels(a->ils, nullptr, num_levels, 1.0f);
        a->num_levels = num_levels;
        a->log_scale_factor = log_scale_factor;
        a->margin = margin;
        a->variant = kFuseMutual;
        a->max_dist = OVS_HAMMING_DIST_THR_HIGH;
    }
    Stager stg(w);   // both directions in one arena: one copy up
    TargetRef r1, r2;
    ovs_status st = resident_side(w, res_1, n1, &r1);
    if (st == OVS_OK) st = resident_side(w, res_2, n2, &r2);
    if (st != OVS_OK) return st;
    MutualStaged m = stage_mutual(stg, a21, a12, res_1 ? &r1 : nullptr, kps_1, desc_1, n1, lm_pos_w_1, lm_dist_1, lm_desc_1, lm_valid_1, res_2 ? &r2 : nullptr, kps_2,
                                  desc_2, n2, lm_pos_w_2, lm_dist_2, lm_desc_2, lm_valid_2);
    if ((st = stg.flush(s)) != OVS_OK) return st;
    // staged targets share the context's one grid: the second is indexed behind the first direction's kernel, in stream order.
    // d_num[1] takes the per-direction counts: scratch
    if ((st = index_target(w, gp_2, n2, &m.t2, s)) != OVS_OK || (st = launch_fuse_best(a21, m.t2, false, m.d_2_in_1, w->d_num + 1, s)) != OVS_OK) return st;
    if ((st = index_target(w, gp_1, n1, &m.t1, s)) != OVS_OK || (st = launch_fuse_best(a12, m.t1, false, m.d_1_in_2, w->d_num + 1, s)) != OVS_OK) return st;
    OVS_HIP_TRY(hipMemsetAsync(w->d_num, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_cross_check, dim3((n1 + 255) / 256), dim3(256), 0, s, (const int32_t*)m.d_2_in_1, (const int32_t*)m.d_1_in_2, n1, n2, w->d_assigned, w->d_num);
    OVS_HIP_TRY(hipGetLastError());
    return fetch_results(w, n1, matched_2_in_1, num_matches, s, false);
}

struct TriParams {   // robust::match_for_triangulation extras (host pointers)
    const float* x_right_1;
    const float* x_right_2;
    const double* bearings_1;
    const double* bearings_2;
    const double* E_12;
    const double* epipole_in_2;
    const float* scale_factors;
    int num_levels;
};

// bow_tree::match_frame_and_keyframe (by_query 0), bow_tree::match_keyframes (1) and robust::match_for_triangulation (1, tri): either side host
// arrays or a resident frame / keyframe; the flags and the BoW feature vectors (node CSRs) always travel
ovs_status bow_match_impl(ovs_wmatcher* w, const ovs_frame_dev* res_kf, const ovs_frame_dev* res_frm, int by_query, const uint8_t* frm_valid, const TriParams* tri,
                          const ovs_keypoint* kf_kps, const uint8_t* kf_desc, const uint8_t* kf_valid, int32_t n_kf, const int32_t* kf_node_ids,
                          const int32_t* kf_node_start, const int32_t* kf_items, int32_t kf_nodes, const ovs_keypoint* frm_kps, const uint8_t* frm_desc,
                          int32_t n_frm, const int32_t* frm_node_ids, const int32_t* frm_node_start, const int32_t* frm_items, int32_t frm_nodes, float lowe_ratio,
                          int32_t check_orientation, int32_t* matched_kf_in_frm, int32_t* num_matches) {
    if (!w || !num_matches || n_kf < 0 || n_frm < 0 || kf_nodes < 0 || frm_nodes < 0) return OVS_ERR_INVALID;
    *num_matches = 0;
    const int n_out = by_query ? n_kf : n_frm;
    if (n_out == 0) return OVS_OK;
    if (!matched_kf_in_frm) return OVS_ERR_INVALID;
    for (int i = 0; i < n_out; ++i) matched_kf_in_frm[i] = -1;
    if (n_frm == 0) return OVS_OK;
    if (n_kf == 0 || kf_nodes == 0 || frm_nodes == 0) return OVS_OK;
    if ((!res_kf && (!kf_kps || !kf_desc)) || !kf_node_ids || !kf_node_start || !kf_items || (!res_frm && (!frm_kps || !frm_desc)) || !frm_node_ids ||
        !frm_node_start || !frm_items)
        return OVS_ERR_INVALID;
    // keypoints (angle, octave), descriptors and for the triangulation matcher stereo_x_right and bearings of either side
    Stager stg(w);
    TargetRef r_kf, r_frm;
    ovs_status st = resident_side(w, res_kf, n_kf, &r_kf);
    if (st == OVS_OK) st = resident_side(w, res_frm, n_frm, &r_frm);
    if (st != OVS_OK) return st;
    const int nq = kf_node_start[kf_nodes], nfi = frm_node_start[frm_nodes];
    if (nq == 0 || nfi == 0) return OVS_OK;
    if (n_frm > w->max_t || n_kf > w->max_q || nq > w->max_q || (by_query && n_kf > std::max(w->max_t, w->max_q))) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    const BowStaged b = stage_bow(stg, res_kf ? &r_kf : nullptr, kf_kps, kf_desc, tri ? tri->x_right_1 : nullptr, tri ? tri->bearings_1 : nullptr, kf_valid, n_kf,
                                  kf_node_ids, kf_node_start, kf_items, kf_nodes, nq, res_frm ? &r_frm : nullptr, frm_kps, frm_desc, tri ? tri->x_right_2 : nullptr,
                                  tri ? tri->bearings_2 : nullptr, frm_valid, n_frm, frm_node_ids, frm_node_start, frm_items, frm_nodes, nfi);
    const TargetRef &kf = b.kf, &frm = b.frm;
    BowArgs a{};
    a.kf_desc = kf.desc;
    a.kf_valid = b.kf_fv.valid;
    a.kf_node_ids = b.kf_fv.node_ids;
    a.kf_node_start = b.kf_fv.node_start;
    a.kf_items = b.kf_fv.items;
    a.kf_nodes = kf_nodes;
    a.n_q = nq;
    a.frm_desc = frm.desc;
    a.frm_valid = b.frm_fv.valid;
    a.frm_node_ids = b.frm_fv.node_ids;
    a.frm_node_start = b.frm_fv.node_start;
    a.frm_items = b.frm_fv.items;
    a.frm_nodes = frm_nodes;
    if ((st = stg.flush(s)) != OVS_OK) return st;   // (a feature vector beyond the arena's CSR budget: OVS_ERR_CAPACITY)
    if (tri) {
        if (!kf.bearings || !frm.bearings) return OVS_ERR_INVALID;
        a.tri = 1;
        a.kf_kps = kf.kps;
        a.kf_bearings = kf.bearings;
        a.frm_bearings = frm.bearings;
        a.kf_x_right = kf.x_right;
        a.frm_x_right = frm.x_right;
        std::memcpy(a.E, tri->E_12, sizeof(double) * 9);
        std::memcpy(a.epipole, tri->epipole_in_2, sizeof(double) * 3);
        pad_levels(a.sf, tri->scale_factors, tri->num_levels, 1.0f);
    }
    a.dead_from = tri ? 0u : dead_from_ratio(OVS_HAMMING_DIST_THR_LOW, lowe_ratio);
    st = build_lists(w, a, nq, k_bow_lists<false>, k_bow_lists<true>, s, 256);
    if (st != OVS_OK) return st;
    ResolveArgs ra = resolve_args(w, nq, n_frm);
    ra.lowe_ratio = lowe_ratio;
    ra.check_orientation = check_orientation;
    ra.q_kps = kf.kps;
    ra.q_items = a.kf_items;
    ra.t_kps = frm.kps;
    ra.bow_by_query = by_query;
    ra.n_out_q = n_kf;
    ra.best_only_thr = OVS_HAMMING_DIST_THR_LOW;
    st = tri ? launch_resolve<kRuleTriang>(ra, s) : launch_resolve<kRuleBow>(ra, s);
    if (st != OVS_OK) return st;
    return fetch_results(w, n_out, matched_kf_in_frm, num_matches, s);
}

}   // namespace

extern "C" {

ovs_status ovs_wmatcher_create(int32_t max_targets, int32_t max_queries, int32_t max_entries, int32_t device, ovs_wmatcher** out) {
    if (!out || max_targets < 1 || max_queries < 1 || max_entries < 1 || max_targets > 65534 || max_queries > 65534) return OVS_ERR_INVALID;
    *out = nullptr;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    if (!resolve_plan(max_queries, max_targets, 0).ok) return OVS_ERR_CAPACITY;   // the resolver could not hold the largest call in LDS
    std::unique_ptr<ovs_wmatcher> owner(new (std::nothrow) ovs_wmatcher());
    ovs_wmatcher* const w = owner.get();
    if (!w) return OVS_ERR_INVALID;
    w->device = device;
    w->max_t = max_targets;
    w->max_q = max_queries;
    w->max_entries = (uint32_t)max_entries;
    OVS_HIP_TRY_RAW(hipSetDevice(device));
    OVS_HIP_TRY_RAW(w->res.stream(&w->stream));
    const size_t T = (size_t)max_targets, Q = (size_t)max_queries, M = std::max(T, Q);
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_cell_of, sizeof(int32_t) * T));
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_cell_start, sizeof(int32_t) * (kMaxGridCells + 1)));
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_items, sizeof(int32_t) * T));
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_counts, sizeof(uint32_t) * (Q + 1)));
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_offsets, sizeof(uint32_t) * (Q + 1)));
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_keys, sizeof(uint32_t) * (size_t)max_entries));
    // result block: [0] overflow flag, [1..4] counts ([1] result count, [2] per-direction scratch count), [8..] assigned
    // (ovs_tracking_search_local_landmarks puts observable[m] behind assigned[m]: Q more bytes)
    const size_t res_bytes = std::max(sizeof(int32_t) * (8 + M), search_result_bytes((int)Q));
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_res_block, res_bytes));
    w->d_overflow = w->d_res_block;
    w->d_num = reinterpret_cast<int32_t*>(w->d_res_block) + 1;
    w->d_assigned = reinterpret_cast<int32_t*>(w->d_res_block) + 8;
    OVS_HIP_TRY_RAW(hipMemset(w->d_res_block, 0, sizeof(int32_t) * 8));
    OVS_HIP_TRY_RAW(w->res.pinned(&w->h_res, res_bytes));
    w->stage_cap = stage_capacity(T, Q);   // room for every array of the call that stages the most at n == max_targets, m == max_queries
    OVS_HIP_TRY_RAW(w->res.pinned(&w->h_stage, w->stage_cap));
    OVS_HIP_TRY_RAW(w->res.dev(&w->d_stage, w->stage_cap));
    *out = owner.release();
    return OVS_OK;
}

ovs_status ovs_wmatcher_destroy(ovs_wmatcher* w) {
    if (!w) return OVS_OK;
    delete w;
    return OVS_OK;
}

// ---- device-array forms (_dev): inputs and outputs in HBM, the caller's stream, nothing staged and nothing synchronised ----

ovs_status ovs_grid_assign_dev(ovs_wmatcher* w, const ovs_grid_params* gp, const ovs_keypoint* d_kps, int32_t n, void* stream) {
    if (!w || !d_kps || n < 0) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(w->device));
    return grid_assign(w, gp, d_kps, n, (hipStream_t)stream);
}

ovs_status ovs_projection_match_frame_and_landmarks_dev(ovs_wmatcher* w, const ovs_grid_params* gp, const ovs_keypoint* d_kps,
                                                        const uint8_t* d_desc, const float* d_stereo_x_right, const uint8_t* d_occupied,
                                                        int32_t n, const float* d_lm_xy, const float* d_lm_x_right,
                                                        const int32_t* d_lm_level, const uint8_t* d_lm_desc, const uint8_t* d_lm_valid,
                                                        int32_t m, const float* scale_factors, int32_t num_levels, float margin,
                                                        float lowe_ratio, int32_t* d_assigned, int32_t* d_num_matches, void* stream) {
    if (!w || !d_kps || !d_desc || n < 0 || m < 0 || !d_assigned || !d_num_matches || !scale_factors || num_levels < 1 ||
        num_levels > OVS_MAX_LEVELS || (m > 0 && (!d_lm_xy || !d_lm_level || !d_lm_desc)) || (d_stereo_x_right && !d_lm_x_right))
        return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {
        OVS_HIP_TRY(hipMemsetAsync(d_num_matches, 0, sizeof(int32_t), s));
        return OVS_OK;
    }
    TargetRef tg{d_kps, d_desc, d_stereo_x_right, nullptr, nullptr, nullptr, GridP{}};
    const ovs_status st = index_target(w, gp, n, &tg, s);
    if (st != OVS_OK) return st;
    return frame_and_landmarks_on_device(w, tg, d_occupied, n, d_lm_xy, d_lm_x_right, d_lm_level, d_lm_desc, d_lm_valid, m, scale_factors, num_levels, margin,
                                         lowe_ratio, d_assigned, d_num_matches, s);
}

ovs_status ovs_area_match_in_consistent_area_dev(ovs_wmatcher* w, const ovs_grid_params* gp, const ovs_keypoint* d_kps_1,
                                                 const uint8_t* d_desc_1, int32_t n1, const ovs_keypoint* d_kps_2,
                                                 const uint8_t* d_desc_2, int32_t n2, float* d_prev_matched_xy,
                                                 int32_t* d_matched_2_in_1, int32_t margin, float lowe_ratio, int32_t check_orientation,
                                                 int32_t* d_num_matches, void* stream) {
    if (!w || n1 < 0 || n2 < 0 || !d_num_matches || (n1 > 0 && (!d_kps_1 || !d_desc_1 || !d_prev_matched_xy || !d_matched_2_in_1)) ||
        (n2 > 0 && (!d_kps_2 || !d_desc_2)))
        return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = (hipStream_t)stream;
    if (n1 == 0) {
        OVS_HIP_TRY(hipMemsetAsync(d_num_matches, 0, sizeof(int32_t), s));
        return OVS_OK;
    }
    TargetRef t2{d_kps_2, d_desc_2, nullptr, nullptr, nullptr, nullptr, GridP{}};
    const ovs_status st = index_target(w, gp, n2, &t2, s);
    if (st != OVS_OK) return st;
    return area_on_device(w, d_kps_1, d_desc_1, n1, t2, n2, d_prev_matched_xy, d_matched_2_in_1, margin, lowe_ratio, check_orientation, d_num_matches, s);
}

ovs_status ovs_tracking_search_local_landmarks_dev(ovs_wmatcher* w, const ovs_camera* cam, const ovs_grid_params* gp, const ovs_keypoint* d_kps,
                                                   const uint8_t* d_desc, const float* d_stereo_x_right, const uint8_t* d_occupied, int32_t n,
                                                   const double* pose_cw, const double* d_lm_pos_w, const float* d_lm_dist_min_max,
                                                   const double* d_lm_normal, const uint8_t* d_lm_desc, const uint8_t* d_lm_search, int32_t m,
                                                   const float* scale_factors, int32_t num_levels, float log_scale_factor, float margin,
                                                   float lowe_ratio, uint8_t* d_observable, double* d_reproj, float* d_x_right, int32_t* d_level,
                                                   int32_t* d_assigned, int32_t* d_num_observable, int32_t* d_num_matches, void* stream) {
    if (!w || !cam || !gp || !d_num_observable || !d_num_matches || n < 0 || m < 0 || !pose_cw || !scale_factors || num_levels < 1 ||
        num_levels > OVS_MAX_LEVELS || (cam->model != 0 && cam->model != 1) ||
        (m > 0 && (!d_observable || !d_assigned || !d_lm_pos_w || !d_lm_dist_min_max || !d_lm_normal || !d_lm_desc || (n > 0 && (!d_kps || !d_desc)))))
        return OVS_ERR_INVALID;
    if (n > w->max_t || m > w->max_q) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {
        OVS_HIP_TRY(hipMemsetAsync(d_num_observable, 0, sizeof(int32_t), s));
        OVS_HIP_TRY(hipMemsetAsync(d_num_matches, 0, sizeof(int32_t), s));
        return OVS_OK;
    }
    CamP cp{};
    fill_cam(cp, cam, gp, pose_cw);
    double cc[3];
    camera_centre(pose_cw, cc);
    // nothing is staged: the context's arena only lends the queries' scratch (the float reprojection; x_right and level where the caller takes none)
    StageWriter scratch(nullptr, w->d_stage, w->stage_cap);
    float* const d_xy = scratch.reserve<float>((size_t)2 * m);
    if (!d_x_right) d_x_right = scratch.reserve<float>((size_t)m);
    if (!d_level) d_level = scratch.reserve<int32_t>((size_t)m);
    if (scratch.overflow) return OVS_ERR_CAPACITY;
    TargetRef tg{d_kps, d_desc, d_stereo_x_right, nullptr, nullptr, nullptr, GridP{}};
    if (n > 0) {
        const ovs_status st = index_target(w, gp, n, &tg, s);
        if (st != OVS_OK) return st;
    }
    return search_local_on_device(w, cp, cc, tg, d_occupied, n, d_lm_pos_w, d_lm_dist_min_max, d_lm_normal, d_lm_desc, d_lm_search, m, scale_factors, num_levels,
                                  log_scale_factor, margin, lowe_ratio, d_xy, d_x_right, d_level, d_observable, d_reproj, d_assigned, d_num_observable,
                                  d_num_matches, s);
}

// ---- data::assign_keypoints_to_grid on its own (the matchers below build or bring their grids themselves) ----

ovs_status ovs_assign_keypoints_to_grid(ovs_wmatcher* w, const ovs_grid_params* gp, const ovs_keypoint* kps, int32_t n,
                                        int32_t* cell_start, int32_t* items, int32_t* n_items) {
    if (!w || !gp || (n > 0 && !kps) || n < 0 || !cell_start || !n_items) return OVS_ERR_INVALID;
    if (n > w->max_t) return OVS_ERR_CAPACITY;
    OVS_HIP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    Stager stg(w);
    const ovs_keypoint* d_kps = stg.put(kps, (size_t)n);
    ovs_status st = stg.flush(s);
    if (st == OVS_OK) st = grid_assign(w, gp, d_kps, n, s);
    if (st != OVS_OK) return st;
    const int nc = gp->cols * gp->rows;
    OVS_HIP_TRY(hipMemcpyAsync(cell_start, w->d_cell_start, sizeof(int32_t) * (nc + 1), hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    *n_items = cell_start[nc];
    if (items && *n_items > 0) {
        OVS_HIP_TRY(hipMemcpyAsync(items, w->d_items, sizeof(int32_t) * *n_items, hipMemcpyDeviceToHost, s));
        OVS_HIP_TRY(hipStreamSynchronize(s));
    }
    return OVS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The matchers: the host-array forms and their resident twins (_f). A twin takes an ovs_frame_dev handle wherever the host form takes
// (grid parameters, keypoints, descriptors, stereo_x_right, n) of a frame / keyframe; everything else -- the landmark side, poses,
// thresholds, outputs -- is unchanged, and so are the results (tests/test_gpu_window.py runs every matcher in both forms against the oracle).
// ---------------------------------------------------------------------------------------------------------------------------

ovs_status ovs_projection_match_frame_and_landmarks(ovs_wmatcher* w, const ovs_grid_params* gp, const ovs_keypoint* kps,
                                                    const uint8_t* desc, const float* stereo_x_right, const uint8_t* occupied, int32_t n,
                                                    const float* lm_xy, const float* lm_x_right, const int32_t* lm_level,
                                                    const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m,
                                                    const float* scale_factors, int32_t num_levels, float margin, float lowe_ratio,
                                                    int32_t* assigned, int32_t* num_matches) {
    return projection_match_frame_and_landmarks_impl(w, nullptr, gp, kps, desc, stereo_x_right, occupied, n, lm_xy, lm_x_right, lm_level, lm_desc, lm_valid, m,
                                                     scale_factors, num_levels, margin, lowe_ratio, assigned, num_matches);
}
ovs_status ovs_projection_match_frame_and_landmarks_f(ovs_wmatcher* w, const ovs_frame_dev* frm, const uint8_t* occupied, const float* lm_xy,
                                                      const float* lm_x_right, const int32_t* lm_level, const uint8_t* lm_desc,
                                                      const uint8_t* lm_valid, int32_t m, const float* scale_factors, int32_t num_levels,
                                                      float margin, float lowe_ratio, int32_t* assigned, int32_t* num_matches) {
    if (!frm) return OVS_ERR_INVALID;
    return projection_match_frame_and_landmarks_impl(w, frm, &frm->gpp, nullptr, nullptr, nullptr, occupied, frm->n, lm_xy, lm_x_right, lm_level, lm_desc, lm_valid,
                                                     m, scale_factors, num_levels, margin, lowe_ratio, assigned, num_matches);
}

ovs_status ovs_tracking_search_local_landmarks(ovs_wmatcher* w, const ovs_camera* cam, const ovs_grid_params* gp, const ovs_keypoint* kps,
                                               const uint8_t* desc, const float* stereo_x_right, const uint8_t* occupied, int32_t n,
                                               const double* pose_cw, const double* lm_pos_w, const float* lm_dist_min_max, const double* lm_normal,
                                               const uint8_t* lm_desc, const uint8_t* lm_search, int32_t m, const float* scale_factors,
                                               int32_t num_levels, float log_scale_factor, float margin, float lowe_ratio, uint8_t* observable,
                                               double* reproj, float* x_right, int32_t* level, int32_t* assigned, int32_t* num_observable,
                                               int32_t* num_matches) {
    return tracking_search_local_landmarks_impl(w, nullptr, cam, gp, kps, desc, stereo_x_right, occupied, n, pose_cw, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc,
                                                lm_search, m, scale_factors, num_levels, log_scale_factor, margin, lowe_ratio, observable, reproj, x_right, level,
                                                assigned, num_observable, num_matches);
}
ovs_status ovs_tracking_search_local_landmarks_f(ovs_wmatcher* w, const ovs_camera* cam, const ovs_frame_dev* frm, const uint8_t* occupied,
                                                 const double* pose_cw, const double* lm_pos_w, const float* lm_dist_min_max, const double* lm_normal,
                                                 const uint8_t* lm_desc, const uint8_t* lm_search, int32_t m, const float* scale_factors,
                                                 int32_t num_levels, float log_scale_factor, float margin, float lowe_ratio, uint8_t* observable,
                                                 double* reproj, float* x_right, int32_t* level, int32_t* assigned, int32_t* num_observable,
                                                 int32_t* num_matches) {
    if (!frm) return OVS_ERR_INVALID;
    return tracking_search_local_landmarks_impl(w, frm, cam, &frm->gpp, nullptr, nullptr, nullptr, occupied, frm->n, pose_cw, lm_pos_w, lm_dist_min_max, lm_normal,
                                                lm_desc, lm_search, m, scale_factors, num_levels, log_scale_factor, margin, lowe_ratio, observable, reproj, x_right,
                                                level, assigned, num_observable, num_matches);
}

ovs_status ovs_area_match_in_consistent_area(ovs_wmatcher* w, const ovs_grid_params* gp, const ovs_keypoint* kps_1, const uint8_t* desc_1,
                                             int32_t n1, const ovs_keypoint* kps_2, const uint8_t* desc_2, int32_t n2,
                                             float* prev_matched_xy, int32_t* matched_2_in_1, int32_t margin, float lowe_ratio,
                                             int32_t check_orientation, int32_t* num_matches) {
    return area_match_in_consistent_area_impl(w, nullptr, nullptr, gp, kps_1, desc_1, n1, kps_2, desc_2, n2, prev_matched_xy, matched_2_in_1, margin, lowe_ratio,
                                              check_orientation, num_matches);
}
ovs_status ovs_area_match_in_consistent_area_f(ovs_wmatcher* w, const ovs_frame_dev* frm_1, const ovs_frame_dev* frm_2, float* prev_matched_xy,
                                               int32_t* matched_2_in_1, int32_t margin, float lowe_ratio, int32_t check_orientation,
                                               int32_t* num_matches) {
    if (!frm_1 || !frm_2) return OVS_ERR_INVALID;
    return area_match_in_consistent_area_impl(w, frm_1, frm_2, &frm_2->gpp, nullptr, nullptr, frm_1->n, nullptr, nullptr, frm_2->n, prev_matched_xy, matched_2_in_1,
                                              margin, lowe_ratio, check_orientation, num_matches);
}

ovs_status ovs_projection_match_current_and_last_frames(ovs_wmatcher* w, const ovs_camera* cam, const ovs_grid_params* gp,
                                                        const ovs_keypoint* curr_kps, const uint8_t* curr_desc,
                                                        const float* curr_stereo_x_right, const uint8_t* curr_occupied, int32_t n_curr,
                                                        const double* pose_cw_curr, const ovs_keypoint* last_kps, const double* last_pos_w,
                                                        const uint8_t* last_lm_desc, const uint8_t* last_valid, int32_t n_last,
                                                        const double* pose_cw_last, const float* scale_factors, int32_t num_levels,
                                                        float margin, int32_t check_orientation, int32_t* assigned, int32_t* num_matches) {
    return projection_match_current_and_last_frames_impl(w, nullptr, cam, gp, curr_kps, curr_desc, curr_stereo_x_right, curr_occupied, n_curr, pose_cw_curr, last_kps,
                                                         last_pos_w, last_lm_desc, last_valid, n_last, pose_cw_last, scale_factors, num_levels, margin,
                                                         check_orientation, assigned, num_matches);
}
ovs_status ovs_projection_match_current_and_last_frames_f(ovs_wmatcher* w, const ovs_camera* cam, const ovs_frame_dev* curr,
                                                          const uint8_t* curr_occupied, const double* pose_cw_curr, const ovs_keypoint* last_kps,
                                                          const double* last_pos_w, const uint8_t* last_lm_desc, const uint8_t* last_valid,
                                                          int32_t n_last, const double* pose_cw_last, const float* scale_factors,
                                                          int32_t num_levels, float margin, int32_t check_orientation, int32_t* assigned,
                                                          int32_t* num_matches) {
    if (!curr) return OVS_ERR_INVALID;
    return projection_match_current_and_last_frames_impl(w, curr, cam, &curr->gpp, nullptr, nullptr, nullptr, curr_occupied, curr->n, pose_cw_curr, last_kps,
                                                         last_pos_w, last_lm_desc, last_valid, n_last, pose_cw_last, scale_factors, num_levels, margin,
                                                         check_orientation, assigned, num_matches);
}

ovs_status ovs_fuse_replace_duplication(ovs_wmatcher* w, const ovs_camera* cam, const ovs_grid_params* gp, const ovs_keypoint* kps, const uint8_t* desc,
                                        const float* stereo_x_right, int32_t n, const double* pose_cw, const double* lm_pos_w, const float* lm_dist_min_max,
                                        const double* lm_normal, const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m, const float* scale_factors,
                                        const float* inv_level_sigma_sq, int32_t num_levels, float log_scale_factor, float margin, int32_t* best_idx,
                                        int32_t* num_fused) {
    return fuse_duplication_impl(w, nullptr, kFuseReplace, cam, gp, kps, desc, stereo_x_right, n, pose_cw, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc, lm_valid, m,
                                 scale_factors, inv_level_sigma_sq, num_levels, log_scale_factor, margin, best_idx, num_fused);
}
ovs_status ovs_fuse_replace_duplication_f(ovs_wmatcher* w, const ovs_camera* cam, const ovs_frame_dev* keyfrm, const double* pose_cw, const double* lm_pos_w,
                                          const float* lm_dist_min_max, const double* lm_normal, const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m,
                                          const float* scale_factors, const float* inv_level_sigma_sq, int32_t num_levels, float log_scale_factor,
                                          float margin, int32_t* best_idx, int32_t* num_fused) {
    if (!keyfrm) return OVS_ERR_INVALID;
    return fuse_duplication_impl(w, keyfrm, kFuseReplace, cam, &keyfrm->gpp, nullptr, nullptr, nullptr, keyfrm->n, pose_cw, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc,
                                 lm_valid, m, scale_factors, inv_level_sigma_sq, num_levels, log_scale_factor, margin, best_idx, num_fused);
}

ovs_status ovs_fuse_detect_duplication(ovs_wmatcher* w, const ovs_camera* cam, const ovs_grid_params* gp, const ovs_keypoint* kps, const uint8_t* desc, int32_t n,
                                       const double* sim3_cw, const double* lm_pos_w, const float* lm_dist_min_max, const double* lm_normal,
                                       const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m, const float* scale_factors, int32_t num_levels,
                                       float log_scale_factor, float margin, int32_t* best_idx, int32_t* num_found) {
    return fuse_duplication_impl(w, nullptr, kFuseDetect, cam, gp, kps, desc, nullptr, n, sim3_cw, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc, lm_valid, m,
                                 scale_factors, nullptr, num_levels, log_scale_factor, margin, best_idx, num_found);
}
ovs_status ovs_fuse_detect_duplication_f(ovs_wmatcher* w, const ovs_camera* cam, const ovs_frame_dev* keyfrm, const double* sim3_cw, const double* lm_pos_w,
                                         const float* lm_dist_min_max, const double* lm_normal, const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m,
                                         const float* scale_factors, int32_t num_levels, float log_scale_factor, float margin, int32_t* best_idx,
                                         int32_t* num_found) {
    if (!keyfrm) return OVS_ERR_INVALID;
    return fuse_duplication_impl(w, keyfrm, kFuseDetect, cam, &keyfrm->gpp, nullptr, nullptr, nullptr, keyfrm->n, sim3_cw, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc,
                                 lm_valid, m, scale_factors, nullptr, num_levels, log_scale_factor, margin, best_idx, num_found);
}

ovs_status ovs_projection_match_frame_and_keyframe(ovs_wmatcher* w, const ovs_camera* cam, const ovs_grid_params* gp, const ovs_keypoint* curr_kps,
                                                   const uint8_t* curr_desc, const uint8_t* curr_occupied, int32_t n_curr, const double* pose_cw_curr,
                                                   const ovs_keypoint* kf_kps, const double* kf_pos_w, const float* kf_dist_min_max, const uint8_t* kf_lm_desc,
                                                   const uint8_t* kf_valid, int32_t n_kf, const float* scale_factors, int32_t num_levels,
                                                   float log_scale_factor, float margin, uint32_t hamm_dist_thr, int32_t check_orientation, int32_t* assigned,
                                                   int32_t* num_matches) {
    return projection_match_frame_and_keyframe_impl(w, nullptr, cam, gp, curr_kps, curr_desc, curr_occupied, n_curr, pose_cw_curr, kf_kps, kf_pos_w, kf_dist_min_max,
                                                    kf_lm_desc, kf_valid, n_kf, scale_factors, num_levels, log_scale_factor, margin, hamm_dist_thr,
                                                    check_orientation, assigned, num_matches);
}
ovs_status ovs_projection_match_frame_and_keyframe_f(ovs_wmatcher* w, const ovs_camera* cam, const ovs_frame_dev* curr, const uint8_t* curr_occupied,
                                                     const double* pose_cw_curr, const ovs_keypoint* kf_kps, const double* kf_pos_w,
                                                     const float* kf_dist_min_max, const uint8_t* kf_lm_desc, const uint8_t* kf_valid, int32_t n_kf,
                                                     const float* scale_factors, int32_t num_levels, float log_scale_factor, float margin,
                                                     uint32_t hamm_dist_thr, int32_t check_orientation, int32_t* assigned, int32_t* num_matches) {
    if (!curr) return OVS_ERR_INVALID;
    return projection_match_frame_and_keyframe_impl(w, curr, cam, &curr->gpp, nullptr, nullptr, curr_occupied, curr->n, pose_cw_curr, kf_kps, kf_pos_w, kf_dist_min_max,
                                                    kf_lm_desc, kf_valid, n_kf, scale_factors, num_levels, log_scale_factor, margin, hamm_dist_thr,
                                                    check_orientation, assigned, num_matches);
}

ovs_status ovs_projection_match_by_sim3_transform(ovs_wmatcher* w, const ovs_camera* cam, const ovs_grid_params* gp, const ovs_keypoint* kps, const uint8_t* desc,
                                                  const uint8_t* occupied, int32_t n, const double* sim3_cw, const double* lm_pos_w,
                                                  const float* lm_dist_min_max, const double* lm_normal, const uint8_t* lm_desc, const uint8_t* lm_valid,
                                                  int32_t m, const float* scale_factors, int32_t num_levels, float log_scale_factor, float margin,
                                                  int32_t* assigned, int32_t* num_matches) {
    return projection_match_by_sim3_transform_impl(w, nullptr, cam, gp, kps, desc, occupied, n, sim3_cw, lm_pos_w, lm_dist_min_max, lm_normal, lm_desc, lm_valid, m,
                                                   scale_factors, num_levels, log_scale_factor, margin, assigned, num_matches);
}
ovs_status ovs_projection_match_by_sim3_transform_f(ovs_wmatcher* w, const ovs_camera* cam, const ovs_frame_dev* keyfrm, const uint8_t* occupied,
                                                    const double* sim3_cw, const double* lm_pos_w, const float* lm_dist_min_max, const double* lm_normal,
                                                    const uint8_t* lm_desc, const uint8_t* lm_valid, int32_t m, const float* scale_factors,
                                                    int32_t num_levels, float log_scale_factor, float margin, int32_t* assigned, int32_t* num_matches) {
    if (!keyfrm) return OVS_ERR_INVALID;
    return projection_match_by_sim3_transform_impl(w, keyfrm, cam, &keyfrm->gpp, nullptr, nullptr, occupied, keyfrm->n, sim3_cw, lm_pos_w, lm_dist_min_max, lm_normal,
                                                   lm_desc, lm_valid, m, scale_factors, num_levels, log_scale_factor, margin, assigned, num_matches);
}

ovs_status ovs_projection_match_keyframes_mutually(ovs_wmatcher* w, const ovs_camera* cam_1, const ovs_grid_params* gp_1, const ovs_keypoint* kps_1,
                                                   const uint8_t* desc_1, int32_t n1, const double* pose_cw_1, const double* lm_pos_w_1,
                                                   const float* lm_dist_1, const uint8_t* lm_desc_1, const uint8_t* lm_valid_1, const ovs_camera* cam_2,
                                                   const ovs_grid_params* gp_2, const ovs_keypoint* kps_2, const uint8_t* desc_2, int32_t n2,
                                                   const double* pose_cw_2, const double* lm_pos_w_2, const float* lm_dist_2, const uint8_t* lm_desc_2,
                                                   const uint8_t* lm_valid_2, double s_12, const double* rot_12, const double* trans_12,
                                                   const float* scale_factors, int32_t num_levels, float log_scale_factor, float margin,
                                                   int32_t* matched_2_in_1, int32_t* num_matches) {
    return projection_match_keyframes_mutually_impl(w, nullptr, nullptr, cam_1, gp_1, kps_1, desc_1, n1, pose_cw_1, lm_pos_w_1, lm_dist_1, lm_desc_1, lm_valid_1, cam_2,
                                                    gp_2, kps_2, desc_2, n2, pose_cw_2, lm_pos_w_2, lm_dist_2, lm_desc_2, lm_valid_2, s_12, rot_12, trans_12,
                                                    scale_factors, num_levels, log_scale_factor, margin, matched_2_in_1, num_matches);
}
ovs_status ovs_projection_match_keyframes_mutually_f(ovs_wmatcher* w, const ovs_camera* cam_1, const ovs_frame_dev* keyfrm_1, const double* pose_cw_1,
                                                     const double* lm_pos_w_1, const float* lm_dist_1, const uint8_t* lm_desc_1, const uint8_t* lm_valid_1,
                                                     const ovs_camera* cam_2, const ovs_frame_dev* keyfrm_2, const double* pose_cw_2,
                                                     const double* lm_pos_w_2, const float* lm_dist_2, const uint8_t* lm_desc_2, const uint8_t* lm_valid_2,
                                                     double s_12, const double* rot_12, const double* trans_12, const float* scale_factors,
                                                     int32_t num_levels, float log_scale_factor, float margin, int32_t* matched_2_in_1,
                                                     int32_t* num_matches) {
    if (!keyfrm_1 || !keyfrm_2) return OVS_ERR_INVALID;
    return projection_match_keyframes_mutually_impl(w, keyfrm_1, keyfrm_2, cam_1, &keyfrm_1->gpp, nullptr, nullptr, keyfrm_1->n, pose_cw_1, lm_pos_w_1, lm_dist_1,
                                                    lm_desc_1, lm_valid_1, cam_2, &keyfrm_2->gpp, nullptr, nullptr, keyfrm_2->n, pose_cw_2, lm_pos_w_2, lm_dist_2,
                                                    lm_desc_2, lm_valid_2, s_12, rot_12, trans_12, scale_factors, num_levels, log_scale_factor, margin,
                                                    matched_2_in_1, num_matches);
}

ovs_status ovs_bow_match_frame_and_keyframe(ovs_wmatcher* w, const ovs_keypoint* kf_kps, const uint8_t* kf_desc, const uint8_t* kf_valid,
                                            int32_t n_kf, const int32_t* kf_node_ids, const int32_t* kf_node_start,
                                            const int32_t* kf_items, int32_t kf_nodes, const ovs_keypoint* frm_kps,
                                            const uint8_t* frm_desc, int32_t n_frm, const int32_t* frm_node_ids,
                                            const int32_t* frm_node_start, const int32_t* frm_items, int32_t frm_nodes, float lowe_ratio,
                                            int32_t check_orientation, int32_t* matched_kf_in_frm, int32_t* num_matches) {
    return bow_match_impl(w, nullptr, nullptr, 0, nullptr, nullptr, kf_kps, kf_desc, kf_valid, n_kf, kf_node_ids, kf_node_start, kf_items, kf_nodes, frm_kps, frm_desc, n_frm,
                          frm_node_ids, frm_node_start, frm_items, frm_nodes, lowe_ratio, check_orientation, matched_kf_in_frm, num_matches);
}
ovs_status ovs_bow_match_frame_and_keyframe_f(ovs_wmatcher* w, const ovs_frame_dev* keyfrm, const uint8_t* kf_valid, const int32_t* kf_node_ids,
                                              const int32_t* kf_node_start, const int32_t* kf_items, int32_t kf_nodes, const ovs_frame_dev* frm,
                                              const int32_t* frm_node_ids, const int32_t* frm_node_start, const int32_t* frm_items, int32_t frm_nodes,
                                              float lowe_ratio, int32_t check_orientation, int32_t* matched_kf_in_frm, int32_t* num_matches) {
    if (!keyfrm || !frm) return OVS_ERR_INVALID;
    return bow_match_impl(w, keyfrm, frm, 0, nullptr, nullptr, nullptr, nullptr, kf_valid, keyfrm->n, kf_node_ids, kf_node_start, kf_items, kf_nodes, nullptr, nullptr,
                          frm->n, frm_node_ids, frm_node_start, frm_items, frm_nodes, lowe_ratio, check_orientation, matched_kf_in_frm, num_matches);
}

ovs_status ovs_bow_match_keyframes(ovs_wmatcher* w, const ovs_keypoint* kps_1, const uint8_t* desc_1, const uint8_t* valid_1, int32_t n1,
                                   const int32_t* node_ids_1, const int32_t* node_start_1, const int32_t* items_1, int32_t nodes_1,
                                   const ovs_keypoint* kps_2, const uint8_t* desc_2, const uint8_t* valid_2, int32_t n2,
                                   const int32_t* node_ids_2, const int32_t* node_start_2, const int32_t* items_2, int32_t nodes_2,
                                   float lowe_ratio, int32_t check_orientation, int32_t* matched_2_in_1, int32_t* num_matches) {
    return bow_match_impl(w, nullptr, nullptr, 1, valid_2, nullptr, kps_1, desc_1, valid_1, n1, node_ids_1, node_start_1, items_1, nodes_1, kps_2, desc_2, n2, node_ids_2,
                          node_start_2, items_2, nodes_2, lowe_ratio, check_orientation, matched_2_in_1, num_matches);
}
ovs_status ovs_bow_match_keyframes_f(ovs_wmatcher* w, const ovs_frame_dev* keyfrm_1, const uint8_t* valid_1, const int32_t* node_ids_1,
                                     const int32_t* node_start_1, const int32_t* items_1, int32_t nodes_1, const ovs_frame_dev* keyfrm_2,
                                     const uint8_t* valid_2, const int32_t* node_ids_2, const int32_t* node_start_2, const int32_t* items_2, int32_t nodes_2,
                                     float lowe_ratio, int32_t check_orientation, int32_t* matched_2_in_1, int32_t* num_matches) {
    if (!keyfrm_1 || !keyfrm_2) return OVS_ERR_INVALID;
    return bow_match_impl(w, keyfrm_1, keyfrm_2, 1, valid_2, nullptr, nullptr, nullptr, valid_1, keyfrm_1->n, node_ids_1, node_start_1, items_1, nodes_1, nullptr, nullptr,
                          keyfrm_2->n, node_ids_2, node_start_2, items_2, nodes_2, lowe_ratio, check_orientation, matched_2_in_1, num_matches);
}

ovs_status ovs_robust_match_for_triangulation(ovs_wmatcher* w, const ovs_keypoint* kps_1, const uint8_t* desc_1, const uint8_t* has_lm_1,
                                              const float* x_right_1, const double* bearings_1, int32_t n1, const int32_t* node_ids_1,
                                              const int32_t* node_start_1, const int32_t* items_1, int32_t nodes_1,
                                              const ovs_keypoint* kps_2, const uint8_t* desc_2, const uint8_t* has_lm_2,
                                              const float* x_right_2, const double* bearings_2, int32_t n2, const int32_t* node_ids_2,
                                              const int32_t* node_start_2, const int32_t* items_2, int32_t nodes_2, const double* E_12,
                                              const double* epipole_in_2, const float* scale_factors, int32_t num_levels,
                                              int32_t check_orientation, int32_t* matched_2_in_1, int32_t* num_matches) {
    if (!bearings_1 || !bearings_2 || !E_12 || !epipole_in_2 || !scale_factors || num_levels < 1 || num_levels > OVS_MAX_LEVELS || n1 < 0 || n2 < 0)
        return OVS_ERR_INVALID;
    const std::vector<uint8_t> v1 = no_landmark_mask(has_lm_1, n1), v2 = no_landmark_mask(has_lm_2, n2);
    TriParams tp{x_right_1, x_right_2, bearings_1, bearings_2, E_12, epipole_in_2, scale_factors, num_levels};
    return bow_match_impl(w, nullptr, nullptr, 1, v2.data(), &tp, kps_1, desc_1, v1.data(), n1, node_ids_1, node_start_1, items_1, nodes_1, kps_2, desc_2, n2,
                          node_ids_2, node_start_2, items_2, nodes_2, 0.0f, check_orientation, matched_2_in_1, num_matches);
}
ovs_status ovs_robust_match_for_triangulation_f(ovs_wmatcher* w, const ovs_frame_dev* keyfrm_1, const uint8_t* has_lm_1, const int32_t* node_ids_1,
                                                const int32_t* node_start_1, const int32_t* items_1, int32_t nodes_1, const ovs_frame_dev* keyfrm_2,
                                                const uint8_t* has_lm_2, const int32_t* node_ids_2, const int32_t* node_start_2, const int32_t* items_2,
                                                int32_t nodes_2, const double* E_12, const double* epipole_in_2, const float* scale_factors,
                                                int32_t num_levels, int32_t check_orientation, int32_t* matched_2_in_1, int32_t* num_matches) {
    if (!keyfrm_1 || !keyfrm_2 || !keyfrm_1->d_bearings || !keyfrm_2->d_bearings || !E_12 || !epipole_in_2 || !scale_factors || num_levels < 1 ||
        num_levels > OVS_MAX_LEVELS)
        return OVS_ERR_INVALID;
    const int n1 = keyfrm_1->n, n2 = keyfrm_2->n;
    const std::vector<uint8_t> v1 = no_landmark_mask(has_lm_1, n1), v2 = no_landmark_mask(has_lm_2, n2);
    TriParams tp{nullptr, nullptr, nullptr, nullptr, E_12, epipole_in_2, scale_factors, num_levels};
    return bow_match_impl(w, keyfrm_1, keyfrm_2, 1, v2.data(), &tp, nullptr, nullptr, v1.data(), n1, node_ids_1, node_start_1, items_1, nodes_1, nullptr, nullptr, n2,
                          node_ids_2, node_start_2, items_2, nodes_2, 0.0f, check_orientation, matched_2_in_1, num_matches);
}

ovs_status ovs_match_set_variant(int32_t which, int32_t value) {
    if (value != 0 && value != 1) return OVS_ERR_INVALID;
    switch (which) {
        case OVS_MATCH_VARIANT_ANGLE_KEEP_RULE: g_angle_keep_rule.store(value, std::memory_order_relaxed); return OVS_OK;
        case OVS_MATCH_VARIANT_ANGLE_TIE_ORDER: g_angle_tie_order.store(value, std::memory_order_relaxed); return OVS_OK;
        case OVS_MATCH_VARIANT_BF_FRAME_MASK: g_bf_frame_mask.store(value, std::memory_order_relaxed); return OVS_OK;
        default: return OVS_ERR_INVALID;
    }
}
int32_t ovs_match_get_variant(int32_t which) {
    switch (which) {
        case OVS_MATCH_VARIANT_ANGLE_KEEP_RULE: return g_angle_keep_rule.load(std::memory_order_relaxed);
        case OVS_MATCH_VARIANT_ANGLE_TIE_ORDER: return g_angle_tie_order.load(std::memory_order_relaxed);
        case OVS_MATCH_VARIANT_BF_FRAME_MASK: return g_bf_frame_mask.load(std::memory_order_relaxed);
        default: return -1;
    }
}

}   // extern "C"
