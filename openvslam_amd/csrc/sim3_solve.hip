// sim3_solve.hip -- solve::sim3_solver (expected: src/openvslam/solve/sim3_solver.{h,cc}): find_via_ransac over a batch of loop candidates
// (loop_detector runs it once per candidate between bow_tree::match_keyframes and projection::match_by_Sim3_transform). Rules: DESIGN.md 3.9.
//
// A problem is one (keyframe 1, keyframe 2) pair with n matches: p1 / p2 (the landmark in camera-1 / camera-2 coordinates), thr1 / thr2 and a
// camera per side. Everything is f64, every operation rounded on its own (the unit is built with -ffp-contract=off).
//
// k_sim3_hypotheses: grid (blocks of kHypPerWave hypotheses, problems), one wavefront per workgroup. Lane l < kHypPerWave solves hypothesis
// h = block * kHypPerWave + l in registers: the counter-based sampler, Horn's closed form with the 4 x 4 cyclic Jacobi unrolled on
// compile-time indices (no local array is indexed dynamically: no scratch), and leaves the model's 17 distinct doubles (R12, t12, s12, s21,
// t21; R21 is R12 read by columns) in LDS. The wave then walks its models with the lanes over the matches: the two observations u1, u2 of a
// round of 64 matches are projected once and kept in registers, every model is a broadcast LDS read, the inlier count of a (model, round)
// is ballot + popcount -- a wave-uniform integer -- and lane m keeps model m's total. A hypothesis's key is (count << 32) | (0xFFFFFFFF - h):
// the largest count wins, the lowest h on a tie. The wave takes the maximum of its keys by shuffles, the lane that holds it copies its
// model to the wave's record in memory (136 bytes per wave) and publishes the key with ONE integer atomicMax, in whatever order the waves
// finish. No floating-point atomics, no waiting between workgroups.
// k_sim3_finish: one workgroup per problem; the winner is its wave's best, so its model is read back from that wave's record -- the doubles the
// hypothesis kernel counted with, not a recomputation (the closed form is a 20 us chain of dependent f64 operations: DESIGN.md 3.9). The
// threads write the flags of their matches with the same inlier function, thread 0 the model, into the page-locked result block.
#include <cmath>
#include <cstring>

#include "ovs_common.h"
#include "solve_internal.inc"

namespace {

constexpr int kHypPerWave = 4;      // hypotheses per wavefront (measured against 8, 16, 32 and 64)
constexpr int kModelDoubles = 17;   // R12 9, t12 3, s12, s21, t21 3
constexpr int kFinishThreads = 256;

// the staged block of one call and one side's camera in it: solve_plan.inc
using splan::sim3::CamRec;
using splan::sim3::Layout;
using splan::sim3::layout_of;

struct Model {
    double R[9], t12[3], s12, s21, t21[3];
};

// rule 2: Horn's closed form on the three sampled matches of hypothesis h
__device__ __forceinline__ Model solve_hypothesis(const double* __restrict__ p1, const double* __restrict__ p2, uint32_t n, uint64_t seed, uint32_t p,
                                                  uint32_t h, bool fix_scale) {
    uint32_t idx[3];
    sample_distinct<3, 4>(seed, p, h, n, idx);   // rule 1
    double a[3][3], b[3][3];   // [k][axis]
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            a[k][x] = p1[3 * (size_t)idx[k] + x];
            b[k][x] = p2[3 * (size_t)idx[k] + x];
        }
    double c1[3], c2[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        c1[x] = ((a[0][x] + a[1][x]) + a[2][x]) / 3.0;
        c2[x] = ((b[0][x] + b[1][x]) + b[2][x]) / 3.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            a[k][x] = a[k][x] - c1[x];
            b[k][x] = b[k][x] - c2[x];
        }
    double M[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = (b[0][r] * a[0][c] + b[1][r] * a[1][c]) + b[2][r] * a[2][c];
    Model m;
    horn_rotation(M, m.R);
    if (fix_scale) {
        m.s12 = 1.0;
    } else {
        double num[3], den[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double r0 = dot3(m.R[0], m.R[1], m.R[2], b[k][0], b[k][1], b[k][2]);
            const double r1 = dot3(m.R[3], m.R[4], m.R[5], b[k][0], b[k][1], b[k][2]);
            const double r2 = dot3(m.R[6], m.R[7], m.R[8], b[k][0], b[k][1], b[k][2]);
            num[k] = dot3(a[k][0], a[k][1], a[k][2], r0, r1, r2);
            den[k] = dot3(r0, r1, r2, r0, r1, r2);
        }
        m.s12 = ((num[0] + num[1]) + num[2]) / ((den[0] + den[1]) + den[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) m.t12[r] = c1[r] - m.s12 * dot3(m.R[3 * r], m.R[3 * r + 1], m.R[3 * r + 2], c2[0], c2[1], c2[2]);
    m.s21 = 1.0 / m.s12;
#pragma unroll
    for (int r = 0; r < 3; ++r) m.t21[r] = -m.s21 * dot3(m.R[r], m.R[3 + r], m.R[6 + r], m.t12[0], m.t12[1], m.t12[2]);
    return m;
}

// rule 3's projections
__device__ __forceinline__ void project(const CamRec& cam, double x, double y, double z, double& u, double& v) {
    if (cam.model == 0) {
        u = cam.a * x / z + cam.c;
        v = cam.b * y / z + cam.d;
    } else {
        const double kPi = 3.14159265358979323846;
        const double L = sqrt((x * x + y * y) + z * z);
        const double theta = ovs_det_atan2(x, z);
        const double phi = -ovs_det_asin(y / L);
        u = cam.a * (0.5 + theta / (2.0 * kPi));
        v = cam.b * (0.5 - phi / kPi);
    }
}

// one match as the inlier test reads it: the two points, their own projections and the two thresholds widened to f64
struct Match {
    double p1[3], p2[3], u1x, u1y, u2x, u2y, thr1, thr2;
};
__device__ __forceinline__ Match load_match(const CamRec& cam1, const CamRec& cam2, const double* __restrict__ p1, const double* __restrict__ p2,
                                            const float* __restrict__ thr1, const float* __restrict__ thr2, size_t i) {
    Match m;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        m.p1[x] = p1[3 * i + x];
        m.p2[x] = p2[3 * i + x];
    }
    m.thr1 = (double)thr1[i];
    m.thr2 = (double)thr2[i];
    project(cam1, m.p1[0], m.p1[1], m.p1[2], m.u1x, m.u1y);
    project(cam2, m.p2[0], m.p2[1], m.p2[2], m.u2x, m.u2y);
    return m;
}

// rule 3: a NaN anywhere leaves every comparison false
__device__ __forceinline__ bool is_inlier(const CamRec& cam1, const CamRec& cam2, const Match& m, const double* R, const double* t12, double s12,
                                          double s21, const double* t21) {
    const double x1 = s12 * dot3(R[0], R[1], R[2], m.p2[0], m.p2[1], m.p2[2]) + t12[0];
    const double y1 = s12 * dot3(R[3], R[4], R[5], m.p2[0], m.p2[1], m.p2[2]) + t12[1];
    const double z1 = s12 * dot3(R[6], R[7], R[8], m.p2[0], m.p2[1], m.p2[2]) + t12[2];
    const double x2 = s21 * dot3(R[0], R[3], R[6], m.p1[0], m.p1[1], m.p1[2]) + t21[0];
    const double y2 = s21 * dot3(R[1], R[4], R[7], m.p1[0], m.p1[1], m.p1[2]) + t21[1];
    const double z2 = s21 * dot3(R[2], R[5], R[8], m.p1[0], m.p1[1], m.p1[2]) + t21[2];
    double v1x, v1y, v2x, v2y;
    project(cam1, x1, y1, z1, v1x, v1y);
    project(cam2, x2, y2, z2, v2x, v2y);
    const double d1x = m.u1x - v1x, d1y = m.u1y - v1y, d2x = m.u2x - v2x, d2y = m.u2y - v2y;
    const double e1 = d1x * d1x + d1y * d1y, e2 = d2x * d2x + d2y * d2y;
    bool ok = e1 < m.thr1 && e2 < m.thr2;
    if (cam1.model == 0) ok = ok && m.p1[2] > 0.0 && z1 > 0.0;
    if (cam2.model == 0) ok = ok && m.p2[2] > 0.0 && z2 > 0.0;
    return ok;
}

__global__ __launch_bounds__(64) void k_sim3_hypotheses(uint8_t* __restrict__ block, int P, int T, int fix_scale, int max_iter, uint64_t seed,
                                                        double* __restrict__ wave_models) {
    __shared__ double models[kHypPerWave * kModelDoubles];
    const Layout lay = layout_of(P, T);
    const int p = blockIdx.y;
    const auto [off, n] = problem_span(block, lay.offsets, p);
    if (n < 3) return;   // rule 4: invalid, k_sim3_finish says so
    const CamRec cam1 = reinterpret_cast<const CamRec*>(block + lay.cams)[2 * p], cam2 = reinterpret_cast<const CamRec*>(block + lay.cams)[2 * p + 1];
    const double* p1 = reinterpret_cast<const double*>(block + lay.p1) + 3 * (size_t)off;
    const double* p2 = reinterpret_cast<const double*>(block + lay.p2) + 3 * (size_t)off;
    const float* thr1 = reinterpret_cast<const float*>(block + lay.thr1) + off;
    const float* thr2 = reinterpret_cast<const float*>(block + lay.thr2) + off;
    const int lane = threadIdx.x;
    const int h0 = blockIdx.x * kHypPerWave;
    const int nh = min(kHypPerWave, max_iter - h0);   // >= 1 by the grid's size
    if (lane < nh) {
        const Model m = solve_hypothesis(p1, p2, (uint32_t)n, seed, (uint32_t)p, (uint32_t)(h0 + lane), fix_scale != 0);
        double* dst = models + lane * kModelDoubles;
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[k] = m.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dst[9 + k] = m.t12[k];
            dst[14 + k] = m.t21[k];
        }
        dst[12] = m.s12;
        dst[13] = m.s21;
    }
    __syncthreads();
    int count = 0;   // lane m: the inliers of model m
    for (int base = 0; base < n; base += 64) {
        const bool have = base + lane < n;
        const Match mt = load_match(cam1, cam2, p1, p2, thr1, thr2, (size_t)(have ? base + lane : 0));
        for (int m = 0; m < nh; ++m) {
            const double* md = models + m * kModelDoubles;   // the same address in every lane: a broadcast read
            const bool inl = have && is_inlier(cam1, cam2, mt, md, md + 9, md[12], md[13], md + 14);
            const int c = __popcll(__ballot(inl));
            if (lane == m) count += c;
        }
    }
    const unsigned long long key = lane < nh ? hypothesis_key(count, (uint32_t)(h0 + lane)) : 0ull;
    unsigned long long best = key;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const unsigned long long other = __shfl_xor(best, d);
        best = other > best ? other : best;
    }
    if (key == best) {   // one lane: the keys of a wave differ in h
        double* dst = wave_models + ((size_t)p * gridDim.x + blockIdx.x) * kModelDoubles;
        const double* src = models + lane * kModelDoubles;
#pragma unroll
        for (int k = 0; k < kModelDoubles; ++k) dst[k] = src[k];
        atomicMax(reinterpret_cast<unsigned long long*>(block + lay.keys) + p, key);
    }
}

__global__ __launch_bounds__(kFinishThreads) void k_sim3_finish(const uint8_t* __restrict__ block, int P, int T, int min_inliers, int waves_per_problem,
                                                                const double* __restrict__ wave_models, ResultRec* __restrict__ out,
                                                                uint8_t* __restrict__ out_flags) {
    const Layout lay = layout_of(P, T);
    const int p = blockIdx.x;
    const auto [off, n] = problem_span(block, lay.offsets, p);
    const unsigned long long key = reinterpret_cast<const unsigned long long*>(block + lay.keys)[p];
    const int count = key_count(key);
    const uint32_t h = key_iter(key);
    const bool valid = n >= 3 && n >= min_inliers && count >= min_inliers;   // rule 4 (n < 3: the key is still zero and never read)
    if (!valid) {
        write_invalid(out_flags + off, n, kFinishThreads, out + p);
        return;
    }
    const CamRec cam1 = reinterpret_cast<const CamRec*>(block + lay.cams)[2 * p], cam2 = reinterpret_cast<const CamRec*>(block + lay.cams)[2 * p + 1];
    const double* p1 = reinterpret_cast<const double*>(block + lay.p1) + 3 * (size_t)off;
    const double* p2 = reinterpret_cast<const double*>(block + lay.p2) + 3 * (size_t)off;
    const float* thr1 = reinterpret_cast<const float*>(block + lay.thr1) + off;
    const float* thr2 = reinterpret_cast<const float*>(block + lay.thr2) + off;
    const double* md = wave_models + ((size_t)p * waves_per_problem + h / kHypPerWave) * kModelDoubles;   // the winner is its wave's best
    double m[kModelDoubles];
#pragma unroll
    for (int k = 0; k < kModelDoubles; ++k) m[k] = md[k];
    for (int i = threadIdx.x; i < n; i += kFinishThreads) {
        const Match mt = load_match(cam1, cam2, p1, p2, thr1, thr2, (size_t)i);
        out_flags[off + i] = is_inlier(cam1, cam2, mt, m, m + 9, m[12], m[13], m + 14) ? 1 : 0;
    }
    if (threadIdx.x == 0) {
        ResultRec r;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.rot[k] = m[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) r.trans[k] = m[9 + k];
        r.scale = m[12];
        r.valid = 1;
        r.best_iter = (int32_t)h;
        r.num_inliers = count;
        r.pad = 0;
        out[p] = r;
    }
}

}   // namespace

struct ovs_sim3 : batch_handle {};

extern "C" {

ovs_status ovs_sim3_create(int32_t device, int32_t max_problems, int32_t max_total_matches, ovs_sim3** out) {
    return batch_create(device, max_problems, max_total_matches, layout_of(max_problems, max_total_matches).bytes,
                        (size_t)max_problems * (256 / kHypPerWave),   // 256 iterations per problem without growing
                        kModelDoubles, sizeof(ResultRec), out, no_extra);
}

ovs_status ovs_sim3_destroy(ovs_sim3* s) { return batch_destroy(s); }

ovs_status ovs_sim3_solve_batch(ovs_sim3* s, int32_t n_problems, const int32_t* offsets, const double* p1, const double* p2, const float* thr1,
                                const float* thr2, const ovs_camera* cams_1, const ovs_camera* cams_2, int32_t fix_scale, int32_t min_num_inliers,
                                int32_t max_num_iter, uint64_t seed, int32_t* out_valid, int32_t* out_best_iter, int32_t* out_num_inliers,
                                double* out_rot_12, double* out_trans_12, double* out_scale_12, uint8_t* out_inlier_flags) {
    const splan::sim3::Call call{s != nullptr, n_problems, offsets, p1, p2, thr1, thr2, cams_1, cams_2, min_num_inliers, max_num_iter, out_valid,
                                 out_best_iter, out_num_inliers, out_rot_12, out_trans_12, out_scale_12, out_inlier_flags};
    const splan::Checked checked = splan::sim3::check(call, caps_of(s));
    const Layout lay = layout_of(n_problems, checked.T);
    const auto hypotheses = [&](hipStream_t st, int blocks, int32_t T) {
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3(blocks, n_problems), dim3(64), 0, st, s->d_block, n_problems, T, fix_scale ? 1 : 0, max_num_iter, seed,
                           s->d_records);
    };
    const auto finish = [&](hipStream_t st, int blocks, int32_t T) {
        hipLaunchKernelGGL(k_sim3_finish, dim3(n_problems), dim3(kFinishThreads), 0, st, s->d_block, n_problems, T, min_num_inliers, blocks, s->d_records,
                           s->m_rec<ResultRec>(), s->m_flags);
    };
    return run_batch(s, checked, lay.bytes, n_problems, max_num_iter, kHypPerWave,
                     {out_valid, out_best_iter, out_num_inliers, out_rot_12, out_trans_12, out_scale_12, out_inlier_flags},
                     [&] { splan::sim3::stage(call, lay, s->h_block); }, hypotheses, finish);
}

}   // extern "C"
