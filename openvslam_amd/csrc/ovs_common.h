// ovs_common.h -- internal declarations shared by the HIP translation units of libovslam_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <stdint.h>

#include "../../include/ovslam_hip.h"
#include "../../include/ovs_detmath.h"
#include "orb_geometry.h"   // the extractor's geometry records and kernel limits (HIP-free: shared with the host planner)

namespace ovs {

// Candidate entry (u64): [score:8 | y:13 | x:13 | node:16], score = FAST response (S-1), x/y = level-image coordinates.
__host__ __device__ inline uint64_t cand_pack(uint32_t x, uint32_t y, uint32_t score, uint32_t node) {
    return ((uint64_t)score << 42) | ((uint64_t)y << 29) | ((uint64_t)x << 16) | (uint64_t)node;
}
__host__ __device__ inline uint32_t cand_x(uint64_t c) { return (uint32_t)(c >> 16) & 0x1FFFu; }
__host__ __device__ inline uint32_t cand_y(uint64_t c) { return (uint32_t)(c >> 29) & 0x1FFFu; }
__host__ __device__ inline uint32_t cand_score(uint64_t c) { return (uint32_t)(c >> 42) & 0xFFu; }
__host__ __device__ inline uint32_t cand_node(uint64_t c) { return (uint32_t)c & 0xFFFFu; }
// Upstream's emission order of a candidate: cell row, cell column, then row-major inside the cell.
__host__ __device__ inline uint32_t cand_order(uint32_t x, uint32_t y, uint32_t ncx) {
    const uint32_t dx = x - kDetOrigin, dy = y - kDetOrigin;
    return (((dy >> 6) * ncx + (dx >> 6)) << 12) | ((dy & 63u) << 6) | (dx & 63u);
}

// Selected keypoint of a level before description (u64): [score:8 | y:13 | x:13].
struct DevBuffers {
    const FrameGeo* geo;          // device copy
    const ResizeTap* taps;        // device
    const CellDesc* cells;        // device, total_cells records
    uint8_t* pyr;                 // max_batch * pyr_frame_bytes (levels >= 1)
    size_t pyr_frame_bytes;
    uint64_t* cand;               // max_batch * cand_frame_entries
    size_t cand_frame_entries;
    uint32_t* cand_count;         // max_batch * num_levels
    uint32_t* nodes;              // max_batch * node_frame_entries * 4 u32 (two ping-pong lists inside)
    size_t node_frame_entries;
    uint64_t* lvl_kps;            // max_batch * total_kp_cap
    uint32_t* lvl_count;          // max_batch * num_levels
};

// ---- kernel launchers (each defined next to its kernel) ----
hipError_t launch_pyramid_chain(const uint8_t* img0, size_t frame_stride0, int pitch0, uint8_t* pyr, size_t pyr_frame_bytes, const FrameGeo* d_geo,
                                const ResizeTap* d_taps, const ChainSpan* d_plan, int TX, int TY, int bufA_bytes, int bufB_bytes, int tap_cap,
                                int batch, hipStream_t s);
hipError_t launch_resize_pair(const uint8_t* src, size_t src_frame_stride, int src_pitch, uint8_t* dst1, int pitch1, int rows1, int cols1,
                              uint8_t* dst2, int pitch2, int rows2, int cols2, size_t dst_frame_stride, const ResizeTap* yt1, const ResizeTap* yt2,
                              const HTapRec* ht1, const HTapRec* ht2, const PairSpan* plan, int batch, hipStream_t s);
bool resize_pair_launchable(const uint8_t* src, size_t src_frame_stride, int src_pitch, int rows2, int cols2, int batch);
hipError_t launch_resize(const uint8_t* src, size_t src_frame_stride, int src_pitch, int srows, int scols, uint8_t* dst,
                         size_t dst_frame_stride, int dst_pitch, int drows, int dcols, const ResizeTap* xt, const ResizeTap* yt,
                         int batch, hipStream_t s, int hwin_ok);
hipError_t launch_fast(const FrameGeo& hgeo, const DevBuffers& d, const uint8_t* img0, size_t stride0, size_t frame_stride0,
                       const uint8_t* mask, int mask_rows, int batch, hipStream_t s, int cell_lo = 0, int n_cells = -1);
hipError_t launch_tree(const FrameGeo& hgeo, const DevBuffers& d, int batch, hipStream_t s, int level_lo = 0, int n_levels = -1);
size_t tree_lds_bytes_for(const FrameGeo& hgeo);
constexpr size_t kMaxLdsPerWorkgroup = 160 * 1024;
hipError_t launch_describe(const FrameGeo& hgeo, const DevBuffers& d, const uint8_t* img0, size_t stride0, size_t frame_stride0,
                           ovs_keypoint* kps, uint8_t* desc, int32_t* counts, int cap, int batch, hipStream_t s, ovs_keypoint* kps_m = nullptr, uint8_t* desc_m = nullptr,
                           int32_t* counts_m = nullptr);

// Environment switches of the launchers. Read from the environment ONCE per process, all in tuning() (first use; thread-safe static
// initialisation) -- the launch paths never call getenv, which is not safe against a host application's concurrent setenv. Unset, every switch
// is the production setting.
constexpr int kMaxTuningDevices = 16;
struct Tuning {
    // -- test hooks: force, at a small size, a path that production selects from the input
    int tree_grid;         // OVS_TREE_GRID: unset = by launch (grid form for batches, sweep form for one frame), 0 = the sweep form only, d > 0 = the
                           //   grid form everywhere with its finest grid at depth min(d, 7) (small d: the in-launch overflow fallback)
    bool chol_resident;    // OVS_CHOL_RESIDENT=0: systems up to 288 unknowns take k_chol_solve (tiles through memory; production above 288)
    bool ba_schur_lists;   // OVS_BA_SCHUR_LISTS=0: every trial's k_schur scans for the pairs' common landmarks itself (production above the pair-list bound)
    int pose_batch_retries;// OVS_POSE_BATCH_RETRIES: the retries 1 .. 9 of an iteration in one pass -- 1 always, 0 never, unset (-1): by work per thread
    bool pose_obs_regs;    // OVS_POSE_OBS_REGS=0: observations re-read from memory in every pass (the form for frames too large for registers)
    bool pose_zero_copy;   // OVS_POSE_ZERO_COPY=0: the pose optimiser's inputs and outputs through copies (the form for frames too large for registers)
    // -- deployment
    bool ba_ll_notify;     // OVS_BA_LL_NOTIFY=0: a local-BA trial's outcome through a D2H copy and a stream synchronisation, not polled from pinned words
    // -- diagnostics and tuning probes
    bool ba_trace;         // OVS_BA_TRACE: per-iteration trace of the LM loops on stderr
    bool fast_timing;      // OVS_FAST_TIMING: per-phase cycle counts of k_fast_cells, printed per launch
    int fast_cells;        // OVS_FAST_CELLS: consecutive cells per FAST workgroup (0 = by launch size)
    int fast_pad_lds;      // OVS_FAST_PAD_LDS: extra dynamic LDS per k_fast_cells workgroup (occupancy probe)
    int pose_threads;      // OVS_POSE_THREADS: 256 / 512 (0 = by problem size)
    int pose_groups;       // OVS_POSE_GROUPS: workgroups a single frame's pose optimisation is spread over (0 = by observation count, 1 = one)
    int resolve_wide_from; // OVS_RESOLVE_WIDE_FROM: queries from which a resolver round takes 512 of them
    int pyr_strip;         // OVS_PYR_STRIP: vertically consecutive tiles per k_resize_pair_u8 workgroup (0 = by launch size, 1 = one tile per workgroup)
    int pyr_chain;         // OVS_PYR_CHAIN: frames per launch up to which the pyramid is ONE k_pyramid_chain launch (default 2: measured 24 vs 37 us for one frame, 33.5 vs 35.7 for two, 73 vs 46 for eight; 0 = never)
};
const Tuning& tuning();

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE: remember the largest size set for one kernel on every device
struct LdsAttrCache {
    std::atomic<size_t> set[kMaxTuningDevices] = {};
    std::mutex mu;   // hipFuncSetAttribute is last-writer-wins: two threads' first launches with different sizes must not leave the smaller one set
};
inline hipError_t ensure_dynamic_lds(const void* fn, size_t bytes, LdsAttrCache& c) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool cached = dev >= 0 && dev < kMaxTuningDevices;
    if (cached && bytes <= c.set[dev].load(std::memory_order_acquire)) return hipSuccess;   // fast path: no lock once the size is covered
    std::lock_guard<std::mutex> lock(c.mu);
    if (cached && bytes <= c.set[dev].load(std::memory_order_acquire)) return hipSuccess;   // another thread set at least this much meanwhile
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && cached) c.set[dev].store(bytes, std::memory_order_release);       // under the lock the attribute only ever grows
    return e;
}

void set_last_error(const char* what, hipError_t e);
// ovs_debug_inject_hip_failures(skip, n): after `skip` further OVS_HIP_TRY-checked calls, the next n of them (the calls themselves
// still run) report hipErrorLaunchFailure. One relaxed atomic load per checked HIP call when nothing is armed.
extern std::atomic<int32_t> g_injected_hip_failures, g_injected_hip_skip;
inline hipError_t fault_filter(hipError_t e) {
    if (g_injected_hip_failures.load(std::memory_order_relaxed) > 0) {
        if (g_injected_hip_skip.load(std::memory_order_relaxed) > 0 && g_injected_hip_skip.fetch_sub(1, std::memory_order_relaxed) > 0) return e;
        if (g_injected_hip_failures.fetch_sub(1, std::memory_order_relaxed) > 0) return hipErrorLaunchFailure;
    }
    return e;
}
void set_last_error_text(const std::string& what);   // failures that are not HIP errors (a refused file, an exception stopped at the ABI)

// Device view of one frame's image pyramid (feature::orb_extractor::image_pyramid_) of an extractor's LAST extract.
struct PyrView {
    const uint8_t* base[OVS_MAX_LEVELS];
    int32_t pitch[OVS_MAX_LEVELS];
    int32_t rows[OVS_MAX_LEVELS], cols[OVS_MAX_LEVELS];
    float scale[OVS_MAX_LEVELS], inv_scale[OVS_MAX_LEVELS];
    int32_t num_levels;
};
// false if the handle has not extracted yet or `frame` is outside its last batch
bool orb_pyramid_view(const ovs_orb* h, int frame, PyrView* out);
int orb_device(const ovs_orb* h);
hipStream_t orb_last_stream(const ovs_orb* h);   // the stream the handle's last extract was enqueued on
// true iff (kps, desc, n) equal what the handle's last HOST-form extract returned; then *d_kps / *d_desc are the device copies still resident
bool orb_host_outputs_equal(const ovs_orb* h, const ovs_keypoint* kps, const uint8_t* desc, int32_t n, const ovs_keypoint** d_kps, const uint8_t** d_desc);

// Stage timer for bench.py: HIP events recorded on the launch stream at stage boundaries; a small ring of call slots.
template <int NSTAGE>
struct StageProfiler {
    static constexpr int kSlots = 64;
    bool enabled = false;
    hipEvent_t ev[kSlots][NSTAGE + 1] = {};
    bool created = false;
    int head = 0, pending = 0;      // slots [head-pending, head) hold un-read calls
    double acc_ms[NSTAGE] = {};
    int acc_calls = 0;
    int cur = -1;

    hipError_t ensure() {
        if (created) return hipSuccess;
        for (int i = 0; i < kSlots; ++i)
            for (int j = 0; j <= NSTAGE; ++j) {
                hipError_t e = hipEventCreate(&ev[i][j]);
                if (e != hipSuccess) return e;
            }
        created = true;
        return hipSuccess;
    }
    hipError_t drain_one() {
        const int slot = ((head - pending) % kSlots + kSlots) % kSlots;
        hipError_t e = hipEventSynchronize(ev[slot][NSTAGE]);
        if (e != hipSuccess) return e;
        for (int j = 0; j < NSTAGE; ++j) {
            float ms = 0;
            e = hipEventElapsedTime(&ms, ev[slot][j], ev[slot][j + 1]);
            if (e != hipSuccess) return e;
            acc_ms[j] += ms;
        }
        ++acc_calls;
        --pending;
        return hipSuccess;
    }
    // begin a call: returns the slot to record into (-1 when disabled)
    hipError_t begin(hipStream_t s) {
        cur = -1;
        if (!enabled) return hipSuccess;
        hipError_t e = ensure();
        if (e != hipSuccess) return e;
        if (pending == kSlots) {
            e = drain_one();
            if (e != hipSuccess) return e;
        }
        cur = head % kSlots;
        head = (head + 1) % kSlots;
        ++pending;
        return hipEventRecord(ev[cur][0], s);
    }
    hipError_t mark(int stage_done, hipStream_t s) {   // stage_done in 1..NSTAGE
        if (cur < 0) return hipSuccess;
        return hipEventRecord(ev[cur][stage_done], s);
    }
    hipError_t read(float* ms, int32_t* ncalls) {
        while (pending > 0) {
            hipError_t e = drain_one();
            if (e != hipSuccess) return e;
        }
        for (int j = 0; j < NSTAGE; ++j) {
            ms[j] = (float)acc_ms[j];
            acc_ms[j] = 0;
        }
        *ncalls = acc_calls;
        acc_calls = 0;
        return hipSuccess;
    }
    void destroy() {
        if (!created) return;
        for (int i = 0; i < kSlots; ++i)
            for (int j = 0; j <= NSTAGE; ++j) (void)hipEventDestroy(ev[i][j]);
        created = false;
    }
};

// 1 / sqrt(p) by v_rsq_f64 + three Newton steps (enough from an 11-bit seed); sqrt(p) = p * that. A Cholesky pivot then costs ~15 dependent
// operations instead of the ~45 of an IEEE sqrt followed by an IEEE division (results differ from those by an ulp or two): the pivots are
// the one chain of a factorisation nothing can overlap (ba_solve.hip: 6 n_free of them; pose_opt.hip: 6 per LM trial on one lane).
#ifdef __HIPCC__
__device__ __forceinline__ double rsqrt_newton(double p) {
    double y = __builtin_amdgcn_rsq(p);
    const double h = 0.5 * p;
#pragma unroll
    for (int i = 0; i < 3; ++i) y = y * __builtin_fma(-h * y, y, 1.5);
    return y;
}
#endif

}   // namespace ovs

#define OVS_HIP_TRY(expr)                                  \
    do {                                                   \
        hipError_t _e = ovs::fault_filter(expr);           \
        if (_e != hipSuccess) {                            \
            ovs::set_last_error(#expr, _e);                \
            return OVS_ERR_HIP;                            \
        }                                                  \
    } while (0)
