// orb_api.hip -- host side of the ORB extractor behind the C ABI (include/ovslam_hip.h): buffer ownership, upload of the geometry plan
// (orb_plan.inc: orb_params tables, level geometry, cv::resize coefficient tables, the pyramid kernels' regions), launch sequence. Replaces
// the body of feature::orb_extractor (expected: src/openvslam/feature/orb_extractor.{h,cc}, orb_params.{h,cc}).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "ovs_common.h"
#include "orb_plan.inc"
#include "owned_internal.inc"
#include "image_prep_internal.inc"

namespace ovs {

static thread_local std::string g_last_error;
void set_last_error(const char* what, hipError_t e) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
}
void set_last_error_text(const std::string& what) { g_last_error = what; }
std::atomic<int32_t> g_injected_hip_failures{0}, g_injected_hip_skip{0};

const Tuning& tuning() {
    static const Tuning t = [] {
        auto num = [](const char* name, int dflt) {
            const char* e = std::getenv(name);
            return e && e[0] ? std::atoi(e) : dflt;
        };
        auto zero = [](const char* name) {   // a "=0" switch: true only when the value starts with '0'
            const char* e = std::getenv(name);
            return e && e[0] == '0';
        };
        Tuning v;
        const char* tree_grid = std::getenv("OVS_TREE_GRID");
        v.tree_grid = tree_grid ? std::atoi(tree_grid) : -1;
        v.chol_resident = num("OVS_CHOL_RESIDENT", 1) != 0;
        v.ba_schur_lists = !zero("OVS_BA_SCHUR_LISTS");
        const char* retries = std::getenv("OVS_POSE_BATCH_RETRIES");
        v.pose_batch_retries = retries && retries[0] ? (std::atoi(retries) != 0 ? 1 : 0) : -1;
        v.pose_obs_regs = !zero("OVS_POSE_OBS_REGS");
        v.pose_zero_copy = !zero("OVS_POSE_ZERO_COPY");
        v.ba_ll_notify = !zero("OVS_BA_LL_NOTIFY");
        v.ba_trace = std::getenv("OVS_BA_TRACE") != nullptr;
        v.fast_timing = std::getenv("OVS_FAST_TIMING") != nullptr;
        v.fast_cells = std::max(0, num("OVS_FAST_CELLS", 0));
        v.fast_pad_lds = std::max(0, num("OVS_FAST_PAD_LDS", 0));
        v.pose_threads = num("OVS_POSE_THREADS", 0);
        v.pose_groups = std::max(0, num("OVS_POSE_GROUPS", 0));
        v.resolve_wide_from = num("OVS_RESOLVE_WIDE_FROM", 1024);
        v.pyr_strip = std::max(0, num("OVS_PYR_STRIP", 0));
        v.pyr_chain = std::max(0, num("OVS_PYR_CHAIN", 2));
        return v;
    }();
    return t;
}

}   // namespace ovs

using namespace ovs;

struct ovs_orb {
    ovs_orb_params p;
    int device = 0;
    int max_rows = 0, max_cols = 0, max_batch = 0;
    Owned res;   // every stream, event, device and pinned block below, the lazily allocated ones included
    hipStream_t stream = nullptr;
    // the A0 tables (plan.tab, from creation on) and the plan of the current image size (cur_rows x cur_cols; 0 x 0: none, the device copy is stale)
    int cur_rows = 0, cur_cols = 0;
    OrbPlan plan;
    // device memory: the plan's copies, allocated for the largest geometry
    FrameGeo* d_geo = nullptr;
    ResizeTap* d_taps = nullptr;
    size_t taps_cap = 0;
    CellDesc* d_cells = nullptr;
    size_t cells_cap = 0;
    ChainSpan* d_chain = nullptr;    // plan.chain.spans
    size_t chain_cap = 0;
    PairSpan* d_pair = nullptr;      // plan.pair_spans
    size_t pair_cap = 0;
    HTapRec* d_htaps = nullptr;      // plan.htaps
    size_t htaps_cap = 0;
    int32_t variant = 0;   // FrameGeo::variant
    DevBuffers d{};
    size_t pyr_cap = 0, cand_cap = 0, node_cap = 0, kps_cap = 0;
    // host-API staging: two slots (double buffering). A slot owns a device image (+ mask), a pinned input staging buffer, a pinned
    // output block [counts 16 B | keypoints | descriptors] and, on demand, a pinned copy of the pyramid block. H2D copies run on
    // copy_stream, kernels and the D2H of the results on `stream`: the upload of frame k+1 overlaps the kernels of frame k.
    struct HostSlot {
        uint8_t* d_img = nullptr;
        uint8_t* d_mask = nullptr;
        uint8_t* h_in = nullptr;     // pinned, img_pitch x max_rows
        uint8_t* h_mask = nullptr;   // pinned, lazily
        uint8_t* h_out = nullptr;    // pinned
        uint8_t* h_pyr = nullptr;    // pinned, lazily (ovs_orb_set_host_pyramid)
        hipEvent_t ev_h2d = nullptr, ev_done = nullptr;
        hipEvent_t t[4] = {};        // profiling: h2d begin / h2d end / kernels end / d2h end
        bool pending = false, has_pyr = false, timed = false;
        int rows = 0, cols = 0;
    };
    HostSlot slot[2];
    // ovs_orb_extract_pair (stereo left / right in one call): two device images (+ masks), one output block for both frames, allocated on
    // first use
    struct PairBuf {
        uint8_t *d_img = nullptr, *d_mask = nullptr, *d_out = nullptr, *h_out = nullptr;
        size_t frame_bytes = 0, off_kps = 0, off_desc = 0, out_bytes = 0;
        int cap = 0;
        hipEvent_t ev_h2d = nullptr;
    } pair;
    hipStream_t copy_stream = nullptr;
    unsigned n_submitted = 0, n_collected = 0;
    int last_slot = -1;              // slot of the last COLLECTED frame (host pyramid getter)
    bool host_pyr = false;
    int host_mode = 0;               // 0: hipMemcpy2DAsync straight from the caller's (pageable) rows (measured 0.054 ms per 1080p frame);
                                     // 1: banded copy through pinned staging (0.12 ms: the CPU memcpy costs more than the runtime's own staging)
    float host_ms[3] = {0, 0, 0};    // h2d | kernels | d2h of the last collected frame (profiling enabled)
    size_t img_pitch = 0;
    ovs_keypoint* d_out_kps = nullptr;
    uint8_t* d_out_desc = nullptr;
    int32_t* d_out_counts = nullptr;
    int out_cap = 0;
    int out_cap_variant[2] = {0, 0};   // by FrameGeo::variant bit 0; buffers are allocated for [1], the layout follows the current variant
    size_t out_block_bytes = 0, out_off_desc = 0;
    void set_out_layout() {
        out_cap = out_cap_variant[variant & 1];
        out_off_desc = (16 + sizeof(ovs_keypoint) * (size_t)out_cap + 31) & ~(size_t)31;
        out_block_bytes = out_off_desc + (size_t)32 * out_cap;
        d_out_desc = reinterpret_cast<uint8_t*>(d_out_counts) + out_off_desc;
    }
    hipStream_t last_stream = nullptr;   // stream of the last extract (device-batch form: the caller's)
    int32_t last_host_count = -1;        // keypoints the last HOST-form extract returned (they are still in d_out_kps / d_out_desc)
    // last extract (for pyramid / debug getters)
    const uint8_t* last_img0 = nullptr;
    size_t last_stride0 = 0, last_frame_stride0 = 0;
    int last_batch = 0;
    StageProfiler<4> prof;
    // optional sub-batch pipelining of the device-batch path (ovs_orb_set_pipeline)
    static constexpr int kMaxSub = 4;
    int pipeline = 1;
    hipStream_t sub_stream[kMaxSub] = {};
    hipEvent_t ev_fork = nullptr, ev_join[kMaxSub] = {};
    StageProfiler<4> prof_sub[kMaxSub];
    // FAST on level 0 needs no pyramid: it runs on aux_stream BESIDE the seven resize launches (VALU-bound next to latency / bandwidth-bound),
    // the remaining levels follow the pyramid on the main stream (ovs_orb_set_fast_split; default on)
    bool fast_split = true;
    int pyr_chain_max = tuning().pyr_chain;   // frames per launch up to which the pyramid is one k_pyramid_chain launch (ovs_orb_set_pyramid_chain; 0 = never)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_aux_fork = nullptr, ev_aux_join = nullptr;
    StageProfiler<1> prof_aux;
    ~ovs_orb() {
        res.clear();   // drains the streams the profilers' events were recorded on
        prof_aux.destroy();
        prof.destroy();
        for (auto& ps : prof_sub) ps.destroy();
    }
};

namespace {

// The plan of rows x cols with the handle's parameters; false if the geometry cannot be processed (the planner's own refusals, or too many
// keypoints on one level for the quad-tree's LDS arrays: that formula lives with k_tree)
bool plan_for(const ovs_orb* h, int rows, int cols, OrbPlan& plan) {
    return build_orb_plan(h->p, h->plan.tab, h->variant, rows, cols, plan) && tree_lds_bytes_for(plan.geo) <= kMaxLdsPerWorkgroup;
}

template <class T>
hipError_t upload(T* dst, const std::vector<T>& v) {
    return v.empty() ? hipSuccess : hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

ovs_status ensure_geometry(ovs_orb* h, int rows, int cols) {
    if (rows == h->cur_rows && cols == h->cur_cols) return OVS_OK;
    if (rows > h->max_rows || cols > h->max_cols) return OVS_ERR_CAPACITY;
    // Build a local plan and commit it only after every check and every upload succeeded: a refused size (e.g. 60 x 1920 on a handle created for
    // 480 x 1920: its 85 root patches need more node / keypoint capacity than the handle has) must leave the handle exactly as it was, so that
    // the next call with the previous, valid size still finds host plan, device copies and cur_rows / cur_cols in agreement.
    OrbPlan plan;
    if (!plan_for(h, rows, cols, plan)) return OVS_ERR_INVALID;
    if (plan.pyr_bytes > h->d.pyr_frame_bytes || plan.cand_entries > h->d.cand_frame_entries || plan.node_entries > h->d.node_frame_entries ||
        plan.taps.size() > h->taps_cap || (size_t)plan.geo.total_kp_cap > h->kps_cap || plan.cells.size() > h->cells_cap)
        return OVS_ERR_CAPACITY;
    // spans that do not fit are not an error: the geometry runs without the chain / without pairs (cannot happen: the capacities cover the largest image)
    if (plan.chain.spans.size() > h->chain_cap) plan.chain.ok = false;
    if (plan.pair_spans.size() > h->pair_cap || plan.htaps.size() > h->htaps_cap) plan.drop_pairs();
    // the buffers keep the strides they were allocated with (max geometry); only offsets inside a frame block change
    OVS_HIP_TRY(hipDeviceSynchronize());   // rare: kernels of an earlier geometry may still read d_geo / d_taps
    // from here on the device copy is being replaced: if an upload fails half way, no size is current any more (and nothing else of the handle changed)
    h->cur_rows = h->cur_cols = 0;
    OVS_HIP_TRY(hipMemcpy(h->d_geo, &plan.geo, sizeof(FrameGeo), hipMemcpyHostToDevice));
    OVS_HIP_TRY(upload(h->d_taps, plan.taps));
    OVS_HIP_TRY(upload(h->d_cells, plan.cells));
    if (plan.chain.ok) OVS_HIP_TRY(upload(h->d_chain, plan.chain.spans));
    OVS_HIP_TRY(upload(h->d_pair, plan.pair_spans));
    OVS_HIP_TRY(upload(h->d_htaps, plan.htaps));
    h->plan = std::move(plan);
    h->cur_rows = rows;
    h->cur_cols = cols;
    return OVS_OK;
}

// One extract of `batch` device frames: what run_extract / run_chain work on
struct ExtractJob {
    const uint8_t* images;
    size_t stride, frame_stride;
    const uint8_t* masks;   // or null
    int rows, cols, batch;
    ovs_keypoint* kps;      // outputs: cap records per frame
    uint8_t* desc;
    int32_t* counts;
    int cap;
    uint8_t* mirror = nullptr;       // a one-frame host call: the pinned block [counts 16 B | keypoints | descriptors] k_describe also writes the results into
    bool counters_cleared = false;   // the caller has already enqueued the clearing of the candidate counters on the job's stream
};

// the handle's buffers as frames [f0, ..) of the batch see them
DevBuffers sub_batch_view(const ovs_orb* h, int f0) {
    const FrameGeo& geo = h->plan.geo;
    DevBuffers d = h->d;
    d.pyr += (size_t)f0 * d.pyr_frame_bytes;
    d.cand += (size_t)f0 * d.cand_frame_entries;
    d.cand_count += (size_t)f0 * geo.num_levels;
    d.nodes += (size_t)f0 * d.node_frame_entries * 4;
    d.lvl_kps += (size_t)f0 * geo.total_kp_cap;
    d.lvl_count += (size_t)f0 * geo.num_levels;
    return d;
}

// A1: each level from the previous one -- for a tracker's single frame (or a stereo pair) all levels in ONE launch (k_pyramid_chain: the
// seven dependent launches cost 40 us of a 0.24 ms extract), for batches level by level (the throughput form)
ovs_status run_pyramid(const ovs_orb* h, const DevBuffers& d, const uint8_t* img, size_t stride, size_t frame_stride, int nb, hipStream_t s) {
    const OrbPlan& plan = h->plan;
    const FrameGeo& geo = plan.geo;
    const int L = geo.num_levels;
    if (plan.chain.ok && L > 1 && nb <= h->pyr_chain_max && !((uintptr_t)img & 3) && !(frame_stride & 3) && !(stride & 3)) {
        OVS_HIP_TRY(launch_pyramid_chain(img, frame_stride, (int)stride, d.pyr, d.pyr_frame_bytes, d.geo, h->d_taps, h->d_chain, plan.chain.TX, plan.chain.TY,
                                         plan.chain.bufA, plan.chain.bufB, plan.chain.tap_cap, nb, s));
        return OVS_OK;
    }
    for (int l = 1; l < L; ++l) {
        const LevelGeo& g = geo.lv[l];
        const LevelGeo& gp = geo.lv[l - 1];
        const uint8_t* src = (l == 1) ? img : d.pyr + gp.plane_off;
        const size_t src_fs = (l == 1) ? frame_stride : d.pyr_frame_bytes;
        const int src_pitch = (l == 1) ? (int)stride : gp.pitch;
        // batches: levels l and l + 1 in one launch where the geometry has a plan for the pair (the middle level is written once, never re-read)
        if (l + 1 < L && plan.pair_off[l + 1] >= 0 && resize_pair_launchable(src, src_fs, src_pitch, geo.lv[l + 1].rows, geo.lv[l + 1].cols, nb)) {
            const LevelGeo& g2 = geo.lv[l + 1];
            OVS_HIP_TRY(launch_resize_pair(src, src_fs, src_pitch, d.pyr + g.plane_off, g.pitch, g.rows, g.cols, d.pyr + g2.plane_off, g2.pitch, g2.rows, g2.cols,
                                           d.pyr_frame_bytes, h->d_taps + g.ytab_off, h->d_taps + g2.ytab_off, h->d_htaps + plan.htab_off[l], h->d_htaps + plan.htab_off[l + 1],
                                           h->d_pair + plan.pair_off[l + 1], nb, s));
            ++l;
            continue;
        }
        OVS_HIP_TRY(launch_resize(src, src_fs, src_pitch, gp.rows, gp.cols, d.pyr + g.plane_off, d.pyr_frame_bytes, g.pitch, g.rows, g.cols,
                                  h->d_taps + g.xtab_off, h->d_taps + g.ytab_off, nb, s, g.resize_hwin_ok));
    }
    return OVS_OK;
}

// pyramid -> FAST -> quad-tree -> describe for frames [f0, f0 + nb) of the job, on stream s
ovs_status run_chain(ovs_orb* h, StageProfiler<4>& prof, const ExtractJob& job, int f0, int nb, hipStream_t s) {
    const FrameGeo& geo = h->plan.geo;
    const int L = geo.num_levels;
    const DevBuffers d = sub_batch_view(h, f0);
    const size_t stride = job.stride, frame_stride = job.frame_stride;
    const uint8_t* img = job.images + (size_t)f0 * frame_stride;
    const uint8_t* msk = job.masks ? job.masks + (size_t)f0 * frame_stride : nullptr;
    OVS_HIP_TRY(prof.begin(s));
    const bool split = h->fast_split && L > 1 && &prof == &h->prof && geo.lv[1].cell_base > 0;
    if (split) {
        OVS_HIP_TRY(hipEventRecord(h->ev_aux_fork, s));
        OVS_HIP_TRY(hipStreamWaitEvent(h->aux_stream, h->ev_aux_fork, 0));
        h->prof_aux.enabled = prof.enabled;
        OVS_HIP_TRY(h->prof_aux.begin(h->aux_stream));
        OVS_HIP_TRY(launch_fast(geo, d, img, stride, frame_stride, msk, job.rows, nb, h->aux_stream, 0, geo.lv[1].cell_base));
        OVS_HIP_TRY(h->prof_aux.mark(1, h->aux_stream));
        // level 0's quad-tree (the longest pole: ~20 k candidates per frame, latency-bound) follows on the same stream, under the FAST of
        // the other levels
        OVS_HIP_TRY(launch_tree(geo, d, nb, h->aux_stream, 0, 1));
        OVS_HIP_TRY(hipEventRecord(h->ev_aux_join, h->aux_stream));
    }
    const ovs_status st = run_pyramid(h, d, img, stride, frame_stride, nb, s);
    if (st != OVS_OK) return st;
    OVS_HIP_TRY(prof.mark(1, s));
    // split: level 0's cells and level were launched on aux_stream above; otherwise all of them here (from cell 0 / level 0 to the last)
    OVS_HIP_TRY(launch_fast(geo, d, img, stride, frame_stride, msk, job.rows, nb, s, split ? geo.lv[1].cell_base : 0, -1));
    OVS_HIP_TRY(prof.mark(2, s));
    OVS_HIP_TRY(launch_tree(geo, d, nb, s, split ? 1 : 0, -1));
    if (split) OVS_HIP_TRY(hipStreamWaitEvent(s, h->ev_aux_join, 0));   // describe needs every level's keypoints
    OVS_HIP_TRY(prof.mark(3, s));
    // a one-frame host call: the results also go straight into its pinned block
    uint8_t* const mo = (job.mirror && nb == 1 && f0 == 0 && job.kps == h->d_out_kps && job.cap == h->out_cap) ? job.mirror : nullptr;
    OVS_HIP_TRY(launch_describe(geo, d, img, stride, frame_stride, job.kps + (size_t)f0 * job.cap, job.desc + (size_t)f0 * job.cap * 32, job.counts + f0, job.cap, nb, s,
                                mo ? reinterpret_cast<ovs_keypoint*>(mo + 16) : nullptr, mo ? mo + h->out_off_desc : nullptr,
                                mo ? reinterpret_cast<int32_t*>(mo) : nullptr));
    OVS_HIP_TRY(prof.mark(4, s));
    return OVS_OK;
}

ovs_status run_extract(ovs_orb* h, const ExtractJob& job, hipStream_t s) {
    ovs_status st = ensure_geometry(h, job.rows, job.cols);
    if (st != OVS_OK) return st;
    const int L = h->plan.geo.num_levels, batch = job.batch;
    if (!job.counters_cleared) OVS_HIP_TRY(hipMemsetAsync(h->d.cand_count, 0, sizeof(uint32_t) * (size_t)batch * L, s));
    const int nsub = std::min(h->pipeline, batch);
    if (nsub <= 1) {
        st = run_chain(h, h->prof, job, 0, batch, s);
        if (st != OVS_OK) return st;
    } else {
        // fork: the sub-batches run their chains on the handle's own streams, so the latency-bound stages of one (pyramid, quad-tree,
        // describe) overlap the VALU-bound FAST pass of another; join: the caller's stream waits for all of them
        OVS_HIP_TRY(hipEventRecord(h->ev_fork, s));
        const int per = (batch + nsub - 1) / nsub;
        for (int k = 0; k < nsub; ++k) {
            const int f0 = k * per, nb = std::min(per, batch - f0);
            if (nb <= 0) break;
            OVS_HIP_TRY(hipStreamWaitEvent(h->sub_stream[k], h->ev_fork, 0));
            h->prof_sub[k].enabled = h->prof.enabled;
            st = run_chain(h, h->prof_sub[k], job, f0, nb, h->sub_stream[k]);
            if (st != OVS_OK) return st;
            OVS_HIP_TRY(hipEventRecord(h->ev_join[k], h->sub_stream[k]));
            OVS_HIP_TRY(hipStreamWaitEvent(s, h->ev_join[k], 0));
        }
    }
    h->last_img0 = job.images;
    h->last_stride0 = job.stride;
    h->last_frame_stride0 = job.frame_stride;
    h->last_batch = batch;
    h->last_stream = s;
    return OVS_OK;
}

}   // namespace

namespace ovs {
bool orb_pyramid_view(const ovs_orb* h, int frame, PyrView* out) {
    if (!h || !out || !h->last_img0 || frame < 0 || frame >= h->last_batch) return false;
    const int L = h->plan.geo.num_levels;
    out->num_levels = L;
    for (int l = 0; l < L; ++l) {
        const LevelGeo& g = h->plan.geo.lv[l];
        if (l == 0) {
            out->base[0] = h->last_img0 + (size_t)frame * h->last_frame_stride0;
            out->pitch[0] = (int32_t)h->last_stride0;
        } else {
            out->base[l] = h->d.pyr + (size_t)frame * h->d.pyr_frame_bytes + g.plane_off;
            out->pitch[l] = g.pitch;
        }
        out->rows[l] = g.rows;
        out->cols[l] = g.cols;
        out->scale[l] = h->plan.tab.sf[l];
        out->inv_scale[l] = h->plan.tab.isf[l];
    }
    return true;
}
int orb_device(const ovs_orb* h) { return h ? h->device : -1; }
hipStream_t orb_last_stream(const ovs_orb* h) { return h ? h->last_stream : nullptr; }

// If (kps, desc, n) are byte-for-byte what the handle's last HOST-form extract returned -- the pinned block the results were downloaded into
// is still there to compare with (120 KB: a few microseconds) -- the same data is also still in the device output block: hand that out.
bool orb_host_outputs_equal(const ovs_orb* h, const ovs_keypoint* kps, const uint8_t* desc, int32_t n, const ovs_keypoint** d_kps,
                            const uint8_t** d_desc) {
    if (!h || h->last_host_count < 0 || h->last_host_count != n || h->n_submitted != h->n_collected || h->last_slot < 0) return false;
    const ovs_orb::HostSlot& sl = h->slot[h->last_slot];
    if (!sl.h_out) return false;
    if (n > 0 && (std::memcmp(kps, sl.h_out + 16, sizeof(ovs_keypoint) * (size_t)n) != 0 || std::memcmp(desc, sl.h_out + h->out_off_desc, (size_t)32 * n) != 0))
        return false;
    *d_kps = h->d_out_kps;
    *d_desc = h->d_out_desc;
    return true;
}
}   // namespace ovs

extern "C" {

const char* ovs_last_error(void) { return g_last_error.c_str(); }

int32_t ovs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

ovs_status ovs_device_arch(int32_t dev, char* buf, size_t buflen) {
    if (!buf || buflen == 0) return OVS_ERR_INVALID;
    hipDeviceProp_t prop;
    OVS_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    std::snprintf(buf, buflen, "%s", prop.gcnArchName);
    return OVS_OK;
}

ovs_status ovs_orb_create(const ovs_orb_params* params, int32_t max_rows, int32_t max_cols, int32_t max_batch, int32_t device,
                          ovs_orb** out) {
    if (!params || !out || params->num_levels < 1 || params->num_levels > OVS_MAX_LEVELS || !(params->scale_factor > 1.0f) ||
        params->max_num_keypts < 1 || max_rows < 1 || max_cols < 1 || max_batch < 1)
        return OVS_ERR_INVALID;
    *out = nullptr;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    std::unique_ptr<ovs_orb> owner(new (std::nothrow) ovs_orb());
    ovs_orb* const h = owner.get();
    if (!h) return OVS_ERR_INVALID;
    h->p = *params;
    h->device = device;
    h->max_rows = max_rows;
    h->max_cols = max_cols;
    h->max_batch = max_batch;
    h->plan.tab = calc_tables(h->p);
    OrbPlan largest;   // the buffers are sized by the plan of the largest geometry
    if (!plan_for(h, max_rows, max_cols, largest)) return OVS_ERR_INVALID;
    const FrameGeo& geo = largest.geo;
    const size_t cand_entries = largest.cand_entries;
    size_t node_entries = largest.node_entries;
    OVS_HIP_TRY_RAW(hipSetDevice(device));
    OVS_HIP_TRY_RAW(h->res.stream(&h->stream));
    const int L = params->num_levels;
    const size_t B = (size_t)max_batch;
    h->d.pyr_frame_bytes = (largest.pyr_bytes + 255) & ~(size_t)255;
    h->d.cand_frame_entries = cand_entries;
    // The per-level node and keypoint capacities depend on the root grid (round(W / H) x 1 patches, at most 64), i.e. on the ASPECT
    // RATIO of the image, not on its size: a small elongated image can need more of both than the largest image the handle was created
    // for (found by tools/fuzz_parity.py: 1664 x 257 on a 2000 x 1300 handle). Size them for the worst grid.
    {
        // (round 6: more than 64 root patches run when the handle was CREATED for such a shape -- the largest image's own root grids count
        // here; a 64:1 strip on a handle created for 4:3 images is refused with OVS_ERR_CAPACITY, not OVS_ERR_INVALID)
        size_t node_worst = 0, kp_worst[2] = {0, 0};
        for (int l = 0; l < L; ++l) {
            const int roots = std::max(64, geo.lv[l].gx * geo.lv[l].gy);
            node_worst += (size_t)2 * 4 * (std::max(geo.lv[l].n_keypts, roots) + 16);
            kp_worst[0] += (size_t)std::max(geo.lv[l].n_keypts + 3, 4 * roots);
            kp_worst[1] += (size_t)std::max(2 * geo.lv[l].n_keypts + 3, 4 * roots);   // ovs_orb_set_variant(TREE_SWITCH_FACTOR, 1)
        }
        node_entries = std::max(node_entries, node_worst);
        h->out_cap_variant[0] = (int)kp_worst[0];
        h->out_cap_variant[1] = (int)kp_worst[1];
    }
    h->d.node_frame_entries = node_entries;
    h->taps_cap = largest.taps.size() + 64;
    h->kps_cap = (size_t)h->out_cap_variant[1];
    OVS_HIP_TRY_RAW(h->res.dev(&h->d_geo, sizeof(FrameGeo)));
    OVS_HIP_TRY_RAW(h->res.dev(&h->d_taps, h->taps_cap * sizeof(ResizeTap)));
    h->cells_cap = largest.cells.size() + 64;   // (the cell count is monotone in rows and cols: the largest image has the most cells)
    OVS_HIP_TRY_RAW(h->res.dev(&h->d_cells, h->cells_cap * sizeof(CellDesc)));
    h->chain_cap = (size_t)L * ((size_t)(max_cols + kChainTileW0 - 1) / kChainTileW0 + (size_t)(max_rows + kChainTileH0 - 1) / kChainTileH0 + 2);   // (the tile grid is monotone in rows and cols)
    OVS_HIP_TRY_RAW(h->res.dev(&h->d_chain, h->chain_cap * sizeof(ChainSpan)));
    h->pair_cap = (size_t)L * ((size_t)(max_cols + kTileW - 1) / kTileW + (size_t)(max_rows + kTileH - 1) / kTileH + 2);   // (every level's tile grid is at most level 0's)
    OVS_HIP_TRY_RAW(h->res.dev(&h->d_pair, h->pair_cap * sizeof(PairSpan)));
    h->htaps_cap = h->taps_cap;   // one record per column pair of every level: fewer than there are taps
    OVS_HIP_TRY_RAW(h->res.dev(&h->d_htaps, h->htaps_cap * sizeof(HTapRec)));
    OVS_HIP_TRY_RAW(h->res.dev(&h->d.pyr, std::max<size_t>(h->d.pyr_frame_bytes * B, 256)));
    OVS_HIP_TRY_RAW(h->res.dev(&h->d.cand, std::max<size_t>(cand_entries * B * sizeof(uint64_t), 256)));
    OVS_HIP_TRY_RAW(h->res.dev(&h->d.cand_count, sizeof(uint32_t) * B * L));
    OVS_HIP_TRY_RAW(h->res.dev(&h->d.nodes, std::max<size_t>(node_entries * B * 16, 256)));
    OVS_HIP_TRY_RAW(h->res.dev(&h->d.lvl_kps, std::max<size_t>(h->kps_cap * B * sizeof(uint64_t), 256)));
    OVS_HIP_TRY_RAW(h->res.dev(&h->d.lvl_count, sizeof(uint32_t) * B * L));
    OVS_HIP_TRY_RAW(hipMemset(h->d.lvl_count, 0, sizeof(uint32_t) * B * L));
    h->d.geo = h->d_geo;
    h->d.taps = h->d_taps;
    h->d.cells = h->d_cells;
    // host-API staging: one frame
    h->img_pitch = ((size_t)max_cols + 255) & ~(size_t)255;
    // one contiguous device output block [counts | keypoints | descriptors] so that ONE D2H brings a frame's results back; allocated
    // for the larger of the two capacities, laid out (and copied) for the current one
    const size_t out_block_alloc = ((16 + sizeof(ovs_keypoint) * (size_t)h->out_cap_variant[1] + 31) & ~(size_t)31) + (size_t)32 * h->out_cap_variant[1];
    OVS_HIP_TRY_RAW(h->res.dev(&h->d_out_counts, out_block_alloc));
    h->d_out_kps = reinterpret_cast<ovs_keypoint*>(reinterpret_cast<uint8_t*>(h->d_out_counts) + 16);
    h->set_out_layout();
    OVS_HIP_TRY_RAW(h->res.stream(&h->copy_stream));
    OVS_HIP_TRY_RAW(h->res.stream(&h->aux_stream));
    OVS_HIP_TRY_RAW(h->res.event(&h->ev_aux_fork, hipEventDisableTiming));
    OVS_HIP_TRY_RAW(h->res.event(&h->ev_aux_join, hipEventDisableTiming));
    for (auto& sl : h->slot) {
        OVS_HIP_TRY_RAW(h->res.dev(&sl.d_img, h->img_pitch * max_rows));
        OVS_HIP_TRY_RAW(h->res.pinned(&sl.h_in, h->img_pitch * max_rows));
        OVS_HIP_TRY_RAW(h->res.pinned(&sl.h_out, out_block_alloc));
        OVS_HIP_TRY_RAW(h->res.event(&sl.ev_h2d, hipEventDisableTiming));
        OVS_HIP_TRY_RAW(h->res.event(&sl.ev_done, hipEventDisableTiming));
    }
    *out = owner.release();
    return OVS_OK;
}

int32_t ovs_orb_device(const ovs_orb* h) { return ovs::orb_device(h); }

ovs_status ovs_orb_destroy(ovs_orb* h) {
    if (!h) return OVS_OK;
    delete h;
    return OVS_OK;
}

ovs_status ovs_orb_tables(const ovs_orb* h, float* sf, float* isf, float* ls, float* ils, int32_t* npl) {
    if (!h) return OVS_ERR_INVALID;
    for (int l = 0; l < h->p.num_levels; ++l) {
        if (sf) sf[l] = h->plan.tab.sf[l];
        if (isf) isf[l] = h->plan.tab.isf[l];
        if (ls) ls[l] = h->plan.tab.ls[l];
        if (ils) ils[l] = h->plan.tab.ils[l];
        if (npl) npl[l] = h->plan.tab.npl[l];
    }
    return OVS_OK;
}

int32_t ovs_orb_max_keypoints(const ovs_orb* h) { return h ? h->out_cap : 0; }

ovs_status ovs_orb_profile_enable(ovs_orb* h, int32_t enable) {
    if (!h) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(h->device));
    h->prof.enabled = enable != 0;
    if (enable) OVS_HIP_TRY(h->prof.ensure());
    for (int k = 0; k < h->pipeline && h->pipeline > 1; ++k) {
        h->prof_sub[k].enabled = h->prof.enabled;
        if (enable) OVS_HIP_TRY(h->prof_sub[k].ensure());
    }
    return OVS_OK;
}

ovs_status ovs_orb_profile_read(ovs_orb* h, float* stage_ms, int32_t* ncalls) {
    if (!h || !stage_ms || !ncalls) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(h->device));
    OVS_HIP_TRY(h->prof.read(stage_ms, ncalls));
    // pipelined calls: every sub-batch recorded its own chain on its own stream; a stage's time is the sum of its launches' own
    // durations (they overlap launches of other stages in wall time)
    for (int k = 0; k < ovs_orb::kMaxSub; ++k) {
        if (!h->prof_sub[k].created) continue;
        float ms[4];
        int32_t nc = 0;
        OVS_HIP_TRY(h->prof_sub[k].read(ms, &nc));
        for (int j = 0; j < 4; ++j) stage_ms[j] += ms[j];
        if (k == 0) *ncalls += nc;
    }
    return OVS_OK;
}

ovs_status ovs_orb_set_variant(ovs_orb* h, int32_t which, int32_t value) {
    if (!h) return OVS_ERR_INVALID;
    int32_t v = h->variant;
    if (which == OVS_VARIANT_TREE_SWITCH_FACTOR && (value == 3 || value == 1)) v = (v & ~1) | (value == 1 ? 1 : 0);
    else if (which == OVS_VARIANT_TREE_TIE_ORDER && (value == 0 || value == 1)) v = (v & ~2) | (value ? 2 : 0);
    else if (which == OVS_VARIANT_BLUR_TAPS && (value == 0 || value == 1)) v = (v & ~4) | (value ? 4 : 0);
    else if (which == OVS_VARIANT_TRIG && (value == 0 || value == 1)) v = (v & ~8) | (value ? 8 : 0);
    else return OVS_ERR_INVALID;
    if (v != h->variant) {
        OVS_HIP_TRY(hipSetDevice(h->device));
        OVS_HIP_TRY(hipDeviceSynchronize());   // the output block's layout follows the variant's capacity: nothing may be in flight
        h->variant = v;
        h->cur_rows = h->cur_cols = 0;   // the device copy of the geometry carries the flags: rebuilt by the next extract
        h->last_host_count = -1;
        h->set_out_layout();             // ovs_orb_max_keypoints changes with TREE_SWITCH_FACTOR
    }
    return OVS_OK;
}

ovs_status ovs_debug_inject_hip_failures(int32_t skip_calls, int32_t n_calls) {
    ovs::g_injected_hip_failures.store(0, std::memory_order_relaxed);
    ovs::g_injected_hip_skip.store(skip_calls > 0 ? skip_calls : 0, std::memory_order_relaxed);
    ovs::g_injected_hip_failures.store(n_calls > 0 ? n_calls : 0, std::memory_order_relaxed);
    return OVS_OK;
}

int64_t ovs_debug_live_resources(void) { return ovs::g_live_resources.load(std::memory_order_relaxed); }

ovs_status ovs_orb_set_fast_split(ovs_orb* h, int32_t enable) {
    if (!h) return OVS_ERR_INVALID;
    h->fast_split = enable != 0;
    return OVS_OK;
}

ovs_status ovs_orb_set_pyramid_chain(ovs_orb* h, int32_t max_frames) {
    if (!h || max_frames < 0) return OVS_ERR_INVALID;
    h->pyr_chain_max = max_frames;
    return OVS_OK;
}

ovs_status ovs_orb_profile_read_aux(ovs_orb* h, float* fast_level0_ms, int32_t* ncalls) {
    if (!h || !fast_level0_ms || !ncalls) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(h->device));
    *fast_level0_ms = 0;
    *ncalls = 0;
    if (!h->prof_aux.created) return OVS_OK;
    OVS_HIP_TRY(h->prof_aux.read(fast_level0_ms, ncalls));
    return OVS_OK;
}

ovs_status ovs_orb_set_pipeline(ovs_orb* h, int32_t n_sub) {
    if (!h || n_sub < 1 || n_sub > ovs_orb::kMaxSub) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(h->device));
    if (n_sub > 1) {
        if (!h->ev_fork) OVS_HIP_TRY(h->res.event(&h->ev_fork, hipEventDisableTiming));
        for (int k = 0; k < n_sub; ++k) {
            if (!h->sub_stream[k]) OVS_HIP_TRY(h->res.stream(&h->sub_stream[k]));
            if (!h->ev_join[k]) OVS_HIP_TRY(h->res.event(&h->ev_join[k], hipEventDisableTiming));
            if (h->prof.enabled) OVS_HIP_TRY(h->prof_sub[k].ensure());
        }
    }
    h->pipeline = n_sub;
    return OVS_OK;
}

ovs_status ovs_orb_extract_batch_dev(ovs_orb* h, const uint8_t* d_images, int32_t batch, int32_t rows, int32_t cols, size_t stride,
                                     size_t frame_stride, const uint8_t* d_masks, ovs_keypoint* d_kps, uint8_t* d_desc,
                                     int32_t* d_counts, int32_t cap, void* stream) {
    if (!h || !d_images || !d_kps || !d_desc || !d_counts || batch < 1 || rows < 1 || cols < 1 || cap < 1) return OVS_ERR_INVALID;
    if (batch > h->max_batch) return OVS_ERR_CAPACITY;
    if (((uintptr_t)d_images & 3) || (stride & 3) || (frame_stride & 3) || stride < (size_t)cols) return OVS_ERR_ALIGN;
    if (d_masks && ((uintptr_t)d_masks & 3)) return OVS_ERR_ALIGN;
    OVS_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;   // verbatim: NULL is HIP's default stream (torch's default stream handle is 0)
    return run_extract(h, ExtractJob{d_images, stride, frame_stride, d_masks, rows, cols, batch, d_kps, d_desc, d_counts, cap}, s);
}

// ---- host-pointer path: submit / collect over two slots; ovs_orb_extract = submit + collect ----------------------------------------
namespace {

// rows of `cols` bytes from the caller's (pageable) buffer to the device image of a slot, on copy_stream
ovs_status upload_plane(ovs_orb* h, const uint8_t* src, size_t stride, int rows, int cols, uint8_t* staging, uint8_t* d_dst) {
    hipStream_t cs = h->copy_stream;
    const size_t pitch = h->img_pitch;
    if (h->host_mode == 0 || !staging) {
        OVS_HIP_TRY(hipMemcpy2DAsync(d_dst, pitch, src, stride, (size_t)cols, (size_t)rows, hipMemcpyHostToDevice, cs));
        return OVS_OK;
    }
    // banded: the CPU copies band k+1 into pinned memory while the DMA engine moves band k (a pageable hipMemcpy does the same inside
    // the runtime, but through its own small staging chunks and with a blocking wait at the end)
    const int band = std::max(32, (rows + 7) / 8);
    for (int r0 = 0; r0 < rows; r0 += band) {
        const int nr = std::min(band, rows - r0);
        uint8_t* st = staging + (size_t)r0 * pitch;
        if (stride == (size_t)cols && pitch == (size_t)cols) {
            std::memcpy(st, src + (size_t)r0 * stride, (size_t)nr * cols);
        } else {
            for (int r = 0; r < nr; ++r) std::memcpy(st + (size_t)r * pitch, src + (size_t)(r0 + r) * stride, (size_t)cols);
        }
        OVS_HIP_TRY(hipMemcpyAsync(d_dst + (size_t)r0 * pitch, st, (size_t)nr * pitch, hipMemcpyHostToDevice, cs));
    }
    return OVS_OK;
}

// The fused entries (ovs_orb_extract_prepared / _pair_prepared): the image argument is the RAW source, staged in the preparer's planes and
// prepared into the plane the gray image is otherwise uploaded into. The arguments have passed imgprep_check; the caller holds p->mu.
struct RawInput {
    ovs_imgprep* p;
    int channels, color_order, rectify;
    uint8_t* gray[2];   // or null: the prepared images on the host
    size_t gray_stride;
};

ovs_status submit_frame(ovs_orb* h, const uint8_t* image, int32_t rows, int32_t cols, size_t stride, const uint8_t* mask, size_t mask_stride,
                        const RawInput* raw) {
    if (!h || !image || rows <= 0 || cols <= 0 || (!raw && stride < (size_t)cols) || (mask && mask_stride < (size_t)cols)) return OVS_ERR_INVALID;
    if (rows > h->max_rows || cols > h->max_cols) return OVS_ERR_CAPACITY;
    if (h->n_submitted - h->n_collected >= 2) return OVS_ERR_CAPACITY;   // both slots in flight: collect first
    OVS_HIP_TRY(hipSetDevice(h->device));
    ovs_orb::HostSlot& sl = h->slot[h->n_submitted & 1];
    hipStream_t s = h->stream, cs = h->copy_stream;
    // a geometry change synchronises the device (ensure_geometry): do it before anything of this frame is enqueued
    ovs_status st = ensure_geometry(h, rows, cols);
    if (st != OVS_OK) return st;
    const bool timed = h->prof.enabled;
    if (timed)
        for (auto& e : sl.t)
            if (!e) OVS_HIP_TRY(h->res.event(&e, hipEventDefault));
    // the candidate counters are cleared while the image is still on its way (a 4 us fill kernel that used to run between the upload and the pyramid)
    OVS_HIP_TRY(hipMemsetAsync(h->d.cand_count, 0, sizeof(uint32_t) * (size_t)h->plan.geo.num_levels, s));
    if (timed) OVS_HIP_TRY(hipEventRecord(sl.t[0], cs));
    if (raw) OVS_HIP_TRY(hipMemcpy2DAsync(raw->p->d_src[0], raw->p->src_pitch, image, stride, (size_t)cols * raw->channels, (size_t)rows, hipMemcpyHostToDevice, cs));
    else st = upload_plane(h, image, stride, rows, cols, sl.h_in, sl.d_img);
    if (st != OVS_OK) return st;
    if (mask) {
        if (!sl.d_mask) OVS_HIP_TRY(h->res.dev(&sl.d_mask, h->img_pitch * h->max_rows));
        if (!sl.h_mask) OVS_HIP_TRY(h->res.pinned(&sl.h_mask, h->img_pitch * h->max_rows));
        st = upload_plane(h, mask, mask_stride, rows, cols, sl.h_mask, sl.d_mask);
        if (st != OVS_OK) return st;
    }
    if (timed) OVS_HIP_TRY(hipEventRecord(sl.t[1], cs));
    OVS_HIP_TRY(hipEventRecord(sl.ev_h2d, cs));
    OVS_HIP_TRY(hipStreamWaitEvent(s, sl.ev_h2d, 0));
    if (raw)
        OVS_HIP_TRY(imgprep_enqueue(raw->p, raw->p->d_src[0], nullptr, rows, cols, raw->p->src_pitch, raw->channels, raw->color_order, raw->rectify, sl.d_img, nullptr,
                                    h->img_pitch, s));
    // the kernels write counts + keypoints + descriptors straight into the slot's pinned block (no D2H copy); the counters are cleared above
    st = run_extract(h, ExtractJob{sl.d_img, h->img_pitch, h->img_pitch * (size_t)rows, mask ? sl.d_mask : nullptr, rows, cols, 1, h->d_out_kps,
                                   h->d_out_desc, h->d_out_counts, h->out_cap, sl.h_out, true}, s);
    if (st != OVS_OK) return st;
    if (timed) OVS_HIP_TRY(hipEventRecord(sl.t[2], s));
    if (raw && raw->gray[0])
        OVS_HIP_TRY(hipMemcpy2DAsync(raw->gray[0], raw->gray_stride, sl.d_img, h->img_pitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, s));
    sl.has_pyr = false;
    if (h->host_pyr && h->p.num_levels > 1) {
        if (!sl.h_pyr) OVS_HIP_TRY(h->res.pinned(&sl.h_pyr, h->d.pyr_frame_bytes));
        const LevelGeo& gl = h->plan.geo.lv[h->p.num_levels - 1];
        const size_t used = (size_t)gl.plane_off + (size_t)gl.pitch * gl.rows;   // levels 1 .. L-1 are contiguous in the frame block
        OVS_HIP_TRY(hipMemcpyAsync(sl.h_pyr, h->d.pyr, used, hipMemcpyDeviceToHost, s));
        sl.has_pyr = true;
    }
    if (timed) OVS_HIP_TRY(hipEventRecord(sl.t[3], s));
    OVS_HIP_TRY(hipEventRecord(sl.ev_done, s));
    sl.pending = true;
    sl.timed = timed;
    sl.rows = rows;
    sl.cols = cols;
    ++h->n_submitted;
    return OVS_OK;
}

}   // namespace

ovs_status ovs_orb_extract_submit(ovs_orb* h, const uint8_t* image, int32_t rows, int32_t cols, size_t stride, const uint8_t* mask,
                                  size_t mask_stride) {
    return submit_frame(h, image, rows, cols, stride, mask, mask_stride, nullptr);
}

ovs_status ovs_orb_extract_collect(ovs_orb* h, ovs_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n_out) {
    if (!h || !n_out || cap < 0 || (cap > 0 && (!kps || !desc))) return OVS_ERR_INVALID;
    *n_out = 0;
    if (h->n_collected == h->n_submitted) return OVS_ERR_INVALID;   // nothing in flight
    OVS_HIP_TRY(hipSetDevice(h->device));
    const int si = (int)(h->n_collected & 1);
    ovs_orb::HostSlot& sl = h->slot[si];
    OVS_HIP_TRY(hipEventSynchronize(sl.ev_done));   // the only wait of a frame
    sl.pending = false;
    ++h->n_collected;
    h->last_slot = si;
    if (sl.timed) {
        OVS_HIP_TRY(hipEventElapsedTime(&h->host_ms[0], sl.t[0], sl.t[1]));
        OVS_HIP_TRY(hipEventElapsedTime(&h->host_ms[1], sl.t[1], sl.t[2]));
        OVS_HIP_TRY(hipEventElapsedTime(&h->host_ms[2], sl.t[2], sl.t[3]));
    }
    const int32_t n = *reinterpret_cast<const int32_t*>(sl.h_out);
    const int32_t m = std::min(n, cap);
    if (m > 0) {
        std::memcpy(kps, sl.h_out + 16, sizeof(ovs_keypoint) * (size_t)m);
        std::memcpy(desc, sl.h_out + h->out_off_desc, (size_t)32 * m);
    }
    *n_out = m;
    h->last_host_count = m;
    return n > cap ? OVS_ERR_CAPACITY : OVS_OK;
}

ovs_status ovs_orb_extract(ovs_orb* h, const uint8_t* image, int32_t rows, int32_t cols, size_t stride, const uint8_t* mask,
                           size_t mask_stride, ovs_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n_out) {
    if (!h || !n_out) return OVS_ERR_INVALID;
    *n_out = 0;
    if (!image || rows <= 0 || cols <= 0) return OVS_OK;   // upstream: empty image -> early return
    if (cap < 0 || (cap > 0 && (!kps || !desc))) return OVS_ERR_INVALID;
    if (h->n_submitted != h->n_collected) return OVS_ERR_INVALID;   // frames submitted asynchronously must be collected first
    const ovs_status st = ovs_orb_extract_submit(h, image, rows, cols, stride, mask, mask_stride);
    if (st != OVS_OK) return st;
    return ovs_orb_extract_collect(h, kps, desc, cap, n_out);
}

namespace {
// ovs_orb_extract_pair; with `raw`, left / right are the raw sources (ovs_orb_extract_pair_prepared)
ovs_status extract_pair(ovs_orb* h, const uint8_t* left, const uint8_t* right, int32_t rows, int32_t cols, size_t stride, const uint8_t* mask_left,
                        const uint8_t* mask_right, size_t mask_stride, ovs_keypoint* kps_left, uint8_t* desc_left, int32_t* n_left, ovs_keypoint* kps_right,
                        uint8_t* desc_right, int32_t* n_right, int32_t cap, const RawInput* raw) {
    if (!h || !n_left || !n_right) return OVS_ERR_INVALID;
    *n_left = *n_right = 0;
    if (!left || !right || rows <= 0 || cols <= 0) return OVS_OK;   // upstream: empty image -> early return
    if (cap < 0 || (cap > 0 && (!kps_left || !desc_left || !kps_right || !desc_right)) || (!raw && stride < (size_t)cols)) return OVS_ERR_INVALID;
    if ((mask_left == nullptr) != (mask_right == nullptr) || (mask_left && mask_stride < (size_t)cols)) return OVS_ERR_INVALID;
    if (h->max_batch < 2 || rows > h->max_rows || cols > h->max_cols) return OVS_ERR_CAPACITY;
    if (h->n_submitted != h->n_collected) return OVS_ERR_INVALID;   // frames submitted asynchronously must be collected first
    OVS_HIP_TRY(hipSetDevice(h->device));
    ovs_status st = ensure_geometry(h, rows, cols);
    if (st != OVS_OK) return st;
    ovs_orb::PairBuf& pb = h->pair;
    if (!pb.d_img) {
        pb.frame_bytes = h->img_pitch * (size_t)h->max_rows;
        OVS_HIP_TRY(h->res.dev(&pb.d_img, 2 * pb.frame_bytes));
        OVS_HIP_TRY(h->res.event(&pb.ev_h2d, hipEventDisableTiming));
    }
    if (pb.cap < h->out_cap_variant[1]) {   // [counts | keypoints of both frames | descriptors of both frames], for the larger capacity
        (void)h->res.drop(&pb.d_out);
        (void)h->res.drop(&pb.h_out);
        pb.cap = h->out_cap_variant[1];
        const size_t bytes = 32 + ((2 * sizeof(ovs_keypoint) * (size_t)pb.cap + 31) & ~(size_t)31) + (size_t)64 * pb.cap;
        OVS_HIP_TRY(h->res.dev(&pb.d_out, bytes));
        OVS_HIP_TRY(h->res.pinned(&pb.h_out, bytes));
    }
    const int fcap = h->out_cap;   // per frame, current variant
    pb.off_kps = 32;
    pb.off_desc = 32 + ((2 * sizeof(ovs_keypoint) * (size_t)fcap + 31) & ~(size_t)31);
    pb.out_bytes = pb.off_desc + (size_t)64 * fcap;
    hipStream_t s = h->stream, cs = h->copy_stream;
    if (raw) {
        const uint8_t* const src[2] = {left, right};
        for (int f = 0; f < 2; ++f)
            OVS_HIP_TRY(hipMemcpy2DAsync(raw->p->d_src[f], raw->p->src_pitch, src[f], stride, (size_t)cols * raw->channels, (size_t)rows, hipMemcpyHostToDevice, cs));
    } else {
        st = upload_plane(h, left, stride, rows, cols, nullptr, pb.d_img);
        if (st == OVS_OK) st = upload_plane(h, right, stride, rows, cols, nullptr, pb.d_img + pb.frame_bytes);
    }
    if (st != OVS_OK) return st;
    if (mask_left) {
        if (!pb.d_mask) OVS_HIP_TRY(h->res.dev(&pb.d_mask, 2 * pb.frame_bytes));
        st = upload_plane(h, mask_left, mask_stride, rows, cols, nullptr, pb.d_mask);
        if (st == OVS_OK) st = upload_plane(h, mask_right, mask_stride, rows, cols, nullptr, pb.d_mask + pb.frame_bytes);
        if (st != OVS_OK) return st;
    }
    OVS_HIP_TRY(hipEventRecord(pb.ev_h2d, cs));
    OVS_HIP_TRY(hipStreamWaitEvent(s, pb.ev_h2d, 0));
    if (raw)
        OVS_HIP_TRY(imgprep_enqueue(raw->p, raw->p->d_src[0], raw->p->d_src[1], rows, cols, raw->p->src_pitch, raw->channels, raw->color_order, raw->rectify, pb.d_img,
                                    pb.d_img + pb.frame_bytes, h->img_pitch, s));
    st = run_extract(h, ExtractJob{pb.d_img, h->img_pitch, pb.frame_bytes, mask_left ? pb.d_mask : nullptr, rows, cols, 2,
                                   reinterpret_cast<ovs_keypoint*>(pb.d_out + pb.off_kps), pb.d_out + pb.off_desc, reinterpret_cast<int32_t*>(pb.d_out), fcap}, s);
    if (st != OVS_OK) return st;
    OVS_HIP_TRY(hipMemcpyAsync(pb.h_out, pb.d_out, pb.out_bytes, hipMemcpyDeviceToHost, s));
    for (int f = 0; raw && raw->gray[0] && f < 2; ++f)
        OVS_HIP_TRY(hipMemcpy2DAsync(raw->gray[f], raw->gray_stride, pb.d_img + pb.frame_bytes * f, h->img_pitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    const int32_t* cnt = reinterpret_cast<const int32_t*>(pb.h_out);
    ovs_keypoint* const kout[2] = {kps_left, kps_right};
    uint8_t* const dout[2] = {desc_left, desc_right};
    int32_t* const nout[2] = {n_left, n_right};
    bool over = false;
    for (int f = 0; f < 2; ++f) {
        const int32_t m = std::min(cnt[f], cap);
        if (m > 0) {
            std::memcpy(kout[f], pb.h_out + pb.off_kps + sizeof(ovs_keypoint) * (size_t)fcap * f, sizeof(ovs_keypoint) * (size_t)m);
            std::memcpy(dout[f], pb.h_out + pb.off_desc + (size_t)32 * fcap * f, (size_t)32 * m);
        }
        *nout[f] = m;
        over |= cnt[f] > cap;
    }
    h->last_host_count = *n_left;
    return over ? OVS_ERR_CAPACITY : OVS_OK;
}
}   // namespace

ovs_status ovs_orb_extract_pair(ovs_orb* h, const uint8_t* left, const uint8_t* right, int32_t rows, int32_t cols, size_t stride,
                                const uint8_t* mask_left, const uint8_t* mask_right, size_t mask_stride, ovs_keypoint* kps_left,
                                uint8_t* desc_left, int32_t* n_left, ovs_keypoint* kps_right, uint8_t* desc_right, int32_t* n_right, int32_t cap) {
    return extract_pair(h, left, right, rows, cols, stride, mask_left, mask_right, mask_stride, kps_left, desc_left, n_left, kps_right, desc_right, n_right, cap,
                        nullptr);
}

ovs_status ovs_orb_extract_pair_prepared(ovs_orb* h, ovs_imgprep* p, const uint8_t* raw_left, const uint8_t* raw_right, int32_t rows, int32_t cols,
                                         size_t stride, int32_t channels, int32_t color_order, int32_t rectify, const uint8_t* mask_left,
                                         const uint8_t* mask_right, size_t mask_stride, ovs_keypoint* kps_left, uint8_t* desc_left, int32_t* n_left,
                                         ovs_keypoint* kps_right, uint8_t* desc_right, int32_t* n_right, int32_t cap, uint8_t* out_gray_left,
                                         uint8_t* out_gray_right, size_t out_gray_stride) {
    if (!h || !p || !n_left || !n_right || !raw_left || !raw_right || (out_gray_left == nullptr) != (out_gray_right == nullptr)) return OVS_ERR_INVALID;
    *n_left = *n_right = 0;
    if (h->device != p->device) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    const ovs_status st = imgprep_check(p, rows, cols, stride, channels, color_order, rectify, 2);
    if (st != OVS_OK) return st;
    if (out_gray_left && out_gray_stride < (size_t)cols) return OVS_ERR_INVALID;
    const RawInput raw{p, channels, color_order, rectify, {out_gray_left, out_gray_right}, out_gray_stride};
    return extract_pair(h, raw_left, raw_right, rows, cols, stride, mask_left, mask_right, mask_stride, kps_left, desc_left, n_left, kps_right, desc_right, n_right,
                        cap, &raw);
}

ovs_status ovs_orb_extract_prepared(ovs_orb* h, ovs_imgprep* p, const uint8_t* raw, int32_t rows, int32_t cols, size_t stride, int32_t channels,
                                    int32_t color_order, int32_t rectify, const uint8_t* mask, size_t mask_stride, ovs_keypoint* kps, uint8_t* desc,
                                    int32_t cap, int32_t* n_out, uint8_t* out_gray, size_t out_gray_stride) {
    if (!h || !p || !n_out || !raw) return OVS_ERR_INVALID;
    *n_out = 0;
    if (h->device != p->device) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    ovs_status st = imgprep_check(p, rows, cols, stride, channels, color_order, rectify, 1);
    if (st != OVS_OK) return st;
    if (out_gray && out_gray_stride < (size_t)cols) return OVS_ERR_INVALID;
    if (rows == 0 || cols == 0) return OVS_OK;   // upstream: empty image -> early return
    if (cap < 0 || (cap > 0 && (!kps || !desc))) return OVS_ERR_INVALID;
    if (h->n_submitted != h->n_collected) return OVS_ERR_INVALID;   // frames submitted asynchronously must be collected first
    const RawInput in{p, channels, color_order, rectify, {out_gray, nullptr}, out_gray_stride};
    st = submit_frame(h, raw, rows, cols, stride, mask, mask_stride, &in);
    if (st != OVS_OK) return st;
    return ovs_orb_extract_collect(h, kps, desc, cap, n_out);   // waits for the frame's last event: the gray download has ended too
}

ovs_status ovs_orb_set_host_pyramid(ovs_orb* h, int32_t enable) {
    if (!h) return OVS_ERR_INVALID;
    h->host_pyr = enable != 0;
    return OVS_OK;
}

ovs_status ovs_orb_set_host_mode(ovs_orb* h, int32_t mode) {
    if (!h || mode < 0 || mode > 1) return OVS_ERR_INVALID;
    h->host_mode = mode;
    return OVS_OK;
}

ovs_status ovs_orb_host_pyramid_level(const ovs_orb* h, int32_t level, const uint8_t** base, int32_t* rows, int32_t* cols, int32_t* pitch) {
    if (!h || level < 0 || level >= h->p.num_levels || h->last_slot < 0) return OVS_ERR_INVALID;
    const ovs_orb::HostSlot& sl = h->slot[h->last_slot];
    const LevelGeo& g = h->plan.geo.lv[level];
    if (rows) *rows = g.rows;
    if (cols) *cols = g.cols;
    if (level == 0) {   // level 0 is the caller's own image (upstream aliases it too)
        if (base) *base = nullptr;
        if (pitch) *pitch = 0;
        return OVS_OK;
    }
    if (!sl.has_pyr || sl.rows != h->cur_rows || sl.cols != h->cur_cols) return OVS_ERR_INVALID;   // enable ovs_orb_set_host_pyramid first
    if (base) *base = sl.h_pyr + g.plane_off;
    if (pitch) *pitch = g.pitch;
    return OVS_OK;
}

ovs_status ovs_orb_host_profile_read(const ovs_orb* h, float* h2d_kernels_d2h_ms) {
    if (!h || !h2d_kernels_d2h_ms) return OVS_ERR_INVALID;
    for (int i = 0; i < 3; ++i) h2d_kernels_d2h_ms[i] = h->host_ms[i];
    return OVS_OK;
}

ovs_status ovs_orb_pyramid_level(ovs_orb* h, int32_t frame, int32_t level, uint8_t* host_dst, int32_t* rows, int32_t* cols) {
    if (!h || level < 0 || level >= h->p.num_levels || frame < 0 || frame >= h->last_batch || !h->last_img0) return OVS_ERR_INVALID;
    const LevelGeo& g = h->plan.geo.lv[level];
    if (rows) *rows = g.rows;
    if (cols) *cols = g.cols;
    if (!host_dst) return OVS_OK;
    OVS_HIP_TRY(hipSetDevice(h->device));
    // only the stream the last extract ran on is waited for -- never the whole device: a second extractor on another thread (stereo
    // left / right) must not be stalled by this getter
    OVS_HIP_TRY(hipStreamSynchronize(h->last_stream));
    hipStream_t s = h->stream;
    if (level == 0)
        OVS_HIP_TRY(hipMemcpy2DAsync(host_dst, g.cols, h->last_img0 + (size_t)frame * h->last_frame_stride0, h->last_stride0, g.cols, g.rows,
                                     hipMemcpyDeviceToHost, s));
    else
        OVS_HIP_TRY(hipMemcpy2DAsync(host_dst, g.cols, h->d.pyr + (size_t)frame * h->d.pyr_frame_bytes + g.plane_off, g.pitch, g.cols, g.rows,
                                     hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    return OVS_OK;
}

ovs_status ovs_orb_debug_candidates(ovs_orb* h, int32_t frame, int32_t level, int32_t* xs, int32_t* ys, int32_t* scores, int32_t cap,
                                    int32_t* n_out) {
    if (!h || !n_out || level < 0 || level >= h->p.num_levels || frame < 0 || frame >= h->last_batch) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(h->device));
    OVS_HIP_TRY(hipDeviceSynchronize());
    const LevelGeo& g = h->plan.geo.lv[level];
    const int L = h->p.num_levels;
    uint32_t n = 0;
    OVS_HIP_TRY(hipMemcpy(&n, h->d.cand_count + (size_t)frame * L + level, sizeof(uint32_t), hipMemcpyDeviceToHost));
    n = std::min<uint32_t>(n, (uint32_t)g.cand_cap);
    std::vector<uint64_t> c(n);
    if (n)
        OVS_HIP_TRY(hipMemcpy(c.data(), h->d.cand + (size_t)frame * h->d.cand_frame_entries + g.cand_off, n * sizeof(uint64_t),
                              hipMemcpyDeviceToHost));
    const uint32_t ncx = (uint32_t)g.ncx;
    std::sort(c.begin(), c.end(), [ncx](uint64_t a, uint64_t b) {
        return cand_order(cand_x(a), cand_y(a), ncx) < cand_order(cand_x(b), cand_y(b), ncx);
    });
    for (uint32_t i = 0; i < n && (int32_t)i < cap; ++i) {
        if (xs) xs[i] = (int32_t)cand_x(c[i]);
        if (ys) ys[i] = (int32_t)cand_y(c[i]);
        if (scores) scores[i] = (int32_t)cand_score(c[i]);
    }
    *n_out = (int32_t)n;
    return OVS_OK;
}

ovs_status ovs_orb_debug_level_counts(ovs_orb* h, int32_t frame, int32_t* counts) {
    if (!h || !counts || frame < 0 || frame >= h->max_batch) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(h->device));
    OVS_HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> c(h->p.num_levels);
    OVS_HIP_TRY(hipMemcpy(c.data(), h->d.lvl_count + (size_t)frame * h->p.num_levels, sizeof(uint32_t) * c.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < c.size(); ++i) counts[i] = (int32_t)c[i];
    return OVS_OK;
}

}   // extern "C"
