// frame_dev.hip -- the resident frame handle (ovs_frame_dev, frame_dev_internal.inc): a frame's matcher-side data -- undistorted keypoints,
// descriptors, stereo_x_right and the keypoint grid -- uploaded and indexed ONCE, for every window matcher's _f form and the landmark upkeep.
// Host code only: the grid kernel lives beside its launcher in match_window.hip, the arena's layout in match_window_plan.inc.
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "frame_dev_internal.inc"

using namespace ovs;

namespace {

// device arenas of destroyed frame handles, kept for the next frame (a tracker creates one handle per frame: a hipMalloc / hipFree pair
// per frame would cost more than the upload). Bounded; keyed by device and size.
struct FrameArenaPool {
    struct Item {
        int device;
        size_t bytes;
        unsigned char* p;
    };
    std::mutex mu;
    std::vector<Item> free_list;
    unsigned char* take(int device, size_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < free_list.size(); ++i)
            if (free_list[i].device == device && free_list[i].bytes == bytes) {
                unsigned char* p = free_list[i].p;
                free_list.erase(free_list.begin() + (long)i);
                return p;
            }
        return nullptr;
    }
    void give(int device, size_t bytes, unsigned char* p) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (free_list.size() < 8) {
                free_list.push_back(Item{device, bytes, p});
                return;
            }
        }
        (void)hipSetDevice(device);
        (void)hipFree(p);
    }
};
FrameArenaPool g_frame_pool;

// pinned staging for the once-per-frame upload, per thread (frames are created by the tracking thread; stereo rigs by two)
struct FrameStage {
    unsigned char* h = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    int device = -1;
    ovs::Owned res;
};

}   // namespace

extern "C" {

ovs_status ovs_frame_dev_destroy(ovs_frame_dev* f) {
    if (!f) return OVS_OK;
    if (f->arena) g_frame_pool.give(f->device, f->arena_bytes, f->arena);
    delete f;
    return OVS_OK;
}

ovs_status ovs_frame_dev_create(int32_t device, const ovs_grid_params* gp, const ovs_keypoint* undist_kps, const uint8_t* desc,
                                const float* stereo_x_right, int32_t n, ovs_frame_dev** out) {
    if (!out || !gp || n < 0 || n > 65534 || (n > 0 && (!undist_kps || !desc))) return OVS_ERR_INVALID;
    *out = nullptr;
    if (!grid_params_ok(gp)) return OVS_ERR_INVALID;
    if (ovs_device_count() <= device || device < 0) return OVS_ERR_NO_DEVICE;
    OVS_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<ovs_frame_dev, decltype(&ovs_frame_dev_destroy)> owner(new (std::nothrow) ovs_frame_dev(), &ovs_frame_dev_destroy);
    ovs_frame_dev* const f = owner.get();
    if (!f) return OVS_ERR_INVALID;
    const FrameArena lay = frame_arena_of(n);
    f->device = device;
    f->n = n;
    f->cap = lay.cap;
    f->n_cells = gp->cols * gp->rows;
    f->has_stereo = stereo_x_right != nullptr;
    f->gpp = *gp;
    f->gp = make_gridp(*gp);
    f->arena_bytes = lay.arena_bytes;
    f->arena = g_frame_pool.take(device, f->arena_bytes);
    if (!f->arena) {
        const hipError_t e = hipMalloc(&f->arena, f->arena_bytes);
        if (e != hipSuccess) {
            ovs::set_last_error("hipMalloc(frame arena)", e);
            return OVS_ERR_HIP;
        }
    }
    f->d_kps = reinterpret_cast<ovs_keypoint*>(f->arena + lay.o_kps);
    f->d_desc = f->arena + lay.o_desc;
    f->d_x_right = reinterpret_cast<float*>(f->arena + lay.o_xr);
    f->d_cell_of = reinterpret_cast<int32_t*>(f->arena + lay.o_cellof);
    f->d_items = reinterpret_cast<int32_t*>(f->arena + lay.o_items);
    f->d_cell_start = reinterpret_cast<int32_t*>(f->arena + lay.o_start);
    static thread_local FrameStage st;
    if (st.device != device) {
        (void)st.res.drop(&st.stream);
        st.device = device;
    }
    if (!st.stream) OVS_HIP_TRY_RAW(st.res.stream(&st.stream));
    const size_t up_bytes = frame_upload_bytes(lay, n, stereo_x_right != nullptr);
    if (st.cap < up_bytes) {
        (void)st.res.drop(&st.h);
        st.cap = 0;
        const size_t want = frame_stage_bytes(lay, up_bytes);
        OVS_HIP_TRY_RAW(st.res.pinned(&st.h, want));
        st.cap = want;
    }
    if (n) {
        std::memcpy(st.h + lay.o_kps, undist_kps, sizeof(ovs_keypoint) * (size_t)n);
        std::memcpy(st.h + lay.o_desc, desc, 32 * (size_t)n);
        if (stereo_x_right) std::memcpy(st.h + lay.o_xr, stereo_x_right, 4 * (size_t)n);
        OVS_HIP_TRY_RAW(hipMemcpyAsync(f->arena, st.h, up_bytes, hipMemcpyHostToDevice, st.stream));
    }
    OVS_HIP_TRY_RAW(launch_grid_assign(f->d_kps, n, f->gp, f->d_cell_of, f->d_cell_start, f->d_items, st.stream));
    OVS_HIP_TRY_RAW(hipStreamSynchronize(st.stream));   // the handle is used from other streams afterwards
    *out = owner.release();
    return OVS_OK;
}

int32_t ovs_frame_dev_num_keypoints(const ovs_frame_dev* f) { return f ? f->n : -1; }
int32_t ovs_frame_dev_device(const ovs_frame_dev* f) { return f ? f->device : -1; }

// 3 doubles per keypoint (data::keyframe::bearings_), uploaded once. Call it before the handle is shared between threads.
ovs_status ovs_frame_dev_attach_bearings(ovs_frame_dev* f, const double* bearings) {
    if (!f || (f->n > 0 && !bearings)) return OVS_ERR_INVALID;
    if (f->n == 0) return OVS_OK;
    OVS_HIP_TRY(hipSetDevice(f->device));
    if (!f->d_bearings) OVS_HIP_TRY(f->res.dev(&f->d_bearings, sizeof(double) * 3 * (size_t)f->cap));
    OVS_HIP_TRY(hipMemcpy(f->d_bearings, bearings, sizeof(double) * 3 * (size_t)f->n, hipMemcpyHostToDevice));
    return OVS_OK;
}

}   // extern "C"
