// frame_dev_internal.inc -- a frame / keyframe resident in HBM (ovs_frame_dev: frame_dev.hip creates and destroys it), as the units of the
// library that work on resident frames read it: the window matchers (match_window.hip) and the landmark upkeep (landmark_update.hip). Not part
// of the C ABI. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include "match_window_plan.inc"
#include "ovs_common.h"
#include "owned_internal.inc"

struct ovs_frame_dev {
    int device = 0;
    int n = 0, cap = 0, n_cells = 0;
    bool has_stereo = false;
    ovs::GridP gp{};
    ovs_grid_params gpp{};
    unsigned char* arena = nullptr;   // ovs::FrameArena: the six arrays below
    size_t arena_bytes = 0;
    ovs_keypoint* d_kps = nullptr;
    uint8_t* d_desc = nullptr;        // n x 32 bytes
    float* d_x_right = nullptr;
    int32_t *d_cell_of = nullptr, *d_cell_start = nullptr, *d_items = nullptr;
    double* d_bearings = nullptr;   // optional (ovs_frame_dev_attach_bearings): 3 doubles per keypoint, for match_for_triangulation
    ovs::Owned res;                 // d_bearings (the arena goes back to the pool: ovs_frame_dev_destroy)
};

namespace ovs {

// k_grid_assign over `n` device keypoints (match_window.hip, beside the kernel): one workgroup, the member lists in LDS when they fit
__attribute__((visibility("hidden"))) hipError_t launch_grid_assign(const ovs_keypoint* d_kps, int n, const GridP& g, int32_t* cell_of, int32_t* cell_start,
                                                                    int32_t* items, hipStream_t s);

}   // namespace ovs
