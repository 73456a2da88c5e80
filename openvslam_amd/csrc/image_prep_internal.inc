// image_prep_internal.inc -- the preparer's handle as the two units that use it see it: csrc/image_prep.hip (its own entries) and
// csrc/orb_api.hip (the fused entries, which stage the raw images in the handle's planes and prepare into the extractor's).
#pragma once
#include <mutex>

#include "ovs_common.h"
#include "owned_internal.inc"

struct ovs_imgprep {
    int device = 0, max_rows = 0, max_cols = 0;
    ovs::Owned res;
    std::mutex mu;
    hipStream_t stream = nullptr;
    // staging planes of the host forms, one per side: raw rows of src_pitch bytes (4 channels fit), prepared rows of out_pitch bytes
    size_t src_pitch = 0, out_pitch = 0;
    uint8_t *d_src[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    // the resident maps (rule I5), rows of map_pitch entries; map_rows x map_cols = 0 x 0: none set
    uint32_t* d_ixy[2] = {nullptr, nullptr};
    uint16_t* d_fxy[2] = {nullptr, nullptr};
    int map_rows = 0, map_cols = 0, map_pitch = 0, map_sides = 0;
};

namespace ovs {

// run_status (image_prep_plan.inc) against the handle's capacity and current map; sides: 1 or 2
ovs_status imgprep_check(const ovs_imgprep* p, int rows, int cols, size_t src_stride, int channels, int color_order, int rectify, int sides);
// the one launch: src / out of side 1 are null for one image. The arguments have passed imgprep_check and rows, cols >= 1; the caller holds p->mu
// where it uses the handle's planes
hipError_t imgprep_enqueue(const ovs_imgprep* p, const uint8_t* d_src_l, const uint8_t* d_src_r, int rows, int cols, size_t src_stride, int channels,
                           int color_order, int rectify, uint8_t* d_out_l, uint8_t* d_out_r, size_t out_stride, hipStream_t s);

}   // namespace ovs
