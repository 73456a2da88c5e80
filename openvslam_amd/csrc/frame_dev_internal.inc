// frame_dev_internal.inc -- what another unit of the library may read of a resident frame (ovs_frame_dev: match_window.hip owns the struct and
// defines this accessor). Not part of the C ABI: the symbol is hidden. (An .inc, not an .h: see solve_internal.inc.)
#pragma once
#include <cstdint>

struct ovs_frame_dev;

namespace ovs {

struct FrameDescriptors {
    int device, n;
    const uint8_t* d_desc;   // n x 32 bytes in device memory, 256-byte aligned
};
__attribute__((visibility("hidden"))) FrameDescriptors frame_descriptors(const ovs_frame_dev* f);

}   // namespace ovs
