// optimize::global_bundle_adjuster through the class layer on a map.msg (tests/test_gpu_global_ba.py).
// usage: test_globalba_shim map.msg LEAD_ID out.bin [fail]
//   runs global_bundle_adjuster(&map_db, 10, true).optimize(LEAD_ID) on the loaded map and dumps, in ascending id, per keyframe the pose
//   (16 doubles), the after-loop-BA pose (16) and the loop-BA identifier (1), then per landmark the position (3), the after-global-BA
//   position (3) and the identifier (1). `fail`: every checked HIP call reports a failure while the class runs (ovs_debug_inject_hip_failures,
//   which makes calls REPORT failure; nothing faults): the policy of util/device_policy.h must leave the map as it was loaded.
#include <cstdio>
#include <cstdlib>
#include <string>

#include <ovslam_hip.h>

#include "openvslam/io/map_database_io.h"
#include "openvslam/optimize/global_bundle_adjuster.h"
#include "openvslam/util/device_policy.h"

using namespace openvslam;

int main(int argc, char** argv) {
    if (argc != 4 && !(argc == 5 && std::string(argv[4]) == "fail")) return 2;
    const bool fail = argc == 5;
    io::loaded_map m = io::map_database_io::load_message_pack(argv[1]);
    data::map_database map_db;
    for (const auto& kf : m.keyframes) map_db.keyframes_.push_back(kf.second.get());
    for (const auto& lm : m.landmarks) map_db.landmarks_.push_back(lm.second.get());
    for (const auto& kf : m.keyframes)
        for (int i = 0; i < 16; ++i) kf.second->cam_pose_cw_after_loop_BA_.m[i] = 0.0;
    for (const auto& lm : m.landmarks)
        for (int a = 0; a < 3; ++a) lm.second->pos_w_after_global_BA_.v[a] = 0.0;
    const unsigned int lead = (unsigned int)std::atoi(argv[2]);
    const unsigned long degraded0 = util::device_failures().degraded;
    if (fail) ovs_debug_inject_hip_failures(0, 1 << 30);
    try {
        optimize::global_bundle_adjuster(&map_db, 10, true).optimize(lead);
    } catch (const std::exception& e) {
        ovs_debug_inject_hip_failures(0, 0);
        std::printf("FAIL an exception reached the caller: %s\n", e.what());
        return 1;
    }
    ovs_debug_inject_hip_failures(0, 0);
    const unsigned long degraded = util::device_failures().degraded - degraded0;
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return 3;
    for (const auto& kf : m.keyframes) {
        const double id = kf.second->loop_BA_identifier_;
        std::fwrite(kf.second->cam_pose_cw_.m, sizeof(double), 16, f);
        std::fwrite(kf.second->cam_pose_cw_after_loop_BA_.m, sizeof(double), 16, f);
        std::fwrite(&id, sizeof(double), 1, f);
    }
    for (const auto& lm : m.landmarks) {
        const double id = lm.second->loop_BA_identifier_;
        std::fwrite(lm.second->pos_w_.v, sizeof(double), 3, f);
        std::fwrite(lm.second->pos_w_after_global_BA_.v, sizeof(double), 3, f);
        std::fwrite(&id, sizeof(double), 1, f);
    }
    std::fclose(f);
    std::printf("global ba shim ok: %zu keyframes, %zu landmarks, lead %u, degraded calls %lu\n", m.keyframes.size(), m.landmarks.size(), lead, degraded);
    return 0;
}
