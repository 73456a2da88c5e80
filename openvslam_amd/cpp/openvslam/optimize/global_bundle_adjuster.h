// optimize::global_bundle_adjuster (expected: src/openvslam/optimize/global_bundle_adjuster.h): bundle adjustment of the whole map, run by
// loop_bundle_adjuster after the pose graph and once after monocular initialisation. Every keyframe and landmark that is not to be erased is
// flattened as upstream hands them to g2o; the one optimisation round runs through ovs_global_ba_optimize (the reduced camera system by the
// one-workgroup Cholesky up to 170 free keyframes, by the conjugate gradient of csrc/ba_pcg.hip beyond); the result is written back as upstream
// writes it, directly for lead keyframe 0 and as the after-loop-BA values otherwise.
#pragma once
#include "../data/frame_stub.h"

namespace openvslam {
namespace optimize {

class global_bundle_adjuster {
public:
    explicit global_bundle_adjuster(data::map_database* map_db, const unsigned int num_iter = 10, const bool use_huber_kernel = true)
        : map_db_(map_db), num_iter_(num_iter), use_huber_kernel_(use_huber_kernel) {}
    virtual ~global_bundle_adjuster() = default;

    void optimize(const unsigned int lead_keyfrm_id_in_global_BA = 0, bool* const force_stop_flag = nullptr) const;

private:
    const data::map_database* map_db_;
    const unsigned int num_iter_;
    const bool use_huber_kernel_;
};

}   // namespace optimize
}   // namespace openvslam
