// optimize::transform_optimizer (expected: src/openvslam/optimize/transform_optimizer.{h,cc}): the Sim3 refinement loop_detector runs on every
// loop candidate after projection::match_by_Sim3_transform. Upstream's constructor and optimize; the optimisation itself -- the Sim3 vertex,
// two reprojection edges per match, two Levenberg-Marquardt rounds with Huber kernels and the chi-square classification -- runs on the device
// (ovs_sim3opt_optimize_batch, csrc/sim3_opt.hip). optimize_batch hands ALL candidates of a keyframe to one call: one launch
// whatever their number. No g2o type exists in this tree: Sim3_12 is (rot_12, trans_12, scale_12), as match::projection::
// match_keyframes_mutually takes it.
// Failure policy (util/device_policy.h): a device failure means one retry on a rebuilt handle, then 0 inliers with the transform and the
// matches untouched -- the loop detector drops the candidate, a state upstream handles. Caller errors (an unknown camera model, ...) throw.
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../data/frame_stub.h"
#include "../match/window_ctx.h"
#include "../solve/ransac_context.h"

namespace openvslam {
namespace optimize {

class transform_optimizer {
public:
    explicit transform_optimizer(const bool fix_scale, const unsigned int num_iter = 10) : fix_scale_(fix_scale), num_iter_(num_iter) {}

    //! one loop candidate of a batch: optimize's arguments; num_inliers is its return value
    struct candidate {
        data::keyframe *keyfrm_1, *keyfrm_2;
        std::vector<data::landmark*>* matched_lms_in_keyfrm_2;
        Mat33_t* rot_12;
        Vec3_t* trans_12;
        double* scale_12;
        unsigned int num_inliers = 0;
    };

    //! the HIP device the optimiser runs on (process-wide; 0 unless an integration places the loop closer elsewhere)
    static void set_device(const int device) { ctx().set_device(device); }

    //! upstream: returns the number of inliers, updates Sim3_12 and nulls the outliers in matched_lms_in_keyfrm_2. With fewer than 10
    //! survivors of the first round the result is 0 and Sim3_12 stays as it was (the outliers found so far are still nulled). A landmark
    //! position or keypoint that is not finite costs the candidate its first round (DESIGN.md 3.11 rule 8): usually 0 inliers.
    unsigned int optimize(data::keyframe* keyfrm_1, data::keyframe* keyfrm_2, std::vector<data::landmark*>& matched_lms_in_keyfrm_2, Mat33_t& rot_12,
                          Vec3_t& trans_12, double& scale_12, const float chi_sq) const {
        std::vector<candidate> one(1);
        one[0].keyfrm_1 = keyfrm_1, one[0].keyfrm_2 = keyfrm_2, one[0].matched_lms_in_keyfrm_2 = &matched_lms_in_keyfrm_2;
        one[0].rot_12 = &rot_12, one[0].trans_12 = &trans_12, one[0].scale_12 = &scale_12;
        optimize_batch(one, fix_scale_, num_iter_, chi_sq);
        return one[0].num_inliers;
    }

    //! every candidate of one loop query in ONE device call
    static void optimize_batch(std::vector<candidate>& candidates, const bool fix_scale, const unsigned int num_iter, const float chi_sq) {
        if (candidates.empty()) return;
        std::vector<int32_t> offsets(1, 0);
        std::vector<double> p1, p2, obs1, obs2, rot_in, trans_in, scale_in;
        std::vector<float> w1, w2;
        std::vector<unsigned int> idx1;   // per collected match: the keypoint index in keyfrm_1 (= the index into matched_lms_in_keyfrm_2)
        std::vector<ovs_camera> cams_1, cams_2;
        for (candidate& c : candidates) {
            c.num_inliers = 0;
            collect(c, p1, p2, obs1, obs2, w1, w2, idx1);
            offsets.push_back((int32_t)idx1.size());
            cams_1.push_back(match::detail::camera_of(c.keyfrm_1->camera_));
            cams_2.push_back(match::detail::camera_of(c.keyfrm_2->camera_));
            rot_in.insert(rot_in.end(), c.rot_12->m, c.rot_12->m + 9);
            trans_in.insert(trans_in.end(), c.trans_12->v, c.trans_12->v + 3);
            scale_in.push_back(*c.scale_12);
        }
        const int32_t P = (int32_t)candidates.size(), T = offsets.back();
        std::vector<int32_t> num((size_t)P);
        std::vector<double> rot(9 * (size_t)P), trans(3 * (size_t)P), scale((size_t)P);
        std::vector<uint8_t> outlier((size_t)std::max(T, 1));
        if (!ctx().run("ovs_sim3opt_optimize_batch", P, T, [&](ovs_sim3opt* handle) {
                return ovs_sim3opt_optimize_batch(handle, P, offsets.data(), p1.data(), p2.data(), obs1.data(), obs2.data(), w1.data(), w2.data(), cams_1.data(),
                                                  cams_2.data(), rot_in.data(), trans_in.data(), scale_in.data(), fix_scale ? 1 : 0, chi_sq,
                                                  (int32_t)std::min<unsigned int>(num_iter, 1u << 30), num.data(), rot.data(), trans.data(), scale.data(),
                                                  outlier.data(), nullptr);
            }))
            return;   // every candidate stays as it came: 0 inliers, the transform and the matches untouched
        for (int32_t p = 0; p < P; ++p) {
            candidate& c = candidates[(size_t)p];
            c.num_inliers = (unsigned int)num[(size_t)p];
            for (int i = 0; i < 9; ++i) c.rot_12->m[i] = rot[9 * (size_t)p + (size_t)i];
            for (int i = 0; i < 3; ++i) (*c.trans_12)(i) = trans[3 * (size_t)p + (size_t)i];
            *c.scale_12 = scale[(size_t)p];
            for (int32_t i = offsets[(size_t)p]; i < offsets[(size_t)p + 1]; ++i)
                if (outlier[(size_t)i]) c.matched_lms_in_keyfrm_2->at(idx1[(size_t)i]) = nullptr;
        }
    }

private:
    //! solve::sim3_solver's skip rules: for every keypoint idx1 of keyfrm_1 with a landmark and a matched landmark of keyfrm_2, neither about to be
    //! erased and both observed in their keyframe: both landmarks in their own keyframe's camera, the two keypoints, their inv_level_sigma_sq
    static void collect(const candidate& c, std::vector<double>& p1, std::vector<double>& p2, std::vector<double>& obs1, std::vector<double>& obs2,
                        std::vector<float>& w1, std::vector<float>& w2, std::vector<unsigned int>& idx1s) {
        const auto keyfrm_1_lms = c.keyfrm_1->get_landmarks();
        const auto& matched = *c.matched_lms_in_keyfrm_2;
        const Mat44_t pose_1w = c.keyfrm_1->get_cam_pose(), pose_2w = c.keyfrm_2->get_cam_pose();
        for (unsigned int idx1 = 0; idx1 < matched.size() && idx1 < keyfrm_1_lms.size(); ++idx1) {
            data::landmark* lm_1 = keyfrm_1_lms.at(idx1);
            data::landmark* lm_2 = matched.at(idx1);
            if (!lm_1 || !lm_2) continue;
            if (lm_1->will_be_erased() || lm_2->will_be_erased()) continue;
            const int idx_1 = lm_1->get_index_in_keyframe(c.keyfrm_1), idx_2 = lm_2->get_index_in_keyframe(c.keyfrm_2);
            if (idx_1 < 0 || idx_2 < 0) continue;
            const cv::KeyPoint& kp_1 = c.keyfrm_1->undist_keypts_.at(idx1);
            const cv::KeyPoint& kp_2 = c.keyfrm_2->undist_keypts_.at((size_t)idx_2);
            w1.push_back(c.keyfrm_1->inv_level_sigma_sq_.at((size_t)kp_1.octave));
            w2.push_back(c.keyfrm_2->inv_level_sigma_sq_.at((size_t)kp_2.octave));
            obs1.push_back((double)kp_1.pt.x), obs1.push_back((double)kp_1.pt.y);
            obs2.push_back((double)kp_2.pt.x), obs2.push_back((double)kp_2.pt.y);
            idx1s.push_back(idx1);
            push_in_camera(pose_1w, lm_1->get_pos_in_world(), p1);
            push_in_camera(pose_2w, lm_2->get_pos_in_world(), p2);
        }
    }
    static void push_in_camera(const Mat44_t& pose_cw, const Vec3_t& pos_w, std::vector<double>& out) {
        for (int r = 0; r < 3; ++r) out.push_back(((pose_cw(r, 0) * pos_w(0) + pose_cw(r, 1) * pos_w(1)) + pose_cw(r, 2) * pos_w(2)) + pose_cw(r, 3));
    }

    using context = solve::ransac_context<ovs_sim3opt, ovs_sim3opt_create, ovs_sim3opt_destroy>;
    static context& ctx() {
        static context c;
        return c;
    }

    const bool fix_scale_;
    const unsigned int num_iter_;
};

}   // namespace optimize
}   // namespace openvslam
