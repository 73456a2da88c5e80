// solve::sim3_solver (expected: src/openvslam/solve/sim3_solver.{h,cc}): the RANSAC loop_detector runs on every loop candidate between
// bow_tree::match_keyframes and projection::match_by_Sim3_transform. Upstream's constructor, find_via_ransac and getters; the RANSAC
// itself -- sampling, Horn's closed form, both reprojections of every match under every hypothesis, the winner -- runs on the device
// (ovs_sim3_solve_batch, csrc/sim3_solve.hip). find_via_ransac_batch hands ALL candidates of a keyframe to one call: two
// launches whatever their number. Upstream draws its samples from random_device; here they are a function of (seed, position in the
// batch, hypothesis), so a run is reproducible; set_seed changes it.
// Failure policy (util/device_policy.h): a device failure means one retry on a rebuilt handle, then solution_is_valid() == false -- the loop
// detector drops the candidate, a state upstream handles. Caller errors (an unknown camera model, ...) throw.
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../data/frame_stub.h"
#include "../match/window_ctx.h"
#include "ransac_context.h"

namespace openvslam {
namespace solve {

class sim3_solver : private ransac_result {
public:
    //! upstream: collects, for every keypoint idx1 of keyfrm_1 with a landmark and a matched landmark of keyfrm_2, both landmarks in their own
    //! keyframe's camera coordinates and 9.21 * level_sigma_sq of the two keypoints' octaves
    sim3_solver(data::keyframe* keyfrm_1, data::keyframe* keyfrm_2, const std::vector<data::landmark*>& matched_lms_in_keyfrm_2,
                const bool fix_scale = true, const unsigned int min_num_inliers = 20)
        : keyfrm_1_(keyfrm_1), keyfrm_2_(keyfrm_2), fix_scale_(fix_scale), min_num_inliers_(min_num_inliers) {
        const auto keyfrm_1_lms = keyfrm_1->get_landmarks();
        const Mat44_t pose_1w = keyfrm_1->get_cam_pose(), pose_2w = keyfrm_2->get_cam_pose();
        for (unsigned int idx1 = 0; idx1 < matched_lms_in_keyfrm_2.size() && idx1 < keyfrm_1_lms.size(); ++idx1) {
            data::landmark* lm_1 = keyfrm_1_lms.at(idx1);
            data::landmark* lm_2 = matched_lms_in_keyfrm_2.at(idx1);
            if (!lm_1 || !lm_2) continue;
            if (lm_1->will_be_erased() || lm_2->will_be_erased()) continue;
            const int idx_1 = lm_1->get_index_in_keyframe(keyfrm_1), idx_2 = lm_2->get_index_in_keyframe(keyfrm_2);
            if (idx_1 < 0 || idx_2 < 0) continue;
            const float sigma_sq_1 = keyfrm_1->level_sigma_sq_.at((size_t)keyfrm_1->undist_keypts_.at((size_t)idx_1).octave);
            const float sigma_sq_2 = keyfrm_2->level_sigma_sq_.at((size_t)keyfrm_2->undist_keypts_.at((size_t)idx_2).octave);
            chi_sq_x_sigma_sq_1_.push_back((float)(9.21 * sigma_sq_1));
            chi_sq_x_sigma_sq_2_.push_back((float)(9.21 * sigma_sq_2));
            matched_indices_1_.push_back(idx1);
            push_in_camera(pose_1w, lm_1->get_pos_in_world(), common_pts_in_keyfrm_1_);
            push_in_camera(pose_2w, lm_2->get_pos_in_world(), common_pts_in_keyfrm_2_);
        }
        num_common_pts_ = (unsigned int)matched_indices_1_.size();
        is_inlier_match_.assign(num_common_pts_, false);
    }

    void set_seed(const uint64_t seed) { seed_ = seed; }
    //! the HIP device the solvers run on (process-wide; 0 unless an integration places the loop closer elsewhere)
    static void set_device(const int device) { ctx().set_device(device); }

    void find_via_ransac(const unsigned int max_num_iter) { find_via_ransac_batch({this}, max_num_iter); }

    //! every candidate of one loop query in ONE device call. The solvers must agree on fix_scale and min_num_inliers; solver i takes its
    //! samples as problem i under the FIRST solver's seed
    static void find_via_ransac_batch(const std::vector<sim3_solver*>& solvers, const unsigned int max_num_iter) {
        if (solvers.empty()) return;
        const sim3_solver& first = *solvers.front();
        std::vector<int32_t> offsets(1, 0);
        std::vector<double> p1, p2, rot(9 * solvers.size()), trans(3 * solvers.size()), scale(solvers.size());
        std::vector<float> thr1, thr2;
        std::vector<ovs_camera> cams_1, cams_2;
        for (sim3_solver* s : solvers) {
            if (s->fix_scale_ != first.fix_scale_ || s->min_num_inliers_ != first.min_num_inliers_)
                throw std::invalid_argument("sim3_solver: the solvers of a batch must share fix_scale and min_num_inliers");
            s->reset();
            p1.insert(p1.end(), s->common_pts_in_keyfrm_1_.begin(), s->common_pts_in_keyfrm_1_.end());
            p2.insert(p2.end(), s->common_pts_in_keyfrm_2_.begin(), s->common_pts_in_keyfrm_2_.end());
            thr1.insert(thr1.end(), s->chi_sq_x_sigma_sq_1_.begin(), s->chi_sq_x_sigma_sq_1_.end());
            thr2.insert(thr2.end(), s->chi_sq_x_sigma_sq_2_.begin(), s->chi_sq_x_sigma_sq_2_.end());
            offsets.push_back(offsets.back() + (int32_t)s->num_common_pts_);
            cams_1.push_back(match::detail::camera_of(s->keyfrm_1_->camera_));
            cams_2.push_back(match::detail::camera_of(s->keyfrm_2_->camera_));
        }
        const int32_t P = (int32_t)solvers.size(), T = offsets.back();
        ransac_batch_out out(P, T);
        if (!ctx().run("ovs_sim3_solve_batch", P, T, [&](ovs_sim3* handle) {
                return ovs_sim3_solve_batch(handle, P, offsets.data(), p1.data(), p2.data(), thr1.data(), thr2.data(), cams_1.data(), cams_2.data(),
                                            first.fix_scale_ ? 1 : 0, (int32_t)first.min_num_inliers_, (int32_t)std::min<unsigned int>(max_num_iter, 1u << 30),
                                            first.seed_, out.valid.data(), out.best_iter.data(), out.num_inliers.data(), rot.data(), trans.data(),
                                            scale.data(), out.flags.data());
            }))
            return;   // every solver stays as reset() left it: solution_is_valid() == false
        for (int32_t p = 0; p < P; ++p) {
            sim3_solver& s = *solvers[(size_t)p];
            s.take(out, p, offsets[(size_t)p]);
            for (int i = 0; i < 9; ++i) s.best_rot_12_.m[i] = rot[9 * (size_t)p + (size_t)i];
            for (int i = 0; i < 3; ++i) s.best_trans_12_(i) = trans[3 * (size_t)p + (size_t)i];
            s.best_scale_12_ = scale[(size_t)p];
        }
    }

    bool solution_is_valid() const { return solution_is_valid_; }
    Mat33_t get_best_rotation_12() const { return best_rot_12_; }
    Vec3_t get_best_translation_12() const { return best_trans_12_; }
    float get_best_scale_12() const { return (float)best_scale_12_; }
    //! per collected pair, in the order of get_matched_indices_1()
    std::vector<bool> get_inlier_flags() const { return is_inlier_match_; }
    //! the keypoint index in keyfrm_1 (= the index into matched_lms_in_keyfrm_2) of every collected pair
    std::vector<unsigned int> get_matched_indices_1() const { return matched_indices_1_; }
    unsigned int get_num_inliers() const { return num_inliers_; }
    int get_best_iter() const { return best_iter_; }   // the winning hypothesis, -1 without a valid solution

private:
    static void push_in_camera(const Mat44_t& pose_cw, const Vec3_t& pos_w, std::vector<double>& out) {
        for (int r = 0; r < 3; ++r) out.push_back(((pose_cw(r, 0) * pos_w(0) + pose_cw(r, 1) * pos_w(1)) + pose_cw(r, 2) * pos_w(2)) + pose_cw(r, 3));
    }
    void reset() {
        ransac_result::reset(num_common_pts_);
        best_rot_12_ = Mat33_t();
        best_trans_12_ = Vec3_t();
        best_scale_12_ = 1.0;
    }

    using context = ransac_context<ovs_sim3, ovs_sim3_create, ovs_sim3_destroy>;
    static context& ctx() {
        static context c;
        return c;
    }

    data::keyframe *keyfrm_1_, *keyfrm_2_;
    const bool fix_scale_;
    const unsigned int min_num_inliers_;
    uint64_t seed_ = 0x53696D33ull;
    unsigned int num_common_pts_ = 0;
    std::vector<double> common_pts_in_keyfrm_1_, common_pts_in_keyfrm_2_;   // 3 per pair
    std::vector<float> chi_sq_x_sigma_sq_1_, chi_sq_x_sigma_sq_2_;
    std::vector<unsigned int> matched_indices_1_;
    Mat33_t best_rot_12_;
    Vec3_t best_trans_12_;
    double best_scale_12_ = 1.0;
};

}   // namespace solve
}   // namespace openvslam
