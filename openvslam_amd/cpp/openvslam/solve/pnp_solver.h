// solve::pnp_solver (expected: src/openvslam/solve/pnp_solver.{h,cc}): the RANSAC module::relocalizer runs on every candidate keyframe
// between bow_tree::match_frame_and_keyframe and optimize::pose_optimizer. Upstream's constructor, find_via_ransac and getters; the RANSAC
// itself -- sampling, EPnP on four matches, the cosine test of every match under every hypothesis, the winner, the refit over its
// inliers -- runs on the device (ovs_pnp_solve_batch, csrc/pnp_solve.hip). find_via_ransac_batch hands ALL candidates of a
// frame to one call: two launches whatever their number. Upstream draws its samples from random_device; here they are a function of
// (seed, position in the batch, hypothesis), so a run is reproducible; set_seed changes it.
// Failure policy (util/device_policy.h): a device failure means one retry on a rebuilt handle, then solution_is_valid() == false -- the
// relocaliser drops the candidate, a state upstream handles. Caller errors (bearings and landmarks of different lengths, an octave without
// a scale factor) throw.
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../data/frame_stub.h"
#include "ransac_context.h"

namespace openvslam {
namespace solve {

class pnp_solver : private ransac_result {
public:
    //! upstream: keeps the bearings and the landmarks and max_cos_errors_ = cos(scale_factors[octave] * 1 degree) per keypoint
    //! (eigen_alloc_vector<Vec3_t> upstream; std::vector here)
    pnp_solver(const std::vector<Vec3_t>& valid_bearings, const std::vector<cv::KeyPoint>& valid_keypts, const std::vector<Vec3_t>& valid_landmarks,
               const std::vector<float>& scale_factors, const unsigned int min_num_inliers = 10)
        : num_matches_((unsigned int)valid_bearings.size()), min_num_inliers_(min_num_inliers) {
        if (valid_keypts.size() != valid_bearings.size() || valid_landmarks.size() != valid_bearings.size())
            throw std::invalid_argument("pnp_solver: bearings, keypoints and landmarks must have one entry per match");
        constexpr double deg = 3.14159265358979323846 / 180.0;
        for (unsigned int i = 0; i < num_matches_; ++i) {
            for (int x = 0; x < 3; ++x) {
                valid_bearings_.push_back(valid_bearings[i](x));
                valid_landmarks_.push_back(valid_landmarks[i](x));
            }
            max_cos_errors_.push_back(std::cos((double)scale_factors.at((size_t)valid_keypts[i].octave) * deg));
        }
        is_inlier_match_.assign(num_matches_, false);
    }

    void set_seed(const uint64_t seed) { seed_ = seed; }
    //! the HIP device the solvers run on (process-wide; 0 unless an integration places the tracker elsewhere)
    static void set_device(const int device) { ctx().set_device(device); }

    void find_via_ransac(const unsigned int max_num_iter, const bool recompute = true) { find_via_ransac_batch({this}, max_num_iter, recompute); }

    //! every candidate of one relocalisation in ONE device call. The solvers must agree on min_num_inliers; solver i takes its samples as
    //! problem i under the FIRST solver's seed
    static void find_via_ransac_batch(const std::vector<pnp_solver*>& solvers, const unsigned int max_num_iter, const bool recompute = true) {
        if (solvers.empty()) return;
        const pnp_solver& first = *solvers.front();
        std::vector<int32_t> offsets(1, 0);
        std::vector<double> bearings, pos_w, max_cos, rot(9 * solvers.size()), trans(3 * solvers.size());
        for (pnp_solver* s : solvers) {
            if (s->min_num_inliers_ != first.min_num_inliers_)
                throw std::invalid_argument("pnp_solver: the solvers of a batch must share min_num_inliers");
            s->reset();
            bearings.insert(bearings.end(), s->valid_bearings_.begin(), s->valid_bearings_.end());
            pos_w.insert(pos_w.end(), s->valid_landmarks_.begin(), s->valid_landmarks_.end());
            max_cos.insert(max_cos.end(), s->max_cos_errors_.begin(), s->max_cos_errors_.end());
            offsets.push_back(offsets.back() + (int32_t)s->num_matches_);
        }
        const int32_t P = (int32_t)solvers.size(), T = offsets.back();
        ransac_batch_out out(P, T);
        if (!ctx().run("ovs_pnp_solve_batch", P, T, [&](ovs_pnp* handle) {
                return ovs_pnp_solve_batch(handle, P, offsets.data(), bearings.data(), pos_w.data(), max_cos.data(), (int32_t)first.min_num_inliers_,
                                           (int32_t)std::min<unsigned int>(max_num_iter, 1u << 30), recompute ? 1 : 0, first.seed_, out.valid.data(),
                                           out.best_iter.data(), out.num_inliers.data(), rot.data(), trans.data(), out.flags.data());
            }))
            return;   // every solver stays as reset() left it: solution_is_valid() == false
        for (int32_t p = 0; p < P; ++p) {
            pnp_solver& s = *solvers[(size_t)p];
            s.take(out, p, offsets[(size_t)p]);
            for (int i = 0; i < 9; ++i) s.best_rot_cw_.m[i] = rot[9 * (size_t)p + (size_t)i];
            for (int i = 0; i < 3; ++i) s.best_trans_cw_(i) = trans[3 * (size_t)p + (size_t)i];
        }
    }

    bool solution_is_valid() const { return solution_is_valid_; }
    Mat33_t get_best_rotation() const { return best_rot_cw_; }
    Vec3_t get_best_translation() const { return best_trans_cw_; }
    Mat44_t get_best_cam_pose() const {
        Mat44_t pose;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) pose(r, c) = best_rot_cw_(r, c);
            pose(r, 3) = best_trans_cw_(r);
        }
        return pose;
    }
    //! per match, in the constructor's order
    std::vector<bool> get_inlier_flags() const { return is_inlier_match_; }
    unsigned int get_num_inliers() const { return num_inliers_; }
    int get_best_iter() const { return best_iter_; }   // the winning hypothesis, -1 without a valid solution

private:
    void reset() {
        ransac_result::reset(num_matches_);
        best_rot_cw_ = Mat33_t();
        best_trans_cw_ = Vec3_t();
    }

    using context = ransac_context<ovs_pnp, ovs_pnp_create, ovs_pnp_destroy>;
    static context& ctx() {
        static context c;
        return c;
    }

    const unsigned int num_matches_, min_num_inliers_;
    uint64_t seed_ = 0x45506E50ull;
    std::vector<double> valid_bearings_, valid_landmarks_;   // 3 per match
    std::vector<double> max_cos_errors_;
    Mat33_t best_rot_cw_;
    Vec3_t best_trans_cw_;
};

}   // namespace solve
}   // namespace openvslam
