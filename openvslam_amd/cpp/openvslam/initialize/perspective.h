// initialize::perspective (expected: src/openvslam/initialize/{base,perspective}.{h,cc}): the monocular initialiser's two-view geometry for a
// perspective camera. Upstream's constructor, initialize() and the four getters of initialize::base. initialize() is two device calls: the
// H and the F RANSAC with the choice between them (solve::find_homography_and_fundamental: ovs_twoview_solve_batch), then the
// chosen model's pose hypotheses, check_pose over every inlier match and find_most_plausible_pose (ovs_reconstruct_batch,
// csrc/two_view_reconstruct.hip) in place of reconstruct_with_H / reconstruct_with_F. No loop over matches runs on the host.
// Failure policy (util/device_policy.h): a device failure in either call means one retry on a rebuilt handle, then initialize() returns
// false -- "wait for the next frame", a state the initialiser is in on most frames anyway. Caller errors (a match that points past the
// keypoints, a camera that is not perspective) throw.
#pragma once
#include <ovslam_hip.h>

#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../data/frame_stub.h"
#include "../solve/fundamental_solver.h"
#include "../solve/homography_solver.h"
#include "../solve/ransac_context.h"

namespace openvslam {
namespace initialize {

class perspective {
public:
    //! upstream keeps the reference frame's camera, undistorted keypoints and bearings
    perspective(const data::frame& ref_frm, const unsigned int num_ransac_iters, const unsigned int min_num_triangulated, const float parallax_deg_thr,
                const float reproj_err_thr)
        : ref_camera_(ref_frm.camera_), ref_undist_keypts_(ref_frm.undist_keypts_), ref_bearings_(ref_frm.bearings_), num_ransac_iters_(num_ransac_iters),
          min_num_triangulated_(min_num_triangulated), parallax_deg_thr_(parallax_deg_thr), reproj_err_thr_(reproj_err_thr) {}

    void set_seed(const uint64_t seed) { seed_ = seed; }
    //! the HIP device both calls run on (process-wide; 0 unless an integration places the tracker elsewhere)
    static void set_device(const int device) {
        solve::two_view_solver::set_device(device);
        ctx().set_device(device);
    }

    //! ref_matches_with_cur[i]: the current frame's keypoint matched to the reference frame's keypoint i, or -1
    bool initialize(const data::frame& cur_frm, const std::vector<int>& ref_matches_with_cur) {
        for (double& v : rot_ref_to_cur_.m) v = 0.0;   // a failed initialisation leaves zeros, as the device call returns them
        trans_ref_to_cur_ = Vec3_t();
        triangulated_pts_.assign(ref_undist_keypts_.size(), Vec3_t());
        is_triangulated_.assign(ref_undist_keypts_.size(), false);
        if (ref_matches_with_cur.size() > ref_undist_keypts_.size()) throw std::invalid_argument("initialize::perspective: more matches than reference keypoints");
        if (!ref_camera_ || ref_camera_->model_type_ != camera::model_type_t::Perspective)
            throw std::invalid_argument("initialize::perspective: the reference frame's camera is not perspective");

        std::vector<std::pair<int, int>> ref_cur_matches;
        for (size_t ref_idx = 0; ref_idx < ref_matches_with_cur.size(); ++ref_idx)
            if (0 <= ref_matches_with_cur[ref_idx]) ref_cur_matches.emplace_back((int)ref_idx, ref_matches_with_cur[ref_idx]);

        // upstream: two threads, then rel_score_H > 0.40 chooses
        solve::homography_solver homography_solver(ref_undist_keypts_, cur_frm.undist_keypts_, ref_cur_matches, 1.0f);
        solve::fundamental_solver fundamental_solver(ref_undist_keypts_, cur_frm.undist_keypts_, ref_cur_matches, 1.0f);
        homography_solver.set_seed(seed_);
        fundamental_solver.set_seed(seed_);
        const int selected = solve::find_homography_and_fundamental(homography_solver, fundamental_solver, num_ransac_iters_);
        if (selected != 1 && selected != 2) return false;
        const Mat33_t model = selected == 1 ? homography_solver.get_best_H_21() : fundamental_solver.get_best_F_21();
        const std::vector<bool> is_inlier_match = selected == 1 ? homography_solver.get_inlier_matches() : fundamental_solver.get_inlier_matches();

        // upstream: reconstruct_with_H / reconstruct_with_F
        const int32_t n = (int32_t)ref_cur_matches.size();
        std::vector<uint8_t> inlier((size_t)n);
        std::vector<double> kp_ref(2 * (size_t)n), kp_cur(2 * (size_t)n), b_ref(3 * (size_t)n), b_cur(3 * (size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) {
            const size_t r = (size_t)ref_cur_matches[i].first, c = (size_t)ref_cur_matches[i].second;
            inlier[i] = is_inlier_match[i] ? 1 : 0;
            kp_ref[2 * i] = (double)ref_undist_keypts_[r].pt.x, kp_ref[2 * i + 1] = (double)ref_undist_keypts_[r].pt.y;
            kp_cur[2 * i] = (double)cur_frm.undist_keypts_.at(c).pt.x, kp_cur[2 * i + 1] = (double)cur_frm.undist_keypts_.at(c).pt.y;
            for (int k = 0; k < 3; ++k) b_ref[3 * i + (size_t)k] = ref_bearings_.at(r)(k), b_cur[3 * i + (size_t)k] = cur_frm.bearings_.at(c)(k);
        }
        ovs_camera cam{};
        cam.model = 0;
        cam.fx = ref_camera_->fx_, cam.fy = ref_camera_->fy_, cam.cx = ref_camera_->cx_, cam.cy = ref_camera_->cy_;
        const int32_t offsets[2] = {0, n}, models[1] = {selected};
        int32_t success = 0, best = -1, counts[8];
        float parallax[8];
        double rot[9], trans[3];
        std::vector<double> pts(3 * (size_t)std::max(n, 1));
        std::vector<uint8_t> flags((size_t)std::max(n, 1));
        const bool ran = ctx().run("ovs_reconstruct_batch", 1, n, [&](ovs_reconstruct* handle) {
            return ovs_reconstruct_batch(handle, 1, offsets, models, model.m, &cam, inlier.data(), kp_ref.data(), kp_cur.data(), b_ref.data(), b_cur.data(),
                                         reproj_err_thr_, parallax_deg_thr_, (int32_t)min_num_triangulated_, &success, &best, rot, trans, counts, parallax,
                                         pts.data(), flags.data());
        });
        if (!ran || !success) return false;
        for (int k = 0; k < 9; ++k) rot_ref_to_cur_.m[k] = rot[k];
        for (int k = 0; k < 3; ++k) trans_ref_to_cur_(k) = trans[k];
        for (size_t i = 0; i < (size_t)n; ++i) {   // upstream stores both by the reference frame's keypoint
            const size_t r = (size_t)ref_cur_matches[i].first;
            for (int k = 0; k < 3; ++k) triangulated_pts_[r](k) = pts[3 * i + (size_t)k];
            is_triangulated_[r] = flags[i] != 0;
        }
        return true;
    }

    // initialize::base's getters
    Mat33_t get_rotation_ref_to_cur() const { return rot_ref_to_cur_; }
    Vec3_t get_translation_ref_to_cur() const { return trans_ref_to_cur_; }
    std::vector<Vec3_t> get_triangulated_pts() const { return triangulated_pts_; }
    std::vector<bool> get_triangulated_flags() const { return is_triangulated_; }

private:
    using context = solve::ransac_context<ovs_reconstruct, ovs_reconstruct_create, ovs_reconstruct_destroy>;
    static context& ctx() {
        static context c;
        return c;
    }

    camera::base* const ref_camera_;
    const std::vector<cv::KeyPoint> ref_undist_keypts_;
    const std::vector<Vec3_t> ref_bearings_;
    const unsigned int num_ransac_iters_, min_num_triangulated_;
    const float parallax_deg_thr_, reproj_err_thr_;
    uint64_t seed_ = 0x48462D32ull;
    Mat33_t rot_ref_to_cur_;
    Vec3_t trans_ref_to_cur_;
    std::vector<Vec3_t> triangulated_pts_;
    std::vector<bool> is_triangulated_;
};

}   // namespace initialize
}   // namespace openvslam
