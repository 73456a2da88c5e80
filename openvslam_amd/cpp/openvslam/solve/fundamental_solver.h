// solve::fundamental_solver (expected: src/openvslam/solve/fundamental_solver.{h,cc}): the RANSAC initialize::perspective::initialize runs on
// every frame until the map exists, beside solve::homography_solver. Upstream's constructor, find_via_ransac and getters; the RANSAC
// itself -- sampling, the normalised eight-point algorithm with the rank-two step, the epipolar test of every match under every
// hypothesis, the winner, the refit over its inliers -- runs on the device (ovs_twoview_solve_batch, csrc/two_view_solve.hip; DESIGN.md
// 3.13). Failure policy: two_view_context.h.
#pragma once
#include "homography_solver.h"
#include "two_view_context.h"

namespace openvslam {
namespace solve {

class fundamental_solver : public two_view_solver {
public:
    fundamental_solver(const std::vector<cv::KeyPoint>& undist_keypts_1, const std::vector<cv::KeyPoint>& undist_keypts_2,
                       const std::vector<std::pair<int, int>>& matches_12, const float sigma)
        : two_view_solver(undist_keypts_1, undist_keypts_2, matches_12, sigma, 2) {}

    Mat33_t get_best_F_21() const { return best_; }
};

//! what initialize::perspective::initialize calls in place of its two threads: both RANSACs in ONE device call (two launches), with
//! upstream's choice between the models as the return value: 1 the homography, 2 the fundamental matrix, 0 neither is valid. Both
//! solvers are built from the same keypoints, matches and sigma. (A caller with several frame pairs: two_view_solver::find_both_via_ransac_batch.)
inline int find_homography_and_fundamental(homography_solver& h, fundamental_solver& f, const unsigned int max_num_iter, const bool recompute = true) {
    return two_view_solver::find_both_via_ransac_batch({{&h, &f}}, max_num_iter, recompute).front();
}

}   // namespace solve
}   // namespace openvslam
