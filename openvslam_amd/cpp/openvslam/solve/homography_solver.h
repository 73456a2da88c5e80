// solve::homography_solver (expected: src/openvslam/solve/homography_solver.{h,cc}): the RANSAC initialize::perspective::initialize runs on
// every frame until the map exists, beside solve::fundamental_solver. Upstream's constructor, find_via_ransac and getters; the RANSAC
// itself -- sampling, the normalised DLT on eight matches, the symmetric transfer test of every match under every hypothesis, the winner,
// the refit over its inliers -- runs on the device (ovs_twoview_solve_batch, csrc/two_view_solve.hip).
// find_homography_and_fundamental (fundamental_solver.h) computes both models in one call. Failure policy: two_view_context.h.
#pragma once
#include "two_view_context.h"

namespace openvslam {
namespace solve {

class homography_solver : public two_view_solver {
public:
    homography_solver(const std::vector<cv::KeyPoint>& undist_keypts_1, const std::vector<cv::KeyPoint>& undist_keypts_2,
                      const std::vector<std::pair<int, int>>& matches_12, const float sigma)
        : two_view_solver(undist_keypts_1, undist_keypts_2, matches_12, sigma, 1) {}

    Mat33_t get_best_H_21() const { return best_; }
};

}   // namespace solve
}   // namespace openvslam
