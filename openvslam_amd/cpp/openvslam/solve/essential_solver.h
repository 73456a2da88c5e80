// solve::essential_solver (expected: src/openvslam/solve/essential_solver.{h,cc}): the bearing-vector eight-point RANSAC
// match::robust::match_frame_and_keyframe runs after its brute-force match. Upstream's constructor (two bearing vectors and the matches),
// find_via_ransac and getters; the RANSAC itself -- sampling, the eight-point null vector with the rank-two step, the epipolar-plane test
// of every match under every hypothesis, the winner, the refit over its inliers -- runs on the device (ovs_essential_solve_batch,
// csrc/essential_solve.hip). Upstream draws its samples from random_device; here they are a function of (seed, position
// in the batch, hypothesis), so a run is reproducible; set_seed changes it. find_via_ransac_batch solves several solvers in ONE call.
// Failure policy (util/device_policy.h): a device failure means one retry on a rebuilt handle, then solution_is_valid() == false -- the
// caller sees zero inlier matches, a state upstream handles. A match that points past its bearing vector throws (std::out_of_range).
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../data/frame_stub.h"
#include "ransac_context.h"

namespace openvslam {
namespace solve {

class essential_solver : protected ransac_result {
public:
    //! upstream keeps references to the bearings and the matches; here the matched bearings are gathered once
    essential_solver(const std::vector<Vec3_t>& bearings_1, const std::vector<Vec3_t>& bearings_2, const std::vector<std::pair<int, int>>& matches_12)
        : num_matches_((unsigned int)matches_12.size()) {
        b1_.reserve(3 * matches_12.size());
        b2_.reserve(3 * matches_12.size());
        for (const auto& m : matches_12) {
            const Vec3_t& a = bearings_1.at((size_t)m.first);
            const Vec3_t& b = bearings_2.at((size_t)m.second);
            for (int k = 0; k < 3; ++k) {
                b1_.push_back(a(k));
                b2_.push_back(b(k));
            }
        }
        is_inlier_match_.assign(num_matches_, false);
    }

    void set_seed(const uint64_t seed) { seed_ = seed; }
    //! upstream's constant (the float 0.01745240643f: one degree) unless set
    void set_residual_cos_thr(const double thr) { residual_cos_thr_ = thr; }
    //! the HIP device the solvers run on (process-wide; 0 unless an integration places the tracker elsewhere)
    static void set_device(const int device) { ctx().set_device(device); }

    void find_via_ransac(const unsigned int max_num_iter, const bool recompute = true) { find_via_ransac_batch({this}, max_num_iter, recompute); }

    //! every solver's RANSAC in ONE device call; solver i takes its samples as problem i under the FIRST solver's seed and threshold
    static void find_via_ransac_batch(const std::vector<essential_solver*>& solvers, const unsigned int max_num_iter, const bool recompute = true) {
        if (solvers.empty()) return;
        std::vector<int32_t> offsets(1, 0);
        std::vector<double> b1, b2;
        for (essential_solver* s : solvers) {
            s->reset();
            b1.insert(b1.end(), s->b1_.begin(), s->b1_.end());
            b2.insert(b2.end(), s->b2_.begin(), s->b2_.end());
            offsets.push_back(offsets.back() + (int32_t)s->num_matches_);
        }
        const int32_t P = (int32_t)solvers.size(), T = offsets.back();
        ransac_batch_out out(P, T);
        std::vector<double> E(9 * (size_t)P), scores((size_t)P);
        const essential_solver& first = *solvers.front();
        if (!ctx().run("ovs_essential_solve_batch", P, T, [&](ovs_essential* handle) {
                return ovs_essential_solve_batch(handle, P, offsets.data(), b1.data(), b2.data(), first.residual_cos_thr_,
                                                 (int32_t)std::min<unsigned int>(max_num_iter, 1u << 30), recompute ? 1 : 0, first.seed_, E.data(),
                                                 scores.data(), out.valid.data(), out.best_iter.data(), out.num_inliers.data(), out.flags.data());
            }))
            return;   // as reset() left them: solution_is_valid() == false
        for (int32_t p = 0; p < P; ++p) {
            essential_solver& s = *solvers[(size_t)p];
            s.take(out, p, offsets[(size_t)p]);
            s.best_score_ = scores[(size_t)p];
            for (int i = 0; i < 9; ++i) s.best_E_21_.m[i] = E[9 * (size_t)p + (size_t)i];
        }
    }

    bool solution_is_valid() const { return solution_is_valid_; }
    double get_best_score() const { return best_score_; }
    Mat33_t get_best_E_21() const { return best_E_21_; }
    //! per match, in the constructor's order
    std::vector<bool> get_inlier_matches() const { return is_inlier_match_; }
    unsigned int get_num_inliers() const { return num_inliers_; }
    int get_best_iter() const { return best_iter_; }   // the winning hypothesis, -1 without a valid solution

private:
    void reset() {
        ransac_result::reset(num_matches_);
        best_score_ = 0.0;
        best_E_21_ = Mat33_t();
    }

    using context = ransac_context<ovs_essential, ovs_essential_create, ovs_essential_destroy>;
    static context& ctx() {
        static context c;
        return c;
    }

    const unsigned int num_matches_;
    uint64_t seed_ = 0x45737365ull;
    double residual_cos_thr_ = (double)0.01745240643f;
    double best_score_ = 0.0;
    Mat33_t best_E_21_;
    std::vector<double> b1_, b2_;   // 3 per match
};

}   // namespace solve
}   // namespace openvslam
