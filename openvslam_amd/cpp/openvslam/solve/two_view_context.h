// What solve::homography_solver and solve::fundamental_solver share: upstream's constructor and getters, the one ABI call under both
// (ovs_twoview_solve_batch, csrc/two_view_solve.hip) and the both-models call initialize::perspective::initialize makes in
// place of its two threads. Upstream draws its samples from random_device; here they are a function of (seed, position in the batch,
// hypothesis) and one sample serves both models, so a run is reproducible; set_seed changes it.
// Failure policy (util/device_policy.h): a device failure means one retry on a rebuilt handle, then solution_is_valid() == false and
// selected 0 -- the initialiser keeps waiting for a better frame, a state upstream handles. Caller errors (a match that points past the
// keypoints, a pair of solvers built from different matches) throw.
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../data/frame_stub.h"
#include "ransac_context.h"

namespace openvslam {
namespace solve {

class two_view_solver : protected ransac_result {
public:
    void set_seed(const uint64_t seed) { seed_ = seed; }
    //! the HIP device the solvers run on (process-wide; 0 unless an integration places the tracker elsewhere)
    static void set_device(const int device) { ctx().set_device(device); }

    void find_via_ransac(const unsigned int max_num_iter, const bool recompute = true) {
        reset();
        batch_out out(1, (int32_t)num_matches_);
        if (!call({this}, model_bit_, max_num_iter, recompute, out)) return;   // as reset() left it: solution_is_valid() == false
        take(out, 0, 0);
    }

    bool solution_is_valid() const { return solution_is_valid_; }
    double get_best_score() const { return best_score_; }
    //! per match, in the constructor's order
    std::vector<bool> get_inlier_matches() const { return is_inlier_match_; }
    unsigned int get_num_inliers() const { return num_inliers_; }
    int get_best_iter() const { return best_iter_; }   // the winning hypothesis, -1 without a valid solution

    //! both models of every (homography, fundamental) pair of solvers in ONE device call; pair i takes its samples as problem i under the
    //! FIRST homography solver's seed. Returns upstream's choice per pair: 1 the homography, 2 the fundamental matrix, 0 neither.
    static std::vector<int> find_both_via_ransac_batch(const std::vector<std::pair<two_view_solver*, two_view_solver*>>& pairs,
                                                       const unsigned int max_num_iter, const bool recompute = true) {
        std::vector<int> selected(pairs.size(), 0);
        if (pairs.empty()) return selected;
        std::vector<const two_view_solver*> src;
        int32_t T = 0;
        for (const auto& pr : pairs) {
            if (!pr.first || !pr.second || pr.first->model_bit_ != 1 || pr.second->model_bit_ != 2 || pr.first->x1_ != pr.second->x1_ ||
                pr.first->x2_ != pr.second->x2_ || pr.first->sigma_ != pr.second->sigma_ || pr.first->sigma_ != pairs.front().first->sigma_)
                throw std::invalid_argument("two_view_solver: a pair is a homography and a fundamental solver over the same matches and sigma");
            pr.first->reset();
            pr.second->reset();
            src.push_back(pr.first);
            T += (int32_t)pr.first->num_matches_;
        }
        batch_out out((int32_t)pairs.size(), T);
        if (!call(src, 3, max_num_iter, recompute, out)) return selected;
        for (size_t p = 0; p < pairs.size(); ++p) {
            pairs[p].first->take(out, (int32_t)p, out.offsets[p]);
            pairs[p].second->take(out, (int32_t)p, out.offsets[p]);
            selected[p] = out.selected[p];
        }
        return selected;
    }

protected:
    //! upstream: keeps the keypoints and the matches; here the matched keypoints, widened to double
    two_view_solver(const std::vector<cv::KeyPoint>& undist_keypts_1, const std::vector<cv::KeyPoint>& undist_keypts_2,
                    const std::vector<std::pair<int, int>>& matches_12, const float sigma, const int model_bit)
        : num_matches_((unsigned int)matches_12.size()), sigma_(sigma), model_bit_(model_bit) {
        for (const auto& m : matches_12) {
            const cv::KeyPoint& a = undist_keypts_1.at((size_t)m.first);
            const cv::KeyPoint& b = undist_keypts_2.at((size_t)m.second);
            x1_.push_back((double)a.pt.x);
            x1_.push_back((double)a.pt.y);
            x2_.push_back((double)b.pt.x);
            x2_.push_back((double)b.pt.y);
        }
        is_inlier_match_.assign(num_matches_, false);
    }

    Mat33_t best_;   // H_21 or F_21

private:
    //! the outputs of one ABI call
    struct batch_out {
        std::vector<int32_t> offsets, valid, best_iter, num_inliers, selected;
        std::vector<double> mat[2], scores;
        std::vector<uint8_t> flags[2];
        batch_out(const int32_t P, const int32_t T)
            : valid(2 * (size_t)P), best_iter(2 * (size_t)P), num_inliers(2 * (size_t)P), selected((size_t)P), scores(2 * (size_t)P) {
            for (int m = 0; m < 2; ++m) {
                mat[m].resize(9 * (size_t)P);
                flags[m].resize((size_t)std::max(T, 1));
            }
        }
    };

    void reset() {
        ransac_result::reset(num_matches_);
        best_score_ = 0.0;
        best_ = Mat33_t();
    }

    static bool call(const std::vector<const two_view_solver*>& src, const int models, const unsigned int max_num_iter, const bool recompute,
                     batch_out& out) {
        std::vector<double> x1, x2;
        out.offsets.assign(1, 0);
        for (const two_view_solver* s : src) {
            x1.insert(x1.end(), s->x1_.begin(), s->x1_.end());
            x2.insert(x2.end(), s->x2_.begin(), s->x2_.end());
            out.offsets.push_back(out.offsets.back() + (int32_t)s->num_matches_);
        }
        const int32_t P = (int32_t)src.size(), T = out.offsets.back();
        const two_view_solver& first = *src.front();
        return ctx().run("ovs_twoview_solve_batch", P, T, [&](ovs_twoview* handle) {
            return ovs_twoview_solve_batch(handle, P, out.offsets.data(), x1.data(), x2.data(), (double)first.sigma_,
                                           (int32_t)std::min<unsigned int>(max_num_iter, 1u << 30), recompute ? 1 : 0, first.seed_, models,
                                           out.mat[0].data(), out.mat[1].data(), out.scores.data(), out.valid.data(), out.best_iter.data(),
                                           out.num_inliers.data(), out.selected.data(), out.flags[0].data(), out.flags[1].data());
        });
    }

    //! this solver's model of problem p of a call, whose matches start at `offset`
    void take(const batch_out& out, const int32_t p, const int32_t offset) {
        const size_t m = (size_t)(model_bit_ - 1), k = 2 * (size_t)p + m;
        solution_is_valid_ = out.valid[k] != 0;
        best_iter_ = out.best_iter[k];
        num_inliers_ = (unsigned int)out.num_inliers[k];
        best_score_ = out.scores[k];
        for (int i = 0; i < 9; ++i) best_.m[i] = out.mat[m][9 * (size_t)p + (size_t)i];
        for (size_t i = 0; i < is_inlier_match_.size(); ++i) is_inlier_match_[i] = out.flags[m][(size_t)offset + i] != 0;
    }

    using context = ransac_context<ovs_twoview, ovs_twoview_create, ovs_twoview_destroy>;
    static context& ctx() {
        static context c;
        return c;
    }

    const unsigned int num_matches_;
    const float sigma_;
    const int model_bit_;   // 1: H, 2: F (the bit of the ABI's `models`)
    uint64_t seed_ = 0x48462D32ull;
    double best_score_ = 0.0;
    std::vector<double> x1_, x2_;   // 2 per match
};

}   // namespace solve
}   // namespace openvslam
