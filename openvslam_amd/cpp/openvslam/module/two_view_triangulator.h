// module::two_view_triangulator (expected: src/openvslam/module/two_view_triangulator.{h,cc}, with solve::triangulator of
// src/openvslam/solve/triangulator.h under it): the triangulation local_map_updater's create_new_landmarks runs on every pair that
// robust::match_for_triangulation returns. Upstream's constructor and triangulate(idx_1, idx_2, pos_w); the choice of the method by parallax,
// the two-view solution or the stereo back-projection and the three gates run on the device (ovs_triangulate_batch, csrc/triangulate.hip;
// DESIGN.md 3.12). triangulate(matches, ...) hands one neighbour's pairs to one call, triangulate_neighbours ALL neighbours of a new keyframe:
// one launch whatever their number.
// Failure policy (util/device_policy.h): a device failure means one retry on a rebuilt handle, then the empty result -- nothing accepted,
// so no landmark is created from this keyframe, a state upstream handles. Caller errors (an unknown camera model, ...) throw.
#pragma once
#include <ovs_detmath.h>
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../data/frame_stub.h"
#include "../match/window_ctx.h"
#include "../solve/ransac_context.h"

namespace openvslam {
namespace module {

class two_view_triangulator {
public:
    using match_list = std::vector<std::pair<unsigned int, unsigned int>>;   // (index in keyframe 1, index in keyframe 2)

    //! upstream's constructor
    explicit two_view_triangulator(data::keyframe* keyfrm_1, data::keyframe* keyfrm_2, const float rays_parallax_deg_thr = 1.0f)
        : keyfrm_1_(keyfrm_1), keyfrm_2_(keyfrm_2), rays_parallax_deg_thr_(rays_parallax_deg_thr) {}

    //! the HIP device the triangulator runs on (process-wide; 0 unless an integration places the mapping thread elsewhere)
    static void set_device(const int device) { ctx().set_device(device); }

    //! upstream: true when the pair gives a landmark, whose position is pos_w. A batch of one.
    bool triangulate(const unsigned int idx_1, const unsigned int idx_2, Vec3_t& pos_w) const {
        std::vector<Vec3_t> positions;
        std::vector<bool> accepted;
        triangulate(match_list(1, std::make_pair(idx_1, idx_2)), positions, accepted);
        pos_w = positions[0];
        return accepted[0];
    }

    //! every pair of this neighbour in ONE device call: positions[i] and accepted[i] are what triangulate(matches[i]) gives; returns the
    //! number accepted
    unsigned int triangulate(const match_list& matches, std::vector<Vec3_t>& positions, std::vector<bool>& accepted) const {
        std::vector<std::vector<Vec3_t>> pos;
        std::vector<std::vector<bool>> acc;
        const std::vector<unsigned int> num = triangulate_neighbours(keyfrm_1_, {keyfrm_2_}, {matches}, pos, acc, rays_parallax_deg_thr_);
        positions = std::move(pos[0]);
        accepted = std::move(acc[0]);
        return num[0];
    }

    //! create_new_landmarks' loop over the neighbours in ONE device call: matches_per_neighbour[k] pairs curr_keyfrm (first) with
    //! neighbours[k] (second). Returns the number accepted per neighbour.
    static std::vector<unsigned int> triangulate_neighbours(data::keyframe* curr_keyfrm, const std::vector<data::keyframe*>& neighbours,
                                                            const std::vector<match_list>& matches_per_neighbour,
                                                            std::vector<std::vector<Vec3_t>>& positions, std::vector<std::vector<bool>>& accepted,
                                                            const float rays_parallax_deg_thr = 1.0f) {
        const size_t K = neighbours.size();
        positions.assign(K, {});
        accepted.assign(K, {});
        std::vector<unsigned int> num_accepted(K, 0);
        if (K == 0) return num_accepted;
        std::vector<int32_t> offsets(1, 0);
        side s1, s2;
        std::vector<ovs_camera> cams_1, cams_2;
        std::vector<double> poses_1, poses_2;
        float scale_factor = curr_keyfrm->scale_factor_;
        for (size_t k = 0; k < K; ++k) {
            const match_list& matches = matches_per_neighbour.at(k);
            for (const auto& m : matches) {
                s1.push(*curr_keyfrm, m.first);
                s2.push(*neighbours[k], m.second);
            }
            positions[k].assign(matches.size(), Vec3_t());
            accepted[k].assign(matches.size(), false);
            offsets.push_back((int32_t)s1.x_right.size());
            cams_1.push_back(match::detail::camera_of(curr_keyfrm->camera_));
            cams_2.push_back(match::detail::camera_of(neighbours[k]->camera_));
            push_pose(curr_keyfrm->get_cam_pose(), poses_1);
            push_pose(neighbours[k]->get_cam_pose(), poses_2);
            scale_factor = std::max(scale_factor, neighbours[k]->scale_factor_);
        }
        const int32_t P = (int32_t)K, T = offsets.back();
        const double cos_rays_parallax_thr = ovs_det_cos((double)rays_parallax_deg_thr * 3.14159265358979323846 / 180.0);
        const float ratio_factor = 1.5f * scale_factor;
        std::vector<double> pos(3 * (size_t)std::max(T, 1));
        std::vector<uint8_t> status((size_t)std::max(T, 1)), method((size_t)std::max(T, 1));
        std::vector<int32_t> num((size_t)P);
        if (!ctx().run("ovs_triangulate_batch", P, T, [&](ovs_triangulate* handle) {
                return ovs_triangulate_batch(handle, P, offsets.data(), s1.bearings.data(), s2.bearings.data(), s1.keypts.data(), s2.keypts.data(),
                                             s1.x_right.data(), s2.x_right.data(), s1.depths.data(), s2.depths.data(), s1.sigma_sq.data(), s2.sigma_sq.data(),
                                             s1.scale_factors.data(), s2.scale_factors.data(), cams_1.data(), cams_2.data(), poses_1.data(), poses_2.data(),
                                             cos_rays_parallax_thr, ratio_factor, pos.data(), status.data(), method.data(), num.data());
            }))
            return num_accepted;   // nothing accepted: no landmark is created
        for (size_t k = 0; k < K; ++k) {
            num_accepted[k] = (unsigned int)num[k];
            for (int32_t i = offsets[k]; i < offsets[k + 1]; ++i) {
                const size_t j = (size_t)(i - offsets[k]);
                for (int x = 0; x < 3; ++x) positions[k][j](x) = pos[3 * (size_t)i + (size_t)x];
                accepted[k][j] = status[(size_t)i] == 0;
            }
        }
        return num_accepted;
    }

private:
    //! one side's per-match arrays of the ABI
    struct side {
        std::vector<double> bearings;
        std::vector<float> keypts, x_right, depths, sigma_sq, scale_factors;
        void push(const data::keyframe& keyfrm, const unsigned int idx) {
            const Vec3_t& b = keyfrm.bearings_.at(idx);
            const cv::KeyPoint& kp = keyfrm.undist_keypts_.at(idx);
            bearings.insert(bearings.end(), b.v, b.v + 3);
            keypts.push_back(kp.pt.x), keypts.push_back(kp.pt.y);
            const float xr = keyfrm.stereo_x_right_.empty() ? -1.0f : keyfrm.stereo_x_right_.at(idx);
            x_right.push_back(xr);
            depths.push_back(xr < 0.0f || keyfrm.depths_.empty() ? -1.0f : keyfrm.depths_.at(idx));
            sigma_sq.push_back(keyfrm.level_sigma_sq_.at((size_t)kp.octave));
            scale_factors.push_back(keyfrm.scale_factors_.at((size_t)kp.octave));
        }
    };
    static void push_pose(const Mat44_t& pose_cw, std::vector<double>& out) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) out.push_back(pose_cw(r, c));
        for (int r = 0; r < 3; ++r) out.push_back(pose_cw(r, 3));
    }

    using context = solve::ransac_context<ovs_triangulate, ovs_triangulate_create, ovs_triangulate_destroy>;
    static context& ctx() {
        static context c;
        return c;
    }

    data::keyframe* const keyfrm_1_;
    data::keyframe* const keyfrm_2_;
    const float rays_parallax_deg_thr_;
};

}   // namespace module
}   // namespace openvslam
