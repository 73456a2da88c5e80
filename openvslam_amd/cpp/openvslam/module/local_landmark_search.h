// module::search_local_landmarks: the body of tracking_module::search_local_landmarks() (expected: src/openvslam/tracking_module.cc) after its
// margin choice. Upstream marks the landmarks the frame already holds, runs frame::can_observe(lm, 0.5, ...) on every other local landmark on
// the host and hands the survivors to projection::match_frame_and_landmarks. Here the first loop and the flattening stay on the host; can_observe
// and the matcher are ONE device call (ovs_tracking_search_local_landmarks_f, csrc/match_window.hip) on the resident frame.
// reproj_in_tracking_ / x_right_in_tracking_ / scale_level_in_tracking_ have one reader, the matcher, which has already run inside the call:
// they are fetched and written only when write_tracking_fields is set.
// Failure policy (util/device_policy.h): a device failure means one retry, then 0 matches -- frm.landmarks_ untouched, every
// local landmark is_observable_in_tracking_ = false, no count raised by the second loop.
#pragma once
#include <ovslam_hip.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../data/frame_stub.h"
#include "../match/window_ctx.h"

namespace openvslam {
namespace module {

inline unsigned int search_local_landmarks(data::frame& curr_frm, const std::vector<data::landmark*>& local_landmarks, const float margin,
                                           const float lowe_ratio = 0.8f, const bool write_tracking_fields = false) {
    namespace detail = match::detail;
    // upstream's first loop: what the frame already holds is not searched again
    for (auto* lm : curr_frm.landmarks_) {
        if (!lm || lm->will_be_erased()) continue;
        lm->is_observable_in_tracking_ = false;
        lm->identifier_in_local_lm_search_ = curr_frm.id_;
        lm->increase_num_observable();
    }
    const int n = (int)curr_frm.num_keypts_, m = (int)local_landmarks.size();
    if (m == 0) return 0;
    std::vector<double>&pos = detail::scratch_vec<double>(0, (size_t)3 * m), &normal = detail::scratch_vec<double>(1, (size_t)3 * m),
                        &reproj = detail::scratch_vec<double>(2, write_tracking_fields ? (size_t)2 * m : 0);
    std::vector<float>&dist = detail::scratch_vec<float>(0, (size_t)2 * m), &x_right = detail::scratch_vec<float>(1, write_tracking_fields ? (size_t)m : 0);
    std::vector<uint8_t>&search = detail::scratch_vec<uint8_t>(0, (size_t)m), &desc = detail::scratch_vec<uint8_t>(1, (size_t)32 * m),
                         &occupied = detail::scratch_vec<uint8_t>(2, (size_t)n), &observable = detail::scratch_vec<uint8_t>(3, (size_t)m);
    std::vector<int32_t>&assigned = detail::scratch_vec<int32_t>(1, (size_t)m), &level = detail::scratch_vec<int32_t>(0, write_tracking_fields ? (size_t)m : 0);
    for (int l = 0; l < m; ++l) {
        const auto* lm = local_landmarks[l];
        search[l] = lm && !lm->will_be_erased() && lm->identifier_in_local_lm_search_ != curr_frm.id_;
        if (!search[l]) {   // defined values for an entry the kernel skips (the staging vectors keep earlier calls' contents)
            for (int a = 0; a < 3; ++a) pos[(size_t)3 * l + a] = normal[(size_t)3 * l + a] = 0.0;
            dist[2 * l] = dist[2 * l + 1] = 0.0f;
            continue;
        }
        const Vec3_t pos_w = lm->get_pos_in_world(), mean_normal = lm->get_obs_mean_normal();
        for (int a = 0; a < 3; ++a) {
            pos[(size_t)3 * l + a] = pos_w(a);
            normal[(size_t)3 * l + a] = mean_normal(a);
        }
        dist[2 * l] = lm->min_valid_dist_;   // the RAW members: the device applies the getters' widening
        dist[2 * l + 1] = lm->max_valid_dist_;
        const cv::Mat d = lm->get_descriptor();
        std::memcpy(&desc[(size_t)32 * l], d.data, 32);
    }
    for (int i = 0; i < n; ++i) occupied[i] = curr_frm.landmarks_[i] && curr_frm.landmarks_[i]->has_observation();
    int32_t num_observable = 0, num_matches = 0;
    const ovs_camera cam = detail::camera_of(curr_frm.camera_);
    double pose[12];
    detail::pose12(curr_frm.cam_pose_cw_, pose);
    const int device = detail::device_of(curr_frm);
    if (!detail::guarded("ovs_tracking_search_local_landmarks_f", [&] {
            const auto h = detail::device_handle_of(curr_frm);
            return ovs_tracking_search_local_landmarks_f(detail::window_ctx(device).get(n, m), &cam, detail::dev(h), occupied.data(), pose, pos.data(), dist.data(),
                                                         normal.data(), desc.data(), search.data(), m, curr_frm.scale_factors_.data(),
                                                         (int)curr_frm.scale_factors_.size(), curr_frm.log_scale_factor_, margin, lowe_ratio, observable.data(),
                                                         write_tracking_fields ? reproj.data() : nullptr, write_tracking_fields ? x_right.data() : nullptr,
                                                         write_tracking_fields ? level.data() : nullptr, assigned.data(), &num_observable, &num_matches);
        }, {curr_frm.device_cache_.get()}, device)) {
        for (auto* lm : local_landmarks)
            if (lm) lm->is_observable_in_tracking_ = false;
        return 0;
    }
    // upstream's second loop, from the device's verdicts
    for (int l = 0; l < m; ++l) {
        if (!search[l]) continue;
        auto* lm = local_landmarks[l];
        lm->is_observable_in_tracking_ = observable[l] != 0;
        if (!observable[l]) continue;
        lm->increase_num_observable();
        if (write_tracking_fields) {
            lm->reproj_in_tracking_(0) = reproj[(size_t)2 * l];
            lm->reproj_in_tracking_(1) = reproj[(size_t)2 * l + 1];
            lm->x_right_in_tracking_ = x_right[l];
            lm->scale_level_in_tracking_ = level[l];
        }
    }
    for (int l = 0; l < m; ++l)
        if (assigned[l] >= 0) curr_frm.landmarks_[assigned[l]] = local_landmarks[l];
    return (unsigned int)num_matches;
}

}   // namespace module
}   // namespace openvslam
