// optimize::global_bundle_adjuster::optimize over the C ABI. Replaces that function's body in src/openvslam/optimize/global_bundle_adjuster.cc:
// steps 1-3 (collect the keyframes, the landmarks and the observations) and 5 (write back) are upstream's host code restated; step 4
// (build the g2o graph, optimizer.optimize(num_iter)) is one call.
#include "global_bundle_adjuster.h"

#include <ovslam_hip.h>

#include "../util/device_policy.h"
#include "se3_quat.h"

#include <stdexcept>
#include <unordered_map>
#include <vector>

namespace openvslam {
namespace optimize {

void global_bundle_adjuster::optimize(const unsigned int lead_keyfrm_id_in_global_BA, bool* const force_stop_flag) const {
    // 1. collect the dataset
    const auto keyfrms = map_db_->get_all_keyframes();
    const auto lms = map_db_->get_all_landmarks();

    // 2. the keyframes: a shot vertex each, keyframe 0 constant
    std::vector<data::keyframe*> used_keyfrms;
    std::unordered_map<data::keyframe*, int32_t> pose_index;
    std::vector<double> poses;
    std::vector<uint8_t> pose_fixed;
    const camera::base* camera = nullptr;
    for (const auto keyfrm : keyfrms) {
        if (!keyfrm) continue;
        if (keyfrm->will_be_erased()) continue;
        if (!camera) camera = keyfrm->camera_;
        // (the perspective / equirectangular switch and the one-camera rule are local_bundle_adjuster.cc's)
        if (keyfrm->camera_ != camera &&
            (keyfrm->camera_->model_type_ != camera->model_type_ || keyfrm->camera_->fx_ != camera->fx_ || keyfrm->camera_->fy_ != camera->fy_ ||
             keyfrm->camera_->cx_ != camera->cx_ || keyfrm->camera_->cy_ != camera->cy_ || keyfrm->camera_->cols_ != camera->cols_ ||
             keyfrm->camera_->rows_ != camera->rows_))
            throw std::runtime_error("global_bundle_adjuster: all keyframes of the map must share one camera");
        pose_index[keyfrm] = (int32_t)used_keyfrms.size();
        used_keyfrms.push_back(keyfrm);
        poses.resize(poses.size() + 7);
        pose_to_se3quat(keyfrm->get_cam_pose(), &poses[poses.size() - 7]);
        pose_fixed.push_back(keyfrm->id_ == 0 ? 1 : 0);
    }

    // 3. the landmarks: a vertex each and one reprojection edge per observation, in upstream's insertion order; a landmark without an edge
    //    leaves the graph again and is not written back
    std::vector<size_t> used_lms;   // index into lms
    std::vector<double> points;
    std::vector<ovs_ba_edge> mono;
    std::vector<ovs_ba_edge_stereo> stereo;
    for (size_t i = 0; i < lms.size(); ++i) {
        auto lm = lms[i];
        if (!lm) continue;
        if (lm->will_be_erased()) continue;
        const int32_t point_idx = (int32_t)used_lms.size();
        unsigned int num_edges = 0;
        const auto observations = lm->get_observations();
        for (const auto& obs : observations) {
            auto keyfrm = obs.first;
            auto idx = obs.second;
            if (!keyfrm) continue;
            if (keyfrm->will_be_erased()) continue;
            const auto pit = pose_index.find(keyfrm);
            if (pit == pose_index.end()) continue;
            const auto& undist_keypt = keyfrm->undist_keypts_.at(idx);
            const float x_right = keyfrm->stereo_x_right_.empty() ? -1.0f : keyfrm->stereo_x_right_.at(idx);
            const float inv_sigma_sq = keyfrm->inv_level_sigma_sq_.at((size_t)undist_keypt.octave);
            if (x_right < 0 || camera->model_type_ == camera::model_type_t::Equirectangular) {
                ovs_ba_edge e;
                e.pose_idx = pit->second;
                e.point_idx = point_idx;
                e.obs_x = undist_keypt.pt.x;
                e.obs_y = undist_keypt.pt.y;
                e.inv_sigma_sq = inv_sigma_sq;
                mono.push_back(e);
            } else {
                ovs_ba_edge_stereo e;
                e.pose_idx = pit->second;
                e.point_idx = point_idx;
                e.obs_x = undist_keypt.pt.x;
                e.obs_y = undist_keypt.pt.y;
                e.obs_x_right = x_right;
                e.inv_sigma_sq = inv_sigma_sq;
                stereo.push_back(e);
            }
            ++num_edges;
        }
        if (num_edges == 0) continue;
        used_lms.push_back(i);
        const Vec3_t pos_w = lm->get_pos_in_world();
        for (int a = 0; a < 3; ++a) points.push_back(pos_w(a));
    }

    // 4. the optimisation: one round, Huber kernels with the deltas local BA's first round uses for the rig
    if (used_keyfrms.empty() || used_lms.empty()) return;
    constexpr double kHuber2D = 0x1.394fbcp+1, kHuber3D = 0x1.65d26ap+1;   // sqrtf(5.99146f), sqrtf(7.81473f)
    const double huber_mono = !use_huber_kernel_ ? 0.0 : camera->setup_type_ == camera::setup_type_t::Monocular ? kHuber2D : kHuber3D;
    const double huber_stereo = use_huber_kernel_ ? kHuber3D : 0.0;
    const ovs_ba_cam cam = {camera->fx_, camera->fy_, camera->cx_, camera->cy_};
    static_assert(sizeof(bool) == 1, "force_stop_flag is polled as a byte");
    // failure policy (util/device_policy.h): one retry from the same start state, then the map is left exactly as it was
    const std::vector<double> poses_in = poses, points_in = points;
    if (!util::run_guarded(
            "ovs_global_ba_optimize",
            [&] {
                poses = poses_in;     // in / out arguments
                points = points_in;
                return camera->model_type_ == camera::model_type_t::Equirectangular
                           ? ovs_global_ba_optimize_equirect(0, poses.data(), pose_fixed.data(), (int32_t)used_keyfrms.size(), points.data(),
                                                             (int32_t)used_lms.size(), mono.empty() ? nullptr : mono.data(), (int32_t)mono.size(),
                                                             (int32_t)camera->cols_, (int32_t)camera->rows_, huber_mono, (int32_t)num_iter_, 0,
                                                             reinterpret_cast<const volatile uint8_t*>(force_stop_flag), nullptr)
                           : ovs_global_ba_optimize(0, poses.data(), pose_fixed.data(), (int32_t)used_keyfrms.size(), points.data(),
                                                    (int32_t)used_lms.size(), mono.empty() ? nullptr : mono.data(), (int32_t)mono.size(),
                                                    stereo.empty() ? nullptr : stereo.data(), (int32_t)stereo.size(), &cam, camera->focal_x_baseline_,
                                                    huber_mono, huber_stereo, (int32_t)num_iter_, 0,
                                                    reinterpret_cast<const volatile uint8_t*>(force_stop_flag), nullptr);
            },
            [] {}))
        return;
    if (force_stop_flag && *force_stop_flag) return;

    // 5. write back: lead keyframe 0 (after initialisation) straight into the map; otherwise as the after-loop-BA values with the lead
    //    keyframe's id, which loop_bundle_adjuster propagates over the spanning tree
    std::lock_guard<std::mutex> lock(data::map_database::mtx_database_);
    for (size_t k = 0; k < used_keyfrms.size(); ++k) {
        auto keyfrm = used_keyfrms[k];
        // a constant vertex keeps its estimate: the keyframe's own matrix, not its trip through the quaternion record and back
        const Mat44_t cam_pose_cw = pose_fixed[k] ? keyfrm->get_cam_pose() : se3quat_to_pose(&poses[7 * k]);
        if (lead_keyfrm_id_in_global_BA == 0) {
            keyfrm->set_cam_pose(cam_pose_cw);
        } else {
            keyfrm->cam_pose_cw_after_loop_BA_ = cam_pose_cw;
            keyfrm->loop_BA_identifier_ = lead_keyfrm_id_in_global_BA;
        }
    }
    for (size_t j = 0; j < used_lms.size(); ++j) {
        auto lm = lms[used_lms[j]];
        Vec3_t pos_w;
        for (int a = 0; a < 3; ++a) pos_w(a) = points[3 * j + a];
        if (lead_keyfrm_id_in_global_BA == 0) {
            lm->set_pos_in_world(pos_w);
            lm->update_normal_and_depth();
        } else {
            lm->pos_w_after_global_BA_ = pos_w;
            lm->loop_BA_identifier_ = lead_keyfrm_id_in_global_BA;
        }
    }
}

}   // namespace optimize
}   // namespace openvslam
