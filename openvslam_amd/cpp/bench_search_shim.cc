// Times tracking_module::search_local_landmarks through the class layer, two ways on the same resident frame:
//   fused     module::search_local_landmarks: flattening, ONE device call (visibility + matcher), write-back
//   two-step  the path without it: a host loop of frame::can_observe over the local landmarks (rules V2 - V5 of DESIGN.md 3.17, this file,
//             the host compiler at -O2), then the existing projection::match_frame_and_landmarks
// 2000 keypoints against m = 2000 and 8000 local landmarks, monocular and stereo. Per configuration: 20 warm-up rounds of both, then `reps`
// rounds that ALTERNATE the two (so that whatever else runs on the host hits both alike); medians with the 10th and 90th percentile, the host
// loop's share on its own, and a check that both ways give the same frm.landmarks_. One JSON line per configuration.
// usage: bench_search_shim [reps = 300] [device = 0]
#include <ovs_detmath.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "openvslam/match/projection.h"
#include "openvslam/module/local_landmark_search.h"

using namespace openvslam;
using clk = std::chrono::steady_clock;

namespace {

struct Scene {
    camera::base cam;
    data::frame frm;
    std::vector<data::landmark> lms;
    std::vector<data::landmark*> local;
};

void build_scene(Scene& s, int n, int m, bool stereo, int device) {
    std::mt19937 rng(12345u + (unsigned)m + (stereo ? 1u : 0u));
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const int cols = 1280, rows = 720;
    s.cam.fx_ = s.cam.fy_ = 0.6 * cols;
    s.cam.cx_ = cols / 2.0;
    s.cam.cy_ = rows / 2.0;
    s.cam.cols_ = cols;
    s.cam.rows_ = rows;
    s.cam.img_bounds_.max_x_ = (float)cols;
    s.cam.img_bounds_.max_y_ = (float)rows;
    s.cam.true_baseline_ = 0.12f;
    s.cam.focal_x_baseline_ = (float)(0.12 * s.cam.fx_);
    if (stereo) s.cam.setup_type_ = camera::setup_type_t::Stereo;
    data::frame& f = s.frm;
    f.camera_ = &s.cam;
    f.id_ = 7;
    f.device_cache_->device = device;
    f.num_keypts_ = (unsigned)n;
    f.scale_factors_.assign(8, 1.0f);
    for (int l = 1; l < 8; ++l) f.scale_factors_[(size_t)l] = f.scale_factors_[(size_t)l - 1] * 1.2f;
    f.log_scale_factor_ = std::log(1.2f);
    const double a = 0.03;   // a small rotation about y and a translation
    f.cam_pose_cw_(0, 0) = std::cos(a), f.cam_pose_cw_(0, 2) = std::sin(a), f.cam_pose_cw_(2, 0) = -std::sin(a), f.cam_pose_cw_(2, 2) = std::cos(a);
    f.cam_pose_cw_(0, 3) = 0.05, f.cam_pose_cw_(1, 3) = -0.02, f.cam_pose_cw_(2, 3) = 0.3;
    f.undist_keypts_.resize((size_t)n);
    f.descriptors_ = cv::Mat(n, 32, cv::CV_8U);
    f.landmarks_.assign((size_t)n, nullptr);
    std::vector<double> depth((size_t)n);
    if (stereo) f.stereo_x_right_.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        cv::KeyPoint& kp = f.undist_keypts_[(size_t)i];
        kp.octave = (int)(U(rng) * 8) & 7;
        kp.pt.x = (float)(30 + U(rng) * (cols - 60));
        kp.pt.y = (float)(30 + U(rng) * (rows - 60));
        kp.angle = (float)(U(rng) * 360);
        depth[(size_t)i] = 2.0 + 18.0 * U(rng);
        for (int b = 0; b < 32; ++b) f.descriptors_.ptr(i)[b] = (uint8_t)(rng() & 255u);
        if (stereo) f.stereo_x_right_[(size_t)i] = U(rng) < 0.7 ? (float)(kp.pt.x - s.cam.focal_x_baseline_ / depth[(size_t)i]) : -1.0f;
    }
    // the local map: the keypoints back-projected (in turn, so that with m > n several landmarks want one keypoint), a tenth of them far off
    const Mat44_t& T = f.cam_pose_cw_;
    double cc[3];
    for (int i = 0; i < 3; ++i) cc[i] = -((T(0, i) * T(0, 3) + T(1, i) * T(1, 3)) + T(2, i) * T(2, 3));
    s.lms.resize((size_t)m);
    for (int l = 0; l < m; ++l) {
        data::landmark& lm = s.lms[(size_t)l];
        const int src = l % n;
        const cv::KeyPoint& kp = f.undist_keypts_[(size_t)src];
        const bool far = U(rng) < 0.1;
        const double z = far ? -depth[(size_t)src] : depth[(size_t)src];
        const double pc[3] = {(kp.pt.x + 1.5 * N(rng) - s.cam.cx_) / s.cam.fx_ * z - T(0, 3), (kp.pt.y + 1.5 * N(rng) - s.cam.cy_) / s.cam.fy_ * z - T(1, 3),
                              z - T(2, 3)};
        double d2 = 0;
        for (int i = 0; i < 3; ++i) {
            lm.pos_w_(i) = (T(0, i) * pc[0] + T(1, i) * pc[1]) + T(2, i) * pc[2];   // R^T (pc - t)
            d2 += (lm.pos_w_(i) - cc[i]) * (lm.pos_w_(i) - cc[i]);
        }
        const double dist = std::sqrt(d2);
        for (int i = 0; i < 3; ++i) lm.mean_normal_(i) = U(rng) < 0.15 ? N(rng) : (lm.pos_w_(i) - cc[i]) / dist;
        const int lvl = std::min(7, kp.octave + (int)(U(rng) * 2));
        lm.max_valid_dist_ = (float)(dist * f.scale_factors_[(size_t)lvl] * (0.85 + 0.15 * U(rng)));
        lm.min_valid_dist_ = lm.max_valid_dist_ / f.scale_factors_[7] * 0.8f;
        lm.descriptor_ = cv::Mat(1, 32, cv::CV_8U);
        for (int b = 0; b < 32; ++b) lm.descriptor_.data[b] = f.descriptors_.ptr(src)[b];
        for (int k = (int)(U(rng) * 40); k > 0; --k) lm.descriptor_.data[rng() & 31u] ^= (uint8_t)(1u << (rng() & 7u));
        lm.id_ = (unsigned)l;
    }
    for (auto& lm : s.lms) s.local.push_back(&lm);
}

// frame::can_observe(lm, 0.5, ...) on the host: camera::perspective::reproject_to_image, landmark::is_inside_in_orb_scale, the viewing angle,
// landmark::predict_scale_level -- the algebra of k_observe_landmarks
bool can_observe(const data::frame& f, const double* P, const double* cc, const data::landmark* lm, Vec2_t& reproj, float& x_right, unsigned int& level) {
    const camera::base& c = *f.camera_;
    const Vec3_t X = lm->get_pos_in_world();
    const double pcx = (P[0] * X(0) + P[1] * X(1)) + P[2] * X(2) + P[9];
    const double pcy = (P[3] * X(0) + P[4] * X(1)) + P[5] * X(2) + P[10];
    const double pcz = (P[6] * X(0) + P[7] * X(1)) + P[8] * X(2) + P[11];
    if (pcz <= 0.0) return false;
    const double z_inv = 1.0 / pcz;
    const double u = c.fx_ * pcx * z_inv + c.cx_, v = c.fy_ * pcy * z_inv + c.cy_;
    x_right = (float)(u - (double)c.focal_x_baseline_ * z_inv);
    if (u < c.img_bounds_.min_x_ || u > c.img_bounds_.max_x_ || v < c.img_bounds_.min_y_ || v > c.img_bounds_.max_y_) return false;
    const double dx = X(0) - cc[0], dy = X(1) - cc[1], dz = X(2) - cc[2];
    const double dist = std::sqrt((dx * dx + dy * dy) + dz * dz);
    if (dist < (double)lm->get_min_valid_distance() || (double)lm->get_max_valid_distance() < dist) return false;
    const Vec3_t nrm = lm->get_obs_mean_normal();
    if (((dx * nrm(0) + dy * nrm(1)) + dz * nrm(2)) / dist < 0.5) return false;
    int lvl = (int)std::ceil(ovs_det_logf(lm->max_valid_dist_ / (float)dist) / f.log_scale_factor_);
    lvl = std::max(0, std::min(lvl, (int)f.scale_factors_.size() - 1));
    reproj(0) = u, reproj(1) = v;
    level = (unsigned)lvl;
    return true;
}

// tracking_module::search_local_landmarks as it stands without the fused call; returns the matches, *loop_ms the host loop's time alone
unsigned int two_step(data::frame& f, const std::vector<data::landmark*>& local, float margin, double* loop_ms) {
    const auto t0 = clk::now();
    for (auto* lm : f.landmarks_) {
        if (!lm || lm->will_be_erased()) continue;
        lm->is_observable_in_tracking_ = false;
        lm->identifier_in_local_lm_search_ = f.id_;
        lm->increase_num_observable();
    }
    double P[12], cc[3];
    match::detail::pose12(f.cam_pose_cw_, P);
    for (int i = 0; i < 3; ++i) cc[i] = -((P[i] * P[9] + P[3 + i] * P[10]) + P[6 + i] * P[11]);
    bool found = false;
    Vec2_t reproj;
    float x_right;
    unsigned int level;
    for (auto* lm : local) {
        if (lm->identifier_in_local_lm_search_ == f.id_ || lm->will_be_erased()) continue;
        if (can_observe(f, P, cc, lm, reproj, x_right, level)) {
            lm->reproj_in_tracking_ = reproj;
            lm->x_right_in_tracking_ = x_right;
            lm->scale_level_in_tracking_ = (int)level;
            lm->is_observable_in_tracking_ = true;
            lm->increase_num_observable();
            found = true;
        } else {
            lm->is_observable_in_tracking_ = false;
        }
    }
    *loop_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    if (!found) return 0;
    return match::projection(0.8f, true).match_frame_and_landmarks(f, local, margin);
}

void reset(Scene& s) {
    std::fill(s.frm.landmarks_.begin(), s.frm.landmarks_.end(), nullptr);
    for (auto& lm : s.lms) lm.identifier_in_local_lm_search_ = 0;
}

struct Stat {
    double median, p10, p90;
};
Stat stat_of(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return Stat{v[v.size() / 2], v[v.size() / 10], v[v.size() * 9 / 10]};
}

}   // namespace

int main(int argc, char** argv) {
    const int reps = argc > 1 ? std::atoi(argv[1]) : 300;
    const int device = argc > 2 ? std::atoi(argv[2]) : 0;
    const int n = 2000;
    int status = 0;
    for (const bool stereo : {false, true})
        for (const int m : {2000, 8000}) {
            Scene s;
            build_scene(s, n, m, stereo, device);
            const float margin = 5.0f;
            std::vector<double> t_fused, t_two, t_loop;
            std::vector<data::landmark*> held_fused, held_two;
            unsigned int n_fused = 0, n_two = 0;
            for (int r = -20; r < reps; ++r) {   // negative rounds warm both ways up
                double loop_ms = 0;
                reset(s);
                auto t0 = clk::now();
                n_fused = module::search_local_landmarks(s.frm, s.local, margin, 0.8f, false);
                const double fused_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
                held_fused = s.frm.landmarks_;
                reset(s);
                t0 = clk::now();
                n_two = two_step(s.frm, s.local, margin, &loop_ms);
                const double two_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
                held_two = s.frm.landmarks_;
                if (r >= 0) {
                    t_fused.push_back(fused_ms);
                    t_two.push_back(two_ms);
                    t_loop.push_back(loop_ms);
                }
            }
            const bool same = n_fused == n_two && held_fused == held_two;
            if (!same || n_fused == 0) status = 1;
            const Stat a = stat_of(t_fused), b = stat_of(t_two), c = stat_of(t_loop);
            std::printf("{\"keypoints\": %d, \"local_landmarks\": %d, \"stereo\": %s, \"reps\": %d, \"matches\": %u, \"same_result\": %s, "
                        "\"fused_ms\": {\"median\": %.4f, \"p10\": %.4f, \"p90\": %.4f}, \"two_step_ms\": {\"median\": %.4f, \"p10\": %.4f, \"p90\": %.4f}, "
                        "\"host_loop_ms\": {\"median\": %.4f, \"p10\": %.4f, \"p90\": %.4f}}\n",
                        n, m, stereo ? "true" : "false", reps, n_fused, same ? "true" : "false", a.median, a.p10, a.p90, b.median, b.p10, b.p90, c.median, c.p10,
                        c.p90);
            std::fflush(stdout);
        }
    const auto& f = util::device_failures();
    if (f.failed_calls.load()) status = 1;
    return status;
}
