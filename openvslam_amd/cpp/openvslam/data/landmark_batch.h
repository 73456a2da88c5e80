// data::update_landmarks: data::landmark::compute_descriptor() and data::landmark::update_normal_and_depth() (expected:
// src/openvslam/data/landmark.{h,cc}) for MANY landmarks in one device call (ovs_landmarks_update_batch_f, csrc/landmark_update.hip;
// DESIGN.md 3.14, rules L1 to L9). What an integration calls where upstream loops over the two functions: local_bundle_adjuster's write-back,
// mapping_module after create_new_landmarks and after the fuse step, map_database::from_json.
// A landmark's observations are handed over in the iteration order of observations_; keyframes get their slots in the order they are first
// met. The descriptors are gathered on the device from the resident keyframes (match::detail::device_handle_on), so a call uploads indices.
// Failure policy (util/device_policy.h): a device failure means one retry on rebuilt handles, then the landmarks are left as they were
// (false is returned). Caller errors throw std::invalid_argument before the device is touched: a reference keyframe that does not observe
// its landmark, keyframes with different scale tables in one call.
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../match/window_ctx.h"
#include "../util/device_policy.h"
#include "frame_stub.h"

namespace openvslam {
namespace data {

namespace detail {
//! the process's ovs_landmarks handle: created on first use, enlarged when a batch outgrows it, dropped after a device failure
class landmarks_context {
public:
    void set_device(const int device) {
        std::lock_guard<std::mutex> lock(mu_);
        drop();
        device_ = device;
    }
    int device() {
        std::lock_guard<std::mutex> lock(mu_);
        return device_;
    }
    //! call(handle) -> ovs_status on a handle with room for the batch, under the failure policy; `reset` drops what else the call uses
    template <class Call, class Reset>
    bool run(const int32_t P, const int32_t T, const int32_t K, Call call, Reset reset) {
        std::lock_guard<std::mutex> lock(mu_);
        return util::run_guarded("ovs_landmarks_update_batch_f", [&] {
            const ovs_status st = ensure(P, T, K);
            return st != OVS_OK ? st : call(handle_);
        }, [&] {
            drop();
            reset();
        });
    }
    ~landmarks_context() { drop(); }

private:
    ovs_status ensure(const int32_t P, const int32_t T, const int32_t K) {
        if (handle_ && P <= max_p_ && T <= max_t_ && K <= max_k_) return OVS_OK;
        drop();
        const int32_t mp = std::min<int32_t>(65535, std::max<int32_t>(1024, 2 * P)), mt = std::max<int32_t>(8192, 2 * T), mk = std::max<int32_t>(256, 2 * K);
        const ovs_status st = ovs_landmarks_create(device_, mp, mt, mk, &handle_);
        if (st == OVS_OK) max_p_ = mp, max_t_ = mt, max_k_ = mk;
        return st;
    }
    void drop() {
        if (handle_) ovs_landmarks_destroy(handle_);
        handle_ = nullptr;
        max_p_ = max_t_ = max_k_ = 0;
    }
    std::mutex mu_;
    int device_ = 0;
    ovs_landmarks* handle_ = nullptr;
    int32_t max_p_ = 0, max_t_ = 0, max_k_ = 0;
};
inline landmarks_context& landmarks_ctx() {
    static landmarks_context c;
    return c;
}
}   // namespace detail

//! the HIP device update_landmarks runs on (process-wide; 0 unless an integration places the mapping thread elsewhere)
inline void set_landmark_update_device(const int device) { detail::landmarks_ctx().set_device(device); }

//! compute_descriptor() (descriptor) and / or update_normal_and_depth() (geometry) for every landmark of the list: mean_normal_,
//! min_valid_dist_, max_valid_dist_, descriptor_ are written, num_normal_updates_ rises by one per landmark when geometry was asked. A landmark
//! without observations is left as it is, as upstream leaves it. Batches beyond 65535 landmarks are split. false: the device failed and
//! nothing was written.
inline bool update_landmarks(const std::vector<landmark*>& landmarks, const bool geometry, const bool descriptor) {
    if (landmarks.empty() || (!geometry && !descriptor)) return true;
    const int32_t what = (geometry ? 1 : 0) | (descriptor ? 2 : 0);
    const size_t chunk = 65535;
    bool ok = true;
    for (size_t at = 0; at < landmarks.size() && ok; at += chunk) {
        const size_t P = std::min(chunk, landmarks.size() - at);
        std::map<keyframe*, int32_t> slot_of;
        std::vector<keyframe*> keyfrms;
        const auto slot = [&](keyframe* kf) {
            const auto it = slot_of.find(kf);
            if (it != slot_of.end()) return it->second;
            if (!keyfrms.empty() && kf->scale_factors_ != keyfrms.front()->scale_factors_)
                throw std::invalid_argument("data::update_landmarks: keyframes with different scale tables in one call");
            slot_of[kf] = (int32_t)keyfrms.size();
            keyfrms.push_back(kf);
            return (int32_t)keyfrms.size() - 1;
        };
        std::vector<int32_t> offsets(1, 0), ref_keyfrm(P, 0), ref_level(P, 0), obs_keyfrm, obs_keypoint;
        std::vector<uint8_t> obs_use;
        std::vector<double> pos_w(3 * P);
        for (size_t p = 0; p < P; ++p) {
            landmark* lm = landmarks[at + p];
            for (int x = 0; x < 3; ++x) pos_w[3 * p + (size_t)x] = lm->pos_w_(x);
            for (const auto& obs : lm->observations_) {
                obs_keyfrm.push_back(slot(obs.first));
                obs_keypoint.push_back((int32_t)obs.second);
                obs_use.push_back(obs.first->will_be_erased() ? 0 : 1);
            }
            offsets.push_back((int32_t)obs_keyfrm.size());
            if (lm->observations_.empty()) continue;
            const auto ref = lm->observations_.find(lm->ref_keyfrm_);
            if (ref == lm->observations_.end())
                throw std::invalid_argument("data::update_landmarks: landmark " + std::to_string(lm->id_) + ": its reference keyframe does not observe it");
            ref_keyfrm[p] = slot(lm->ref_keyfrm_);
            ref_level[p] = lm->ref_keyfrm_->undist_keypts_.at(ref->second).octave;
        }
        const int32_t T = offsets.back(), K = (int32_t)keyfrms.size();
        if (T == 0) {   // nothing observed: nothing to do (rule L1)
            if (geometry)
                for (size_t p = 0; p < P; ++p) ++landmarks[at + p]->num_normal_updates_;
            continue;
        }
        const std::vector<float>& scale_factors = keyfrms.front()->scale_factors_;
        std::vector<double> cam_centers(3 * (size_t)K);
        for (int32_t k = 0; k < K; ++k) {
            const Vec3_t c = keyfrms[(size_t)k]->get_cam_center();
            for (int x = 0; x < 3; ++x) cam_centers[3 * (size_t)k + (size_t)x] = c(x);
        }
        std::vector<double> normal(3 * P);
        std::vector<float> range(2 * P);
        std::vector<int32_t> best(P);
        std::vector<uint8_t> desc(32 * P), status(P);
        const int device = detail::landmarks_ctx().device();
        ok = detail::landmarks_ctx().run(
            (int32_t)P, T, K,
            [&](ovs_landmarks* handle) {
                // the keyframes resident on the call's device; the references live until the call returns
                std::vector<std::shared_ptr<void>> held((size_t)K);
                std::vector<const ovs_frame_dev*> handles((size_t)K);
                for (int32_t k = 0; k < K; ++k) {
                    held[(size_t)k] = match::detail::device_handle_on(*keyfrms[(size_t)k], device);
                    handles[(size_t)k] = match::detail::dev(held[(size_t)k]);
                }
                return ovs_landmarks_update_batch_f(handle, what, (int32_t)P, offsets.data(), pos_w.data(), ref_keyfrm.data(), ref_level.data(), obs_keyfrm.data(),
                                                    handles.data(), obs_keypoint.data(), obs_use.data(), cam_centers.data(), K, scale_factors.data(),
                                                    (int32_t)scale_factors.size(), normal.data(), range.data(), best.data(), desc.data(), status.data());
            },
            [&] {
                for (keyframe* kf : keyfrms) kf->device_cache_->drop();
            });
        if (!ok) break;
        for (size_t p = 0; p < P; ++p) {
            landmark* lm = landmarks[at + p];
            if (geometry) ++lm->num_normal_updates_;   // the call, as the stub's update_normal_and_depth() counts it
            if (status[p] != 0) continue;
            if (geometry) {
                for (int x = 0; x < 3; ++x) lm->mean_normal_(x) = normal[3 * p + (size_t)x];
                lm->min_valid_dist_ = range[2 * p];
                lm->max_valid_dist_ = range[2 * p + 1];
            }
            if (descriptor && best[p] >= 0) {
                cv::Mat d(1, 32, cv::CV_8U);
                std::memcpy(d.data, &desc[32 * p], 32);
                lm->descriptor_ = d;
            }
        }
    }
    return ok;
}

}   // namespace data
}   // namespace openvslam
