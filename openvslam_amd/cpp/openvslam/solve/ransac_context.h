// What solve::sim3_solver, solve::pnp_solver and optimize::transform_optimizer share around their one ABI call: the process's device handle
// (ransac_context: created on first use, enlarged when a batch outgrows it, dropped after a device failure) and, for the two RANSAC
// solvers, the part of a result that every RANSAC has.
// Failure policy: util/device_policy.h.
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../util/device_policy.h"

namespace openvslam {
namespace solve {

//! the process's handle of one solver: Handle with the ABI's create / destroy pair
template <class Handle, ovs_status (*Create)(int32_t, int32_t, int32_t, Handle**), ovs_status (*Destroy)(Handle*)>
class ransac_context {
public:
    //! the HIP device the next handle is created on
    void set_device(const int device) {
        std::lock_guard<std::mutex> lock(mu_);
        drop();
        device_ = device;
    }
    //! call(handle) -> ovs_status on a handle with room for P problems of T matches in all, under the failure policy: false when the
    //! caller has to leave its empty result
    template <class Call>
    bool run(const char* what, const int32_t P, const int32_t T, Call call) {
        std::lock_guard<std::mutex> lock(mu_);
        return util::run_guarded(what, [&] {
            const ovs_status st = ensure(P, T);
            return st != OVS_OK ? st : call(handle_);
        }, [&] { drop(); });
    }
    ~ransac_context() { drop(); }

private:
    ovs_status ensure(const int32_t P, const int32_t T) {
        if (handle_ && P <= max_problems_ && T <= max_total_matches_) return OVS_OK;
        drop();
        const int32_t mp = std::max<int32_t>(16, 2 * P), mt = std::max<int32_t>(4096, 2 * T);
        const ovs_status st = Create(device_, mp, mt, &handle_);
        if (st == OVS_OK) max_problems_ = mp, max_total_matches_ = mt;
        return st;
    }
    void drop() {
        if (handle_) Destroy(handle_);
        handle_ = nullptr;
        max_problems_ = max_total_matches_ = 0;
    }

    std::mutex mu_;
    int device_ = 0;
    Handle* handle_ = nullptr;
    int32_t max_problems_ = 0, max_total_matches_ = 0;
};

//! what every solve_batch call returns per problem and per match
struct ransac_batch_out {
    std::vector<int32_t> valid, best_iter, num_inliers;
    std::vector<uint8_t> flags;
    ransac_batch_out(const int32_t P, const int32_t T) : valid((size_t)P), best_iter((size_t)P), num_inliers((size_t)P), flags((size_t)std::max(T, 1)) {}
};

//! the solver's share of it
class ransac_result {
protected:
    void reset(const unsigned int num_matches) {
        solution_is_valid_ = false;
        best_iter_ = -1;
        num_inliers_ = 0;
        is_inlier_match_.assign(num_matches, false);
    }
    //! problem p of a batch, whose matches start at `offset`
    void take(const ransac_batch_out& out, const int32_t p, const int32_t offset) {
        solution_is_valid_ = out.valid[(size_t)p] != 0;
        best_iter_ = out.best_iter[(size_t)p];
        num_inliers_ = (unsigned int)out.num_inliers[(size_t)p];
        for (size_t i = 0; i < is_inlier_match_.size(); ++i) is_inlier_match_[i] = out.flags[(size_t)offset + i] != 0;
    }

    bool solution_is_valid_ = false;
    int best_iter_ = -1;
    unsigned int num_inliers_ = 0;
    std::vector<bool> is_inlier_match_;
};

}   // namespace solve
}   // namespace openvslam
