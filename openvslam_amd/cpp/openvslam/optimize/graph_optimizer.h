// optimize::graph_optimizer (expected: src/openvslam/optimize/graph_optimizer.{h,cc}): the Sim3 pose-graph optimisation over the essential graph
// that module::loop_closer runs after an accepted loop, and its write-back of every keyframe pose and landmark. Upstream's constructor and
// optimize; the graph is built here as upstream builds it (as recalled) and optimised on the device in one call
// (ovs_posegraph_optimize, csrc/pose_graph.hip). No g2o type exists in this tree: a Sim3 is (rot, trans, scale).
// Where upstream walks maps and sets keyed by pointer, which is no order, this walks ascending keyframe ids, so that the result is a function
// of the map; openvslam_amd.io.pose_graph_problem builds the same graph.
// Failure policy (util/device_policy.h): a device failure means one retry on a rebuilt handle, then the map left untouched -- a loop that
// was not closed, which the next detection closes. Caller errors throw.
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "../data/frame_stub.h"
#include "../util/device_policy.h"

namespace openvslam {
namespace optimize {

//! g2o::Sim3 stand-in: x -> scale * rot * x + trans
struct Sim3 {
    Mat33_t rot;
    Vec3_t trans;
    double scale = 1.0;
};

}   // namespace optimize

namespace module {
using keyframe_Sim3_pairs_t = std::map<data::keyframe*, optimize::Sim3>;
}   // namespace module

namespace optimize {

class graph_optimizer {
public:
    explicit graph_optimizer(data::map_database* map_db, const bool fix_scale) : map_db_(map_db), fix_scale_(fix_scale) {}

    //! the HIP device the optimiser runs on (process-wide)
    static void set_device(const int device) { ctx().set_device(device); }

    //! upstream: corrects every keyframe pose and landmark position of the map. num_iter is upstream's optimizer.optimize(50).
    void optimize(data::keyframe* loop_keyfrm, data::keyframe* curr_keyfrm, const module::keyframe_Sim3_pairs_t& non_corrected_Sim3s,
                  const module::keyframe_Sim3_pairs_t& pre_corrected_Sim3s,
                  const std::map<data::keyframe*, std::set<data::keyframe*>>& loop_connections, const unsigned int num_iter = 50) const {
        constexpr unsigned int min_weight = 100;
        std::vector<data::keyframe*> keyfrms;
        for (data::keyframe* k : map_db_->get_all_keyframes())
            if (k && !k->will_be_erased()) keyfrms.push_back(k);
        std::sort(keyfrms.begin(), keyfrms.end(), by_id);
        std::map<data::keyframe*, int32_t> index;
        for (size_t i = 0; i < keyfrms.size(); ++i) index[keyfrms[i]] = (int32_t)i;
        const int32_t n_v = (int32_t)keyfrms.size();

        // 1. vertices: the pre-corrected Sim3 where there is one, otherwise the pose with unit scale; the loop keyframe is fixed
        std::vector<Sim3> start((size_t)n_v);
        std::vector<uint8_t> fixed((size_t)n_v);
        for (int32_t i = 0; i < n_v; ++i) {
            const auto it = pre_corrected_Sim3s.find(keyfrms[(size_t)i]);
            start[(size_t)i] = it != pre_corrected_Sim3s.end() ? it->second : of_pose(keyfrms[(size_t)i]);
            fixed[(size_t)i] = keyfrms[(size_t)i] == loop_keyfrm ? 1 : 0;
        }

        // 2. edges: measurement Sim3_21 = Sim3_2w Sim3_1w^-1, vertex 0 = keyframe 1
        std::vector<int32_t> edge_ij;
        std::vector<double> edge_rot, edge_trans, edge_scale;
        std::set<std::pair<unsigned int, unsigned int>> inserted;
        const auto insert = [&](data::keyframe* k1, data::keyframe* k2, const Sim3& S_1w, const Sim3& S_2w) {
            const Sim3 M = product(S_2w, inverse(S_1w));
            edge_ij.push_back(index.at(k1)), edge_ij.push_back(index.at(k2));
            edge_rot.insert(edge_rot.end(), M.rot.m, M.rot.m + 9);
            edge_trans.insert(edge_trans.end(), M.trans.v, M.trans.v + 3);
            edge_scale.push_back(M.scale);
        };
        // (a) the loop connections, from the vertices' start states
        std::vector<data::keyframe*> firsts;
        for (const auto& lc : loop_connections)
            if (index.count(lc.first)) firsts.push_back(lc.first);
        std::sort(firsts.begin(), firsts.end(), by_id);
        for (data::keyframe* k1 : firsts) {
            std::vector<data::keyframe*> connected;
            for (data::keyframe* k2 : loop_connections.at(k1))
                if (index.count(k2)) connected.push_back(k2);
            std::sort(connected.begin(), connected.end(), by_id);
            for (data::keyframe* k2 : connected) {
                if ((k1 != curr_keyfrm || k2 != loop_keyfrm) && k1->graph_node_->get_weight(k2) < min_weight) continue;
                insert(k1, k2, start[(size_t)index.at(k1)], start[(size_t)index.at(k2)]);
                inserted.insert(std::make_pair(std::min(k1->id_, k2->id_), std::max(k1->id_, k2->id_)));
            }
        }
        // (b) to (d): per keyframe the spanning-tree parent, the earlier loop edges and the strong covisibilities, with the non-corrected Sim3 of
        // either end where there is one
        const auto nc_of = [&](data::keyframe* k) -> const Sim3& {
            const auto it = non_corrected_Sim3s.find(k);
            return it != non_corrected_Sim3s.end() ? it->second : start[(size_t)index.at(k)];
        };
        for (data::keyframe* k1 : keyfrms) {
            data::keyframe* parent = k1->graph_node_->get_spanning_parent();
            if (parent && !index.count(parent)) parent = nullptr;
            if (parent) insert(k1, parent, nc_of(k1), nc_of(parent));
            const std::set<data::keyframe*> loop_edges = k1->graph_node_->get_loop_edges();
            std::vector<data::keyframe*> earlier;
            for (data::keyframe* k2 : loop_edges)
                if (index.count(k2) && k2->id_ < k1->id_) earlier.push_back(k2);
            std::sort(earlier.begin(), earlier.end(), by_id);
            for (data::keyframe* k2 : earlier) insert(k1, k2, nc_of(k1), nc_of(k2));
            for (data::keyframe* k2 : k1->graph_node_->get_covisibilities_over_weight(min_weight)) {
                if (!k2 || !index.count(k2)) continue;
                if (k2 == parent || k1->graph_node_->has_spanning_child(k2) || loop_edges.count(k2)) continue;
                if (!(k2->id_ < k1->id_)) continue;
                if (inserted.count(std::make_pair(k2->id_, k1->id_))) continue;
                insert(k1, k2, nc_of(k1), nc_of(k2));
            }
        }
        const int32_t n_e = (int32_t)edge_scale.size();

        // 3. landmarks: each moves with the start state of its reference keyframe (upstream's Sim3s_cw)
        std::vector<data::landmark*> lms;
        for (data::landmark* lm : map_db_->get_all_landmarks())
            if (lm && !lm->will_be_erased()) lms.push_back(lm);
        std::sort(lms.begin(), lms.end(), [](const data::landmark* a, const data::landmark* b) { return a->id_ < b->id_; });
        const int32_t n_l = (int32_t)lms.size();
        std::vector<int32_t> lm_ref((size_t)n_l);
        std::vector<double> lm_pos(3 * (size_t)n_l);
        for (int32_t m = 0; m < n_l; ++m) {
            const auto it = lms[(size_t)m]->ref_keyfrm_ ? index.find(lms[(size_t)m]->ref_keyfrm_) : index.end();
            lm_ref[(size_t)m] = it == index.end() ? -1 : it->second;
            const Vec3_t p = lms[(size_t)m]->get_pos_in_world();
            for (int x = 0; x < 3; ++x) lm_pos[3 * (size_t)m + (size_t)x] = p(x);
        }

        std::vector<double> rot(9 * (size_t)n_v), trans(3 * (size_t)n_v), scale((size_t)n_v);
        for (int32_t i = 0; i < n_v; ++i) {
            std::copy(start[(size_t)i].rot.m, start[(size_t)i].rot.m + 9, rot.begin() + 9 * i);
            std::copy(start[(size_t)i].trans.v, start[(size_t)i].trans.v + 3, trans.begin() + 3 * i);
            scale[(size_t)i] = start[(size_t)i].scale;
        }
        std::vector<double> out_rot(rot.size()), out_trans(trans.size()), out_scale(scale.size()), out_lm(lm_pos.size());
        if (!ctx().run("ovs_posegraph_optimize", n_v, n_e, n_l, [&](ovs_posegraph* handle) {
                return ovs_posegraph_optimize(handle, n_v, rot.data(), trans.data(), scale.data(), fixed.data(), rot.data(), trans.data(), scale.data(), n_e,
                                              edge_ij.data(), edge_rot.data(), edge_trans.data(), edge_scale.data(), fix_scale_ ? 1 : 0,
                                              (int32_t)std::min<unsigned int>(std::max(num_iter, 1u), 1u << 30), 0, n_l, lm_ref.data(), lm_pos.data(),
                                              out_rot.data(), out_trans.data(), out_scale.data(), out_lm.data(), nullptr);
            }))
            return;   // the map stays as it came

        // 4. write-back under the map's lock: rot_cw = R, trans_cw = t / s; every landmark with its reference keyframe
        std::lock_guard<std::mutex> lock(data::map_database::mtx_database_);
        for (int32_t i = 0; i < n_v; ++i) {
            Mat44_t pose;
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) pose(r, c) = out_rot[9 * (size_t)i + 3 * (size_t)r + (size_t)c];
                pose(r, 3) = out_trans[3 * (size_t)i + (size_t)r] / out_scale[(size_t)i];
            }
            keyfrms[(size_t)i]->set_cam_pose(pose);
        }
        for (int32_t m = 0; m < n_l; ++m) {
            Vec3_t p;
            for (int x = 0; x < 3; ++x) p(x) = out_lm[3 * (size_t)m + (size_t)x];
            lms[(size_t)m]->set_pos_in_world(p);
            lms[(size_t)m]->update_normal_and_depth();
        }
    }

    //! DESIGN.md 3.19 rule G1: R' = R^T, s' = 1 / s, t' = (-s') (R^T t)
    static Sim3 inverse(const Sim3& S) {
        Sim3 o;
        o.scale = 1.0 / S.scale;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) o.rot(r, c) = S.rot(c, r);
            o.trans(r) = (-o.scale) * ((S.rot(0, r) * S.trans(0) + S.rot(1, r) * S.trans(1)) + S.rot(2, r) * S.trans(2));
        }
        return o;
    }
    //! rule G1: A B = (R_A R_B, s_A (R_A t_B) + t_A, s_A s_B), every sum left to right
    static Sim3 product(const Sim3& A, const Sim3& B) {
        Sim3 o;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) o.rot(i, j) = (A.rot(i, 0) * B.rot(0, j) + A.rot(i, 1) * B.rot(1, j)) + A.rot(i, 2) * B.rot(2, j);
            o.trans(i) = A.scale * ((A.rot(i, 0) * B.trans(0) + A.rot(i, 1) * B.trans(1)) + A.rot(i, 2) * B.trans(2)) + A.trans(i);
        }
        o.scale = A.scale * B.scale;
        return o;
    }

private:
    static bool by_id(const data::keyframe* a, const data::keyframe* b) { return a->id_ < b->id_; }
    static Sim3 of_pose(const data::keyframe* k) {
        Sim3 S;
        S.rot = k->get_rotation();
        S.trans = k->get_translation();
        return S;
    }

    //! the process's handle: created on first use, enlarged when a map outgrows it, dropped after a device failure
    class context {
    public:
        void set_device(const int device) {
            std::lock_guard<std::mutex> lock(mu_);
            drop();
            device_ = device;
        }
        template <class Call>
        bool run(const char* what, const int32_t n_v, const int32_t n_e, const int32_t n_l, Call call) {
            std::lock_guard<std::mutex> lock(mu_);
            return util::run_guarded(what, [&] {
                const ovs_status st = ensure(n_v, n_e, n_l);
                return st != OVS_OK ? st : call(handle_);
            }, [&] { drop(); });
        }
        ~context() { drop(); }

    private:
        ovs_status ensure(const int32_t n_v, const int32_t n_e, const int32_t n_l) {
            if (handle_ && n_v <= cap_[0] && n_e <= cap_[1] && n_l <= cap_[2]) return OVS_OK;
            drop();
            const int32_t want[3] = {std::max<int32_t>(256, 2 * n_v), std::max<int32_t>(1024, 2 * n_e), std::max<int32_t>(4096, 2 * n_l)};
            const ovs_status st = ovs_posegraph_create(device_, want[0], want[1], want[2], &handle_);
            if (st == OVS_OK) std::copy(want, want + 3, cap_);
            return st;
        }
        void drop() {
            if (handle_) ovs_posegraph_destroy(handle_);
            handle_ = nullptr;
            cap_[0] = cap_[1] = cap_[2] = 0;
        }
        std::mutex mu_;
        int device_ = 0;
        ovs_posegraph* handle_ = nullptr;
        int32_t cap_[3] = {0, 0, 0};
    };
    static context& ctx() {
        static context c;
        return c;
    }

    data::map_database* map_db_;
    const bool fix_scale_;
};

}   // namespace optimize
}   // namespace openvslam
