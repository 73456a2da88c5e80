// data::bow_database (expected: src/openvslam/data/bow_database.{h,cc}): the keyframes' BoW vectors and the two candidate queries,
// acquire_loop_candidates (loop_detector) and acquire_relocalization_candidates (relocalizer). Upstream keeps an inverted file
// word -> keyframes on the host; here the vectors are resident in HBM and one launch scores the query against all of them
// (ovs_bowdb_query: L1 score, shared-word count and the common-word gate, DESIGN.md 3.8 rules 1 to 3). The score gate and the
// covisibility totals (rules 4 to 6) run here over the survivors: a few hundred records and the host's covisibility graph.
// Candidates come back in ascending keyframe id order of their records (upstream's order is that of an unordered container).
#pragma once
#include <ovslam_hip.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "../util/device_policy.h"
#include "bow_vocabulary.h"
#include "frame_stub.h"

namespace openvslam {
namespace data {

class bow_database {
public:
    explicit bow_database(bow_vocabulary* bow_vocab, int max_keyframes = 4096, int max_words = 4096)
        : bow_vocab_(bow_vocab), max_keyframes_(max_keyframes), max_words_(max_words) {}
    ~bow_database() {
        if (db_) ovs_bowdb_destroy(db_);
    }
    bow_database(const bow_database&) = delete;
    bow_database& operator=(const bow_database&) = delete;

    //! upstream: registers keyfrm under every word of keyfrm->bow_vec_
    void add_keyframe(keyframe* keyfrm) {
        std::lock_guard<std::mutex> lock(mtx_);
        const int32_t id = (int32_t)keyfrm->id_;
        if (!keyfrms_.emplace(id, keyfrm).second) throw std::invalid_argument("bow_database: keyframe " + std::to_string(id) + " is already registered");
        wanted_words_ = (int)keyfrm->bow_vec_.size();
        // failure policy (util/device_policy.h): one retry on a rebuilt handle; if the device stays away the keyframe stays registered
        // here and is uploaded with the others by the next call that reaches the device
        try {
            util::run_guarded("ovs_bowdb_add", [&] { return ensure(); }, [&] { drop(); }, [&] { return grow(); });
        } catch (...) {   // a caller-side error (an unusable vector): the keyframe is not registered
            keyfrms_.erase(id);
            throw;
        }
    }

    void erase_keyframe(keyframe* keyfrm) {
        std::lock_guard<std::mutex> lock(mtx_);
        const int32_t id = (int32_t)keyfrm->id_;
        if (!keyfrms_.erase(id)) throw std::invalid_argument("bow_database: keyframe " + std::to_string(id) + " is not registered");
        if (!db_ || !uploaded_.erase(id)) return;
        util::run_guarded("ovs_bowdb_erase", [&] { return db_ ? ovs_bowdb_erase(db_, id) : (ovs_status)OVS_OK; }, [&] { drop(); });
    }

    void clear() {
        std::lock_guard<std::mutex> lock(mtx_);
        keyfrms_.clear();
        uploaded_.clear();
        if (db_) util::run_guarded("ovs_bowdb_clear", [&] { return db_ ? ovs_bowdb_clear(db_) : (ovs_status)OVS_OK; }, [&] { drop(); });
    }

    //! loop_detector: keyframes that look like qry_keyfrm, outside its own neighbourhood, scoring at least min_score
    std::vector<keyframe*> acquire_loop_candidates(keyframe* qry_keyfrm, const float min_score) {
        std::vector<int32_t> reject{(int32_t)qry_keyfrm->id_};
        for (keyframe* k : qry_keyfrm->graph_node_->get_connected_keyframes()) reject.push_back((int32_t)k->id_);
        return candidates(qry_keyfrm->bow_vec_, reject, min_score);
    }

    //! relocalizer: keyframes that look like qry_frm
    std::vector<keyframe*> acquire_relocalization_candidates(frame* qry_frm) { return candidates(qry_frm->bow_vec_, {}, 0.0f); }

private:
    static void flatten(const bow_vector& v, std::vector<int32_t>& ids, std::vector<double>& values) {
        ids.clear();
        values.clear();
        for (const auto& e : v) {   // std::map order = ascending word id
            ids.push_back((int32_t)e.first);
            values.push_back(e.second);
        }
    }
    ovs_status ensure() {   // the handle, holding every registered keyframe
        if (!db_) {
            const ovs_status st = ovs_bowdb_create(0, max_keyframes_, max_words_, &db_);
            if (st != OVS_OK) return st;
            uploaded_.clear();
        }
        if (uploaded_.size() == keyfrms_.size()) return OVS_OK;
        std::vector<int32_t> ids;
        std::vector<double> values;
        for (const auto& e : keyfrms_) {
            if (uploaded_.count(e.first)) continue;
            flatten(e.second->bow_vec_, ids, values);
            const ovs_status st = ovs_bowdb_add(db_, e.first, ids.data(), values.data(), (int32_t)ids.size());
            if (st != OVS_OK) return st;
            uploaded_.insert(e.first);
        }
        return OVS_OK;
    }
    void drop() {
        if (db_) ovs_bowdb_destroy(db_);
        db_ = nullptr;
        uploaded_.clear();
    }
    bool grow() {   // after OVS_ERR_CAPACITY: a larger handle, filled again by ensure()
        bool grown = false;
        if ((int)keyfrms_.size() >= max_keyframes_) {
            max_keyframes_ *= 2;
            grown = true;
        }
        if (wanted_words_ > max_words_ && wanted_words_ <= kMaxWords) {
            max_words_ = std::min(kMaxWords, std::max(wanted_words_, 2 * max_words_));
            grown = true;
        }
        if (grown) drop();
        return grown;
    }

    std::vector<keyframe*> candidates(const bow_vector& bow_vec, const std::vector<int32_t>& reject, const float min_score) {
        std::lock_guard<std::mutex> lock(mtx_);
        if (keyfrms_.empty()) return {};
        std::vector<int32_t> q_ids;
        std::vector<double> q_values;
        flatten(bow_vec, q_ids, q_values);
        wanted_words_ = (int)q_ids.size();
        const int32_t cap = (int32_t)keyfrms_.size();
        std::vector<int32_t> ids((size_t)cap), num_common((size_t)cap);
        std::vector<double> scores((size_t)cap);
        int32_t n = 0, max_common = 0;
        // failure policy (util/device_policy.h): one retry on a rebuilt handle, then no candidates -- the loop detector finds no loop this
        // time, the relocaliser stays lost for this frame; both are states upstream handles
        if (!util::run_guarded("ovs_bowdb_query", [&] {
                const ovs_status st = ensure();
                if (st != OVS_OK) return st;
                return ovs_bowdb_query(db_, q_ids.data(), q_values.data(), (int32_t)q_ids.size(), reject.data(), (int32_t)reject.size(), ids.data(),
                                       num_common.data(), scores.data(), cap, &n, &max_common);
            }, [&] { drop(); }, [&] { return grow(); }))
            return {};
        // rule 4: upstream stores the score in a float and compares it with min_score
        std::unordered_map<int32_t, float> score_of;
        std::vector<int32_t> kept;
        for (int32_t i = 0; i < n; ++i) {
            const float s = (float)scores[(size_t)i];
            if (s >= min_score) {
                score_of[ids[(size_t)i]] = s;
                kept.push_back(ids[(size_t)i]);   // ascending keyframe id, as the ABI returns them
            }
        }
        if (kept.empty()) return {};
        // rule 5: every kept keyframe gathers the scores of its ten strongest covisibilities that were kept too
        std::vector<std::pair<float, keyframe*>> records;
        float best_total = 0.0f;
        for (size_t i = 0; i < kept.size(); ++i) {
            keyframe* c = keyfrms_.at(kept[i]);
            float total = score_of.at(kept[i]);
            float best_score = total;
            keyframe* best = c;
            for (keyframe* nb : c->graph_node_->get_top_n_covisibilities(10)) {
                const auto it = score_of.find((int32_t)nb->id_);
                if (it == score_of.end()) continue;
                total += it->second;
                if (best_score < it->second) {
                    best_score = it->second;
                    best = nb;
                }
            }
            records.emplace_back(total, best);
            if (i == 0 || best_total < total) best_total = total;
        }
        // rule 6
        const float thr = 0.75f * best_total;
        std::vector<keyframe*> out;
        std::set<keyframe*> seen;
        for (const auto& r : records)
            if (r.first > thr && seen.insert(r.second).second) out.push_back(r.second);
        return out;
    }

    static constexpr int kMaxWords = 13653;   // 160 KB of LDS at 12 B per query word
    bow_vocabulary* bow_vocab_;               // upstream keeps it for compute_bow; the queries read the vectors already computed
    int max_keyframes_, max_words_, wanted_words_ = 0;
    mutable std::mutex mtx_;
    ovs_bowdb* db_ = nullptr;
    std::map<int32_t, keyframe*> keyfrms_;    // everything registered
    std::set<int32_t> uploaded_;              // ... of which the handle holds
};

}   // namespace data
}   // namespace openvslam
