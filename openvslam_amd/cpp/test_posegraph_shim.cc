// Drives optimize::graph_optimizer through the class on a map tests/test_posegraph_ref.py writes: builds the keyframes with their essential
// graph and the landmarks, runs optimize once and writes what it leaves in the map. usage: test_posegraph_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, the map untouched)
//
// scene.bin: a flat array of f64 (counts and ids as doubles): fix_scale, num_iter, loop keyframe id, current keyframe id, n_keyframes; per
// keyframe: id, 16 pose_cw row-major, parent id or -1, n_children and their ids, n_loop_edges and their ids, n_weights and (id, weight)
// pairs; n_non_corrected and per entry (id, 9 rot, 3 trans, scale); n_pre_corrected likewise; n_loop_connections and per entry (id, n, ids);
// n_landmarks and per landmark (id, reference keyframe id or -1, 3 pos_w).
// out.bin: f64: per keyframe in the file's order 16 pose_cw; per landmark 3 pos_w and its normal-update count; then the failed ABI calls.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <vector>

#include "openvslam/optimize/graph_optimizer.h"

using namespace openvslam;

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        std::fprintf(stderr, "usage: %s scene.bin out.bin [device]\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> in;
    double buf[512];
    size_t got;
    while ((got = std::fread(buf, 8, 512, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    size_t at = 0;
    const auto next = [&]() -> double {
        if (at >= in.size()) {
            std::fprintf(stderr, "scene file too short\n");
            std::exit(2);
        }
        return in[at++];
    };
    if (argc == 4) optimize::graph_optimizer::set_device(std::atoi(argv[3]));

    const bool fix_scale = next() != 0.0;
    const unsigned int num_iter = (unsigned int)next();
    const unsigned int loop_id = (unsigned int)next(), curr_id = (unsigned int)next();
    const int n_kf = (int)next();
    std::vector<std::unique_ptr<data::keyframe>> kfs;
    std::map<unsigned int, data::keyframe*> by_id;
    struct Links {
        int parent;
        std::vector<unsigned int> children, loop_edges;
        std::vector<std::pair<unsigned int, unsigned int>> weights;
    };
    std::vector<Links> links((size_t)n_kf);
    for (int k = 0; k < n_kf; ++k) {
        kfs.emplace_back(new data::keyframe());
        data::keyframe& kf = *kfs.back();
        kf.id_ = (unsigned int)next();
        for (double& v : kf.cam_pose_cw_.m) v = next();
        Links& l = links[(size_t)k];
        l.parent = (int)next();
        l.children.resize((size_t)next());
        for (auto& c : l.children) c = (unsigned int)next();
        l.loop_edges.resize((size_t)next());
        for (auto& c : l.loop_edges) c = (unsigned int)next();
        l.weights.resize((size_t)next());
        for (auto& w : l.weights) {
            w.first = (unsigned int)next();
            w.second = (unsigned int)next();
        }
        by_id[kf.id_] = &kf;
    }
    data::map_database map_db;
    for (int k = 0; k < n_kf; ++k) {
        data::graph_node* g = kfs[(size_t)k]->graph_node_;
        const Links& l = links[(size_t)k];
        if (l.parent >= 0) g->spanning_parent_ = by_id.at((unsigned int)l.parent);
        for (unsigned int c : l.children) g->spanning_children_.insert(by_id.at(c));
        for (unsigned int c : l.loop_edges) g->loop_edges_.insert(by_id.at(c));
        for (const auto& w : l.weights) g->connected_keyfrms_and_weights_[by_id.at(w.first)] = w.second;
        map_db.keyframes_.push_back(kfs[(size_t)k].get());
    }
    const auto read_sim3s = [&](module::keyframe_Sim3_pairs_t& out) {
        const int n = (int)next();
        for (int k = 0; k < n; ++k) {
            data::keyframe* kf = by_id.at((unsigned int)next());
            optimize::Sim3 S;
            for (double& v : S.rot.m) v = next();
            for (double& v : S.trans.v) v = next();
            S.scale = next();
            out[kf] = S;
        }
    };
    module::keyframe_Sim3_pairs_t non_corrected, pre_corrected;
    read_sim3s(non_corrected);
    read_sim3s(pre_corrected);
    std::map<data::keyframe*, std::set<data::keyframe*>> loop_connections;
    const int n_lc = (int)next();
    for (int k = 0; k < n_lc; ++k) {
        data::keyframe* kf = by_id.at((unsigned int)next());
        const int n = (int)next();
        for (int i = 0; i < n; ++i) loop_connections[kf].insert(by_id.at((unsigned int)next()));
    }
    const int n_lm = (int)next();
    std::vector<std::unique_ptr<data::landmark>> lms;
    for (int m = 0; m < n_lm; ++m) {
        lms.emplace_back(new data::landmark());
        lms.back()->id_ = (unsigned int)next();
        const int ref = (int)next();
        lms.back()->ref_keyfrm_ = ref < 0 ? nullptr : by_id.at((unsigned int)ref);
        Vec3_t p;
        for (double& v : p.v) v = next();
        lms.back()->set_pos_in_world(p);
        map_db.landmarks_.push_back(lms.back().get());
    }

    const optimize::graph_optimizer optimizer(&map_db, fix_scale);
    optimizer.optimize(by_id.at(loop_id), by_id.at(curr_id), non_corrected, pre_corrected, loop_connections, num_iter);

    std::vector<double> out;
    for (const auto& kf : kfs) out.insert(out.end(), kf->cam_pose_cw_.m, kf->cam_pose_cw_.m + 16);
    for (const auto& lm : lms) {
        const Vec3_t p = lm->get_pos_in_world();
        out.insert(out.end(), p.v, p.v + 3);
        out.push_back((double)lm->num_normal_updates_);
    }
    const auto& c = util::device_failures();
    out.push_back((double)c.failed_calls.load());
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(out.data(), 8, out.size(), o);
    std::fclose(o);
    std::printf("%d keyframes, %d landmarks; ABI calls failed %lu, degraded %lu\n", n_kf, n_lm, c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
