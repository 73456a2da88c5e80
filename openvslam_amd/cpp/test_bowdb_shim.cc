// Drives data::bow_database through the class on a scene tests/test_gpu_bowdb.py writes: keyframes with their BoW vectors, ordered
// covisibilities and connected keyframes; one loop query (a keyframe id and min_score) and one relocalisation query (a frame's BoW
// vector). Writes the ids both queries return. usage: test_bowdb_shim scene.bin out.bin
//
// scene.bin (little endian): i32 n_keyframes, then per keyframe: i32 id, i32 n_words, n_words x (i32 word, f64 value), i32 n_covisibilities,
// ids (strongest first), i32 n_connected, ids; then i32 loop query keyframe id, f32 min_score; then i32 n_words, n_words x (i32, f64) of the frame.
// out.bin: i32 n_loop, ids, i32 n_reloc, ids.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "openvslam/data/bow_database.h"

using namespace openvslam;

namespace {
struct Reader {
    const unsigned char *p, *end;
    template <typename T>
    T get() {
        if (p + sizeof(T) > end) {
            std::fprintf(stderr, "scene file too short\n");
            std::exit(2);
        }
        T v;
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
};
void read_vector(Reader& r, data::bow_vector& v) {
    const int n = r.get<int32_t>();
    for (int i = 0; i < n; ++i) {
        const int32_t w = r.get<int32_t>();
        v[(unsigned)w] = r.get<double>();
    }
}
}   // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> buf((size_t)size);
    if (std::fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    std::fclose(f);
    Reader r{buf.data(), buf.data() + buf.size()};

    const int n_kf = r.get<int32_t>();
    std::vector<std::unique_ptr<data::keyframe>> kfs;
    std::map<int32_t, data::keyframe*> by_id;
    std::vector<std::vector<int32_t>> covis((size_t)n_kf), connected((size_t)n_kf);
    for (int k = 0; k < n_kf; ++k) {
        kfs.emplace_back(new data::keyframe());
        kfs.back()->id_ = (unsigned)r.get<int32_t>();
        by_id[(int32_t)kfs.back()->id_] = kfs.back().get();
        read_vector(r, kfs.back()->bow_vec_);
        for (auto* list : {&covis[(size_t)k], &connected[(size_t)k]}) {
            const int n = r.get<int32_t>();
            for (int i = 0; i < n; ++i) list->push_back(r.get<int32_t>());
        }
    }
    for (int k = 0; k < n_kf; ++k) {
        for (int32_t id : covis[(size_t)k]) kfs[(size_t)k]->graph_node_->covisibilities_.push_back(by_id.at(id));
        for (int32_t id : connected[(size_t)k]) kfs[(size_t)k]->graph_node_->connected_keyfrms_.insert(by_id.at(id));
    }
    const int32_t qry_id = r.get<int32_t>();
    const float min_score = r.get<float>();
    data::frame frm;
    read_vector(r, frm.bow_vec_);

    data::bow_database db(nullptr, std::max(n_kf, 1));
    for (auto& k : kfs) db.add_keyframe(k.get());
    // an erase and a re-add on the way, as the mapping module's keyframe culling does
    db.erase_keyframe(kfs.front().get());
    db.add_keyframe(kfs.front().get());
    const std::vector<data::keyframe*> loop = db.acquire_loop_candidates(by_id.at(qry_id), min_score);
    const std::vector<data::keyframe*> reloc = db.acquire_relocalization_candidates(&frm);
    const auto failures = util::device_failures().failed_calls.load();
    if (failures) {
        std::fprintf(stderr, "%lu ABI calls failed\n", failures);
        return 1;
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (const auto* list : {&loop, &reloc}) {
        const int32_t n = (int32_t)list->size();
        std::fwrite(&n, 4, 1, o);
        for (const data::keyframe* k : *list) {
            const int32_t id = (int32_t)k->id_;
            std::fwrite(&id, 4, 1, o);
        }
    }
    std::fclose(o);
    std::printf("loop candidates %zu, relocalisation candidates %zu\n", loop.size(), reloc.size());
    return 0;
}
