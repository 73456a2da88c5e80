// Drives solve::sim3_solver through the class on keyframe pairs tests/sim3_scene_io.py writes: every pair solved on its own, then all of
// them by one find_via_ransac_batch. Writes what the getters return. usage: test_sim3_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, solution_is_valid() == false)
//
// scene.bin (little endian): i32 fix_scale, min_num_inliers, max_num_iter, u64 seed, i32 n_levels, f32 level_sigma_sq[n_levels], i32 n_pairs;
// per pair two keyframes (i32 model (0 perspective, 1 equirectangular), f64 fx fy cx cy, i32 cols rows, 16 f64 pose row-major, i32 n,
// n i32 octaves, 3 n f64 landmark positions, n u8 will_be_erased), then i32 n_1 and n_1 i32 matched (landmark of keyframe 2, or -1).
// out.bin: for the single runs, then for the batch, per pair: i32 valid, best_iter, num_inliers, 9 f64 rotation, 3 f64 translation,
// f32 scale, i32 n, n i32 keypoint indices in keyframe 1, n u8 inlier flags.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "openvslam/solve/sim3_solver.h"

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

struct Keyframe {
    camera::base cam;
    data::keyframe kf;
    std::vector<std::unique_ptr<data::landmark>> lms;
};

void read_keyframe(Reader& r, const std::vector<float>& sigma_sq, Keyframe& k) {
    k.cam.model_type_ = r.get<int32_t>() == 1 ? camera::model_type_t::Equirectangular : camera::model_type_t::Perspective;
    k.cam.fx_ = r.get<double>();
    k.cam.fy_ = r.get<double>();
    k.cam.cx_ = r.get<double>();
    k.cam.cy_ = r.get<double>();
    k.cam.cols_ = (unsigned)r.get<int32_t>();
    k.cam.rows_ = (unsigned)r.get<int32_t>();
    k.kf.camera_ = &k.cam;
    k.kf.level_sigma_sq_ = sigma_sq;
    for (int i = 0; i < 16; ++i) k.kf.cam_pose_cw_.m[i] = r.get<double>();
    const int n = r.get<int32_t>();
    k.kf.undist_keypts_.resize((size_t)n);
    k.kf.landmarks_.resize((size_t)n);
    for (int i = 0; i < n; ++i) k.kf.undist_keypts_[(size_t)i].octave = r.get<int32_t>();
    for (int i = 0; i < n; ++i) {
        k.lms.emplace_back(new data::landmark());
        Vec3_t pos;
        for (int x = 0; x < 3; ++x) pos(x) = r.get<double>();
        k.lms.back()->set_pos_in_world(pos);
        k.lms.back()->add_observation(&k.kf, (unsigned)i);
        k.kf.landmarks_[(size_t)i] = k.lms.back().get();
    }
    for (int i = 0; i < n; ++i) k.lms[(size_t)i]->will_be_erased_ = r.get<uint8_t>() != 0;
}

void write_result(FILE* o, const solve::sim3_solver& s) {
    const int32_t head[3] = {s.solution_is_valid() ? 1 : 0, s.get_best_iter(), (int32_t)s.get_num_inliers()};
    std::fwrite(head, 4, 3, o);
    const Mat33_t R = s.get_best_rotation_12();
    const Vec3_t t = s.get_best_translation_12();
    const float scale = s.get_best_scale_12();
    std::fwrite(R.m, 8, 9, o);
    std::fwrite(t.v, 8, 3, o);
    std::fwrite(&scale, 4, 1, o);
    const std::vector<unsigned int> idx1 = s.get_matched_indices_1();
    const std::vector<bool> flags = s.get_inlier_flags();
    const int32_t n = (int32_t)idx1.size();
    std::fwrite(&n, 4, 1, o);
    for (const unsigned int i : idx1) {
        const int32_t v = (int32_t)i;
        std::fwrite(&v, 4, 1, o);
    }
    for (const bool f : flags) {
        const uint8_t v = f ? 1 : 0;
        std::fwrite(&v, 1, 1, o);
    }
}
}   // namespace

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        std::fprintf(stderr, "usage: %s scene.bin out.bin [device]\n", argv[0]);
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
    if (argc == 4) solve::sim3_solver::set_device(std::atoi(argv[3]));

    const bool fix_scale = r.get<int32_t>() != 0;
    const unsigned int min_num_inliers = (unsigned)r.get<int32_t>();
    const unsigned int max_num_iter = (unsigned)r.get<int32_t>();
    const uint64_t seed = r.get<uint64_t>();
    std::vector<float> sigma_sq((size_t)r.get<int32_t>());
    for (float& s : sigma_sq) s = r.get<float>();
    const int n_pairs = r.get<int32_t>();
    std::vector<std::unique_ptr<Keyframe>> kfs;
    std::vector<std::unique_ptr<solve::sim3_solver>> solvers;
    for (int p = 0; p < n_pairs; ++p) {
        kfs.emplace_back(new Keyframe());
        kfs.emplace_back(new Keyframe());
        Keyframe &k1 = *kfs[kfs.size() - 2], &k2 = *kfs.back();
        read_keyframe(r, sigma_sq, k1);
        read_keyframe(r, sigma_sq, k2);
        std::vector<data::landmark*> matched((size_t)r.get<int32_t>(), nullptr);
        for (auto& m : matched) {
            const int32_t j = r.get<int32_t>();
            m = j < 0 ? nullptr : k2.kf.landmarks_.at((size_t)j);
        }
        solvers.emplace_back(new solve::sim3_solver(&k1.kf, &k2.kf, matched, fix_scale, min_num_inliers));
        solvers.back()->set_seed(seed);
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    int n_valid = 0;
    for (auto& s : solvers) {
        s->find_via_ransac(max_num_iter);
        write_result(o, *s);
        n_valid += s->solution_is_valid();
    }
    std::vector<solve::sim3_solver*> all;
    for (auto& s : solvers) all.push_back(s.get());
    solve::sim3_solver::find_via_ransac_batch(all, max_num_iter);
    for (auto& s : solvers) write_result(o, *s);
    std::fclose(o);
    const auto& c = util::device_failures();
    std::printf("%d pairs, %d valid alone; ABI calls failed %lu, degraded %lu\n", n_pairs, n_valid, c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
