// Drives optimize::transform_optimizer through the class on keyframe pairs tests/transform_scene_io.py writes: every pair optimised on its own,
// then all of them by one optimize_batch. Writes what optimize returns and leaves. usage: test_transform_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, 0 inliers, the transform and the matches untouched)
//
// scene.bin (little endian): i32 fix_scale, num_iter, f32 chi_sq, i32 n_levels, f32 inv_level_sigma_sq[n_levels], i32 n_pairs; per pair two
// keyframes (i32 model (0 perspective, 1 equirectangular), f64 fx fy cx cy, i32 cols rows, 16 f64 pose row-major, i32 n, n i32 octaves,
// 2 n f32 undistorted keypoints, 3 n f64 landmark positions, n u8 will_be_erased), i32 n_1 and n_1 i32 matched (landmark of keyframe 2, or -1),
// then the start: 9 f64 rotation, 3 f64 translation, f64 scale.
// out.bin: for the single runs, then for the batch, per pair: i32 num_inliers, 9 f64 rotation, 3 f64 translation, f64 scale, i32 n_1,
// n_1 u8 (1 where matched_lms_in_keyfrm_2 still holds a landmark).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "openvslam/optimize/transform_optimizer.h"

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

void read_keyframe(Reader& r, const std::vector<float>& inv_sigma_sq, Keyframe& k) {
    k.cam.model_type_ = r.get<int32_t>() == 1 ? camera::model_type_t::Equirectangular : camera::model_type_t::Perspective;
    k.cam.fx_ = r.get<double>();
    k.cam.fy_ = r.get<double>();
    k.cam.cx_ = r.get<double>();
    k.cam.cy_ = r.get<double>();
    k.cam.cols_ = (unsigned)r.get<int32_t>();
    k.cam.rows_ = (unsigned)r.get<int32_t>();
    k.kf.camera_ = &k.cam;
    k.kf.inv_level_sigma_sq_ = inv_sigma_sq;
    for (int i = 0; i < 16; ++i) k.kf.cam_pose_cw_.m[i] = r.get<double>();
    const int n = r.get<int32_t>();
    k.kf.undist_keypts_.resize((size_t)n);
    k.kf.landmarks_.resize((size_t)n);
    for (int i = 0; i < n; ++i) k.kf.undist_keypts_[(size_t)i].octave = r.get<int32_t>();
    for (int i = 0; i < n; ++i) {
        k.kf.undist_keypts_[(size_t)i].pt.x = r.get<float>();
        k.kf.undist_keypts_[(size_t)i].pt.y = r.get<float>();
    }
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

struct Pair {
    Keyframe k1, k2;
    std::vector<data::landmark*> matched;
    Mat33_t rot;
    Vec3_t trans;
    double scale = 1.0;
};

void write_result(FILE* o, unsigned int num_inliers, const std::vector<data::landmark*>& matched, const Mat33_t& R, const Vec3_t& t, double scale) {
    const int32_t num = (int32_t)num_inliers, n = (int32_t)matched.size();
    std::fwrite(&num, 4, 1, o);
    std::fwrite(R.m, 8, 9, o);
    std::fwrite(t.v, 8, 3, o);
    std::fwrite(&scale, 8, 1, o);
    std::fwrite(&n, 4, 1, o);
    for (const data::landmark* lm : matched) {
        const uint8_t v = lm ? 1 : 0;
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
    if (argc == 4) optimize::transform_optimizer::set_device(std::atoi(argv[3]));

    const bool fix_scale = r.get<int32_t>() != 0;
    const unsigned int num_iter = (unsigned)r.get<int32_t>();
    const float chi_sq = r.get<float>();
    std::vector<float> inv_sigma_sq((size_t)r.get<int32_t>());
    for (float& s : inv_sigma_sq) s = r.get<float>();
    const int n_pairs = r.get<int32_t>();
    std::vector<std::unique_ptr<Pair>> pairs;
    for (int p = 0; p < n_pairs; ++p) {
        pairs.emplace_back(new Pair());
        Pair& q = *pairs.back();
        read_keyframe(r, inv_sigma_sq, q.k1);
        read_keyframe(r, inv_sigma_sq, q.k2);
        q.matched.assign((size_t)r.get<int32_t>(), nullptr);
        for (auto& m : q.matched) {
            const int32_t j = r.get<int32_t>();
            m = j < 0 ? nullptr : q.k2.kf.landmarks_.at((size_t)j);
        }
        for (double& v : q.rot.m) v = r.get<double>();
        for (double& v : q.trans.v) v = r.get<double>();
        q.scale = r.get<double>();
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const optimize::transform_optimizer optimizer(fix_scale, num_iter);
    unsigned int total = 0;
    for (auto& q : pairs) {   // on copies: the batch below starts from the same inputs
        std::vector<data::landmark*> matched = q->matched;
        Mat33_t R = q->rot;
        Vec3_t t = q->trans;
        double s = q->scale;
        const unsigned int num = optimizer.optimize(&q->k1.kf, &q->k2.kf, matched, R, t, s, chi_sq);
        write_result(o, num, matched, R, t, s);
        total += num;
    }
    std::vector<optimize::transform_optimizer::candidate> all(pairs.size());
    for (size_t p = 0; p < pairs.size(); ++p) {
        Pair& q = *pairs[p];
        all[p].keyfrm_1 = &q.k1.kf, all[p].keyfrm_2 = &q.k2.kf, all[p].matched_lms_in_keyfrm_2 = &q.matched;
        all[p].rot_12 = &q.rot, all[p].trans_12 = &q.trans, all[p].scale_12 = &q.scale;
    }
    optimize::transform_optimizer::optimize_batch(all, fix_scale, num_iter, chi_sq);
    for (size_t p = 0; p < pairs.size(); ++p) write_result(o, all[p].num_inliers, pairs[p]->matched, pairs[p]->rot, pairs[p]->trans, pairs[p]->scale);
    std::fclose(o);
    const auto& c = util::device_failures();
    std::printf("%d pairs, %u inliers alone; ABI calls failed %lu, degraded %lu\n", n_pairs, total, c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
