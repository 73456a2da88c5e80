// Drives module::search_local_landmarks through the class layer on a frame and its local map as tests/observe_scenes.py writes them: once with
// write_tracking_fields off and once with it on, each on a fresh copy of the scene.
// usage: test_search_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, 0 matches, frm.landmarks_ untouched, nothing observable)
//
// scene.bin (little endian): i32 model (0 perspective, 1 equirectangular), f64 fx fy cx cy, f32 focal_x_baseline true_baseline, i32 cols rows;
// f32 margin lowe_ratio, u32 frame id, i32 n_levels, f32 scale_factors[n_levels], f32 log_scale_factor; 16 f64 pose row-major; i32 n, i32 stereo,
// n cv::KeyPoint, n x 32 u8 descriptors, [n f32 stereo_x_right]; i32 m, 3 m f64 positions, 3 m f64 mean normals, 2 m f32 (min, max) valid distance,
// m x 32 u8 descriptors, m u8 will_be_erased, n i32 landmark the frame already holds at that keypoint (-1 none).
// out.bin, per run: u32 num_matches, n i32 frm.landmarks_ (index into the local map or -1), then per local landmark u8 is_observable_in_tracking_,
// u32 num_observable_, 2 f64 reproj_in_tracking_, f32 x_right_in_tracking_, i32 scale_level_in_tracking_.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "openvslam/module/local_landmark_search.h"

using namespace openvslam;

namespace {
struct Reader {
    const unsigned char *p, *end;
    void read(void* dst, size_t bytes) {
        if (p + bytes > end) {
            std::fprintf(stderr, "scene file too short\n");
            std::exit(2);
        }
        std::memcpy(dst, p, bytes);
        p += bytes;
    }
    template <typename T>
    T get() {
        T v;
        read(&v, sizeof(T));
        return v;
    }
};

struct Scene {
    camera::base cam;
    data::frame frm;
    std::vector<data::landmark> lms;
    std::vector<data::landmark*> local;
    float margin = 5.0f, lowe_ratio = 0.8f;
};

void read_scene(const std::vector<unsigned char>& buf, int device, Scene& s) {
    Reader r{buf.data(), buf.data() + buf.size()};
    s.cam.model_type_ = r.get<int32_t>() == 1 ? camera::model_type_t::Equirectangular : camera::model_type_t::Perspective;
    s.cam.fx_ = r.get<double>();
    s.cam.fy_ = r.get<double>();
    s.cam.cx_ = r.get<double>();
    s.cam.cy_ = r.get<double>();
    s.cam.focal_x_baseline_ = r.get<float>();
    s.cam.true_baseline_ = r.get<float>();
    s.cam.cols_ = (unsigned)r.get<int32_t>();
    s.cam.rows_ = (unsigned)r.get<int32_t>();
    s.cam.img_bounds_.max_x_ = (float)s.cam.cols_;
    s.cam.img_bounds_.max_y_ = (float)s.cam.rows_;
    s.margin = r.get<float>();
    s.lowe_ratio = r.get<float>();
    s.frm.id_ = r.get<uint32_t>();
    s.frm.camera_ = &s.cam;
    s.frm.device_cache_->device = device;
    s.frm.scale_factors_.resize((size_t)r.get<int32_t>());
    for (float& v : s.frm.scale_factors_) v = r.get<float>();
    s.frm.log_scale_factor_ = r.get<float>();
    for (int i = 0; i < 16; ++i) s.frm.cam_pose_cw_.m[i] = r.get<double>();
    const size_t n = (size_t)r.get<int32_t>();
    const bool stereo = r.get<int32_t>() != 0;
    if (stereo) s.cam.setup_type_ = camera::setup_type_t::Stereo;
    s.frm.num_keypts_ = (unsigned)n;
    s.frm.undist_keypts_.resize(n);
    r.read(s.frm.undist_keypts_.data(), n * sizeof(cv::KeyPoint));
    s.frm.descriptors_ = cv::Mat((int)n, 32, cv::CV_8U);
    r.read(s.frm.descriptors_.data, n * 32);
    if (stereo) {
        s.frm.stereo_x_right_.resize(n);
        r.read(s.frm.stereo_x_right_.data(), n * sizeof(float));
    }
    const size_t m = (size_t)r.get<int32_t>();
    s.lms.resize(m);
    for (auto& lm : s.lms)
        for (int a = 0; a < 3; ++a) lm.pos_w_(a) = r.get<double>();
    for (auto& lm : s.lms)
        for (int a = 0; a < 3; ++a) lm.mean_normal_(a) = r.get<double>();
    for (auto& lm : s.lms) {
        lm.min_valid_dist_ = r.get<float>();
        lm.max_valid_dist_ = r.get<float>();
    }
    for (auto& lm : s.lms) {
        lm.descriptor_ = cv::Mat(1, 32, cv::CV_8U);
        r.read(lm.descriptor_.data, 32);
    }
    for (auto& lm : s.lms) lm.will_be_erased_ = r.get<uint8_t>() != 0;
    for (size_t l = 0; l < m; ++l) {
        s.lms[l].id_ = (unsigned)l;
        s.local.push_back(&s.lms[l]);
    }
    s.frm.landmarks_.assign(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        const int32_t l = r.get<int32_t>();
        if (l >= 0) s.frm.landmarks_[i] = &s.lms[(size_t)l];
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
    const int device = argc == 4 ? std::atoi(argv[3]) : 0;

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    unsigned int matches[2] = {0, 0};
    for (int run = 0; run < 2; ++run) {
        Scene s;
        read_scene(buf, device, s);
        const uint32_t num = module::search_local_landmarks(s.frm, s.local, s.margin, s.lowe_ratio, run == 1);
        matches[run] = num;
        std::fwrite(&num, 4, 1, o);
        for (const data::landmark* lm : s.frm.landmarks_) {
            const int32_t idx = lm ? (int32_t)(lm - s.lms.data()) : -1;
            std::fwrite(&idx, 4, 1, o);
        }
        for (const data::landmark& lm : s.lms) {
            const uint8_t obs = lm.is_observable_in_tracking_ ? 1 : 0;
            const uint32_t num_observable = lm.num_observable_;
            const int32_t level = lm.scale_level_in_tracking_;
            std::fwrite(&obs, 1, 1, o);
            std::fwrite(&num_observable, 4, 1, o);
            std::fwrite(lm.reproj_in_tracking_.v, 8, 2, o);
            std::fwrite(&lm.x_right_in_tracking_, 4, 1, o);
            std::fwrite(&level, 4, 1, o);
        }
    }
    std::fclose(o);
    const auto& c = util::device_failures();
    std::printf("search_local_landmarks: %u matches, %u with the tracking fields written; ABI calls failed %lu, degraded %lu\n", matches[0], matches[1],
                c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
