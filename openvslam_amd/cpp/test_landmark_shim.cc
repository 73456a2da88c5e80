// Drives data::update_landmarks (openvslam/data/landmark_batch.h) on stub keyframes and landmarks as tests/landmark_io.py writes them: both
// parts in one call, then the two caller errors, which have to throw.
// usage: test_landmark_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, the landmarks left as they were)
//
// scene.bin (little endian): i32 n_keyframes, n_landmarks, n_levels; f32 scale_factors[n_levels]; per keyframe i32 n_keypts, i32 will_be_erased,
// f64 cam_center[3], i32 octaves[n_keypts], u8 descriptors[n_keypts][32]; per landmark f64 pos_w[3], i32 ref_keyfrm, i32 n_obs, n_obs x {i32
// keyframe, i32 keypoint}. The keyframes live in one array, so that the iteration order of a landmark's observations_ (a std::map keyed by the
// keyframe's address) is ascending keyframe number.
// out.bin: per landmark 3 f64 mean_normal_, f32 min_valid_dist_, f32 max_valid_dist_, i32 num_normal_updates_, i32 has_descriptor, then its 32
// bytes if it has one.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "openvslam/data/landmark_batch.h"

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
}   // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s scene.bin out.bin [device]\n", argv[0]);
        return 2;
    }
    const int device = argc > 3 ? std::atoi(argv[3]) : 0;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> buf((size_t)size);
    if (std::fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    std::fclose(f);
    Reader r{buf.data(), buf.data() + buf.size()};

    const int K = r.get<int32_t>(), n = r.get<int32_t>(), L = r.get<int32_t>();
    std::vector<float> scale_factors((size_t)L);
    for (float& v : scale_factors) v = r.get<float>();
    camera::base cam;
    cam.cols_ = 640, cam.rows_ = 480;
    cam.img_bounds_.max_x_ = 640.0f, cam.img_bounds_.max_y_ = 480.0f;
    std::vector<data::keyframe> keyfrms((size_t)K);   // one array: ascending address = ascending number
    for (int k = 0; k < K; ++k) {
        data::keyframe& kf = keyfrms[(size_t)k];
        const int nkp = r.get<int32_t>();
        kf.id_ = (unsigned)k;
        kf.will_be_erased_ = r.get<int32_t>() != 0;
        kf.camera_ = &cam;
        kf.device_cache_->device = device;
        kf.scale_factors_ = scale_factors;
        for (int x = 0; x < 3; ++x) kf.cam_pose_cw_(x, 3) = -r.get<double>();   // R = I: the centre is -t
        kf.num_keypts_ = (unsigned)nkp;
        kf.undist_keypts_.resize((size_t)nkp);
        for (int i = 0; i < nkp; ++i) {
            kf.undist_keypts_[(size_t)i].pt.x = (float)(7 * i % 640);
            kf.undist_keypts_[(size_t)i].pt.y = (float)(11 * i % 480);
            kf.undist_keypts_[(size_t)i].octave = r.get<int32_t>();
        }
        kf.keypts_ = kf.undist_keypts_;
        kf.descriptors_.create(nkp, 32, cv::CV_8U);
        for (int i = 0; i < nkp; ++i)
            for (int b = 0; b < 32; ++b) kf.descriptors_.ptr(i)[b] = r.get<uint8_t>();
    }
    std::vector<data::landmark> landmarks((size_t)n);
    std::vector<data::landmark*> list;
    for (int p = 0; p < n; ++p) {
        data::landmark& lm = landmarks[(size_t)p];
        lm.id_ = (unsigned)p;
        lm.num_observations_ = 0;
        for (int x = 0; x < 3; ++x) lm.pos_w_(x) = r.get<double>();
        lm.ref_keyfrm_ = &keyfrms[(size_t)r.get<int32_t>()];
        for (int k = r.get<int32_t>(); k > 0; --k) {
            const int kf = r.get<int32_t>(), idx = r.get<int32_t>();
            lm.add_observation(&keyfrms[(size_t)kf], (unsigned)idx);
        }
        lm.mean_normal_(0) = -7.0, lm.min_valid_dist_ = -3.0f, lm.max_valid_dist_ = -3.0f;   // what a landmark left alone keeps
        list.push_back(&lm);
    }

    data::set_landmark_update_device(device);
    const bool ok = data::update_landmarks(list, true, true);
    std::printf("update_landmarks %s\n", ok ? "ok" : "degraded");

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (const data::landmark& lm : landmarks) {
        std::fwrite(lm.mean_normal_.v, 8, 3, o);
        std::fwrite(&lm.min_valid_dist_, 4, 1, o);
        std::fwrite(&lm.max_valid_dist_, 4, 1, o);
        const int32_t updates = (int32_t)lm.num_normal_updates_, has = lm.descriptor_.empty() ? 0 : 1;
        std::fwrite(&updates, 4, 1, o);
        std::fwrite(&has, 4, 1, o);
        if (has) std::fwrite(lm.descriptor_.data, 1, 32, o);
    }
    std::fclose(o);

    // the caller errors: both are decided before the device is touched
    int thrown = 0;
    for (data::landmark& lm : landmarks) {
        if (lm.observations_.empty() || (int)lm.observations_.size() == K) continue;
        data::keyframe* const was = lm.ref_keyfrm_;
        for (data::keyframe& kf : keyfrms)
            if (!lm.is_observed_in_keyframe(&kf)) lm.ref_keyfrm_ = &kf;
        try {
            data::update_landmarks({&lm}, true, false);
        } catch (const std::invalid_argument&) {
            ++thrown;
        }
        lm.ref_keyfrm_ = was;
        break;
    }
    for (data::landmark& lm : landmarks) {
        if (lm.observations_.size() < 2) continue;
        data::keyframe* const last = lm.observations_.rbegin()->first;
        last->scale_factors_.back() += 1.0f;
        try {
            data::update_landmarks({&lm}, false, true);
        } catch (const std::invalid_argument&) {
            ++thrown;
        }
        last->scale_factors_.back() -= 1.0f;
        break;
    }
    std::printf("caller errors thrown %d\n", thrown);
    const auto& c = util::device_failures();
    std::printf("ABI calls failed %lu, degraded %lu\n", c.failed_calls.load(), c.degraded.load());
    return 0;
}
