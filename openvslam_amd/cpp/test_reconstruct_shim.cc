// Drives initialize::perspective through the class on the problems tests/reconstruct_io.py writes: every problem through a perspective of
// its own (the H and F RANSAC, then the pose recovery), then a caller error. Writes what the getters return.
// usage: test_reconstruct_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, initialize() == false, zeros)
//
// scene.bin (little endian): f32 reproj_err_thr, f32 parallax_deg_thr, i32 min_num_triangulated, i32 num_ransac_iters, u64 seed, f64 fx fy cx cy,
// i32 n_problems; per problem i32 n, 2 n f32 keypoints of the reference frame, 2 n f32 keypoints of the current frame (match i pairs keypoint
// i of both; the current frame's are stored in reverse here and matched across, and the reference frame gets five unmatched keypoints more).
// out.bin: per problem i32 initialised, 9 f64 rotation, 3 f64 translation, i32 m (the reference frame's keypoints), m x {3 f64 point, u8 flag}.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "openvslam/initialize/perspective.h"

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

// camera::perspective::convert_keypoints_to_bearings
void fill_bearings(data::frame& frm, const camera::base& cam) {
    frm.bearings_.resize(frm.undist_keypts_.size());
    for (size_t i = 0; i < frm.undist_keypts_.size(); ++i) {
        const double x = ((double)frm.undist_keypts_[i].pt.x - cam.cx_) / cam.fx_, y = ((double)frm.undist_keypts_[i].pt.y - cam.cy_) / cam.fy_;
        const double l = std::sqrt((x * x + y * y) + 1.0);
        frm.bearings_[i](0) = x / l, frm.bearings_[i](1) = y / l, frm.bearings_[i](2) = 1.0 / l;
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
    if (argc == 4) initialize::perspective::set_device(std::atoi(argv[3]));

    const float reproj_err_thr = r.get<float>(), parallax_deg_thr = r.get<float>();
    const unsigned int min_num_triangulated = (unsigned)r.get<int32_t>(), num_ransac_iters = (unsigned)r.get<int32_t>();
    const uint64_t seed = r.get<uint64_t>();
    camera::base cam;
    cam.fx_ = r.get<double>(), cam.fy_ = r.get<double>(), cam.cx_ = r.get<double>(), cam.cy_ = r.get<double>();
    const int n_problems = r.get<int32_t>();

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    int n_initialised = 0;
    data::frame last_ref, last_cur;
    std::vector<int> last_matches;
    for (int p = 0; p < n_problems; ++p) {
        const int n = r.get<int32_t>();
        data::frame ref_frm, cur_frm;
        ref_frm.camera_ = cur_frm.camera_ = &cam;
        ref_frm.undist_keypts_.resize((size_t)n + 5);
        cur_frm.undist_keypts_.resize((size_t)n);
        std::vector<int> ref_matches_with_cur((size_t)n + 5, -1);
        for (int i = 0; i < n; ++i) ref_frm.undist_keypts_[(size_t)i].pt.x = r.get<float>(), ref_frm.undist_keypts_[(size_t)i].pt.y = r.get<float>();
        for (int i = 0; i < n; ++i) {
            cv::KeyPoint& k = cur_frm.undist_keypts_[(size_t)(n - 1 - i)];
            k.pt.x = r.get<float>(), k.pt.y = r.get<float>();
            ref_matches_with_cur[(size_t)i] = n - 1 - i;
        }
        fill_bearings(ref_frm, cam);
        fill_bearings(cur_frm, cam);
        initialize::perspective init(ref_frm, num_ransac_iters, min_num_triangulated, parallax_deg_thr, reproj_err_thr);
        init.set_seed(seed);
        const int32_t ok = init.initialize(cur_frm, ref_matches_with_cur) ? 1 : 0;
        n_initialised += ok;
        std::fwrite(&ok, 4, 1, o);
        const Mat33_t R = init.get_rotation_ref_to_cur();
        const Vec3_t t = init.get_translation_ref_to_cur();
        std::fwrite(R.m, 8, 9, o);
        std::fwrite(t.v, 8, 3, o);
        const std::vector<Vec3_t> pts = init.get_triangulated_pts();
        const std::vector<bool> flags = init.get_triangulated_flags();
        const int32_t m = (int32_t)pts.size();
        std::fwrite(&m, 4, 1, o);
        for (size_t i = 0; i < pts.size(); ++i) {
            const uint8_t v = flags[i] ? 1 : 0;
            std::fwrite(pts[i].v, 8, 3, o);
            std::fwrite(&v, 1, 1, o);
        }
        last_ref = ref_frm, last_cur = cur_frm, last_matches = ref_matches_with_cur;
    }
    std::fclose(o);
    // a caller error throws whatever the device does: a match that points past the current frame's keypoints
    bool thrown = false;
    if (n_problems > 0) {
        last_matches[0] = (int)last_cur.undist_keypts_.size();
        initialize::perspective init(last_ref, num_ransac_iters, min_num_triangulated, parallax_deg_thr, reproj_err_thr);
        try {
            init.initialize(last_cur, last_matches);
        } catch (const std::exception&) {
            thrown = true;
        }
        if (!thrown) {
            std::fprintf(stderr, "a match past the keypoints did not throw\n");
            return 1;
        }
    }
    const auto& c = util::device_failures();
    std::printf("%d problems, %d initialised, caller error thrown %d; ABI calls failed %lu, degraded %lu\n", n_problems, n_initialised, thrown ? 1 : 0,
                c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
