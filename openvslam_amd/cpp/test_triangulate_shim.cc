// Drives module::two_view_triangulator through the class on a keyframe and its neighbours as tests/triangulate_io.py writes them: every pair
// on its own (upstream's triangulate), every neighbour by one call, then all neighbours by one triangulate_neighbours.
// usage: test_triangulate_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, nothing accepted)
//
// scene.bin (little endian): f32 rays_parallax_deg_thr, f32 scale_factor, i32 n_levels, f32 scale_factors[n_levels], f32 level_sigma_sq[n_levels],
// i32 n_neighbours; the current keyframe, then per neighbour its keyframe, i32 n_matches and n_matches x {i32 idx_1, i32 idx_2}.
// A keyframe: i32 model (0 perspective, 1 equirectangular), f64 fx fy cx cy, f32 focal_x_baseline true_baseline, i32 cols rows, 16 f64 pose
// row-major, i32 n, n i32 octaves, 2 n f32 undistorted keypoints, 3 n f64 bearings, n f32 stereo_x_right, n f32 depths.
// out.bin: three sections (single, per neighbour, all neighbours), each per neighbour: i32 n_matches, i32 num_accepted, n_matches x {u8 accepted,
// 3 f64 pos_w}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "openvslam/module/two_view_triangulator.h"

using namespace openvslam;
using triangulator = module::two_view_triangulator;

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
};

void read_keyframe(Reader& r, float scale_factor, const std::vector<float>& scale_factors, const std::vector<float>& level_sigma_sq, Keyframe& k) {
    k.cam.model_type_ = r.get<int32_t>() == 1 ? camera::model_type_t::Equirectangular : camera::model_type_t::Perspective;
    k.cam.fx_ = r.get<double>();
    k.cam.fy_ = r.get<double>();
    k.cam.cx_ = r.get<double>();
    k.cam.cy_ = r.get<double>();
    k.cam.focal_x_baseline_ = r.get<float>();
    k.cam.true_baseline_ = r.get<float>();
    k.cam.cols_ = (unsigned)r.get<int32_t>();
    k.cam.rows_ = (unsigned)r.get<int32_t>();
    k.kf.camera_ = &k.cam;
    k.kf.scale_factor_ = scale_factor;
    k.kf.scale_factors_ = scale_factors;
    k.kf.level_sigma_sq_ = level_sigma_sq;
    for (int i = 0; i < 16; ++i) k.kf.cam_pose_cw_.m[i] = r.get<double>();
    const size_t n = (size_t)r.get<int32_t>();
    k.kf.undist_keypts_.resize(n);
    k.kf.bearings_.resize(n);
    k.kf.stereo_x_right_.resize(n);
    k.kf.depths_.resize(n);
    for (size_t i = 0; i < n; ++i) k.kf.undist_keypts_[i].octave = r.get<int32_t>();
    for (size_t i = 0; i < n; ++i) {
        k.kf.undist_keypts_[i].pt.x = r.get<float>();
        k.kf.undist_keypts_[i].pt.y = r.get<float>();
    }
    for (size_t i = 0; i < n; ++i)
        for (int x = 0; x < 3; ++x) k.kf.bearings_[i](x) = r.get<double>();
    for (size_t i = 0; i < n; ++i) k.kf.stereo_x_right_[i] = r.get<float>();
    for (size_t i = 0; i < n; ++i) k.kf.depths_[i] = r.get<float>();
}

void write_neighbour(FILE* o, unsigned int num_accepted, const std::vector<Vec3_t>& positions, const std::vector<bool>& accepted) {
    const int32_t n = (int32_t)positions.size(), num = (int32_t)num_accepted;
    std::fwrite(&n, 4, 1, o);
    std::fwrite(&num, 4, 1, o);
    for (size_t i = 0; i < positions.size(); ++i) {
        const uint8_t ok = accepted[i] ? 1 : 0;
        std::fwrite(&ok, 1, 1, o);
        std::fwrite(positions[i].v, 8, 3, o);
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
    if (argc == 4) triangulator::set_device(std::atoi(argv[3]));

    const float deg_thr = r.get<float>(), scale_factor = r.get<float>();
    std::vector<float> scale_factors((size_t)r.get<int32_t>()), level_sigma_sq(scale_factors.size());
    for (float& v : scale_factors) v = r.get<float>();
    for (float& v : level_sigma_sq) v = r.get<float>();
    const int n_neighbours = r.get<int32_t>();
    Keyframe curr;
    read_keyframe(r, scale_factor, scale_factors, level_sigma_sq, curr);
    std::vector<std::unique_ptr<Keyframe>> neighbours;
    std::vector<data::keyframe*> neighbour_ptrs;
    std::vector<triangulator::match_list> matches((size_t)n_neighbours);
    for (int k = 0; k < n_neighbours; ++k) {
        neighbours.emplace_back(new Keyframe());
        read_keyframe(r, scale_factor, scale_factors, level_sigma_sq, *neighbours.back());
        neighbour_ptrs.push_back(&neighbours.back()->kf);
        for (int n = r.get<int32_t>(); n > 0; --n) {
            const unsigned int idx_1 = (unsigned)r.get<int32_t>(), idx_2 = (unsigned)r.get<int32_t>();
            matches[(size_t)k].emplace_back(idx_1, idx_2);
        }
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    unsigned int total = 0;
    for (int k = 0; k < n_neighbours; ++k) {   // upstream's loop: one pair at a time
        const triangulator t(&curr.kf, neighbour_ptrs[(size_t)k], deg_thr);
        std::vector<Vec3_t> positions;
        std::vector<bool> accepted;
        unsigned int num = 0;
        for (const auto& m : matches[(size_t)k]) {
            Vec3_t pos_w;
            accepted.push_back(t.triangulate(m.first, m.second, pos_w));
            positions.push_back(pos_w);
            num += accepted.back() ? 1 : 0;
        }
        write_neighbour(o, num, positions, accepted);
        total += num;
    }
    for (int k = 0; k < n_neighbours; ++k) {   // one neighbour per call
        const triangulator t(&curr.kf, neighbour_ptrs[(size_t)k], deg_thr);
        std::vector<Vec3_t> positions;
        std::vector<bool> accepted;
        const unsigned int num = t.triangulate(matches[(size_t)k], positions, accepted);
        write_neighbour(o, num, positions, accepted);
    }
    {   // all neighbours in one call
        std::vector<std::vector<Vec3_t>> positions;
        std::vector<std::vector<bool>> accepted;
        const std::vector<unsigned int> num = triangulator::triangulate_neighbours(&curr.kf, neighbour_ptrs, matches, positions, accepted, deg_thr);
        for (int k = 0; k < n_neighbours; ++k) write_neighbour(o, num[(size_t)k], positions[(size_t)k], accepted[(size_t)k]);
    }
    std::fclose(o);
    const auto& c = util::device_failures();
    std::printf("%d neighbours, %u accepted pair by pair; ABI calls failed %lu, degraded %lu\n", n_neighbours, total, c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
