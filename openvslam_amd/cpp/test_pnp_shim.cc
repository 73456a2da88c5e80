// Drives solve::pnp_solver through the class on the candidates tests/pnp_scene_io.py writes: every candidate solved on its own, then all of
// them by one find_via_ransac_batch. Writes what the getters return. usage: test_pnp_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, solution_is_valid() == false)
//
// scene.bin (little endian): i32 min_num_inliers, max_num_iter, recompute, u64 seed, i32 n_levels, f32 scale_factors[n_levels],
// i32 n_candidates; per candidate i32 n, 3 n f64 bearings, n i32 octaves, 3 n f64 landmark positions.
// out.bin: for the single runs, then for the batch, per candidate: i32 valid, best_iter, num_inliers, 9 f64 rotation, 3 f64 translation,
// 16 f64 get_best_cam_pose, i32 n, n u8 inlier flags.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "openvslam/solve/pnp_solver.h"

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

void write_result(FILE* o, const solve::pnp_solver& s) {
    const int32_t head[3] = {s.solution_is_valid() ? 1 : 0, s.get_best_iter(), (int32_t)s.get_num_inliers()};
    std::fwrite(head, 4, 3, o);
    const Mat33_t R = s.get_best_rotation();
    const Vec3_t t = s.get_best_translation();
    const Mat44_t pose = s.get_best_cam_pose();
    std::fwrite(R.m, 8, 9, o);
    std::fwrite(t.v, 8, 3, o);
    std::fwrite(pose.m, 8, 16, o);
    const std::vector<bool> flags = s.get_inlier_flags();
    const int32_t n = (int32_t)flags.size();
    std::fwrite(&n, 4, 1, o);
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
    if (argc == 4) solve::pnp_solver::set_device(std::atoi(argv[3]));

    const unsigned int min_num_inliers = (unsigned)r.get<int32_t>();
    const unsigned int max_num_iter = (unsigned)r.get<int32_t>();
    const bool recompute = r.get<int32_t>() != 0;
    const uint64_t seed = r.get<uint64_t>();
    std::vector<float> scale_factors((size_t)r.get<int32_t>());
    for (float& s : scale_factors) s = r.get<float>();
    const int n_candidates = r.get<int32_t>();
    std::vector<std::unique_ptr<solve::pnp_solver>> solvers;
    for (int p = 0; p < n_candidates; ++p) {
        const int n = r.get<int32_t>();
        std::vector<Vec3_t> bearings((size_t)n), landmarks((size_t)n);
        std::vector<cv::KeyPoint> keypts((size_t)n);
        for (auto& b : bearings)
            for (int x = 0; x < 3; ++x) b(x) = r.get<double>();
        for (auto& k : keypts) k.octave = r.get<int32_t>();
        for (auto& l : landmarks)
            for (int x = 0; x < 3; ++x) l(x) = r.get<double>();
        solvers.emplace_back(new solve::pnp_solver(bearings, keypts, landmarks, scale_factors, min_num_inliers));
        solvers.back()->set_seed(seed);
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    int n_valid = 0;
    for (auto& s : solvers) {
        s->find_via_ransac(max_num_iter, recompute);
        write_result(o, *s);
        n_valid += s->solution_is_valid();
    }
    std::vector<solve::pnp_solver*> all;
    for (auto& s : solvers) all.push_back(s.get());
    solve::pnp_solver::find_via_ransac_batch(all, max_num_iter, recompute);
    for (auto& s : solvers) write_result(o, *s);
    std::fclose(o);
    const auto& c = util::device_failures();
    std::printf("%d candidates, %d valid alone; ABI calls failed %lu, degraded %lu\n", n_candidates, n_valid, c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
