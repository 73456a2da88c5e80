// Drives solve::homography_solver and solve::fundamental_solver through the classes on the problems tests/twoview_scene_io.py writes: every
// problem through each class on its own, then all of them by one both-models call. Writes what the getters return.
// usage: test_twoview_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, solution_is_valid() == false, selected 0)
//
// scene.bin (little endian): f32 sigma, i32 max_num_iter, recompute, u64 seed, i32 n_problems; per problem i32 n, 2 n f32 keypoints of
// frame 1, 2 n f32 keypoints of frame 2 (match i pairs keypoint i of both; frame 2's are stored in reverse here and matched across).
// out.bin: for the single runs, then for the both-models call, per problem: for H, then F: i32 valid, best_iter, num_inliers, f64 score,
// 9 f64 matrix, i32 n, n u8 inlier flags; then i32 selected (0 in the single runs).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "openvslam/solve/fundamental_solver.h"
#include "openvslam/solve/homography_solver.h"

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

void write_result(FILE* o, const solve::two_view_solver& s, const Mat33_t& M) {
    const int32_t head[3] = {s.solution_is_valid() ? 1 : 0, s.get_best_iter(), (int32_t)s.get_num_inliers()};
    std::fwrite(head, 4, 3, o);
    const double score = s.get_best_score();
    std::fwrite(&score, 8, 1, o);
    std::fwrite(M.m, 8, 9, o);
    const std::vector<bool> flags = s.get_inlier_matches();
    const int32_t n = (int32_t)flags.size();
    std::fwrite(&n, 4, 1, o);
    for (const bool f : flags) {
        const uint8_t v = f ? 1 : 0;
        std::fwrite(&v, 1, 1, o);
    }
}
void write_pair(FILE* o, const solve::homography_solver& h, const solve::fundamental_solver& f, const int32_t selected) {
    write_result(o, h, h.get_best_H_21());
    write_result(o, f, f.get_best_F_21());
    std::fwrite(&selected, 4, 1, o);
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
    if (argc == 4) solve::two_view_solver::set_device(std::atoi(argv[3]));

    const float sigma = r.get<float>();
    const unsigned int max_num_iter = (unsigned)r.get<int32_t>();
    const bool recompute = r.get<int32_t>() != 0;
    const uint64_t seed = r.get<uint64_t>();
    const int n_problems = r.get<int32_t>();
    std::vector<std::unique_ptr<solve::homography_solver>> hs;
    std::vector<std::unique_ptr<solve::fundamental_solver>> fs;
    for (int p = 0; p < n_problems; ++p) {
        const int n = r.get<int32_t>();
        std::vector<cv::KeyPoint> keypts_1((size_t)n), keypts_2((size_t)n);
        std::vector<std::pair<int, int>> matches;
        for (auto& k : keypts_1) k.pt.x = r.get<float>(), k.pt.y = r.get<float>();
        for (int i = 0; i < n; ++i) {
            cv::KeyPoint& k = keypts_2[(size_t)(n - 1 - i)];
            k.pt.x = r.get<float>(), k.pt.y = r.get<float>();
            matches.emplace_back(i, n - 1 - i);
        }
        hs.emplace_back(new solve::homography_solver(keypts_1, keypts_2, matches, sigma));
        fs.emplace_back(new solve::fundamental_solver(keypts_1, keypts_2, matches, sigma));
        hs.back()->set_seed(seed);
        fs.back()->set_seed(seed);
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    int n_valid = 0;
    for (int p = 0; p < n_problems; ++p) {
        hs[(size_t)p]->find_via_ransac(max_num_iter, recompute);
        fs[(size_t)p]->find_via_ransac(max_num_iter, recompute);
        write_pair(o, *hs[(size_t)p], *fs[(size_t)p], 0);
        n_valid += hs[(size_t)p]->solution_is_valid() + fs[(size_t)p]->solution_is_valid();
    }
    std::vector<std::pair<solve::two_view_solver*, solve::two_view_solver*>> pairs;
    for (int p = 0; p < n_problems; ++p) pairs.emplace_back(hs[(size_t)p].get(), fs[(size_t)p].get());
    const std::vector<int> selected = solve::two_view_solver::find_both_via_ransac_batch(pairs, max_num_iter, recompute);
    for (int p = 0; p < n_problems; ++p) write_pair(o, *hs[(size_t)p], *fs[(size_t)p], selected[(size_t)p]);
    if (n_problems > 0) {   // the initialiser's own call, on the first problem: what the batch gave its position 0
        const int one = solve::find_homography_and_fundamental(*hs[0], *fs[0], max_num_iter, recompute);
        if (one != selected[0]) {
            std::fprintf(stderr, "find_homography_and_fundamental chose %d, the batch %d\n", one, selected[0]);
            return 1;
        }
    }
    std::fclose(o);
    const auto& c = util::device_failures();
    std::printf("%d problems, %d models valid alone; ABI calls failed %lu, degraded %lu\n", n_problems, n_valid, c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
