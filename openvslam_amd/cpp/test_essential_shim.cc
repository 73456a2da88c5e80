// Drives solve::essential_solver through the class on the problems tests/essential_scene_io.py writes: every problem through the class on
// its own, then all of them by one find_via_ransac_batch. Writes what the getters return.
// usage: test_essential_shim scene.bin out.bin [device]
// (a device that does not exist shows the degraded result: no exception, solution_is_valid() == false)
//
// scene.bin (little endian): f64 residual_cos_thr, i32 max_num_iter, recompute, u64 seed, i32 n_problems; per problem i32 n, 3 n f64
// bearings of frame 1, 3 n f64 bearings of frame 2 (match i pairs bearing i of both; frame 2's are stored in reverse here and matched
// across).
// out.bin: for the single runs, then for the batch call, per problem: i32 valid, best_iter, num_inliers, f64 score, 9 f64 E_21, i32 n,
// n u8 inlier flags.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "openvslam/solve/essential_solver.h"

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

struct Frames {
    std::vector<Vec3_t> bearings_1, bearings_2;
    std::vector<std::pair<int, int>> matches;
};

void write_result(FILE* o, const solve::essential_solver& s) {
    const int32_t head[3] = {s.solution_is_valid() ? 1 : 0, s.get_best_iter(), (int32_t)s.get_num_inliers()};
    std::fwrite(head, 4, 3, o);
    const double score = s.get_best_score();
    std::fwrite(&score, 8, 1, o);
    const Mat33_t E = s.get_best_E_21();
    std::fwrite(E.m, 8, 9, o);
    const std::vector<bool> flags = s.get_inlier_matches();
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
    if (argc == 4) solve::essential_solver::set_device(std::atoi(argv[3]));

    const double thr = r.get<double>();
    const unsigned int max_num_iter = (unsigned)r.get<int32_t>();
    const bool recompute = r.get<int32_t>() != 0;
    const uint64_t seed = r.get<uint64_t>();
    const int n_problems = r.get<int32_t>();
    std::vector<Frames> frames((size_t)n_problems);
    std::vector<std::unique_ptr<solve::essential_solver>> solvers;
    for (Frames& fr : frames) {
        const int n = r.get<int32_t>();
        fr.bearings_1.resize((size_t)n);
        fr.bearings_2.resize((size_t)n);
        for (Vec3_t& b : fr.bearings_1)
            for (int k = 0; k < 3; ++k) b(k) = r.get<double>();
        for (int i = 0; i < n; ++i) {
            Vec3_t& b = fr.bearings_2[(size_t)(n - 1 - i)];
            for (int k = 0; k < 3; ++k) b(k) = r.get<double>();
            fr.matches.emplace_back(i, n - 1 - i);
        }
        solvers.emplace_back(new solve::essential_solver(fr.bearings_1, fr.bearings_2, fr.matches));
        solvers.back()->set_seed(seed);
        solvers.back()->set_residual_cos_thr(thr);
    }
    {   // a match that points past its bearing vector is the caller's error
        Frames bad;
        bad.bearings_1.resize(2);
        bad.bearings_2.resize(2);
        bad.matches.emplace_back(0, 2);
        bool thrown = false;
        try {
            solve::essential_solver s(bad.bearings_1, bad.bearings_2, bad.matches);
        } catch (const std::out_of_range&) {
            thrown = true;
        }
        if (!thrown) {
            std::fprintf(stderr, "a match index outside its bearing vector did not throw\n");
            return 1;
        }
    }

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    int n_valid = 0;
    for (auto& s : solvers) {
        s->find_via_ransac(max_num_iter, recompute);
        write_result(o, *s);
        n_valid += s->solution_is_valid();
    }
    std::vector<solve::essential_solver*> all;
    for (auto& s : solvers) all.push_back(s.get());
    solve::essential_solver::find_via_ransac_batch(all, max_num_iter, recompute);
    for (auto& s : solvers) write_result(o, *s);
    std::fclose(o);
    const auto& c = util::device_failures();
    std::printf("%d problems, %d valid alone; ABI calls failed %lu, degraded %lu\n", n_problems, n_valid, c.failed_calls.load(), c.degraded.load());
    if (argc == 3 && c.failed_calls.load()) return 1;   // on the default device nothing may fail
    return 0;
}
