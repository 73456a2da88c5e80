// The triangulator's algebra (openvslam_amd/csrc/triangulate_math.inc) run by a plain host compiler, one match after the other:
// tests/test_triangulate_ref.py builds this with g++ -ffp-contract=off and compares every output with the Python reference bit for bit; built
// with -fsanitize=address,undefined it has to run clean. It is also the host loop tools/time_triangulate.py times the device call against.
// usage: triangulate_host case.bin            one line per match: status method and the three doubles of pos_w as hex bit patterns
//        triangulate_host case.bin --time N   N passes over the file's matches: the median and the minimum of a pass in milliseconds
//
// case.bin (little endian): f64 cos_rays_parallax_thr, f32 ratio_factor, i32 n_problems; per problem 2 x {i32 model, f64 fx fy cx cy
// focal_x_baseline true_baseline, i32 cols rows}, f64 pose_cw_1[12], pose_cw_2[12], i32 n, n x {f64 bearing_1[3] bearing_2[3], f32 kp_1[2] kp_2[2]
// x_right_1 x_right_2 depth_1 depth_2 sigma_sq_1 sigma_sq_2 scale_factor_1 scale_factor_2}.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "triangulate_math.inc"

namespace {
struct Reader {
    const unsigned char *p, *end;
    template <typename T>
    T get() {
        if (p + sizeof(T) > end) {
            std::fprintf(stderr, "input too short\n");
            std::exit(2);
        }
        T v;
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
};

tri::Cam read_cam(Reader& r) {
    tri::Cam c;
    c.model = r.get<int32_t>();
    c.pad = 0;
    const double fx = r.get<double>(), fy = r.get<double>(), cx = r.get<double>(), cy = r.get<double>();
    c.focal_x_baseline = r.get<double>();
    c.true_baseline = r.get<double>();
    const int32_t cols = r.get<int32_t>(), rows = r.get<int32_t>();
    if (c.model == 0) c.a = fx, c.b = fy, c.c = cx, c.d = cy;
    else c.a = (double)cols, c.b = (double)rows, c.c = 0.0, c.d = 0.0;
    return c;
}

struct Batch {
    std::vector<tri::Problem> problems;
    std::vector<int> problem_of;
    std::vector<tri::Match> matches;
};
}   // namespace

int main(int argc, char** argv) {
    if (argc != 2 && !(argc == 4 && !std::strcmp(argv[2], "--time"))) {
        std::fprintf(stderr, "usage: %s case.bin [--time passes]\n", argv[0]);
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> buf((size_t)size);
    if (std::fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    std::fclose(f);
    Reader r{buf.data(), buf.data() + buf.size()};

    tri::Params prm;
    prm.cos_thr = r.get<double>();
    prm.ratio_factor = (double)r.get<float>();
    Batch b;
    const int n_problems = r.get<int32_t>();
    for (int p = 0; p < n_problems; ++p) {
        tri::Problem q;
        q.cam[0] = read_cam(r);
        q.cam[1] = read_cam(r);
        for (double& v : q.pose[0]) v = r.get<double>();
        for (double& v : q.pose[1]) v = r.get<double>();
        tri::set_centres(q);
        b.problems.push_back(q);
        for (int n = r.get<int32_t>(); n > 0; --n) {
            tri::Match m;
            for (double& v : m.b1) v = r.get<double>();
            for (double& v : m.b2) v = r.get<double>();
            for (double& v : m.kp1) v = (double)r.get<float>();
            for (double& v : m.kp2) v = (double)r.get<float>();
            m.x_right1 = (double)r.get<float>(), m.x_right2 = (double)r.get<float>();
            m.depth1 = (double)r.get<float>(), m.depth2 = (double)r.get<float>();
            m.sigma_sq1 = (double)r.get<float>(), m.sigma_sq2 = (double)r.get<float>();
            m.scale_factor1 = (double)r.get<float>(), m.scale_factor2 = (double)r.get<float>();
            b.matches.push_back(m);
            b.problem_of.push_back(p);
        }
    }
    std::vector<tri::Result> out(b.matches.size());
    const auto pass = [&] {
        for (size_t i = 0; i < b.matches.size(); ++i) out[i] = tri::triangulate(b.problems[(size_t)b.problem_of[i]], b.matches[i], prm);
    };
    if (argc == 4) {
        const int passes = std::max(1, std::atoi(argv[3]));
        std::vector<double> ms;
        unsigned long accepted = 0;
        for (int k = 0; k < passes + 5; ++k) {   // the first five are warm-up
            const auto t0 = std::chrono::steady_clock::now();
            pass();
            const auto t1 = std::chrono::steady_clock::now();
            for (const tri::Result& v : out) accepted += v.status == 0 ? 1 : 0;
            if (k >= 5) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("{\"matches\": %zu, \"passes\": %d, \"median_ms\": %.6f, \"min_ms\": %.6f, \"p90_ms\": %.6f, \"accepted_per_pass\": %lu}\n", b.matches.size(), passes,
                    ms[ms.size() / 2], ms.front(), ms[(ms.size() * 9) / 10], accepted / (unsigned long)(passes + 5));
        return 0;
    }
    pass();
    for (const tri::Result& v : out) {
        unsigned long long u[3];
        std::memcpy(u, v.pos_w, 24);
        std::printf("%d %d %016llx %016llx %016llx\n", v.status, v.method, u[0], u[1], u[2]);
    }
    return 0;
}
