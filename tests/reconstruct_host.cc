// The monocular initialiser's pose recovery (openvslam_amd/csrc/reconstruct_math.inc) run by a plain host compiler, one problem, one
// hypothesis and one match after the other: tests/test_reconstruct_ref.py builds this with g++ -ffp-contract=off and compares every output
// with the Python reference bit for bit. It is also the host loop tools/time_reconstruct.py times the device call against.
// usage: reconstruct_host case.bin            per problem: "P success best" and the 12 doubles of the pose as hex bit patterns, the eight
//                                             counts, the eight parallaxes as float bit patterns, then one line per match: flag and pos
//        reconstruct_host case.bin --time N   N passes over the file's problems: the median and the minimum of a pass in milliseconds
//
// case.bin (little endian): f32 reproj_err_thr, f32 parallax_deg_thr, i32 min_num_triangulated, i32 n_problems; per problem i32 model,
// f64 mat[9], f64 fx fy cx cy, i32 n, n x {u8 inlier, f64 kp_ref[2] kp_cur[2] bearing_ref[3] bearing_cur[3]}.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "reconstruct_math.inc"

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

struct Case {
    rec::Problem q;
    std::vector<unsigned char> inlier;
    std::vector<rec::Match> matches;
};

struct Outcome {
    int success = 0, best = -1;
    double rot[9] = {}, trans[3] = {};
    int32_t counts[rec::kMaxHypotheses] = {};
    float parallax[rec::kMaxHypotheses] = {};
    std::vector<double> pos;
    std::vector<unsigned char> flags;
};

// check_pose of hypothesis h; the points and flags where `keep` is given
void check_pose(const Case& c, const rec::Hyp& hyp, float thr_sq, int32_t& count, float& parallax, Outcome* keep) {
    std::vector<uint32_t> keys;
    for (size_t i = 0; i < c.matches.size(); ++i) {
        if (!c.inlier[i]) continue;
        const rec::Point pt = rec::check_match(c.q, hyp, c.matches[i], thr_sq);
        if (!pt.ok) continue;
        keys.push_back(rec::key_of(pt.cos));
        if (keep) {
            for (int k = 0; k < 3; ++k) keep->pos[3 * i + k] = pt.pos[k];
            keep->flags[i] = pt.small ? 0 : 1;
        }
    }
    count = (int32_t)keys.size();
    parallax = 0.0f;
    if (!keys.empty()) {
        std::sort(keys.begin(), keys.end());
        parallax = rec::parallax_deg(rec::float_of_key(keys[(size_t)rec::parallax_rank(count)]));
    }
}

Outcome reconstruct(const Case& c, float thr_sq, float parallax_deg_thr, int32_t min_num_triangulated) {
    Outcome o;
    o.pos.assign(3 * c.matches.size(), 0.0);
    o.flags.assign(c.matches.size(), 0);
    int n_hyp = 0;
    for (int h = 0; h < rec::kMaxHypotheses; ++h) {
        rec::Hyp hyp;
        if (!rec::hypothesis(c.q, h, hyp)) continue;
        n_hyp = rec::hypotheses_of_model(c.q.model);
        check_pose(c, hyp, thr_sq, o.counts[h], o.parallax[h], nullptr);
    }
    o.best = rec::most_plausible(o.counts, o.parallax, n_hyp, parallax_deg_thr, min_num_triangulated);
    if (o.best >= 0) {
        rec::Hyp hyp;
        rec::hypothesis(c.q, o.best, hyp);
        int32_t count;
        float parallax;
        check_pose(c, hyp, thr_sq, count, parallax, &o);
        o.success = 1;
        std::memcpy(o.rot, hyp.R, sizeof(o.rot));
        std::memcpy(o.trans, hyp.t, sizeof(o.trans));
    }
    return o;
}
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

    const float thr_sq = rec::threshold_sq(r.get<float>());
    const float parallax_deg_thr = r.get<float>();
    const int32_t min_num_triangulated = r.get<int32_t>();
    std::vector<Case> cases((size_t)r.get<int32_t>());
    size_t total = 0;
    for (Case& c : cases) {
        c.q.model = r.get<int32_t>();
        c.q.pad = 0;
        for (double& v : c.q.mat) v = r.get<double>();
        c.q.fx = r.get<double>(), c.q.fy = r.get<double>(), c.q.cx = r.get<double>(), c.q.cy = r.get<double>();
        for (int n = r.get<int32_t>(); n > 0; --n) {
            c.inlier.push_back(r.get<unsigned char>());
            rec::Match m;
            for (double& v : m.kp1) v = r.get<double>();
            for (double& v : m.kp2) v = r.get<double>();
            for (double& v : m.b1) v = r.get<double>();
            for (double& v : m.b2) v = r.get<double>();
            c.matches.push_back(m);
        }
        total += c.matches.size();
    }
    std::vector<Outcome> out(cases.size());
    const auto pass = [&] {
        for (size_t p = 0; p < cases.size(); ++p) out[p] = reconstruct(cases[p], thr_sq, parallax_deg_thr, min_num_triangulated);
    };
    if (argc == 4) {
        const int passes = std::max(1, std::atoi(argv[3]));
        std::vector<double> ms;
        unsigned long succeeded = 0;
        for (int k = 0; k < passes + 5; ++k) {   // the first five are warm-up
            const auto t0 = std::chrono::steady_clock::now();
            pass();
            const auto t1 = std::chrono::steady_clock::now();
            for (const Outcome& o : out) succeeded += (unsigned long)o.success;
            if (k >= 5) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("{\"problems\": %zu, \"matches\": %zu, \"passes\": %d, \"median_ms\": %.6f, \"min_ms\": %.6f, \"succeeded_per_pass\": %lu}\n", cases.size(), total,
                    passes, ms[ms.size() / 2], ms.front(), succeeded / (unsigned long)(passes + 5));
        return 0;
    }
    pass();
    const auto hex = [](double v) {
        unsigned long long u;
        std::memcpy(&u, &v, 8);
        return u;
    };
    for (const Outcome& o : out) {
        std::printf("P %d %d", o.success, o.best);
        for (double v : o.rot) std::printf(" %016llx", hex(v));
        for (double v : o.trans) std::printf(" %016llx", hex(v));
        std::printf("\nC");
        for (int32_t v : o.counts) std::printf(" %d", v);
        std::printf("\nA");
        for (float v : o.parallax) {
            unsigned u;
            std::memcpy(&u, &v, 4);
            std::printf(" %08x", u);
        }
        std::printf("\n");
        for (size_t i = 0; i < o.flags.size(); ++i) std::printf("M %d %016llx %016llx %016llx\n", (int)o.flags[i], hex(o.pos[3 * i]), hex(o.pos[3 * i + 1]), hex(o.pos[3 * i + 2]));
    }
    return 0;
}
