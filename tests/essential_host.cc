// The essential-matrix RANSAC's algebra (openvslam_amd/csrc/essential_math.inc) run by a plain host compiler, one problem, one hypothesis
// and one match after the other: tests/test_essential_ref.py builds this with g++ -ffp-contract=off and compares every output with the
// Python reference bit for bit. It is also the host loop tools/time_essential.py times the device call against.
// usage: essential_host case.bin            per problem: "P valid best_iter num_inliers" and the score and the 9 doubles of E_21 as hex bit
//                                           patterns, then one line "F" with the flags
//        essential_host case.bin --time N   N passes over the file's problems: the median and the minimum of a pass in milliseconds
//
// case.bin (little endian): f64 residual_cos_thr, i32 max_num_iter, i32 recompute, u64 seed, i32 n_problems; per problem i32 n,
// 3 n f64 bearings of frame 1, 3 n f64 bearings of frame 2. Problem p of the file is problem p of a batch.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "essential_math.inc"

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
    std::vector<double> b1, b2;   // 3 per match
    int n() const { return (int)(b1.size() / 3); }
};

struct Outcome {
    int valid = 0, best_iter = -1, num_inliers = 0;
    double score = 0.0, E[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    std::vector<unsigned char> flags;
};

// rule E1 (3.13 rule 2): eight distinct indices below n, a function of (seed, p, h)
uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
void sample(uint64_t seed, uint32_t p, uint32_t h, uint32_t n, int (&idx)[8]) {
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    const uint64_t base = seed + G * (((((uint64_t)p) << 20) + h) * 16 + 1);
    std::vector<uint32_t> sorted;
    for (int k = 0; k < 8; ++k) {
        uint32_t v = (uint32_t)(mix64(base + G * (uint64_t)k) % (n - (uint32_t)k));
        for (const uint32_t e : sorted)
            if (v >= e) ++v;
        idx[k] = (int)v;
        sorted.insert(std::upper_bound(sorted.begin(), sorted.end(), v), v);
    }
}

// rule 6 of 3.10: 64 strided partial sums, then the pairwise tree
double tsum(const std::vector<double>& terms) {
    double part[64];
    for (double& v : part) v = 0.0;
    for (size_t i = 0; i < terms.size(); ++i) part[i % 64] = part[i % 64] + terms[i];
    for (int d = 32; d; d >>= 1)
        for (int j = 0; j < d; ++j) part[j] = part[j] + part[j + d];
    return part[0];
}

// rules E2 to E4 over the matches idx, in that order
void fit(const Case& c, const std::vector<int>& idx, double (&E)[9]) {
    std::vector<double> rows(9 * idx.size());
    for (size_t i = 0; i < idx.size(); ++i) {
        double a[9];
        ess::row_of(&c.b1[3 * (size_t)idx[i]], &c.b2[3 * (size_t)idx[i]], a);
        std::memcpy(&rows[9 * i], a, sizeof(a));
    }
    double A[9][9], V[9][9];
    std::vector<double> terms(idx.size());
    for (int r = 0; r < 9; ++r)
        for (int q = r; q < 9; ++q) {
            for (size_t i = 0; i < idx.size(); ++i) terms[i] = rows[9 * i + (size_t)r] * rows[9 * i + (size_t)q];
            A[r][q] = A[q][r] = tsum(terms);
        }
    for (int r = 0; r < 9; ++r)
        for (int q = 0; q < 9; ++q) V[r][q] = r == q ? 1.0 : 0.0;
    ess::jacobi_rounds(A, V);
    int best = 0;
    for (int i = 1; i < 9; ++i)
        if (A[i][i] < A[best][best]) best = i;
    double G[9];
    for (int j = 0; j < 9; ++j) G[j] = V[j][best];
    ess::rank_two(G, E);
}

// rule E5 over every match
double check(const Case& c, const double (&E)[9], double thr, std::vector<unsigned char>& flags, int& count) {
    const int n = c.n();
    std::vector<double> terms((size_t)n);
    flags.assign((size_t)n, 0);
    count = 0;
    for (int i = 0; i < n; ++i) {
        bool inlier;
        double r2, r1;
        terms[(size_t)i] = ess::match_term(E, &c.b1[3 * (size_t)i], &c.b2[3 * (size_t)i], thr, inlier, r2, r1);
        flags[(size_t)i] = inlier ? 1 : 0;
        count += inlier ? 1 : 0;
    }
    return tsum(terms);
}

Outcome solve(const Case& c, uint32_t p, double thr, int max_num_iter, bool recompute, uint64_t seed) {
    Outcome o;
    const int n = c.n();
    o.flags.assign((size_t)n, 0);
    if (n < 8) return o;
    double best = 0.0, E[9], Eb[9];
    int best_iter = -1, count;
    std::vector<unsigned char> flags;
    for (int h = 0; h < max_num_iter; ++h) {
        int idx[8];
        sample(seed, p, (uint32_t)h, (uint32_t)n, idx);
        fit(c, std::vector<int>(idx, idx + 8), E);
        const double score = check(c, E, thr, flags, count);
        if (best < score) {   // strict: the lowest h of a tie stays; a NaN never wins
            best = score, best_iter = h;
            std::memcpy(Eb, E, sizeof(E));
        }
    }
    if (best_iter < 0) return o;
    double score = check(c, Eb, thr, flags, count);
    if (!(score > 0.0 && count >= 8)) return o;
    if (recompute) {   // rule E7
        std::vector<int> inliers;
        for (int i = 0; i < n; ++i)
            if (flags[(size_t)i]) inliers.push_back(i);
        fit(c, inliers, E);
        bool finite = true;
        for (const double v : E) finite = finite && std::isfinite(v);
        if (finite) {
            std::memcpy(Eb, E, sizeof(E));
            score = check(c, Eb, thr, flags, count);
            if (!(score > 0.0 && count >= 8)) return o;
        }
    }
    o.valid = 1, o.best_iter = best_iter, o.num_inliers = count, o.score = score;
    std::memcpy(o.E, Eb, sizeof(Eb));
    o.flags = flags;
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

    const double thr = r.get<double>();
    const int max_num_iter = r.get<int32_t>();
    const bool recompute = r.get<int32_t>() != 0;
    const uint64_t seed = r.get<uint64_t>();
    std::vector<Case> cases((size_t)r.get<int32_t>());
    size_t total = 0;
    for (Case& c : cases) {
        const int n = r.get<int32_t>();
        for (int i = 0; i < 3 * n; ++i) c.b1.push_back(r.get<double>());
        for (int i = 0; i < 3 * n; ++i) c.b2.push_back(r.get<double>());
        total += (size_t)n;
    }
    std::vector<Outcome> out(cases.size());
    const auto pass = [&] {
        for (size_t p = 0; p < cases.size(); ++p) out[p] = solve(cases[p], (uint32_t)p, thr, max_num_iter, recompute, seed);
    };
    if (argc == 4) {
        const int passes = std::max(1, std::atoi(argv[3]));
        std::vector<double> ms;
        unsigned long valid = 0;
        for (int k = 0; k < passes + 5; ++k) {   // the first five are warm-up
            const auto t0 = std::chrono::steady_clock::now();
            pass();
            const auto t1 = std::chrono::steady_clock::now();
            for (const Outcome& o : out) valid += (unsigned long)o.valid;
            if (k >= 5) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("{\"problems\": %zu, \"matches\": %zu, \"passes\": %d, \"median_ms\": %.6f, \"min_ms\": %.6f, \"valid_per_pass\": %lu}\n", cases.size(), total,
                    passes, ms[ms.size() / 2], ms.front(), valid / (unsigned long)(passes + 5));
        return 0;
    }
    pass();
    const auto hex = [](double v) {
        unsigned long long u;
        std::memcpy(&u, &v, 8);
        return u;
    };
    for (const Outcome& o : out) {
        std::printf("P %d %d %d %016llx", o.valid, o.best_iter, o.num_inliers, hex(o.score));
        for (const double v : o.E) std::printf(" %016llx", hex(v));
        std::printf("\nF");
        for (const unsigned char v : o.flags) std::printf(" %d", (int)v);
        std::printf("\n");
    }
    return 0;
}
