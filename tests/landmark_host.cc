// The landmark upkeep's algebra (openvslam_amd/csrc/landmark_math.inc) run by a plain host compiler, one landmark after the other:
// tests/test_landmark_ref.py builds this with g++ -ffp-contract=off and compares every output with the Python reference bit for bit; built
// with -fsanitize=address,undefined it has to run clean. It is also the host loop tools/time_landmarks.py times the device call against.
// usage: landmark_host case.bin                  per landmark one line: status, the three doubles of the normal and the two floats of the range as hex
//                                                bit patterns, best_obs, the 32 descriptor bytes as hex ("-" for what rule L1 / L6 leave untouched)
//        landmark_host case.bin --time N WHAT    N passes over the file's landmarks (WHAT: 1 geometry, 2 descriptor, 3 both): the median and the
//                                                minimum of a pass in milliseconds
//
// case.bin (little endian): i32 n, T, K, L, has_use; i32 offsets[n + 1]; f64 pos_w[n][3]; i32 ref_keyfrm[n]; i32 ref_level[n]; i32 obs_keyfrm[T];
// u8 obs_desc[T][32]; u8 obs_use[T] (if has_use); f64 cam_centers[K][3]; f32 scale_factors[L].
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "landmark_math.inc"

namespace {
struct Reader {
    const unsigned char *p, *end;
    template <typename T>
    std::vector<T> get(size_t count) {
        if ((size_t)(end - p) < sizeof(T) * count) {
            std::fprintf(stderr, "input too short\n");
            std::exit(2);
        }
        std::vector<T> v(count);
        if (count) std::memcpy(v.data(), p, sizeof(T) * count);
        p += sizeof(T) * count;
        return v;
    }
};

struct Case {
    int n, T, K, L;
    std::vector<int32_t> offsets, ref_keyfrm, ref_level, obs_keyfrm;
    std::vector<double> pos_w, cam_centers;
    std::vector<uint8_t> obs_desc, obs_use;
    std::vector<float> scale_factors;
};

struct Result {
    int status = 1, best_obs = -2;   // -2: rule L1 left it untouched
    double normal[3] = {0, 0, 0};
    float min_valid = 0, max_valid = 0;
};

void geometry(const Case& c, int p, Result& r) {
    const double* pos = &c.pos_w[3 * (size_t)p];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int t = c.offsets[p]; t < c.offsets[p + 1]; ++t) {
        const double* centre = &c.cam_centers[3 * (size_t)c.obs_keyfrm[t]];
        lmk::add_ray(pos[0], pos[1], pos[2], centre[0], centre[1], centre[2], sx, sy, sz);
    }
    const int count = c.offsets[p + 1] - c.offsets[p];
    r.normal[0] = lmk::mean_of(sx, count), r.normal[1] = lmk::mean_of(sy, count), r.normal[2] = lmk::mean_of(sz, count);
    const double* centre = &c.cam_centers[3 * (size_t)c.ref_keyfrm[p]];
    lmk::valid_range(pos[0], pos[1], pos[2], centre[0], centre[1], centre[2], c.scale_factors[(size_t)c.ref_level[p]], c.scale_factors[(size_t)c.L - 1], r.min_valid,
                     r.max_valid);
}

void descriptor(const Case& c, int p, Result& r, std::vector<int>& used, std::vector<lmk::Desc>& descs, std::vector<int>& row) {
    used.clear();
    descs.clear();
    for (int t = c.offsets[p]; t < c.offsets[p + 1]; ++t)
        if (c.obs_use.empty() || c.obs_use[(size_t)t]) {
            lmk::Desc d;
            std::memcpy(d.w, &c.obs_desc[32 * (size_t)t], 32);
            used.push_back(t);
            descs.push_back(d);
        }
    const int M = (int)used.size();
    if (M == 0) {
        r.best_obs = -1;
        return;
    }
    const int rank = lmk::median_rank(M);
    uint32_t best = lmk::kNoWinner;
    row.resize((size_t)M);
    for (int i = 0; i < M; ++i) {
        for (int j = 0; j < M; ++j) row[(size_t)j] = lmk::hamming256(descs[(size_t)i], descs[(size_t)j]);
        const int median = lmk::kth_by_bisection(rank, [&](int v) {
            int count = 0;
            for (int j = 0; j < M; ++j) count += row[(size_t)j] <= v ? 1 : 0;
            return count;
        });
        best = std::min(best, lmk::winner_key(median, i));
    }
    r.best_obs = used[(size_t)lmk::winner_ordinal(best)] - c.offsets[p];
}
}   // namespace

int main(int argc, char** argv) {
    if (argc != 2 && !(argc == 5 && !std::strcmp(argv[2], "--time"))) {
        std::fprintf(stderr, "usage: %s case.bin [--time passes what]\n", argv[0]);
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
    Reader rd{buf.data(), buf.data() + buf.size()};

    Case c;
    const std::vector<int32_t> head = rd.get<int32_t>(5);
    c.n = head[0], c.T = head[1], c.K = head[2], c.L = head[3];
    if (c.n < 0 || c.T < 0 || c.K < 0 || c.L < 1) return 2;
    c.offsets = rd.get<int32_t>((size_t)c.n + 1);
    c.pos_w = rd.get<double>(3 * (size_t)c.n);
    c.ref_keyfrm = rd.get<int32_t>((size_t)c.n);
    c.ref_level = rd.get<int32_t>((size_t)c.n);
    c.obs_keyfrm = rd.get<int32_t>((size_t)c.T);
    c.obs_desc = rd.get<uint8_t>(32 * (size_t)c.T);
    if (head[4]) c.obs_use = rd.get<uint8_t>((size_t)c.T);
    c.cam_centers = rd.get<double>(3 * (size_t)c.K);
    c.scale_factors = rd.get<float>((size_t)c.L);

    std::vector<Result> out((size_t)c.n);
    std::vector<int> used, row;
    std::vector<lmk::Desc> descs;
    const auto pass = [&](int what) {
        for (int p = 0; p < c.n; ++p) {
            Result& r = out[(size_t)p];
            r.status = c.offsets[p + 1] == c.offsets[p] ? 1 : 0;
            if (r.status) continue;
            if (what & 1) geometry(c, p, r);
            if (what & 2) descriptor(c, p, r, used, descs, row);
        }
    };
    if (argc == 5) {
        const int passes = std::max(1, std::atoi(argv[3])), what = std::atoi(argv[4]);
        std::vector<double> ms;
        long checksum = 0;
        for (int k = 0; k < passes + 5; ++k) {   // the first five are warm-up
            const auto t0 = std::chrono::steady_clock::now();
            pass(what);
            const auto t1 = std::chrono::steady_clock::now();
            for (const Result& v : out) checksum += v.best_obs + (v.normal[2] > 0.0 ? 1 : 0);
            if (k >= 5) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("{\"landmarks\": %d, \"observations\": %d, \"what\": %d, \"passes\": %d, \"median_ms\": %.6f, \"min_ms\": %.6f, \"p90_ms\": %.6f, \"checksum\": %ld}\n",
                    c.n, c.T, what, passes, ms[ms.size() / 2], ms.front(), ms[(ms.size() * 9) / 10], checksum);
        return 0;
    }
    pass(3);
    for (int p = 0; p < c.n; ++p) {
        const Result& v = out[(size_t)p];
        if (v.status) {
            std::printf("1 - - - - - -2 -\n");
            continue;
        }
        unsigned long long u[3];
        unsigned int w[2];
        std::memcpy(u, v.normal, 24);
        std::memcpy(&w[0], &v.min_valid, 4);
        std::memcpy(&w[1], &v.max_valid, 4);
        std::printf("0 %016llx %016llx %016llx %08x %08x %d ", u[0], u[1], u[2], w[0], w[1], v.best_obs);
        if (v.best_obs < 0) {
            std::printf("-\n");
            continue;
        }
        const uint8_t* d = &c.obs_desc[32 * (size_t)(c.offsets[p] + v.best_obs)];
        for (int k = 0; k < 32; ++k) std::printf("%02x", d[k]);
        std::printf("\n");
    }
    return 0;
}
