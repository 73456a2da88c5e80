// The brute-force matcher's host plan (openvslam_amd/csrc/match_bf_plan.inc) as a stand-alone host program: no device, no library, the plain host
// compiler. usage: match_bf_plan_host ROW...   one line of output per row, read by tests/test_match_bf_plan.py. Fields are decimal integers; F is a
// float given as the hexadecimal of its bits. H = 1: the call has a handle (of capacities C1 x C2, CB problems), 0: it has none.
//   consts                                    ->  kNearSplit kNearSeg kTopK kNearQueries kNearPopcQueries
//   thr:F ratio                               ->  near_threshold
//   resolve:N1:N2                             ->  refused staged waves block lds_bytes raise_attr   mark claimed tops cnts total   (bf_resolve_plan, bf_resolve_lds)
//   near:N2:BATCH:PATH                        ->  chunks total_wg grid                                                            (bf_near_launch; PATH 0 matrix, 1 popcount)
//   buffers:N1:N2:B                           ->  near_cnt near_list near_top desc_1 desc_2 valid valid_1 n pairs count best_idx best second
//   create:OUT:N1:N2:B                        ->  status                                                                          (bf_check_create)
//   match:H:C1:C2:D1:n1:D2:n2:PAIRS:cap:NOUT  ->  status run n_out   (bf_check_match; D1 D2 PAIRS NOUT = 1: that pointer is set; n_out starts at 7)
//   batch:H:C1:C2:CB:SET:a1:s1:a2:s2:batch:cap ->  status            (bf_check_batch_dev; a = a descriptor block's address, s = its stride)
//   best2:H:C1:C2:Q:nq:T:nt:OUT               ->  status run                                                                      (bf_check_best2)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "match_bf_plan.inc"

using namespace ovs;

static std::vector<std::string> split(const char* row) {
    std::vector<std::string> v(1);
    for (const char* c = row; *c; ++c) {
        if (*c == ':') v.emplace_back();
        else v.back().push_back(*c);
    }
    return v;
}
static bool g_bad = false;
static long long num(const std::string& s, int base = 10) {
    char* end = nullptr;
    const long long x = base == 10 ? std::strtoll(s.c_str(), &end, 10) : (long long)std::strtoull(s.c_str(), &end, base);
    if (s.empty() || *end) g_bad = true;
    return x;
}
static int I(const std::string& s) { return (int)num(s); }
static float F(const std::string& s) {
    const uint32_t b = (uint32_t)num(s, 16);
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

static bool row(const char* text) {
    const std::vector<std::string> v = split(text);
    const std::string& k = v[0];
    const size_t n = v.size() - 1;
    g_bad = false;
    if (k == "consts" && n == 0) {
        std::printf("%d %d %d %d %d\n", kNearSplit, kNearSeg, kTopK, kNearQueries, kNearPopcQueries);
    } else if (k == "thr" && n == 1) {
        const float ratio = F(v[1]);
        if (g_bad) return false;
        std::printf("%u\n", near_threshold(ratio));
    } else if (k == "resolve" && n == 2) {
        const int n1 = I(v[1]), n2 = I(v[2]);
        if (g_bad || n1 < 1 || n2 < 1) return false;
        const BfResolvePlan p = bf_resolve_plan(n1, n2);
        const BfResolveLds l = bf_resolve_lds(n1, n2);
        std::printf("%d %d %d %d %zu %d %zu %zu %zu %zu %zu\n", p.refused ? 1 : 0, p.staged ? 1 : 0, p.waves, p.block, p.lds_bytes, p.raise_attr ? 1 : 0, l.mark,
                    l.claimed, l.tops, l.cnts, l.total);
    } else if (k == "near" && n == 3) {
        const BfNearLaunch l = bf_near_launch(I(v[1]), I(v[2]), I(v[3]));
        if (g_bad) return false;
        std::printf("%d %d %d\n", l.chunks, l.total_wg, l.grid);
    } else if (k == "buffers" && n == 3) {
        const BfCaps c{I(v[1]), I(v[2]), I(v[3])};
        if (g_bad || c.max_n1 < 1 || c.max_n2 < 1 || c.max_batch < 1) return false;
        const BfBuffers b = bf_buffer_bytes(c);
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", b.near_cnt, b.near_list, b.near_top, b.desc_1, b.desc_2, b.valid, b.valid_1, b.n,
                    b.pairs, b.count, b.best_idx, b.best, b.second);
    } else if (k == "create" && n == 4) {
        const ovs_status st = bf_check_create(I(v[1]) != 0, I(v[2]), I(v[3]), I(v[4]));
        if (g_bad) return false;
        std::printf("%d\n", (int)st);
    } else if (k == "match" && n == 10) {
        const BfCaps c{I(v[2]), I(v[3]), 1};
        int32_t n_out = 7;
        bool run = true;
        const ovs_status st = bf_check_match(I(v[1]) ? &c : nullptr, I(v[4]) != 0, I(v[5]), I(v[6]) != 0, I(v[7]), I(v[8]) != 0, I(v[9]), I(v[10]) ? &n_out : nullptr,
                                             &run);
        if (g_bad) return false;
        std::printf("%d %d %d\n", (int)st, run ? 1 : 0, (int)n_out);
    } else if (k == "batch" && n == 11) {
        const BfCaps c{I(v[2]), I(v[3]), I(v[4])};
        const ovs_status st = bf_check_batch_dev(I(v[1]) ? &c : nullptr, I(v[5]) != 0, (uintptr_t)num(v[6]), (size_t)num(v[7]), (uintptr_t)num(v[8]),
                                                 (size_t)num(v[9]), I(v[10]), I(v[11]));
        if (g_bad) return false;
        std::printf("%d\n", (int)st);
    } else if (k == "best2" && n == 8) {
        const BfCaps c{I(v[2]), I(v[3]), 1};
        bool run = true;
        const ovs_status st = bf_check_best2(I(v[1]) ? &c : nullptr, I(v[4]) != 0, I(v[5]), I(v[6]) != 0, I(v[7]), I(v[8]) != 0, &run);
        if (g_bad) return false;
        std::printf("%d %d\n", (int)st, run ? 1 : 0);
    } else {
        return false;
    }
    return true;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (!row(argv[i])) return 2;
    return 0;
}
