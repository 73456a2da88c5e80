// The window matchers' host plan (openvslam_amd/csrc/match_window_plan.inc) as a stand-alone host program: no device, no library, the plain host
// compiler. usage: match_window_plan_host ROW...   one line of output per row, read by tests/test_match_window_plan.py. Fields are decimal integers;
// F is a float and D a double given (and printed) as the hexadecimal of its bits.
//   resolve:NQ:NT:WIDE_FROM                 ->  ok fixed_bytes offsets_in_lds lds_bytes key_pool width                     (resolve_plan, resolve_lds_bytes)
//   grid:N:CELLS                            ->  items_in_lds lds_bytes raise_attr                                          (grid_launch_plan)
//   gridok:COLS:ROWS:F minx:F miny:F maxx:F maxy  ->  0 | 1                                                               (grid_params_ok)
//   gridp:COLS:ROWS:F minx:F miny:F maxx:F maxy   ->  F min_x  F min_y  F inv_w  F inv_h  cols rows                        (make_gridp)
//   dead:THR:F ratio                        ->  dead_from_ratio          deadthr:THR  ->  dead_from_thr
//   centre:D x 12                           ->  D x 3                                                                      (camera_centre)
//   sim3:D x 12                             ->  D x 12 (P)  D x 3 (centre)                                                 (decompose_sim3)
//   motion:SETUP:D baseline:D x 12:D x 12   ->  forward backward                                                           (motion_direction: current, last)
//   twoway:D s:D x 9 rot:D x 3 trans        ->  D x 12 (S12)  D x 12 (S21)                                                 (sim3_both_ways)
//   pad:NUM_LEVELS:HAS_SRC                  ->  16 numbers: src[l] = l + 1 for the levels in use, 0.5 beyond               (pad_levels)
//   arena:N:STEREO                          ->  cap o_kps o_desc o_xr o_cellof o_items o_start arena_bytes upload_bytes stage_bytes
//   capacity:T:Q                            ->  stage_capacity
//   stage:ENTRY:T:Q:RESIDENT[:KF_NODES:NQ:FRM_NODES:NFI]  ->  need capacity overflow  then one  off,bytes,copied  per placed array
//       ENTRY: grid frame_and_landmarks area current_and_last frame_and_keyframe sim3_transform fuse mutual bow tri (the last two take the four CSR
//       sizes). need: the entry's staging over a counting writer; the rest from a second run into a real buffer of stage_capacity(T, Q) bytes:
//       copied = 1 the array's bytes lie at its offset, 0 they do not, - the array is reserved (a kernel fills it).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "match_window_plan.inc"

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
static double D(const std::string& s) {
    const uint64_t b = (uint64_t)num(s, 16);
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}
static void outF(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    std::printf("%08" PRIx32 " ", b);
}
static void outD(const double* d, int n) {
    for (int i = 0; i < n; ++i) {
        uint64_t b;
        std::memcpy(&b, d + i, 8);
        std::printf("%016" PRIx64 " ", b);
    }
}
static void doubles(const std::vector<std::string>& v, size_t at, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = D(v[at + i]);
}

static size_t run_entry(const std::string& e, StageWriter& w, const StageSources& s, int T, int Q, bool res, const int* csr) {
    if (e == "grid") return stage_need_grid(w, s, T);
    if (e == "frame_and_landmarks") return stage_need_frame_and_landmarks(w, s, T, Q, res);
    if (e == "area") return stage_need_area(w, s, T, Q, res);
    if (e == "current_and_last") return stage_need_current_and_last(w, s, T, Q, res);
    if (e == "frame_and_keyframe") return stage_need_frame_and_keyframe(w, s, T, Q, res);
    if (e == "sim3_transform") return stage_need_sim3_transform(w, s, T, Q, res);
    if (e == "fuse") return stage_need_fuse(w, s, T, Q, res);
    if (e == "mutual") return stage_need_mutual(w, s, std::min(T, Q), std::min(T, Q), res);
    if (e == "bow" || e == "tri") return stage_need_bow(w, s, T, Q, csr[0], csr[1], csr[2], csr[3], e == "tri", res);
    g_bad = true;
    return 0;
}

static bool stage_row(const std::vector<std::string>& v) {
    const bool bow = v.size() > 1 && (v[1] == "bow" || v[1] == "tri");
    if (v.size() != (bow ? 9u : 5u)) return false;
    const int T = I(v[2]), Q = I(v[3]);
    const bool res = I(v[4]) != 0;
    int csr[4] = {0, 0, 0, 0};
    for (int i = 0; bow && i < 4; ++i) csr[i] = I(v[5 + i]);
    if (g_bad || T < 1 || Q < 1) return false;
    StageCount count;
    const size_t need = run_entry(v[1], count.w, count.s, T, Q, res, csr);
    if (g_bad) return false;
    // the same staging into a real buffer: sources of every element type, large enough for the longest array of that type, no two bytes in a row equal
    const size_t M = (size_t)std::max(T, Q), cap = stage_capacity((size_t)T, (size_t)Q);
    std::vector<ovs_keypoint> kps(M);
    std::vector<uint8_t> u8(32 * M);
    std::vector<float> f32(std::max<size_t>(2 * M, OVS_MAX_LEVELS));
    std::vector<double> f64(3 * M);
    std::vector<int32_t> i32(std::max<size_t>(M + 1, (size_t)std::max(std::max(csr[0], csr[2]) + 1, std::max(csr[1], csr[3]))));
    uint32_t x = 12345u;
    const auto fill = [&](void* p, size_t bytes) {
        for (size_t i = 0; i < bytes; ++i) static_cast<unsigned char*>(p)[i] = (unsigned char)((x = x * 1664525u + 1013904223u) >> 24);
    };
    fill(kps.data(), sizeof(ovs_keypoint) * kps.size());
    fill(u8.data(), u8.size());
    fill(f32.data(), 4 * f32.size());
    fill(f64.data(), 8 * f64.size());
    fill(i32.data(), 4 * i32.size());
    std::vector<unsigned char> h(cap, 0), d(cap, 0);
    StagePlacement trace[64];
    StageWriter w(h.data(), d.data(), cap);
    w.trace = trace;
    const StageSources src{kps.data(), u8.data(), f32.data(), f64.data(), i32.data()};
    const size_t used = run_entry(v[1], w, src, T, Q, res, csr);
    std::printf("%zu %zu %d", need, cap, (w.overflow || count.w.overflow || used != need) ? 1 : 0);
    for (int i = 0; i < w.placed && i < 64; ++i) {
        const StagePlacement& p = trace[i];
        std::printf(" %zu,%zu,%s", p.off, p.bytes, !p.src ? "-" : (std::memcmp(h.data() + p.off, p.src, p.bytes) == 0 ? "1" : "0"));
    }
    std::printf("\n");
    return true;
}

static bool row(const char* text) {
    const std::vector<std::string> v = split(text);
    const std::string& k = v[0];
    const size_t n = v.size() - 1;
    g_bad = false;
    if (k == "resolve" && n == 3) {
        const ResolveLaunch l = resolve_plan(I(v[1]), I(v[2]), I(v[3]));
        if (g_bad) return false;
        std::printf("%d %zu %d %zu %u %d\n", l.ok ? 1 : 0, resolve_lds_bytes(I(v[1]), I(v[2])), l.offsets_in_lds, l.lds_bytes, l.key_pool, l.width);
    } else if (k == "grid" && n == 2) {
        const GridLaunch l = grid_launch_plan(I(v[1]), I(v[2]));
        if (g_bad) return false;
        std::printf("%d %zu %d\n", l.items_in_lds, l.lds_bytes, l.raise_attr ? 1 : 0);
    } else if ((k == "gridok" || k == "gridp") && n == 6) {
        const ovs_grid_params p{F(v[3]), F(v[4]), F(v[5]), F(v[6]), I(v[1]), I(v[2])};
        if (g_bad) return false;
        if (k == "gridok") {
            std::printf("%d\n", grid_params_ok(&p) ? 1 : 0);
        } else {
            const GridP g = make_gridp(p);
            outF(g.min_x), outF(g.min_y), outF(g.inv_w), outF(g.inv_h);
            std::printf("%d %d\n", g.cols, g.rows);
        }
    } else if (k == "dead" && n == 2) {
        const uint32_t d = dead_from_ratio((uint32_t)I(v[1]), F(v[2]));
        if (g_bad) return false;
        std::printf("%u\n", d);
    } else if (k == "deadthr" && n == 1) {
        const uint32_t d = dead_from_thr((uint32_t)I(v[1]));
        if (g_bad) return false;
        std::printf("%u\n", d);
    } else if (k == "centre" && n == 12) {
        double P[12], cc[3];
        doubles(v, 1, 12, P);
        if (g_bad) return false;
        camera_centre(P, cc);
        outD(cc, 3);
        std::printf("\n");
    } else if (k == "sim3" && n == 12) {
        double S[12], P[12], cc[3];
        doubles(v, 1, 12, S);
        if (g_bad) return false;
        decompose_sim3(S, P, cc);
        outD(P, 12), outD(cc, 3);
        std::printf("\n");
    } else if (k == "motion" && n == 26) {
        ovs_camera cam{};
        double cur[12], last[12];
        cam.setup = I(v[1]);
        cam.true_baseline = D(v[2]);
        doubles(v, 3, 12, cur), doubles(v, 15, 12, last);
        if (g_bad) return false;
        int fwd, bwd;
        motion_direction(&cam, cur, last, &fwd, &bwd);
        std::printf("%d %d\n", fwd, bwd);
    } else if (k == "twoway" && n == 13) {
        double r[9], t[3], S12[12], S21[12];
        const double s = D(v[1]);
        doubles(v, 2, 9, r), doubles(v, 11, 3, t);
        if (g_bad) return false;
        sim3_both_ways(s, r, t, S12, S21);
        outD(S12, 12), outD(S21, 12);
        std::printf("\n");
    } else if (k == "pad" && n == 2) {
        float src[OVS_MAX_LEVELS], dst[OVS_MAX_LEVELS];
        for (int l = 0; l < OVS_MAX_LEVELS; ++l) src[l] = (float)(l + 1);
        const int levels = I(v[1]), has = I(v[2]);
        if (g_bad || levels < 1 || levels > OVS_MAX_LEVELS) return false;
        pad_levels(dst, has ? src : nullptr, levels, 0.5f);
        for (int l = 0; l < OVS_MAX_LEVELS; ++l) std::printf("%g ", dst[l]);
        std::printf("\n");
    } else if (k == "arena" && n == 2) {
        const int nk = I(v[1]), stereo = I(v[2]);
        if (g_bad || nk < 0) return false;
        const FrameArena a = frame_arena_of(nk);
        const size_t up = frame_upload_bytes(a, nk, stereo != 0);
        std::printf("%d %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", a.cap, a.o_kps, a.o_desc, a.o_xr, a.o_cellof, a.o_items, a.o_start, a.arena_bytes, up,
                    frame_stage_bytes(a, up));
    } else if (k == "capacity" && n == 2) {
        const size_t c = stage_capacity((size_t)I(v[1]), (size_t)I(v[2]));
        if (g_bad) return false;
        std::printf("%zu\n", c);
    } else if (k == "stage") {
        return stage_row(v);
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
