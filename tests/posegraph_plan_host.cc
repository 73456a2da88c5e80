// posegraph_plan_host.cc -- openvslam_amd/csrc/pose_graph_plan.inc through a plain host compiler, for tests/test_posegraph_ref.py (which builds
// it under AddressSanitizer and UndefinedBehaviorSanitizer): the incidence CSR against a brute-force count on generated graphs and on the
// size-zero inputs, every OVS_ERR_INVALID and OVS_ERR_CAPACITY case of check_call, and the arena's order and alignment. Every array is sized
// exactly as the plan says, so a write past one stops the program. Prints one line per group and "ok"; exit status 1 on the first miss.
// With a file argument (i32 n_v, n_e, then 2 n_e i32) it prints that graph's inc_row and inc for the test to compare with its own lists.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pose_graph_plan.inc"

namespace {

int g_checks = 0;
void expect(bool ok, const char* what, int a = 0, int b = 0) {
    ++g_checks;
    if (!ok) {
        std::printf("FAILED: %s (%d, %d)\n", what, a, b);
        std::exit(1);
    }
}

struct Lcg {
    uint64_t s;
    uint32_t next(uint32_t n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((s >> 33) % n);
    }
};

void check_graph(int32_t n_v, const std::vector<int32_t>& ij, const std::vector<uint8_t>& fixed) {
    const int32_t n_e = (int32_t)(ij.size() / 2);
    std::vector<int32_t> inc_row((size_t)n_v + 1), inc(2 * (size_t)n_e);
    const int32_t n_free = pgplan::build_incidence(n_v, n_e, ij.data(), fixed.data(), inc_row.data(), inc.data());
    int32_t want_free = 0;
    for (int32_t v = 0; v < n_v; ++v) want_free += fixed[(size_t)v] ? 0 : 1;
    expect(n_free == want_free, "free vertices", n_free, want_free);
    expect(inc_row[0] == 0 && inc_row[(size_t)n_v] == 2 * n_e, "the lists cover every end once", inc_row[(size_t)n_v], 2 * n_e);
    for (int32_t v = 0; v < n_v; ++v) {
        std::vector<int32_t> want;   // brute force: every end of every edge, in ascending edge index
        for (int32_t e = 0; e < n_e; ++e)
            for (int32_t side = 0; side < 2; ++side)
                if (ij[2 * (size_t)e + (size_t)side] == v) want.push_back(2 * e + side);
        expect(inc_row[(size_t)v + 1] - inc_row[(size_t)v] == (int32_t)want.size(), "a vertex's degree", v, (int)want.size());
        for (size_t k = 0; k < want.size(); ++k) expect(inc[(size_t)inc_row[(size_t)v] + k] == want[k], "a vertex's list", v, (int)k);
    }
}

}   // namespace

int main(int argc, char** argv) {
    if (argc == 2) {
        FILE* f = std::fopen(argv[1], "rb");
        int32_t head[2];
        if (!f || std::fread(head, 4, 2, f) != 2) return 2;
        std::vector<int32_t> ij(2 * (size_t)head[1]);
        if (!ij.empty() && std::fread(ij.data(), 4, ij.size(), f) != ij.size()) return 2;
        std::fclose(f);
        std::vector<uint8_t> fixed((size_t)head[0], 0);
        std::vector<int32_t> inc_row((size_t)head[0] + 1), inc(ij.size());
        pgplan::build_incidence(head[0], head[1], ij.data(), fixed.data(), inc_row.data(), inc.data());
        for (int32_t v : inc_row) std::printf("%d ", v);
        std::printf("\n");
        for (int32_t v : inc) std::printf("%d ", v);
        std::printf("\n");
        return 0;
    }

    // ---- the incidence CSR
    Lcg rng{12345};
    for (int round = 0; round < 60; ++round) {
        const int32_t n_v = 2 + (int32_t)rng.next(70), n_e = (int32_t)rng.next(300);
        std::vector<int32_t> ij;
        std::vector<uint8_t> fixed((size_t)n_v);
        for (auto& b : fixed) b = rng.next(4) == 0;
        for (int32_t e = 0; e < n_e; ++e) {
            const int32_t i = (int32_t)rng.next((uint32_t)n_v);
            int32_t j = (int32_t)rng.next((uint32_t)n_v - 1);
            j += j >= i ? 1 : 0;
            ij.push_back(round % 7 == 0 ? 0 : i), ij.push_back(round % 7 == 0 ? 1 + j % (n_v - 1) : j);   // every seventh graph is a hub
        }
        check_graph(n_v, ij, fixed);
    }
    check_graph(1, {}, {0});                      // one vertex, no edge
    check_graph(3, {}, {1, 0, 0});                // vertices without edges
    check_graph(2, {0, 1, 1, 0, 0, 1}, {0, 0});   // a pair joined three times, once reversed
    {
        int32_t inc_row[1] = {7};
        expect(pgplan::build_incidence(0, 0, nullptr, nullptr, inc_row, nullptr) == 0 && inc_row[0] == 0, "the empty graph");
    }
    std::printf("incidence: %d checks\n", g_checks);

    // ---- check_call
    const double R[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1}, t[6] = {0, 0, 0, 1, 0, 0}, s[2] = {1, 1};
    const uint8_t fixed[2] = {1, 0};
    const int32_t ij[2] = {0, 1}, ref[2] = {-1, 1};
    const double pos[6] = {0, 0, 1, 0, 1, 0};
    double o_rot[18], o_trans[6], o_scale[2], o_lm[6], o_info[8];
    const pgplan::Call good{2, R, t, s, fixed, R, t, s, 1, ij, R, t, s, 0, 50, 0, 2, ref, pos, o_rot, o_trans, o_scale, o_lm, o_info};
    const auto st = [&](const pgplan::Call& c, int mv = 2, int me = 1, int ml = 2) { return (int)pgplan::check_call(c, mv, me, ml); };
    expect(st(good) == OVS_OK, "a good call");
    {
        pgplan::Call c = good;
        c.out_info = nullptr;
        expect(st(c) == OVS_OK, "out_info may be NULL");
    }
#define REFUSED(field, value, what)                    \
    {                                                  \
        pgplan::Call c = good;                         \
        c.field = value;                               \
        expect(st(c) == OVS_ERR_INVALID, what);        \
    }
    REFUSED(rot_in, nullptr, "rot_in NULL")
    REFUSED(trans_in, nullptr, "trans_in NULL")
    REFUSED(scale_in, nullptr, "scale_in NULL")
    REFUSED(fixed, nullptr, "fixed NULL")
    REFUSED(nc_rot, nullptr, "nc_rot NULL")
    REFUSED(nc_trans, nullptr, "nc_trans NULL")
    REFUSED(nc_scale, nullptr, "nc_scale NULL")
    REFUSED(edge_ij, nullptr, "edge_ij NULL")
    REFUSED(edge_rot, nullptr, "edge_rot NULL")
    REFUSED(edge_trans, nullptr, "edge_trans NULL")
    REFUSED(edge_scale, nullptr, "edge_scale NULL")
    REFUSED(lm_ref_vertex, nullptr, "lm_ref_vertex NULL")
    REFUSED(lm_pos_in, nullptr, "lm_pos_in NULL")
    REFUSED(out_rot, nullptr, "out_rot NULL")
    REFUSED(out_trans, nullptr, "out_trans NULL")
    REFUSED(out_scale, nullptr, "out_scale NULL")
    REFUSED(out_lm_pos, nullptr, "out_lm_pos NULL")
    REFUSED(n_vertices, -1, "negative vertices")
    REFUSED(n_edges, -1, "negative edges")
    REFUSED(n_landmarks, -1, "negative landmarks")
    REFUSED(num_iter, 0, "num_iter < 1")
    REFUSED(pcg_max_iter, -1, "pcg_max_iter < 0")
    REFUSED(n_vertices, 1, "an edge beyond the vertices")
    const int32_t neg[2] = {-1, 1}, self[2] = {1, 1}, high[2] = {0, 2};
    REFUSED(edge_ij, neg, "a negative edge index")
    REFUSED(edge_ij, self, "i == j")
    REFUSED(edge_ij, high, "an edge index out of range")
    const int32_t ref_low[2] = {-2, 0}, ref_high[2] = {0, 2};
    REFUSED(lm_ref_vertex, ref_low, "a landmark reference below -1")
    REFUSED(lm_ref_vertex, ref_high, "a landmark reference out of range")
    const uint8_t fixed_bad[2] = {0, 2};
    REFUSED(fixed, fixed_bad, "a fixed byte other than 0 or 1")
#undef REFUSED
    expect(st(good, 1, 1, 2) == OVS_ERR_CAPACITY && st(good, 2, 0, 2) == OVS_ERR_CAPACITY && st(good, 2, 1, 1) == OVS_ERR_CAPACITY, "capacity");
    {
        pgplan::Call c = good;   // an invalid call beyond the capacity is invalid
        c.num_iter = 0;
        expect(st(c, 1, 0, 0) == OVS_ERR_INVALID, "invalid before capacity");
        pgplan::Call z{};        // nothing at all: every pointer NULL, every count zero
        z.num_iter = 1;
        expect(st(z, 1, 0, 0) == OVS_OK, "the empty call");
        pgplan::Call l = z;      // landmarks alone, none referring to a vertex
        const int32_t none[2] = {-1, -1};
        l.n_landmarks = 2, l.lm_ref_vertex = none, l.lm_pos_in = pos, l.out_lm_pos = o_lm;
        expect(st(l, 1, 0, 2) == OVS_OK, "landmarks without vertices");
        l.lm_ref_vertex = ref;
        expect(st(l, 1, 0, 2) == OVS_ERR_INVALID, "a reference into no vertices");
    }
    expect(pgplan::create_ok(1, 0, 0) && !pgplan::create_ok(0, 1, 1) && !pgplan::create_ok(1, -1, 0) && !pgplan::create_ok(1, 0, -1), "create");
    std::printf("check_call: %d checks\n", g_checks);

    // ---- the arena: in order, 256-byte aligned, the uploaded part first, growing with every count
    const int sizes[][3] = {{0, 0, 0}, {1, 0, 0}, {2, 1, 1}, {40, 115, 65}, {300, 1100, 3000}, {4000, 12000, 40000}};
    size_t last_bytes = 0;
    for (const auto& n : sizes) {
        const pgplan::Arena a = pgplan::arena_of(n[0], n[1], n[2]);
        const size_t off[] = {a.o_fixed, a.o_edge_ij, a.o_inc_row, a.o_inc, a.o_lm_ref, a.o_V,  a.o_nc, a.o_meas, a.o_lm_pos, a.upload_bytes, a.o_edge,
                              a.o_chi_e, a.o_Hd,      a.o_Lf,      a.o_g,   a.o_x,      a.o_r,  a.o_z,  a.o_p,    a.o_q,      a.o_val,        a.o_lm_out,
                              a.o_info,  a.arena_bytes};
        expect(a.o_Vt == a.upload_bytes, "the kernels' arrays begin where the upload ends");
        for (size_t k = 0; k + 1 < sizeof(off) / sizeof(off[0]); ++k) expect(off[k] % 256 == 0 && off[k] < off[k + 1], "order and alignment", n[0], (int)k);
        expect(a.o_nc - a.o_V >= 104 * (size_t)n[0] && a.o_chi_e - a.o_edge >= pgplan::kEdgeBytes * (size_t)n[1] && a.o_Lf - a.o_Hd >= 392 * (size_t)n[0] &&
                   a.arena_bytes - a.o_info >= 64 && a.o_info - a.o_lm_out >= 24 * (size_t)n[2],
               "room", n[0]);
        expect(a.arena_bytes > last_bytes || n[0] == 0, "the arena grows", n[0]);
        last_bytes = a.arena_bytes;
    }
    std::printf("arena: %d checks\nok\n", g_checks);
    return 0;
}
