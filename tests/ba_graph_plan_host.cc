// The local-BA graph's host plan (openvslam_amd/csrc/ba_graph_plan.inc) as a stand-alone host program: no device, no library, the plain host compiler.
// usage: ba_graph_plan_host ROW...   one line of output per row, sections separated by " | ", read by tests/test_ba_graph_plan.py:
//   lm:COUNTS                              ->  n_lm_wg pl_bound | wg_first[0 .. n_lm_wg]                     (partition_landmarks)
//   chunks:COUNTS                          ->  n_chunks max_chunks | chunk_start[0 .. n_pose] | chunk_kf     (partition_chunks, graph_arena_of)
//   pairs:NFREE                            ->  n_pairs cap n_pair_wg | pair_ab | wg_pair[8 cap]              (pair_table, pair_work_order)
//   slots:FLAGS  |  slots:none:N           ->  n_free | slot[N] | slot_pose[n_free]                          (assign_slots; FLAGS: a digit per keyframe)
//   graph:NPOSE:NPT:NEDGE:NFREE            ->  the 21 offsets in arena order | early upload dup_host image arena | max_chunks n_pairs cap
//   solver:NPOSE:NPT:NEDGE:NFREE:NPAIRS:PL_BOUND:SOLVE_DOUBLES  ->  the 10 offsets in arena order | arena n_lists ff_bytes pl_ok
//   index:FILE                             ->  bad E   or   ok | lm_start | lm_edges | lm_nmono | pose_start | pose_edges | pose_pt | pose pt of every record
//                                              | ox oy oxr w of every record (%a)                            (index_pass1, index_pass2)
// COUNTS: comma-separated edge counts of consecutive landmarks / keyframes, CxR = R times C.
// FILE: int32 n_pose, n_pt, n_mono, n_stereo, then the ovs_ba_edge and the ovs_ba_edge_stereo records.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba_graph_plan.inc"

static bool fields(const char* row, const char* kind, size_t want, std::vector<long long>& v) {
    const size_t k = std::strlen(kind);
    if (std::strncmp(row, kind, k) != 0 || row[k] != ':') return false;
    v.clear();
    for (const char* at = row + k; *at == ':';) {
        char* end = nullptr;
        v.push_back(std::strtoll(at + 1, &end, 10));
        if (end == at + 1) return false;
        at = end;
    }
    return v.size() == want;
}

// "3,1x256,0" -> starts of the lists: 0 3 4 5 ... (the prefix sums the partitions read)
static bool starts_of(const char* spec, std::vector<int32_t>& start) {
    start.assign(1, 0);
    for (const char* at = spec; *at;) {
        char* end = nullptr;
        const long c = std::strtol(at, &end, 10);
        if (end == at || c < 0) return false;
        long rep = 1;
        if (*end == 'x') {
            at = end + 1;
            rep = std::strtol(at, &end, 10);
            if (end == at || rep < 1) return false;
        }
        for (long i = 0; i < rep; ++i) start.push_back(start.back() + (int32_t)c);
        if (*end == ',') ++end;
        else if (*end) return false;
        at = end;
    }
    return start.size() > 1;
}

template <class T>
static void put(const T* p, size_t n, const char* sep = " | ") {
    std::fputs(sep, stdout);
    for (size_t i = 0; i < n; ++i) std::printf(i ? " %lld" : "%lld", (long long)p[i]);
}

static bool index_row(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t h[4];
    bool ok = std::fread(h, sizeof(int32_t), 4, f) == 4 && h[0] >= 1 && h[1] >= 1 && h[2] >= 0 && h[3] >= 0;
    std::vector<ovs_ba_edge> mono(ok ? (size_t)h[2] : 0);
    std::vector<ovs_ba_edge_stereo> stereo(ok ? (size_t)h[3] : 0);
    ok = ok && std::fread(mono.data(), sizeof(ovs_ba_edge), mono.size(), f) == mono.size() &&
         std::fread(stereo.data(), sizeof(ovs_ba_edge_stereo), stereo.size(), f) == stereo.size();
    std::fclose(f);
    if (!ok) return false;
    const int n_pose = h[0], n_pt = h[1], n_mono = h[2], n_stereo = h[3], ne = n_mono + n_stereo;
    // every array exactly as long as the plan says it is: an overrun is the sanitizer's to find
    std::vector<ovs::EdgeRec> edges((size_t)ne);
    std::vector<int32_t> edge_pose((size_t)ne), edge_pt((size_t)ne), lm_start((size_t)n_pt + 1), lm_nmono((size_t)n_pt), pose_start((size_t)n_pose + 1),
        lm_cursor((size_t)n_pt), pose_cursor((size_t)n_pose), lm_edges((size_t)ne), pose_edges((size_t)ne), pose_pt((size_t)ne);
    const int bad = ovs::index_pass1(mono.data(), n_mono, stereo.data(), n_stereo, n_pose, n_pt, edges.data(), edge_pose.data(), edge_pt.data(),
                                     lm_start.data(), lm_nmono.data(), pose_start.data());
    if (bad >= 0) {
        std::printf("bad %d\n", bad);
        return true;
    }
    ovs::index_pass2(edge_pose.data(), edge_pt.data(), ne, n_pose, n_pt, lm_start.data(), pose_start.data(), lm_cursor.data(), pose_cursor.data(),
                     lm_edges.data(), pose_edges.data(), pose_pt.data());
    std::fputs("ok", stdout);
    put(lm_start.data(), lm_start.size());
    put(lm_edges.data(), lm_edges.size());
    put(lm_nmono.data(), lm_nmono.size());
    put(pose_start.data(), pose_start.size());
    put(pose_edges.data(), pose_edges.size());
    put(pose_pt.data(), pose_pt.size());
    std::fputs(" |", stdout);
    for (const ovs::EdgeRec& e : edges) std::printf(" %d %d", e.pose, e.pt);
    std::fputs(" |", stdout);
    for (const ovs::EdgeRec& e : edges) std::printf(" %a %a %a %a", e.ox, e.oy, e.oxr, e.w);
    std::fputs("\n", stdout);
    return true;
}

int main(int argc, char** argv) {
    std::vector<long long> v;
    std::vector<int32_t> start;
    for (int i = 1; i < argc; ++i) {
        const char* row = argv[i];
        if (std::strncmp(row, "lm:", 3) == 0 && starts_of(row + 3, start)) {
            const int n_pt = (int)start.size() - 1;
            std::vector<int32_t> wg_first((size_t)n_pt + 1);
            ovs::GraphPartition part;
            ovs::partition_landmarks(start.data(), n_pt, wg_first.data(), part);
            std::printf("%d %zu", part.n_lm_wg, part.pl_bound);
            put(wg_first.data(), (size_t)part.n_lm_wg + 1);
            std::fputs("\n", stdout);
        } else if (std::strncmp(row, "chunks:", 7) == 0 && starts_of(row + 7, start)) {
            const int n_pose = (int)start.size() - 1;
            const ovs::GraphArena a = ovs::graph_arena_of(n_pose, 1, start.back(), n_pose);
            std::vector<int32_t> chunk_kf(a.max_chunks), chunk_start((size_t)n_pose + 1);   // (as long as the arena makes them)
            ovs::GraphPartition part;
            ovs::partition_chunks(start.data(), n_pose, chunk_kf.data(), chunk_start.data(), part);
            std::printf("%d %zu", part.n_chunks, a.max_chunks);
            put(chunk_start.data(), chunk_start.size());
            put(chunk_kf.data(), (size_t)part.n_chunks);
            std::fputs("\n", stdout);
        } else if (fields(row, "pairs", 1, v) && v[0] >= 0 && v[0] <= 4096) {
            const int nf = (int)v[0];
            const ovs::GraphArena a = ovs::graph_arena_of(std::max(nf, 1), 1, 0, nf);
            std::vector<int32_t> pair_ab(2 * (size_t)a.n_pairs), wg_pair(nf ? (size_t)ovs::kXcds * (size_t)a.wg_pair_cap : 0);
            ovs::GraphPartition part;
            ovs::pair_table(nf, nf ? pair_ab.data() : nullptr);   // (no free keyframe: graph_create calls neither; both must leave the pointer alone)
            ovs::pair_work_order(nf, nf ? wg_pair.data() : nullptr, part);
            std::printf("%d %d %d", a.n_pairs, a.wg_pair_cap, part.n_pair_wg);
            put(pair_ab.data(), pair_ab.size());
            put(wg_pair.data(), wg_pair.size());
            std::fputs("\n", stdout);
        } else if (std::strncmp(row, "slots:", 6) == 0) {
            std::vector<uint8_t> flags;
            bool none = false;
            if (fields(row + 6, "none", 1, v) && v[0] >= 1) {
                none = true;
                flags.resize((size_t)v[0]);
            } else {
                for (const char* c = row + 6; *c; ++c) {
                    if (*c < '0' || *c > '9') return 2;
                    flags.push_back((uint8_t)(*c - '0'));
                }
            }
            if (flags.empty()) return 2;
            std::vector<int32_t> slot(flags.size()), slot_pose(flags.size());
            const int nf = ovs::assign_slots(none ? nullptr : flags.data(), (int)flags.size(), slot.data(), slot_pose.data());
            std::printf("%d", nf);
            put(slot.data(), slot.size());
            put(slot_pose.data(), (size_t)nf);
            std::fputs("\n", stdout);
        } else if (fields(row, "graph", 4, v)) {
            const ovs::GraphArena a = ovs::graph_arena_of((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
            const size_t off[21] = {a.o_edges,       a.o_lm_start, a.o_lm_edges, a.o_lm_nmono, a.o_pose_start,  a.o_pose_edges, a.o_fixed,
                                    a.o_active,      a.o_slot_of_pose, a.o_pose_pt, a.o_pair_ab, a.o_slot_pose, a.o_wg_pair,    a.o_lm_wg_first,
                                    a.o_chunk_kf,    a.o_chunk_start,  a.o_lm_of_slot, a.o_dup,  a.o_lm_tmp,    a.o_pose_part,  a.o_ledges};
            put(off, 21, "");
            const size_t sizes[5] = {a.early_bytes, a.upload_bytes, a.o_dup_host, a.image_bytes, a.arena_bytes};
            put(sizes, 5);
            std::printf(" | %zu %d %d\n", a.max_chunks, a.n_pairs, a.wg_pair_cap);
        } else if (fields(row, "solver", 7, v)) {
            const ovs::SolverArena a = ovs::solver_arena_of((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (size_t)v[5], (size_t)v[6]);
            const size_t off[10] = {a.o_hinv, a.o_y, a.o_s, a.o_dxp, a.o_scal, a.o_fail, a.o_edge_of, a.o_pl_cnt, a.o_pl_off, a.o_pl_ent};
            put(off, 10, "");
            std::printf(" | %zu %zu %zu %d\n", a.arena_bytes, a.n_lists, a.ff_bytes, a.pl_ok ? 1 : 0);
        } else if (std::strncmp(row, "index:", 6) == 0 && index_row(row + 6)) {
        } else {
            return 2;
        }
    }
    return 0;
}
