// The ORB extractor's geometry planner (openvslam_amd/csrc/orb_plan.inc) as a stand-alone host program: no device, no library, the plain host
// compiler. usage: orb_plan_host OUT rows cols levels scale nfeat [variant]   (FAST thresholds 20 / 7, as orb_params' defaults)
// OUT receives the plan as sections [name: 8 bytes, zero padded | payload bytes: u64 | payload], read by tests/test_orb_plan.py:
//   result  i32 ok: the planner's verdict; nothing but `limits` follows when it is 0
//   limits  i32[]: the kernel limits of orb_geometry.h and the record sizes, in the order of kLimits below
//   geo     FrameGeo, exactly the bytes ensure_geometry uploads        taps   ResizeTap[]        cells  CellDesc[]
//   chain   i32 ok, TX, TY, bufA, bufB, tap_cap, LDS bytes, span count, then ChainSpan[]
//   pairs   i32 pair_off[OVS_MAX_LEVELS], then PairSpan[]               htaps  i32 htab_off[OVS_MAX_LEVELS], then HTapRec[]
//   totals  u64 pyr_bytes, cand_entries, node_entries                   tables i32 L, f32 sf[L], isf[L], ls[L], ils[L], i32 npl[L]
#include <cstdio>
#include <cstdlib>
#include <string>

#include "orb_geometry.h"
// the limits as the header alone defines them, taken before the planner is seen
constexpr int kLimits[] = {ovs::kTileW,        ovs::kTileH,        ovs::kSrcWords,  ovs::kSrcRows,    ovs::kPairSrcWords, ovs::kPairSrcRows,
                           ovs::kPairGroups,   ovs::kChainTileW0,  ovs::kChainTileH0, ovs::kChainMaxW, ovs::kChainMaxW0,  ovs::kChainMaxH0,
                           ovs::kChainMaxLds,  (int)sizeof(ovs::FrameGeo), (int)sizeof(ovs::LevelGeo), OVS_MAX_LEVELS};
#include "orb_plan.inc"
namespace ovs {   // what the planner's namespace sees under these names is what the header defined: the planner has no definition of its own
static_assert(kTileW == kLimits[0] && kTileH == kLimits[1] && kSrcWords == kLimits[2] && kSrcRows == kLimits[3] && kPairSrcWords == kLimits[4] &&
                  kPairSrcRows == kLimits[5] && kPairGroups == kLimits[6] && kChainTileW0 == kLimits[7] && kChainTileH0 == kLimits[8] &&
                  kChainMaxW == kLimits[9] && kChainMaxW0 == kLimits[10] && kChainMaxH0 == kLimits[11] && kChainMaxLds == kLimits[12],
              "the planner sees the limits of orb_geometry.h");
}   // namespace ovs

static void section(std::string& out, const char* name, const std::string& payload) {
    char tag[8] = {};
    std::snprintf(tag, sizeof(tag), "%s", name);
    const uint64_t n = payload.size();
    out.append(tag, 8).append(reinterpret_cast<const char*>(&n), 8).append(payload);
}
template <class T>
static void put(std::string& s, const T* v, size_t n) {
    if (n) s.append(reinterpret_cast<const char*>(v), n * sizeof(T));
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    ovs_orb_params p = {};
    p.num_levels = std::atoi(argv[4]);
    p.scale_factor = (float)std::atof(argv[5]);
    p.max_num_keypts = std::atoi(argv[6]);
    p.ini_fast_thr = 20;
    p.min_fast_thr = 7;
    const int32_t variant = argc > 7 ? std::atoi(argv[7]) : 0;
    if (rows < 1 || cols < 1 || p.num_levels < 1 || p.num_levels > OVS_MAX_LEVELS || !(p.scale_factor > 1.0f) || p.max_num_keypts < 1) return 2;   // ovs_orb_create's refusals

    const ovs::OrbTables tab = ovs::calc_tables(p);
    ovs::OrbPlan plan;
    const int32_t ok = ovs::build_orb_plan(p, tab, variant, rows, cols, plan) ? 1 : 0;
    std::string out, s;
    put(s, &ok, 1);
    section(out, "result", s);
    s.clear();
    put(s, kLimits, sizeof(kLimits) / sizeof(kLimits[0]));
    section(out, "limits", s);
    if (ok) {
        s.clear();
        put(s, &plan.geo, 1);
        section(out, "geo", s);
        s.clear();
        put(s, plan.taps.data(), plan.taps.size());
        section(out, "taps", s);
        s.clear();
        put(s, plan.cells.data(), plan.cells.size());
        section(out, "cells", s);
        const ovs::ChainPlanHost& c = plan.chain;
        const int32_t head[8] = {c.ok ? 1 : 0, c.TX, c.TY, c.bufA, c.bufB, c.tap_cap, (int32_t)ovs::chain_lds_bytes(c.bufA, c.bufB, c.tap_cap), (int32_t)c.spans.size()};
        s.clear();
        put(s, head, 8);
        put(s, c.spans.data(), c.spans.size());
        section(out, "chain", s);
        s.clear();
        put(s, plan.pair_off, OVS_MAX_LEVELS);
        put(s, plan.pair_spans.data(), plan.pair_spans.size());
        section(out, "pairs", s);
        s.clear();
        put(s, plan.htab_off, OVS_MAX_LEVELS);
        put(s, plan.htaps.data(), plan.htaps.size());
        section(out, "htaps", s);
        const uint64_t totals[3] = {plan.pyr_bytes, plan.cand_entries, plan.node_entries};
        s.clear();
        put(s, totals, 3);
        section(out, "totals", s);
        const int32_t L = p.num_levels;
        s.clear();
        put(s, &L, 1);
        put(s, plan.tab.sf.data(), L);
        put(s, plan.tab.isf.data(), L);
        put(s, plan.tab.ls.data(), L);
        put(s, plan.tab.ils.data(), L);
        put(s, plan.tab.npl.data(), L);
        section(out, "tables", s);
    }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    const bool written = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && written) ? 0 : 3;
}
