// orb_plan.inc -- the ORB extractor's geometry planner: orb_params tables (A0), level geometry, cv::resize coefficient tables, and the regions the
// three pyramid kernels (orb_pyramid.hip) may assume. Plain integer / float host code over orb_geometry.h, no HIP: orb_api.hip includes it for the
// handle, tests/orb_plan_host.cc builds it with the host compiler alone. The plan is the only thing that keeps k_resize_linear_u8, k_resize_pair_u8
// and k_pyramid_chain inside their LDS tiles: every limit it checks is the kernels' own name from orb_geometry.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "orb_geometry.h"

namespace ovs {

// A0: orb_params' per-level tables
struct OrbTables {
    std::vector<float> sf, isf, ls, ils;   // scale factor, its inverse, level sigma^2, its inverse
    std::vector<int> npl;                  // keypoints per level
};

// The tile grid and the per-level regions of k_pyramid_chain (orb_pyramid.hip) for one geometry. Both axes separately: tile t of T owns
// [t size_l / T, (t + 1) size_l / T) of level l (a partition of every level); it computes, bottom-up, R_{L-1} = owned and
// R_{l-1} = hull(owned_{l-1}, tap footprint of R_l); R_0 is the footprint alone (level 0 is only read). ok = false when a region exceeds what
// the kernel stages (unusual scale factors or level counts): the per-level launches run then.
struct ChainPlanHost {
    bool ok = false;
    int TX = 0, TY = 0, bufA = 0, bufB = 0, tap_cap = 0;
    std::vector<ChainSpan> spans;   // [level][TX x-spans, TY y-spans]
};

// Everything the host decides for one (params, variant, rows, cols): what ensure_geometry uploads and what the launch sequence reads.
struct OrbPlan {
    OrbTables tab;
    FrameGeo geo;
    std::vector<ResizeTap> taps;
    std::vector<CellDesc> cells;
    ChainPlanHost chain;                // chain.ok: k_pyramid_chain may run this geometry
    std::vector<PairSpan> pair_spans;   // k_resize_pair_u8's regions, all level pairs; pair_off[l2] = offset of the pair (l2 - 1, l2), -1 = no plan
    int pair_off[OVS_MAX_LEVELS];
    std::vector<HTapRec> htaps;         // column-pair records of the levels a pair plan reads; htab_off[l] = level l's offset, -1 = none
    int htab_off[OVS_MAX_LEVELS];
    size_t pyr_bytes = 0, cand_entries = 0, node_entries = 0;   // per frame
    OrbPlan() { drop_pairs(); }
    void drop_pairs() {   // every level runs as a single launch
        pair_spans.clear();
        htaps.clear();
        for (int l = 0; l < OVS_MAX_LEVELS; ++l) pair_off[l] = htab_off[l] = -1;
    }
};

static inline int cv_round_f(float v) { return (int)std::nearbyintf(v); }

static OrbTables calc_tables(const ovs_orb_params& p) {
    OrbTables t;
    const int L = p.num_levels;
    t.sf = t.isf = t.ls = t.ils = std::vector<float>(L, 1.0f);
    for (int l = 1; l < L; ++l) t.sf[l] = p.scale_factor * t.sf[l - 1];   // cumulative float product
    for (int l = 0; l < L; ++l) {
        t.isf[l] = 1.0f / t.sf[l];
        t.ls[l] = t.sf[l] * t.sf[l];
        t.ils[l] = 1.0f / t.ls[l];
    }
    t.npl.assign(L, 0);
    double desired = p.max_num_keypts * (1.0 - 1.0 / p.scale_factor) / (1.0 - std::pow(1.0 / p.scale_factor, (double)L));
    int total = 0;
    for (int l = 0; l < L - 1; ++l) {
        t.npl[l] = (int)std::round(desired);
        total += t.npl[l];
        desired *= 1.0 / p.scale_factor;
    }
    t.npl[L - 1] = std::max(p.max_num_keypts - total, 0);
    return t;
}

// cv::resize INTER_LINEAR tables for one axis (OpenCV resize.cpp: fx = (float)((dx+0.5)*scale - 0.5); sx = cvFloor(fx);
// fx -= sx; clamp; ialpha = saturate_cast<short>(cbuf * INTER_RESIZE_COEF_SCALE)).
static void build_taps(int ssize, int dsize, ResizeTap* out) {
    const double scale = (double)ssize / dsize;
    for (int d = 0; d < dsize; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (s < 0) { f = 0; s = 0; }
        if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        out[d].o0 = (uint16_t)s;
        out[d].o1 = (uint16_t)std::min(s + 1, ssize - 1);
        out[d].a0 = (int16_t)cv_round_f((1.f - f) * 2048.f);
        out[d].a1 = (int16_t)cv_round_f(f * 2048.f);
    }
}

// Conditions under which k_resize_linear_u8 (v4, orb_pyramid.hip) may run a level: every kTileW x kTileH output tile's source rectangle fits the
// kernel's LDS tile (kSrcWords words x kSrcRows rows, the rectangle starting on a 16-byte boundary), and the four source bytes of every column pair
// (x even, min(x + 1, dcols - 1)) lie inside the two aligned words that start at o0(x) & ~3.
static bool resize_windows_ok(const ResizeTap* xt, int dcols, const ResizeTap* yt, int drows) {
    for (int x0 = 0; x0 < dcols; x0 += kTileW) {
        const int x1 = std::min(x0 + kTileW, dcols) - 1;
        const int lo = xt[x0].o0 & ~15, hi = xt[x1].o1;
        if (hi < lo || (hi - lo) / 4 + 1 > kSrcWords) return false;
    }
    for (int y0 = 0; y0 < drows; y0 += kTileH) {
        const int y1 = std::min(y0 + kTileH, drows) - 1;
        if (yt[y1].o1 < yt[y0].o0 || yt[y1].o1 - yt[y0].o0 + 1 > kSrcRows) return false;
    }
    for (int x = 0; x < dcols; x += 2) {
        const int xb = std::min(x + 1, dcols - 1);
        const int base = xt[x].o0 & ~3;
        const int o[4] = {xt[x].o0, xt[x].o1, xt[xb].o0, xt[xb].o1};
        for (int k = 0; k < 4; ++k)
            if (o[k] < base || o[k] > base + 7) return false;
        if (xt[x].a0 < 0 || xt[x].a1 < 0 || xt[xb].a0 < 0 || xt[xb].a1 < 0 || xt[x].a0 > 2048 || xt[x].a1 > 2048 || xt[xb].a0 > 2048 || xt[xb].a1 > 2048)
            return false;
    }
    for (int y = 0; y < drows; ++y)
        if (yt[y].a0 < 0 || yt[y].a1 < 0 || yt[y].a0 > 2048 || yt[y].a1 > 2048) return false;
    return true;
}

static void build_chain_plan(const FrameGeo& geo, const std::vector<ResizeTap>& taps, ChainPlanHost& out) {
    out = ChainPlanHost();
    const int L = geo.num_levels;
    if (L < 2) return;
    const int TX = std::max(1, (geo.lv[0].cols + kChainTileW0 - 1) / kChainTileW0), TY = std::max(1, (geo.lv[0].rows + kChainTileH0 - 1) / kChainTileH0);
    out.TX = TX;
    out.TY = TY;
    out.spans.assign((size_t)L * (TX + TY), ChainSpan{0, 0, 0, 0});
    bool ok = true;
    for (int axis = 0; axis < 2; ++axis) {
        const int T = axis ? TY : TX;
        for (int t = 0; t < T; ++t) {
            int c0[OVS_MAX_LEVELS], c1[OVS_MAX_LEVELS], o0[OVS_MAX_LEVELS], o1[OVS_MAX_LEVELS];
            for (int l = 0; l < L; ++l) {
                const int64_t size = axis ? geo.lv[l].rows : geo.lv[l].cols;
                o0[l] = (int)(t * size / T);
                o1[l] = (int)((t + 1) * size / T);
            }
            c0[L - 1] = o0[L - 1];
            c1[L - 1] = o1[L - 1];
            for (int l = L - 1; l >= 1; --l) {
                const ResizeTap* tab = taps.data() + (axis ? geo.lv[l].ytab_off : geo.lv[l].xtab_off);
                int f0 = 0, f1 = 0;
                if (c1[l] > c0[l]) {
                    f0 = tab[c0[l]].o0;
                    f1 = tab[c1[l] - 1].o1 + 1;
                    for (int i = c0[l]; i < c1[l]; ++i) {   // (the tables are monotone; this does not rely on it)
                        f0 = std::min(f0, (int)tab[i].o0);
                        f1 = std::max(f1, (int)tab[i].o1 + 1);
                    }
                }
                if (l - 1 == 0) {
                    o0[0] = o1[0] = 0;
                    c0[0] = axis ? f0 : (f0 & ~3);
                    c1[0] = f1;
                } else if (o1[l - 1] > o0[l - 1] && f1 > f0) {
                    c0[l - 1] = std::min(o0[l - 1], f0);
                    c1[l - 1] = std::max(o1[l - 1], f1);
                } else if (f1 > f0) {
                    c0[l - 1] = f0;
                    c1[l - 1] = f1;
                } else {
                    c0[l - 1] = o0[l - 1];
                    c1[l - 1] = o1[l - 1];
                }
            }
            for (int l = 0; l < L; ++l) {
                if (c1[l] > 32767) ok = false;
                out.spans[(size_t)l * (TX + TY) + (axis ? TX + t : t)] = ChainSpan{(int16_t)c0[l], (int16_t)c1[l], (int16_t)o0[l], (int16_t)o1[l]};
                const int ext = c1[l] - c0[l];
                if (l == 0 ? (axis ? ext > kChainMaxH0 : ext > kChainMaxW0) : (!axis && ext > kChainMaxW)) ok = false;
            }
        }
    }
    // LDS: level 0, 2, 4, .. regions in buffer A, the odd levels in buffer B; the taps of the tile with the most of them
    int bufA = 16, bufB = 16, tap_cap = 0;
    for (int tj = 0; tj < TY; ++tj)
        for (int ti = 0; ti < TX; ++ti) {
            int ntap = 0;
            for (int l = 0; l < L; ++l) {
                const ChainSpan X = out.spans[(size_t)l * (TX + TY) + ti], Y = out.spans[(size_t)l * (TX + TY) + TX + tj];
                const int W = X.c1 - X.c0, H = Y.c1 - Y.c0, bytes = (((W + 3) & ~3) * H + 15) & ~15;
                (l & 1 ? bufB : bufA) = std::max(l & 1 ? bufB : bufA, bytes);
                if (l >= 1) ntap += W + H;
            }
            tap_cap = std::max(tap_cap, ntap);
        }
    out.bufA = bufA;
    out.bufB = bufB;
    out.tap_cap = tap_cap;
    if (chain_lds_bytes(bufA, bufB, tap_cap) > (size_t)kChainMaxLds) ok = false;
    out.ok = ok;
}

// HTapRec of every column pair of a level (orb_geometry.h): make_htaps of orb_pyramid.hip with absolute offsets -- the selectors do not depend on the
// tile origin (a multiple of 4), the first source word becomes relative by one subtraction in the kernel.
static void build_htaps(const ResizeTap* xt, int cols, std::vector<HTapRec>& out) {
    for (int x = 0; x < cols; x += 2) {
        const ResizeTap ta = xt[x], tb = xt[std::min(x + 1, cols - 1)];
        HTapRec r = {};
        r.wa = (uint32_t)(ta.o0 >> 2);
        const int base = 4 * (int)r.wa;
        const uint32_t sa0 = (uint32_t)(ta.o0 - base) & 7u, sa1 = (uint32_t)(ta.o1 - base) & 7u;
        const uint32_t sb0 = (uint32_t)(tb.o0 - base) & 7u, sb1 = (uint32_t)(tb.o1 - base) & 7u;
        r.sel_a = sa0 | 0x0c00u | (sa1 << 16) | 0x0c000000u;
        r.sel_b = sb0 | 0x0c00u | (sb1 << 16) | 0x0c000000u;
        r.ca = ((uint32_t)(uint16_t)ta.a0 << 4) | ((uint32_t)(uint16_t)ta.a1 << 20);
        r.cb = ((uint32_t)(uint16_t)tb.a0 << 4) | ((uint32_t)(uint16_t)tb.a1 << 20);
        out.push_back(r);
    }
}

// The regions of k_resize_pair_u8 (orb_pyramid.hip) for the level pair (l2 - 1, l2) computed from level l2 - 2: one PairSpan per tile column and
// per tile row of level l2's kTileW x kTileH grid, x spans first. Returns false -- the pair then runs as two per-level launches -- unless both levels
// pass v4's window checks, every region fits the kernel's LDS buffers (the middle region in v4's tile, at most kPairGroups groups wide; the lower
// rectangle in kPairSrcWords x kPairSrcRows), and the owned ranges partition the middle level.
static bool build_pair_plan(const FrameGeo& geo, const std::vector<ResizeTap>& taps, int l2, std::vector<PairSpan>& out) {
    out.clear();
    if (l2 < 2 || l2 >= geo.num_levels) return false;
    const LevelGeo &g1 = geo.lv[l2 - 1], &g2 = geo.lv[l2];
    if (!g1.resize_hwin_ok || !g2.resize_hwin_ok) return false;
    for (int axis = 0; axis < 2; ++axis) {
        const ResizeTap* t1 = taps.data() + (axis ? g1.ytab_off : g1.xtab_off);
        const ResizeTap* t2 = taps.data() + (axis ? g2.ytab_off : g2.xtab_off);
        const int size1 = axis ? g1.rows : g1.cols, size2 = axis ? g2.rows : g2.cols, step = axis ? kTileH : kTileW;
        int expect_b0 = 0;   // the owned ranges must follow each other from 0
        for (int p0 = 0; p0 < size2; p0 += step) {
            const int p1 = std::min(p0 + step, size2) - 1;
            const bool last = p0 + step >= size2;
            PairSpan sp = {};
            const int first = t2[p0].o0;
            const int b0 = axis ? first : (first & ~3), b1 = last ? size1 - 1 : t2[p1].o1;
            if (b1 < t2[p1].o1 || b0 != expect_b0) return false;
            sp.s_lo = (int16_t)(axis ? first : (first & ~15));
            sp.b0 = (int16_t)b0;
            int n, own, hi;   // computed extent (groups / rows), owned extent, last middle index that exists
            if (!axis) {
                n = (b1 - b0) / 4 + 1;
                hi = std::min(b0 + 4 * n - 1, size1 - 1);
                const int next_b0 = last ? b0 + 4 * n : (t2[p0 + step].o0 & ~3);
                own = (next_b0 - b0) / 4;
                if (n > kPairGroups || (b0 - sp.s_lo) / 4 + n > kSrcWords) return false;
                expect_b0 = next_b0;
            } else {
                n = b1 - b0 + 1;
                hi = b1;
                const int next_b0 = last ? b0 + n : t2[p0 + step].o0;
                own = next_b0 - b0;
                if (n > kSrcRows) return false;
                expect_b0 = next_b0;
            }
            if (own < 1 || own > n) return false;
            int a_lo = t1[b0].o0, a_hi = t1[hi].o1;
            for (int i = b0; i <= hi; ++i) {   // (the tables are monotone; this does not rely on it)
                a_lo = std::min(a_lo, (int)t1[i].o0);
                a_hi = std::max(a_hi, (int)t1[i].o1);
            }
            if (!axis) a_lo &= ~15;
            const int an = axis ? a_hi - a_lo + 1 : (a_hi - a_lo) / 4 + 1;
            if (an > (axis ? kPairSrcRows : kPairSrcWords)) return false;
            sp.n = (int16_t)n;
            sp.own = (int16_t)own;
            sp.a0 = (int16_t)a_lo;
            sp.an = (int16_t)an;
            out.push_back(sp);
        }
        if (expect_b0 < size1) return false;   // the last tile's region ends where the middle level ends
    }
    return true;
}

// Level sizes, cell grids, root grids, capacities and offsets for an image of rows x cols: plan.geo, taps, cells and the three totals. Returns
// false if the geometry cannot be processed (level too small for the packed formats, too many root patches).
static bool build_geometry(const ovs_orb_params& p, const OrbTables& tab, int32_t variant, int rows, int cols, OrbPlan& plan) {
    FrameGeo& geo = plan.geo;
    std::vector<ResizeTap>& taps = plan.taps;
    const int L = p.num_levels;
    std::memset(&geo, 0, sizeof(geo));
    geo.num_levels = L;
    geo.variant = variant;
    geo.ini_thr = std::min(std::max(p.ini_fast_thr, 0), 255);
    geo.min_thr = std::min(std::max(p.min_fast_thr, 0), 255);
    taps.clear();
    plan.cells.clear();
    size_t &pyr_bytes = plan.pyr_bytes, &cand_entries = plan.cand_entries, &node_entries = plan.node_entries;
    pyr_bytes = cand_entries = node_entries = 0;
    int cell_base = 0, kp_base = 0;
    int prev_rows = rows, prev_cols = cols;
    if (rows > 8191 || cols > 8191) return false;
    for (int l = 0; l < L; ++l) {
        LevelGeo& g = geo.lv[l];
        if (l == 0) {
            g.rows = rows;
            g.cols = cols;
        } else {
            const double scale = tab.sf[l];   // compute_image_pyramid: size from the ORIGINAL image
            g.cols = (int)std::round(cols * 1.0 / scale);
            g.rows = (int)std::round(rows * 1.0 / scale);
            if (g.rows < 1 || g.cols < 1) return false;
            g.pitch = (g.cols + 255) & ~255;
            g.plane_off = (int64_t)pyr_bytes;
            pyr_bytes += (size_t)g.pitch * g.rows;
            g.xtab_off = (int64_t)taps.size();
            taps.resize(taps.size() + g.cols);
            build_taps(prev_cols, g.cols, &taps[g.xtab_off]);
            g.ytab_off = (int64_t)taps.size();
            taps.resize(taps.size() + g.rows);
            build_taps(prev_rows, g.rows, &taps[g.ytab_off]);
            g.resize_hwin_ok = resize_windows_ok(&taps[g.xtab_off], g.cols, &taps[g.ytab_off], g.rows) ? 1 : 0;
        }
        prev_rows = g.rows;
        prev_cols = g.cols;
        g.scale = tab.sf[l];
        g.kp_size = (float)(unsigned)(kFastPatchSize * tab.sf[l]);
        g.max_bx = g.cols - kOrbPatchRadius;
        g.max_by = g.rows - kOrbPatchRadius;
        const int W = g.max_bx - kOrbPatchRadius, H = g.max_by - kOrbPatchRadius;
        // valid cells: 19 + 64*i < max_border - overlap
        g.ncx = W > kCellOverlap ? (W - kCellOverlap + kCellSize - 1) / kCellSize : 0;
        g.ncy = H > kCellOverlap ? (H - kCellOverlap + kCellSize - 1) / kCellSize : 0;
        if (g.ncx == 0 || g.ncy == 0) g.ncx = g.ncy = 0;
        g.inv_ncx = g.ncx ? 1.0f / (float)g.ncx : 0.0f;
        g.ncx_magic = g.ncx > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)g.ncx - 1) / (uint64_t)g.ncx) : 0u;   // ncx == 1: see k_fast_cells
        g.cell_base = cell_base;
        cell_base += g.ncx * g.ncy;
        g.n_keypts = tab.npl[l];
        g.gx = g.gy = 1;
        g.dx = g.dy = 1.0;
        if (g.ncx) {
            // initialize_nodes: a row (landscape) or column (portrait) of near-square root patches
            const double ratio = (double)W / H;
            if (ratio > 1) {
                g.gx = (int)std::round(ratio);
                g.gy = 1;
                g.dx = (double)W / g.gx;
                g.dy = H;
            } else {
                g.gx = 1;
                g.gy = (int)std::round(1 / ratio);
                g.dx = W;
                g.dy = (double)H / g.gy;
            }
            if (g.gx * g.gy > 4096) return false;   // (16-bit node ids: max_nodes below is the binding limit)
        }
        const int nc = std::max(g.n_keypts, g.gx * g.gy) + 16;
        g.max_nodes = 4 * nc;
        if (g.max_nodes > 65535) return false;
        // the tree ends with fewer than N + 3 nodes when the pool is split one at a time from N < size + 3 * pool on (rule 6 as fixed);
        // with the factor-1 variant the last all-at-once pass starts from size + pool <= N and may end with up to size + 3 * pool <= 2 N
        g.kp_cap = std::max(((geo.variant & 1) ? 2 * g.n_keypts : g.n_keypts) + 3, 4 * g.gx * g.gy);
        g.kp_base = kp_base;
        kp_base += g.kp_cap;
        g.cand_cap = g.ncx * g.ncy * 1024;   // NMS leaves at most one survivor per 2x2 block of a 64x64 cell
        g.cand_off = (int64_t)cand_entries;
        cand_entries += (size_t)g.cand_cap;
        g.node_off = (int64_t)node_entries;
        node_entries += (size_t)2 * g.max_nodes;
    }
    geo.total_cells = cell_base;
    plan.cells.reserve((size_t)cell_base);
    for (int l = 0; l < L; ++l) {
        const LevelGeo& g = geo.lv[l];
        for (int ci = 0; ci < g.ncy; ++ci)
            for (int cj = 0; cj < g.ncx; ++cj) {
                CellDesc c{};
                const int min_x = kOrbPatchRadius + cj * kCellSize, min_y = kOrbPatchRadius + ci * kCellSize;
                c.min_x = (uint16_t)min_x;
                c.min_y = (uint16_t)min_y;
                c.cw = (uint8_t)(std::min(min_x + kCellSize + kCellOverlap, (int)g.max_bx) - min_x);
                c.ch = (uint8_t)(std::min(min_y + kCellSize + kCellOverlap, (int)g.max_by) - min_y);
                c.level = (uint8_t)l;
                plan.cells.push_back(c);
            }
    }
    geo.total_kp_cap = kp_base;
    for (int l = 0; l < OVS_MAX_LEVELS; ++l) geo.cell_base_tab[l] = l < L ? geo.lv[l].cell_base : INT32_MAX;
    return true;
}

// The planner's entry point: the whole plan of one geometry. Returns false if the geometry cannot be processed; the plan is then unspecified.
// A level pair gets spans where build_pair_plan admits it, and a level gets HTapRec records where a pair plan reads them.
static bool build_orb_plan(const ovs_orb_params& p, const OrbTables& tab, int32_t variant, int rows, int cols, OrbPlan& plan) {
    plan.tab = tab;
    plan.chain = ChainPlanHost();
    plan.drop_pairs();
    if (!build_geometry(p, tab, variant, rows, cols, plan)) return false;
    const FrameGeo& geo = plan.geo;
    build_chain_plan(geo, plan.taps, plan.chain);
    std::vector<PairSpan> one;
    for (int l2 = 2; l2 < geo.num_levels; ++l2)
        if (build_pair_plan(geo, plan.taps, l2, one)) {
            plan.pair_off[l2] = (int)plan.pair_spans.size();
            plan.pair_spans.insert(plan.pair_spans.end(), one.begin(), one.end());
        }
    for (int l = 1; l < geo.num_levels; ++l)
        if ((l + 1 < geo.num_levels && plan.pair_off[l + 1] >= 0) || plan.pair_off[l] >= 0) {
            plan.htab_off[l] = (int)plan.htaps.size();
            build_htaps(plan.taps.data() + geo.lv[l].xtab_off, geo.lv[l].cols, plan.htaps);
        }
    return true;
}

}   // namespace ovs
