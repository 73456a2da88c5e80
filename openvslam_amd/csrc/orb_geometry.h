// orb_geometry.h -- what the ORB extractor's host planner (orb_plan.inc) and its kernels share: the geometry records in device memory and every
// tile / LDS limit, each defined once. No HIP: a plain host compiler builds the planner from this header alone (tests/orb_plan_host.cc).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ovslam_hip.h"

namespace ovs {

constexpr int kOrbPatchRadius = 19;   // orb_extractor::orb_patch_radius_
constexpr int kFastPatchSize = 31;    // fast_patch_size_
constexpr int kCellSize = 64;         // compute_fast_keypoints cell_size
constexpr int kCellOverlap = 6;       // compute_fast_keypoints overlap
constexpr int kDetOrigin = kOrbPatchRadius + 3;   // first pixel FAST can test (cell's own 3-px dead frame)

// One bilinear tap pair of cv::resize's 11-bit fixed-point tables (computed on the host, double/float as OpenCV does).
struct ResizeTap {
    uint16_t o0, o1;   // source indices (o1 = min(o0+1, size-1))
    int16_t a0, a1;    // 11-bit coefficients
};

// Geometry of one pyramid level for the handle's current (rows, cols). Lives in device memory; kernels read it uniformly.
struct LevelGeo {
    int32_t rows, cols;
    int32_t pitch;            // bytes per row of this level's plane (levels >= 1; level 0 uses the caller's stride)
    int32_t ncx, ncy;         // valid FAST cells
    int32_t cell_base;        // prefix sum of ncx*ncy over lower levels
    int32_t max_bx, max_by;   // cols-19, rows-19
    int32_t n_keypts;         // N_level (num_keypts_per_level_)
    int32_t kp_cap;           // N_level + 3
    int32_t kp_base;          // prefix sum of kp_cap over lower levels
    int32_t cand_cap;         // capacity of this level's candidate list
    int32_t gx, gy;           // root grid of the quad-tree
    int32_t max_nodes;        // 4*N_level + 16
    float inv_ncx;            // 1 / ncx (k_fast_cells_v3: cell -> (row, column) through a float product)
    int32_t resize_hwin_ok;   // level >= 1: every tile of k_resize_linear_u8 (v4) finds its source rectangle inside the LDS tile and every
                              // column pair's four source bytes inside two aligned words (checked on the host against the tap tables)
    uint32_t ncx_magic;       // ceil(2^32 / ncx): cell / ncx == umulhi(cell, ncx_magic) for cell * ncx < 2^32 (scalar unit, no conversions)
    int64_t plane_off;        // byte offset of the plane inside one frame's pyramid block (levels >= 1)
    int64_t cand_off;         // entry offset of the candidate list inside one frame's candidate block
    int64_t node_off;         // entry offset of the node scratch inside one frame's node block
    int64_t xtab_off, ytab_off;   // ResizeTap offsets (level >= 1: taps from level-1 to level)
    double dx, dy;            // root patch size
    float scale;              // scale_factors_[level]
    float kp_size;            // (float)(unsigned)(31*scale)
};

// One FAST cell of the current geometry (k_fast_cells reads ITS cells' records with one load instead of deriving them from the level tables
// through a chain of dependent scalar loads): cell origin, clipped size, level. 8 bytes, table order = cell id.
struct CellDesc {
    uint16_t min_x, min_y;   // 19 + 64 * column / row
    uint8_t cw, ch;          // min(70, distance to the level's border): the tile is cw x ch, the testable area (cw - 6) x (ch - 6)
    uint8_t level, pad;
};
static_assert(sizeof(CellDesc) == 8, "CellDesc is read as one 64-bit word");

struct FrameGeo {
    int32_t num_levels;
    int32_t total_cells;
    int32_t total_kp_cap;
    int32_t ini_thr, min_thr;
    int32_t variant;   // ORACLE_SPEC rules 6, 7, 10 as run-time variants: bit 0 quad-tree switch factor 1 (default 3), bit 1 equal-count tie order
                       // earlier-created first (default later first), bit 2 blur taps 18,34,49,55 saturating (default 18,34,48,56), bit 3 steering by libm's cosf / sinf (default util::cos / util::sin)
    int32_t cell_base_tab[OVS_MAX_LEVELS];   // lv[l].cell_base for l < num_levels, INT32_MAX above: one scalar load finds a cell's level
    LevelGeo lv[OVS_MAX_LEVELS];
};

// k_resize_linear_u8 (v4, orb_pyramid.hip): a workgroup produces one kTileW x kTileH output tile from a source rectangle of at most kSrcWords
// 32-bit words x kSrcRows rows staged in LDS. The planner admits a level (LevelGeo::resize_hwin_ok) only if every tile's rectangle fits.
constexpr int kTileW = 128, kTileH = 32;
constexpr int kSrcWords = 48;    // 192-byte LDS pitch: source span of 128 output px is <= 128*src/dst + 2 <= 160 at scale <= 1.25, + 15
                                 // bytes so that the staged rectangle starts on a 16-byte boundary (16-byte staging loads)
constexpr int kSrcRows = 44;     // 32 output rows span <= 32 * 1.25 + 2 source rows (16-row tiles: 0.167 ms, 32: 0.142, 64: 0.165)
// k_resize_pair_u8: the lower level's staged rectangle and the middle region; its stage B runs on v4's tile (kSrcWords x kSrcRows)
constexpr int kPairSrcWords = 56;     // 224-byte pitch of the lower rectangle: 160 middle columns x 1.25 + 2 + 15 <= 217
constexpr int kPairSrcRows = 52;      // 44 middle rows x 1.2 + 2 (host-checked)
constexpr int kPairGroups = 40;       // 4-pixel groups per row of the middle region (160 columns)

// k_pyramid_chain (orb_pyramid.hip): what one tile column (or row) of the TX x TY tile grid covers of one level: the pixels it COMPUTES
// [c0, c1) and, inside them, the pixels it OWNS, i.e. stores to the level's plane, [o0, o1). Level 0: the source rectangle to stage (c0 of
// a column span is a multiple of 4), nothing owned.
struct ChainSpan {
    int16_t c0, c1, o0, o1;
};
// k_resize_pair_u8 (orb_pyramid.hip): what one tile column (or tile row) of the UPPER level's 128 x 32 tile grid needs of the two levels below it.
// Column spans: s_lo = origin of stage B's LDS tile (first tap & ~15), b0 = first middle column the tile computes (first tap & ~3), n = 4-pixel
// groups of the middle region, own = groups it stores (up to the next tile's b0; all of them for the last tile), a0 = first lower column staged
// (& ~15), an = 32-bit words per staged row. Row spans: s_lo = b0 = first middle row, n = rows of the region, own = rows stored, a0 / an = first
// lower row / rows staged.
struct PairSpan {
    int16_t s_lo, b0, n, own, a0, an, pad0, pad1;
};
static_assert(sizeof(PairSpan) == 16, "PairSpan is read as one 128-bit word");
// k_resize_pair_u8's horizontal pass for the column pair (2 j, min(2 j + 1, cols - 1)) of a level, built on the host from the level's x taps
// (orb_plan.inc build_htaps; the kernel used to derive it per thread and tile: ~25 vector instructions three times over): the two v_perm_b32
// selectors that pair (S[o0], S[o1]) out of the two aligned source words starting at word wa, and the two coefficient words (16 a0 | 16 a1 << 16).
struct HTapRec {
    uint32_t sel_a, sel_b, ca, cb;
    uint32_t wa;   // o0(2 j) >> 2, in words from the start of the source row
    uint32_t pad0, pad1, pad2;
};
static_assert(sizeof(HTapRec) == 32, "HTapRec: one 128-bit load + one word");
constexpr int kChainTileW0 = 128, kChainTileH0 = 96;   // level-0 pixels per tile of the planner's TX x TY grid
constexpr int kChainMaxW = 192;        // widest computed region of a level >= 1 (three 64-lane column chunks)
constexpr int kChainMaxW0 = 256;       // widest staged level-0 rectangle (64 words)
constexpr int kChainMaxH0 = 128;       // its height (16 waves x 8 rows)
constexpr int kChainMaxLds = 64 * 1024;
// dynamic LDS of one k_pyramid_chain workgroup (bufA, bufB multiples of 16): two buffers, the tile's spans, one 16-byte record per level, taps
inline size_t chain_lds_bytes(int bufA_bytes, int bufB_bytes, int tap_cap) {
    return (size_t)bufA_bytes + bufB_bytes + sizeof(ChainSpan) * 2 * OVS_MAX_LEVELS + (size_t)16 * OVS_MAX_LEVELS + sizeof(ResizeTap) * (size_t)tap_cap;
}

}   // namespace ovs
