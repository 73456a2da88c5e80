// fast_order.inc -- k_fast_cells' work order and a thread's pixel mask in a clipped cell, as plain constexpr functions: the kernel and
// launch_fast (orb_fast.hip) and a plain host compiler (tests/fast_order_host.cc) run the same text. No HIP, no other header of the project.
#pragma once
#include <stdint.h>

namespace ovs {

// launch-size bound of launch_fast: with per_xcd = ceil(n_cells / 8), per_xcd * batch * batch < 2^32. For the cell counts a geometry can have
// (sides <= 8191: < 2^16 cells) that alone keeps the grid, (n_cells + 7) * batch at most, inside 32 bits; the second condition says so for every
// int n_cells, so that n_groups * batch, 8 * share and the grid size below never wrap.
constexpr bool fast_launch_admitted(int n_cells, int batch) {
    return n_cells > 0 && batch > 0 && (uint64_t)(((unsigned)n_cells + 7u) / 8u) * (uint64_t)batch * (uint64_t)batch < (1ull << 32) &&
           ((uint64_t)(unsigned)n_cells + 7u) * (uint64_t)batch < (1ull << 32);
}

// Work order (group-major, XCD-aware): the (frame, group) pairs are numbered gid = frame * n_groups + group; XCD k (= blockIdx & 7) takes
// the k-th contiguous run of `share` of them. The grid is 8 * ceil(n_groups / 8) * batch >= 8 * share workgroups.
struct FastOrder {
    uint32_t n_groups;   // ceil(n_cells / cells_per_wg)
    uint32_t share;      // ceil(n_groups * batch / 8)
    uint32_t total;      // n_groups * batch
    uint32_t magic;      // floor(2^32 / n_groups), saturated for n_groups == 1
    uint32_t grid;       // workgroups to launch
};
constexpr uint32_t fast_order_magic(uint32_t d) {   // d >= 1
    const uint64_t m = (1ull << 32) / d;
    return m > 0xffffffffull ? 0xffffffffu : (uint32_t)m;
}
constexpr FastOrder fast_order(int n_cells, int cells_per_wg, int batch) {
    FastOrder o = {};
    o.n_groups = ((uint32_t)n_cells + (uint32_t)cells_per_wg - 1u) / (uint32_t)cells_per_wg;
    o.total = o.n_groups * (uint32_t)batch;
    o.share = (o.total + 7u) >> 3;
    o.magic = fast_order_magic(o.n_groups);
    o.grid = 8u * ((o.n_groups + 7u) / 8u) * (uint32_t)batch;
    return o;
}
// gid of workgroup `block`, or `total` (no work) where the block lies beyond its XCD's share or beyond the list
constexpr uint32_t fast_order_gid(uint32_t block, uint32_t share, uint32_t total) {
    const uint32_t xcd = block & 7u, idx = block >> 3;
    const uint32_t gid = xcd * share + idx;
    return (idx < share && gid < total) ? gid : total;
}
// gid / n_groups without a division (hipcc expands a run-time division through the vector unit's float reciprocal even where every operand
// is wave-uniform). With magic = floor(2^32 / d) (2^32 - 1 for d = 1) the remainder 2^32 - magic * d lies in [0, d], so
//     0 <= gid / d - gid * magic / 2^32 = gid * (2^32 - magic * d) / (d * 2^32) <= gid / 2^32 < 1        for every 32-bit gid:
// q' = mulhi(gid, magic) is floor(gid / d) or one less, and one compare of the remainder puts it right. Exact for EVERY 32-bit gid and
// d >= 1, not only below the launch bound; mulhi, multiply, subtract and select of uniform values stay on the scalar unit.
constexpr uint32_t fast_order_frame(uint32_t gid, uint32_t n_groups, uint32_t magic) {
    const uint32_t q = (uint32_t)(((uint64_t)gid * (uint64_t)magic) >> 32);
    return q + ((gid - q * n_groups >= n_groups) ? 1u : 0u);
}

// Candidate-mask layout of k_fast_cells: thread (run, rp) owns pixels c0 = 8 * run .. c0 + 7 of rows row0 = 2 * rp and row0 + 1; bit
// 8 * b + 2 * R0 + G <-> pixel c0 + 4 * G + b of row row0 + R0. This is the mask of the thread's pixels inside the iw x ih testable area
// (0x0f0f0f0f for an unclipped cell). With n = iw - c0 valid columns, columns 0 .. 3 (G = 0) fill bytes 0 .. min(n, 4) - 1 of 0x01010101 and
// columns 4 .. 7 (G = 1) the same bytes one bit up: two 64-bit shifts instead of sixteen compare / select pairs.
constexpr uint32_t fast_valid_mask(int c0, int row0, int iw, int ih) {
    const int n = iw - c0;
    const int n0 = n < 0 ? 0 : (n > 4 ? 4 : n), n1 = n < 4 ? 0 : (n > 8 ? 4 : n - 4);
    const uint32_t col = (uint32_t)((0x01010101ull << (8 * n0)) >> 32) | ((uint32_t)((0x01010101ull << (8 * n1)) >> 32) << 1);
    return (row0 < ih ? col : 0u) | (row0 + 1 < ih ? col << 2 : 0u);
}

}   // namespace ovs
