// k_fast_cells' work order and clipped-cell pixel mask (openvslam_amd/csrc/fast_order.inc) as a stand-alone host program: no device, no library,
// the plain host compiler. The kernel and launch_fast compile the same functions; tests/test_orb_plan_fast_order.py drives this program.
//   fast_order_host order n_cells cells_per_wg batch
//       walks every workgroup of the launch and every gid: prints "admitted n_groups share total grid covered bad_frame bad_group bad_gid"
//       covered   = gids below `total` reached by exactly one workgroup
//       bad_frame = gids whose magic quotient differs from gid / n_groups;  bad_group likewise for the remainder
//       bad_gid   = workgroups whose gid differs from the plain form (xcd * share + idx; beyond the share or the list: none)
//   fast_order_host mask
//       every (c0, row0, iw, ih) of a 64 x 64 cell against the mask's definition: prints "checked bad"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fast_order.inc"

static uint32_t mask_by_definition(int c0, int row0, int iw, int ih) {
    uint32_t valid = 0;
    for (int b = 0; b < 4; ++b)
        for (int G = 0; G < 2; ++G) {
            const uint32_t colok = (c0 + 4 * G + b < iw) ? 1u : 0u;
            valid |= ((row0 < ih ? colok : 0u) << (8 * b + G)) | ((row0 + 1 < ih ? colok : 0u) << (8 * b + 2 + G));
        }
    return valid;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "mask")) {
        unsigned long long checked = 0, bad = 0;
        for (int run = 0; run < 8; ++run)
            for (int rp = 0; rp < 32; ++rp)
                for (int iw = -2; iw <= 70; ++iw)
                    for (int ih = -2; ih <= 70; ++ih) {
                        ++checked;
                        bad += ovs::fast_valid_mask(8 * run, 2 * rp, iw, ih) != mask_by_definition(8 * run, 2 * rp, iw, ih);
                    }
        std::printf("%llu %llu\n", checked, bad);
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "magic")) {   // divisors argv[2..]: the quotient at the edges of every 32-bit range, beyond any launch
        unsigned long long checked = 0, bad = 0;
        for (int a = 2; a < argc; ++a) {
            const uint64_t d = std::strtoull(argv[a], nullptr, 10);
            if (d < 1 || d > 0xffffffffull) return 2;
            const uint32_t magic = ovs::fast_order_magic((uint32_t)d);
            auto check = [&](uint64_t gid) {
                if (gid > 0xffffffffull) return;
                ++checked;
                bad += ovs::fast_order_frame((uint32_t)gid, (uint32_t)d, magic) != (uint32_t)(gid / d);
            };
            const uint64_t nq = 0xffffffffull / d + 1, step = nq / 200000 + 1;   // multiples of d, about 200 000 of them, and both neighbours
            for (uint64_t k = 0; k < nq; k += step)
                for (int e = -1; e <= 1; ++e) check(k * d + (uint64_t)(int64_t)e);
            for (uint64_t g = 0; g < 100000; ++g) {   // both ends of the range
                check(g);
                check(0xffffffffull - g);
            }
        }
        std::printf("%llu %llu\n", checked, bad);
        return 0;
    }
    if (argc != 5 || std::strcmp(argv[1], "order")) return 2;
    const long long n_cells = std::atoll(argv[2]), cpw = std::atoll(argv[3]), batch = std::atoll(argv[4]);
    if (n_cells < 1 || n_cells > INT32_MAX || cpw < 1 || cpw > INT32_MAX || batch < 1 || batch > INT32_MAX) return 2;
    if (!ovs::fast_launch_admitted((int)n_cells, (int)batch)) {
        std::printf("0\n");
        return 0;
    }
    const ovs::FastOrder o = ovs::fast_order((int)n_cells, (int)cpw, (int)batch);
    unsigned long long covered = 0, bad_frame = 0, bad_group = 0, bad_gid = 0;
    std::vector<uint8_t> seen(o.total, 0);
    for (uint64_t block = 0; block < o.grid; ++block) {
        const uint32_t gid = ovs::fast_order_gid((uint32_t)block, o.share, o.total);
        // the plain form, in 64 bits
        const uint64_t xcd = block & 7, idx = block >> 3, plain = xcd * o.share + idx;
        const bool works = idx < o.share && plain < o.total;
        bad_gid += works ? (gid != plain) : (gid < o.total);
        if (gid >= o.total) continue;
        const uint32_t frame = ovs::fast_order_frame(gid, o.n_groups, o.magic);
        bad_frame += frame != gid / o.n_groups;
        bad_group += gid - frame * o.n_groups != gid % o.n_groups;
        if (seen[gid] < 2) ++seen[gid];
    }
    for (uint8_t s : seen) covered += s == 1;
    std::printf("1 %u %u %u %u %llu %llu %llu %llu\n", o.n_groups, o.share, o.total, o.grid, covered, bad_frame, bad_group, bad_gid);
    return 0;
}
