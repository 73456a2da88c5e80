// The image front end's host side (openvslam_amd/csrc/image_prep_plan.inc: rules I3 to I5, the argument checks, the launch geometry) run by a plain
// host compiler, with rules I1, I2, I6 and I7 as a sequential loop over the pixels written here: tests/test_imgprep_ref.py builds this with
// g++ -ffp-contract=off and compares the fixed map and the prepared images with the Python reference (tests/imgprep_ref.py). The loop is also
// the "same algebra as a host loop on one core" the device call's timings are set against.
// usage: imgprep_host case.bin out.bin            per side: the fixed map (if the case rectifies), then the prepared image. Exit status 3 and the word
//                                                  "refused" for a rig the ABI answers with OVS_ERR_INVALID
//        imgprep_host case.bin --time N           N passes of the loop over the case's images (the map is built once, outside): median and minimum
//                                                  of a pass in milliseconds
//        imgprep_host --status rows cols src_stride channels color_order rectify sides max_rows max_cols map_rows map_cols map_sides
//                                                  the ovs_status run_status gives these arguments
//        imgprep_host --launch rows cols sides    the launch geometry: gx gy gz bx by
//
// case.bin (little endian): i32 rows, cols, channels, color_order, rectify, sides; f64 rect_fx_fy_cx_cy[4]; per side i32 model, n_dist, f64 K[9], D[8],
// R[9]; per side u8 image[rows][cols][channels].
// out.bin: per side [i16 ixy[rows][cols][2], u8 fxy[rows][cols][2] if rectify], u8 gray[rows][cols].
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "image_prep_plan.inc"

namespace {

struct Case {
    int32_t rows, cols, channels, color_order, rectify, sides;
    double P[4];
    ovs_rectify_side side[2];
    std::vector<uint8_t> img[2];
};

bool read_case(const char* path, Case& c) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    bool ok = std::fread(&c.rows, 4, 6, f) == 6 && std::fread(c.P, 8, 4, f) == 4 && c.rows >= 0 && c.cols >= 0 && c.rows <= imgprep::kMaxDim &&
              c.cols <= imgprep::kMaxDim && c.sides >= 1 && c.sides <= 2 && (c.channels == 1 || c.channels == 3 || c.channels == 4);
    for (int s = 0; ok && s < c.sides; ++s)
        ok = std::fread(&c.side[s].model, 4, 1, f) == 1 && std::fread(&c.side[s].n_dist, 4, 1, f) == 1 && std::fread(c.side[s].K, 8, 9, f) == 9 &&
             std::fread(c.side[s].D, 8, 8, f) == 8 && std::fread(c.side[s].R, 8, 9, f) == 9;
    for (int s = 0; ok && s < c.sides; ++s) {
        c.img[s].resize((size_t)c.rows * c.cols * c.channels);
        ok = c.img[s].empty() || std::fread(c.img[s].data(), 1, c.img[s].size(), f) == c.img[s].size();
    }
    std::fclose(f);
    return ok;
}

// rule I6: channel ch of the source pixel (x, y), 0 outside
inline int32_t tap(const Case& c, const uint8_t* src, int x, int y, int ch) {
    if (x < 0 || y < 0 || x >= c.cols || y >= c.rows) return 0;
    return src[((size_t)y * c.cols + x) * c.channels + ch];
}

// rules I1, I2, I6, I7 for one image, pixel after pixel
void prepare(const Case& c, const uint8_t* src, const imgprep::FixedMap* map, const int32_t w[3], uint8_t* out) {
    const int nc = c.channels == 1 ? 1 : 3;
    for (int v = 0; v < c.rows; ++v)
        for (int u = 0; u < c.cols; ++u) {
            int32_t o[3] = {0, 0, 0};
            if (map) {
                const uint32_t e = map->ixy[(size_t)v * map->pitch + u];
                const uint16_t f = map->fxy[(size_t)v * map->pitch + u];
                const int ix = (int16_t)(e & 0xffffu), iy = (int16_t)(e >> 16), fx = f & 0xff, fy = f >> 8;
                for (int ch = 0; ch < nc; ++ch)
                    o[ch] = imgprep::blend(tap(c, src, ix, iy, ch), tap(c, src, ix + 1, iy, ch), tap(c, src, ix, iy + 1, ch), tap(c, src, ix + 1, iy + 1, ch), fx, fy);
            } else {
                for (int ch = 0; ch < nc; ++ch) o[ch] = tap(c, src, u, v, ch);
            }
            out[(size_t)v * c.cols + u] = (uint8_t)(nc == 1 ? o[0] : imgprep::gray_of(w, o[0], o[1], o[2]));
        }
}

}   // namespace

#ifndef IMGPREP_HOST_NO_MAIN   // (openvslam_amd/cpp/test_imgprep_shim.cc includes this file for the loop above)
int main(int argc, char** argv) {
    if (argc == 14 && !std::strcmp(argv[1], "--status")) {
        long a[12];
        for (int i = 0; i < 12; ++i) a[i] = std::atol(argv[2 + i]);
        std::printf("%d\n", (int)imgprep::run_status((int)a[0], (int)a[1], (size_t)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9],
                                                     (int)a[10], (int)a[11]));
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "--launch")) {
        const imgprep::Launch g = imgprep::launch_for(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
        std::printf("%u %u %u %u %u\n", g.gx, g.gy, g.gz, g.bx, g.by);
        return 0;
    }
    if (argc < 3) {
        std::fprintf(stderr, "usage: imgprep_host case.bin out.bin | case.bin --time N | --status ... | --launch rows cols sides\n");
        return 2;
    }
    Case c;
    if (!read_case(argv[1], c)) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int32_t w[3];
    if (!imgprep::gray_weights(c.channels, c.color_order, w)) {
        std::printf("refused\n");
        return 3;
    }
    imgprep::FixedMap map[2];
    for (int s = 0; c.rectify && s < c.sides; ++s)
        if (!imgprep::build_fixed_map(&c.side[s], c.P, c.rows, c.cols, map[s])) {
            std::printf("refused\n");
            return 3;
        }
    std::vector<uint8_t> out[2];
    for (int s = 0; s < c.sides; ++s) out[s].resize((size_t)c.rows * c.cols);
    if (argc == 4 && !std::strcmp(argv[2], "--time")) {
        const int n = std::max(1, std::atoi(argv[3]));
        std::vector<double> ms;
        for (int i = 0; i < n; ++i) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int s = 0; s < c.sides; ++s) prepare(c, c.img[s].data(), c.rectify ? &map[s] : nullptr, w, out[s].data());
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("median_ms %.4f min_ms %.4f checksum %u\n", ms[ms.size() / 2], ms[0], out[0].empty() ? 0u : (unsigned)out[0][out[0].size() / 2]);
        return 0;
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    for (int s = 0; s < c.sides; ++s) {
        prepare(c, c.img[s].data(), c.rectify ? &map[s] : nullptr, w, out[s].data());
        if (c.rectify)
            for (int pass = 0; pass < 2; ++pass)
                for (int v = 0; v < c.rows; ++v)
                    for (int u = 0; u < c.cols; ++u) {
                        const uint32_t e = map[s].ixy[(size_t)v * map[s].pitch + u];
                        const uint16_t fr = map[s].fxy[(size_t)v * map[s].pitch + u];
                        if (pass == 0) std::fwrite(&e, 4, 1, f);
                        else std::fwrite(&fr, 2, 1, f);
                    }
        std::fwrite(out[s].data(), 1, out[s].size(), f);
    }
    std::fclose(f);
    return 0;
}
#endif
