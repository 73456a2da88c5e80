// util::stereo_rectifier, util::convert_to_grayscale and feature::orb_extractor::extract_pair_prepared through the class layer, on a case file of
// tests/imgprep_host.cc (a rig and a raw pair): tests/test_imgprep_shim.py compares what this writes with arrays the reference computed.
// usage: test_imgprep_shim case.bin out.bin      out.bin: the rectified pair (rows x cols x channels each), the gray images of the RAW pair (rows x cols
//                                                each), the prepared pair of the fused call (rows x cols each), i32 n_left, n_right. The program itself holds
//                                                the fused call's keypoints and descriptors to rectify + convert_to_grayscale + extract per side, and
//                                                checks the degraded result under injected device failures and the correct result of the call after
//        test_imgprep_shim case.bin --degraded   with no device (or with failures injected into every call where there is one): every class returns its
//                                                empty result and throws nothing
//        test_imgprep_shim case.bin --time N     N repetitions of extract_pair_prepared against the host loop of imgprep_host.cc on one core followed by
//                                                ovs_orb_extract_pair: median and interval of each in milliseconds
#define IMGPREP_HOST_NO_MAIN
#include "../../tests/imgprep_host.cc"

#include <ovslam_hip.h>

#include "openvslam/feature/orb_extractor.h"
#include "openvslam/util/image_converter.h"
#include "openvslam/util/stereo_rectifier.h"

using namespace openvslam;

namespace {

cv::Mat mat_of(const Case& c, int s) {
    return cv::Mat(c.rows, c.cols, c.channels == 1 ? cv::CV_8UC1 : (c.channels == 3 ? cv::CV_8UC3 : cv::CV_8UC4), const_cast<uint8_t*>(c.img[s].data()),
                   (size_t)c.cols * c.channels);
}

util::stereo_rectifier_config config_of(const Case& c) {
    util::stereo_rectifier_config cfg;
    cfg.model = c.side[0].model;
    cfg.rows = c.rows, cfg.cols = c.cols;
    cfg.fx = c.P[0], cfg.fy = c.P[1], cfg.cx = c.P[2], cfg.cy = c.P[3];
    std::vector<double>* K[2] = {&cfg.K_left, &cfg.K_right};
    std::vector<double>* D[2] = {&cfg.D_left, &cfg.D_right};
    std::vector<double>* R[2] = {&cfg.R_left, &cfg.R_right};
    for (int s = 0; s < 2; ++s) {
        K[s]->assign(c.side[s].K, c.side[s].K + 9);
        D[s]->assign(c.side[s].D, c.side[s].D + c.side[s].n_dist);
        R[s]->assign(c.side[s].R, c.side[s].R + 9);
    }
    return cfg;
}

bool same(const cv::Mat& a, const cv::Mat& b) {
    if (a.rows != b.rows || a.cols != b.cols || a.channels() != b.channels()) return false;
    for (int y = 0; y < a.rows; ++y)
        if (std::memcmp(a.ptr(y), b.ptr(y), (size_t)a.cols * a.channels()) != 0) return false;
    return true;
}

bool same_keypoints(const std::vector<cv::KeyPoint>& a, const cv::Mat& da, const std::vector<cv::KeyPoint>& b, const cv::Mat& db) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(cv::KeyPoint)) == 0) && same(da, db);
}

void write_mat(FILE* f, const cv::Mat& m) {
    for (int y = 0; y < m.rows; ++y) std::fwrite(m.ptr(y), 1, (size_t)m.cols * m.channels(), f);
}

int fail(const char* what) {
    std::fprintf(stderr, "test_imgprep_shim: %s\n", what);
    return 1;
}

struct Stats {
    double median, lo, hi;
};
Stats stats_of(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return Stats{v[v.size() / 2], v.front(), v.back()};
}

}   // namespace

int main(int argc, char** argv) {
    Case c;
    if (argc < 3 || !read_case(argv[1], c) || c.sides != 2 || c.rows < 1 || c.cols < 1) return fail("usage: test_imgprep_shim case.bin out.bin | --degraded | --time N");
    const camera::color_order_t order = (camera::color_order_t)c.color_order;
    const cv::Mat raw[2] = {mat_of(c, 0), mat_of(c, 1)};
    util::stereo_rectifier rectifier(config_of(c));
    const bool timing = !std::strcmp(argv[2], "--time");
    feature::orb_extractor extractor(timing ? 2000 : 500, 1.2f, 8, 20, 7);   // (timing: upstream's default feature count)
    std::vector<cv::KeyPoint> kl, kr;
    cv::Mat dl, dr, gl, gr;

    if (!std::strcmp(argv[2], "--degraded")) {
        const bool device = ovs_device_count() > 0;
        if (device) ovs_debug_inject_hip_failures(0, 1 << 20);
        cv::Mat rl, rr, g = raw[0].clone();
        rectifier.rectify(raw[0], raw[1], rl, rr);
        if (c.channels > 1) util::convert_to_grayscale(g, order);
        extractor.extract_pair_prepared(&rectifier, raw[0], raw[1], order, cv::_InputArray(), cv::_InputArray(), kl, dl, kr, dr, &gl, &gr);
        if (device) ovs_debug_inject_hip_failures(0, 0);
        if (!rl.empty() || !rr.empty() || (c.channels > 1 && !g.empty()) || !kl.empty() || !kr.empty() || !gl.empty() || !gr.empty() || dl.rows != 0 || dr.rows != 0)
            return fail("a class returned something under device failure");
        std::printf("degraded ok (%s)\n", device ? "failures injected" : "no device");
        return 0;
    }

    if (timing) {
        const int n = argc > 3 ? std::max(3, std::atoi(argv[3])) : 20;
        int32_t w[3];
        imgprep::gray_weights(c.channels, c.color_order, w);
        imgprep::FixedMap map[2];
        for (int s = 0; s < 2; ++s)
            if (!imgprep::build_fixed_map(&c.side[s], c.P, c.rows, c.cols, map[s])) return fail("the rig was refused");
        std::vector<uint8_t> gray[2] = {std::vector<uint8_t>((size_t)c.rows * c.cols), std::vector<uint8_t>((size_t)c.rows * c.cols)};
        ovs_orb_params p{2000, 1.2f, 8, 20, 7};
        ovs_orb* h = nullptr;
        if (ovs_orb_create(&p, c.rows, c.cols, 2, 0, &h) != OVS_OK) return fail("ovs_orb_create");
        const int cap = ovs_orb_max_keypoints(h);
        std::vector<ovs_keypoint> k0(cap), k1(cap);
        std::vector<uint8_t> d0((size_t)cap * 32), d1((size_t)cap * 32);
        std::vector<double> fused, loop, pair;
        for (int i = -3; i < n; ++i) {   // three warm-up rounds
            auto t0 = std::chrono::steady_clock::now();
            extractor.extract_pair_prepared(&rectifier, raw[0], raw[1], order, cv::_InputArray(), cv::_InputArray(), kl, dl, kr, dr);
            auto t1 = std::chrono::steady_clock::now();
            for (int s = 0; s < 2; ++s) prepare(c, c.img[s].data(), &map[s], w, gray[s].data());
            auto t2 = std::chrono::steady_clock::now();
            int32_t n0 = 0, n1 = 0;
            if (ovs_orb_extract_pair(h, gray[0].data(), gray[1].data(), c.rows, c.cols, (size_t)c.cols, nullptr, nullptr, 0, k0.data(), d0.data(), &n0, k1.data(), d1.data(), &n1,
                                     cap) != OVS_OK)
                return fail("ovs_orb_extract_pair");
            auto t3 = std::chrono::steady_clock::now();
            if (i < 0) continue;
            if ((size_t)n0 != kl.size() || (size_t)n1 != kr.size()) return fail("the two paths disagree");
            fused.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            loop.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
            pair.push_back(std::chrono::duration<double, std::milli>(t3 - t2).count());
        }
        ovs_orb_destroy(h);
        const Stats f = stats_of(fused), l = stats_of(loop), q = stats_of(pair);
        std::printf("%d x %d x %d, %d repetitions: extract_pair_prepared %.3f ms [%.3f, %.3f]; host loop %.3f ms [%.3f, %.3f] + extract_pair %.3f ms [%.3f, %.3f]\n", c.cols,
                    c.rows, c.channels, n, f.median, f.lo, f.hi, l.median, l.lo, l.hi, q.median, q.lo, q.hi);
        return 0;
    }

    // the classes one after the other: upstream's stereo frame constructor
    cv::Mat rect[2], gray_raw[2] = {raw[0].clone(), raw[1].clone()};
    rectifier.rectify(raw[0], raw[1], rect[0], rect[1]);
    if (rect[0].empty() || rect[1].empty()) return fail("rectify returned nothing");
    for (cv::Mat& g : gray_raw) util::convert_to_grayscale(g, order);
    cv::Mat two_step[2] = {rect[0].clone(), rect[1].clone()};
    std::vector<cv::KeyPoint> wk[2];
    cv::Mat wd[2];
    for (int s = 0; s < 2; ++s) {
        util::convert_to_grayscale(two_step[s], order);
        extractor.extract(two_step[s], cv::_InputArray(), wk[s], wd[s]);
    }
    // the fused call
    extractor.extract_pair_prepared(&rectifier, raw[0], raw[1], order, cv::_InputArray(), cv::_InputArray(), kl, dl, kr, dr, &gl, &gr);
    if (!same(gl, two_step[0]) || !same(gr, two_step[1])) return fail("the fused call's gray images differ from rectify + convert_to_grayscale");
    if (!same_keypoints(kl, dl, wk[0], wd[0]) || !same_keypoints(kr, dr, wk[1], wd[1])) return fail("the fused call's keypoints differ from the classes one after the other");
    std::vector<cv::KeyPoint> kl2, kr2;
    cv::Mat dl2, dr2;
    extractor.extract_pair_prepared(&rectifier, raw[0], raw[1], order, cv::_InputArray(), cv::_InputArray(), kl2, dl2, kr2, dr2);   // nothing comes down but the keypoints
    if (!same_keypoints(kl, dl, kl2, dl2) || !same_keypoints(kr, dr, kr2, dr2)) return fail("without gray outputs the keypoints differ");
    // gray conversion alone through the fused call
    cv::Mat g0, g1;
    extractor.extract_pair_prepared(nullptr, raw[0], raw[1], order, cv::_InputArray(), cv::_InputArray(), kl2, dl2, kr2, dr2, &g0, &g1);
    if (!same(g0, gray_raw[0]) || !same(g1, gray_raw[1])) return fail("the fused call without a rectifier differs from convert_to_grayscale");
    // a device failure that outlasts the retry: the empty result; the call after it is correct again
    ovs_debug_inject_hip_failures(0, 1 << 20);
    cv::Mat el, er;
    rectifier.rectify(raw[0], raw[1], el, er);
    ovs_debug_inject_hip_failures(0, 0);
    if (!el.empty() || !er.empty()) return fail("rectify returned something under device failure");
    rectifier.rectify(raw[0], raw[1], el, er);
    if (!same(el, rect[0]) || !same(er, rect[1])) return fail("the call after a device failure is wrong");

    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return fail("cannot write the output");
    for (int s = 0; s < 2; ++s) write_mat(f, rect[s]);
    for (int s = 0; s < 2; ++s) write_mat(f, gray_raw[s]);
    write_mat(f, gl);
    write_mat(f, gr);
    const int32_t n[2] = {(int32_t)kl.size(), (int32_t)kr.size()};
    std::fwrite(n, 4, 2, f);
    std::fclose(f);
    std::printf("ok: %d + %d keypoints\n", n[0], n[1]);
    return 0;
}
