// util::convert_to_grayscale -- upstream's public surface (expected: src/openvslam/util/image_converter.h), body on the MI355X: rule I1 of
// DESIGN.md 3.18 by the library's k_image_prep instead of cv::cvtColor. The frame constructors call it on every image; a tracker that goes through
// feature::orb_extractor::extract_prepared / extract_pair_prepared does not need it at all (the conversion happens on the way into the extractor).
#pragma once
#include <ovslam_hip.h>

#include <string>

#include "../../cv_stub.h"
#include "device_policy.h"

namespace openvslam {
namespace camera {
// upstream: src/openvslam/camera/base.h
enum class color_order_t { Gray = 0, RGB = 1, BGR = 2 };
}   // namespace camera

namespace util {
namespace detail {

// one preparer per thread and device for the callers that have no rig (gray conversion alone), grown to the largest image seen
struct thread_preparer {
    ovs_imgprep* p = nullptr;
    int rows = 0, cols = 0, device = -1;
    ~thread_preparer() { drop(); }
    void drop() {
        if (p) ovs_imgprep_destroy(p);
        p = nullptr;
        rows = cols = 0;
    }
    // throws device_error inside a guarded call
    ovs_imgprep* get(int dev, int r, int c) {
        if (p && dev == device && r <= rows && c <= cols) return p;
        const int nr = r > rows ? r : rows, nc = c > cols ? c : cols;
        drop();
        const int st = ovs_imgprep_create(dev, nr, nc, &p);
        if (st != OVS_OK) {
            p = nullptr;
            throw device_error(st, std::string("ovs_imgprep_create: ") + ovs_last_error());
        }
        rows = nr, cols = nc, device = dev;
        return p;
    }
    static thread_preparer& of_this_thread() {
        static thread_local thread_preparer t;
        return t;
    }
};

}   // namespace detail

//! Convert an 8-bit image of 3 or 4 channels to gray in place (a 1-channel image is left as it is). On a device failure (device_policy.h: one
//! retry on a rebuilt context) the image becomes the empty Mat, which every consumer treats as "no frame".
inline void convert_to_grayscale(cv::Mat& img, const camera::color_order_t in_color_order, const int device = 0) {
    if (img.empty() || img.channels() == 1) return;
    cv::Mat gray(img.rows, img.cols, cv::CV_8UC1);
    detail::thread_preparer& tp = detail::thread_preparer::of_this_thread();
    const bool ok = run_guarded(
        "convert_to_grayscale",
        [&] {
            return (int)ovs_imgprep_run(tp.get(device, img.rows, img.cols), img.data, nullptr, img.rows, img.cols, img.step, img.channels(), (int)in_color_order, 0,
                                        gray.data, nullptr, gray.step);
        },
        [&] { tp.drop(); });
    img = ok ? gray : cv::Mat();
}

}   // namespace util
}   // namespace openvslam
