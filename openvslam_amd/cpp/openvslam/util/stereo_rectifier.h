// util::stereo_rectifier -- upstream's public surface (expected: src/openvslam/util/stereo_rectifier.h), body on the MI355X: the maps of
// cv::initUndistortRectifyMap by rules I3 to I5 of DESIGN.md 3.18, the two cv::remap calls of rectify() by one launch of the library's
// k_image_prep. Upstream constructs it from the camera and the "StereoRectifier" YAML node; this tree has neither yaml-cpp nor camera::base, so
// the constructor takes the same values as a plain struct (INTEGRATION.md names the YAML keys).
#pragma once
#include <ovslam_hip.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../cv_stub.h"
#include "device_policy.h"

namespace openvslam {
namespace util {

struct stereo_rectifier_config {
    int model = OVS_RECTIFY_PERSPECTIVE;       // "StereoRectifier.model": perspective | fisheye
    int rows = 0, cols = 0;                    // the rectified camera: camera->rows_, cols_, fx_, fy_, cx_, cy_
    double fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<double> K_left, D_left, R_left, K_right, D_right, R_right;   // "StereoRectifier.K_left" ... (3x3 row-major; D: 0, 4, 5 or 8 values)
};

class stereo_rectifier {
public:
    explicit stereo_rectifier(const stereo_rectifier_config& cfg, const int device = 0) : cfg_(cfg), device_(device) {}
    virtual ~stereo_rectifier() { release(); }
    stereo_rectifier(const stereo_rectifier&) = delete;
    stereo_rectifier& operator=(const stereo_rectifier&) = delete;

    //! Apply stereo-rectification: every channel of both images through the rig's maps. On a device failure (device_policy.h: one retry on a
    //! rebuilt context) both outputs are the empty Mat.
    void rectify(const cv::Mat& in_img_l, const cv::Mat& in_img_r, cv::Mat& out_img_l, cv::Mat& out_img_r) const {
        if (in_img_l.empty() || in_img_r.empty()) {
            out_img_l = out_img_r = cv::Mat();
            return;
        }
        const int rows = in_img_l.rows, cols = in_img_l.cols, ch = in_img_l.channels();
        cv::Mat out[2] = {cv::Mat(rows, cols, in_img_l.type()), cv::Mat(rows, cols, in_img_l.type())};
        const cv::Mat* in[2] = {&in_img_l, &in_img_r};
        std::lock_guard<std::mutex> lock(mtx_);
        const bool ok = run_guarded(
            "stereo_rectifier::rectify",
            [&]() -> int {
                ovs_imgprep* p = ensure();
                if (ch == 1 && in_img_l.step == in_img_r.step)
                    return ovs_imgprep_run(p, in_img_l.data, in_img_r.data, rows, cols, in_img_l.step, 1, OVS_COLOR_GRAY, 1, out[0].data, out[1].data, out[0].step);
                // the channels are independent (rule I2 remaps each and rounds it to a byte): one plane of the pair at a time
                std::vector<uint8_t> plane[2] = {std::vector<uint8_t>((size_t)rows * cols), std::vector<uint8_t>((size_t)rows * cols)}, res[2] = {plane[0], plane[1]};
                for (int c = 0; c < ch; ++c) {
                    for (int s = 0; s < 2; ++s)
                        for (int y = 0; y < rows; ++y)
                            for (int x = 0; x < cols; ++x) plane[s][(size_t)y * cols + x] = in[s]->ptr(y)[(size_t)x * ch + c];
                    const int st = ovs_imgprep_run(p, plane[0].data(), plane[1].data(), rows, cols, (size_t)cols, 1, OVS_COLOR_GRAY, 1, res[0].data(), res[1].data(), (size_t)cols);
                    if (st != OVS_OK) return st;
                    for (int s = 0; s < 2; ++s)
                        for (int y = 0; y < rows; ++y)
                            for (int x = 0; x < cols; ++x) out[s].ptr(y)[(size_t)x * ch + c] = res[s][(size_t)y * cols + x];
                }
                return OVS_OK;
            },
            [&] { release(); });
        out_img_l = ok ? out[0] : cv::Mat();
        out_img_r = ok ? out[1] : cv::Mat();
    }

    // ---- additions of the MI355X backend ----
    //! the preparer with this rig's maps resident, for feature::orb_extractor::extract_pair_prepared; throws util::device_error inside a guarded call
    ovs_imgprep* preparer() const {
        std::lock_guard<std::mutex> lock(mtx_);
        return ensure();
    }
    //! drops the device context (rebuilt, maps included, on the next use)
    void reset() const {
        std::lock_guard<std::mutex> lock(mtx_);
        release();
    }
    int get_device() const { return device_; }

private:
    ovs_imgprep* ensure() const {
        if (p_) return p_;
        int st = ovs_imgprep_create(device_, cfg_.rows, cfg_.cols, &p_);
        if (st != OVS_OK) {
            p_ = nullptr;
            throw device_error(st, std::string("ovs_imgprep_create: ") + ovs_last_error());
        }
        ovs_rectify_side side[2];
        const std::vector<double>* K[2] = {&cfg_.K_left, &cfg_.K_right};
        const std::vector<double>* D[2] = {&cfg_.D_left, &cfg_.D_right};
        const std::vector<double>* R[2] = {&cfg_.R_left, &cfg_.R_right};
        st = OVS_OK;
        for (int s = 0; s < 2; ++s) {
            if (K[s]->size() != 9 || R[s]->size() != 9 || D[s]->size() > 8) st = OVS_ERR_INVALID;
            if (st != OVS_OK) break;
            side[s].model = cfg_.model;
            side[s].n_dist = (int32_t)D[s]->size();
            for (int i = 0; i < 9; ++i) side[s].K[i] = (*K[s])[i], side[s].R[i] = (*R[s])[i];
            for (int i = 0; i < 8; ++i) side[s].D[i] = i < (int)D[s]->size() ? (*D[s])[i] : 0.0;
        }
        const double P[4] = {cfg_.fx, cfg_.fy, cfg_.cx, cfg_.cy};
        if (st == OVS_OK) st = ovs_imgprep_set_rectifier(p_, cfg_.rows, cfg_.cols, &side[0], &side[1], P);
        if (st != OVS_OK) {
            const std::string msg = std::string("ovs_imgprep_set_rectifier: ") + ovs_last_error();
            release();
            throw device_error(st, msg);
        }
        return p_;
    }
    void release() const {
        if (p_) ovs_imgprep_destroy(p_);
        p_ = nullptr;
    }

    const stereo_rectifier_config cfg_;
    const int device_;
    mutable std::mutex mtx_;
    mutable ovs_imgprep* p_ = nullptr;
};

}   // namespace util
}   // namespace openvslam
