// image_prep_plan.inc -- the host-only part of the image front end (DESIGN.md 3.18): the rectification map of a camera (rules I3 and I4), its
// conversion to the resident fixed-point form (I5), the argument checks of the C ABI and the launch geometry of k_image_prep. Plain C++, no
// HIP: csrc/image_prep.hip includes it for the library, tests/imgprep_host.cc for the stand-alone host program the CPU tier compares with the
// Python reference (tests/imgprep_ref.py). Every f64 operation is rounded on its own (both are built with -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ovslam_hip.h"
#include "../../include/ovs_detmath.h"

// the two integer rules are shared with the kernel (the only lines of this file a device compiler sees as device code)
#if defined(__HIPCC__) || defined(__HIP__)
#define IMGPREP_FN __host__ __device__ inline
#else
#define IMGPREP_FN inline
#endif

namespace imgprep {

// ---- launch geometry: a lane owns 4 consecutive pixels of a row, a workgroup 64 lanes x 4 rows = 256 x 4 pixels, the side is grid.z ----
constexpr int kPixPerLane = 4, kLanesX = 64, kRowsPerGroup = 4;
constexpr int kSpanX = kPixPerLane * kLanesX;
// an int16 integer part saturates at 32767: every image narrower and lower than that sees a saturated coordinate as outside (I5, I6)
constexpr int kMaxDim = 16384;

struct Launch {
    unsigned gx, gy, gz, bx, by;
};
inline Launch launch_for(int rows, int cols, int sides) {
    return Launch{(unsigned)((cols + kSpanX - 1) / kSpanX), (unsigned)((rows + kRowsPerGroup - 1) / kRowsPerGroup), (unsigned)sides, (unsigned)kLanesX,
                  (unsigned)kRowsPerGroup};
}

// ---- I1: the weights of channels 0, 1, 2 of the source ----
inline bool gray_weights(int channels, int color_order, int32_t w[3]) {
    w[0] = w[1] = w[2] = 0;
    if (channels == 1) return color_order == OVS_COLOR_GRAY || color_order == OVS_COLOR_RGB || color_order == OVS_COLOR_BGR;   // passes through
    if (channels != 3 && channels != 4) return false;
    if (color_order != OVS_COLOR_RGB && color_order != OVS_COLOR_BGR) return false;
    w[1] = 9617;
    w[color_order == OVS_COLOR_RGB ? 0 : 2] = 4899;
    w[color_order == OVS_COLOR_RGB ? 2 : 0] = 1868;
    return true;
}

// ---- I5: the resident map. Rows of `pitch` entries (cols rounded up to the lane's four pixels; the padding reads as far outside) ----
struct FixedMap {
    int rows = 0, cols = 0, pitch = 0;
    std::vector<uint32_t> ixy;   // (uint16)ix | (uint16)iy << 16
    std::vector<uint16_t> fxy;   // fx | fy << 8
    void resize(int r, int c) {
        rows = r, cols = c, pitch = (c + kPixPerLane - 1) / kPixPerLane * kPixPerLane;
        ixy.assign((size_t)r * pitch, 0x80008000u);
        fxy.assign((size_t)r * pitch, 0);
    }
};
constexpr int32_t kFarOutside = -32768;

// one coordinate: the integer part (saturated to int16) and the 5-bit fraction of lrintf(m * 32); NaN or |m * 32| beyond 2^30: far outside
inline void fix_coord(float m, int32_t& ip, int32_t& fr) {
    const float s = m * 32.0f;
    if (!(std::fabs(s) <= 1073741824.0f)) {
        ip = kFarOutside;
        fr = 0;
        return;
    }
    const int32_t q = (int32_t)lrintf(s);   // ties to even (the default rounding mode)
    const int32_t i = q >> 5;
    ip = i < -32768 ? -32768 : (i > 32767 ? 32767 : i);
    fr = q & 31;
}
inline void fix_entry(float mx, float my, uint32_t& ixy, uint16_t& fxy) {
    int32_t ix, iy, fx, fy;
    fix_coord(mx, ix, fx);
    fix_coord(my, iy, fy);
    ixy = ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
    fxy = (uint16_t)(fx | (fy << 8));
}
// float maps of rows x cols with strides in floats
inline void fix_maps(const float* map_x, const float* map_y, int rows, int cols, size_t stride, FixedMap& out) {
    out.resize(rows, cols);
    for (int v = 0; v < rows; ++v)
        for (int u = 0; u < cols; ++u)
            fix_entry(map_x[(size_t)v * stride + u], map_y[(size_t)v * stride + u], out.ixy[(size_t)v * out.pitch + u], out.fxy[(size_t)v * out.pitch + u]);
}

// ---- argument checks ----
inline bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
inline bool side_ok(const ovs_rectify_side* s) {
    if (!s) return false;
    if (s->model == OVS_RECTIFY_PERSPECTIVE) {
        if (s->n_dist != 0 && s->n_dist != 4 && s->n_dist != 5 && s->n_dist != 8) return false;
    } else if (s->model == OVS_RECTIFY_FISHEYE) {
        if (s->n_dist != 4) return false;
    } else {
        return false;
    }
    return all_finite(s->K, 9) && all_finite(s->D, s->n_dist) && all_finite(s->R, 9);
}
// the size of a map or an image against the handle's: OVS_ERR_INVALID (negative), OVS_ERR_CAPACITY (too large) or OVS_OK (0 x 0 included)
inline ovs_status size_status(int rows, int cols, int max_rows, int max_cols) {
    if (rows < 0 || cols < 0) return OVS_ERR_INVALID;
    if (rows > max_rows || cols > max_cols) return OVS_ERR_CAPACITY;
    return OVS_OK;
}
// everything ovs_imgprep_run and its relatives refuse that does not need the pointers: map_rows x map_cols is the handle's current map (0 x 0: none),
// map_sides the sides it has
inline ovs_status run_status(int rows, int cols, size_t src_stride, int channels, int color_order, int rectify, int sides, int max_rows, int max_cols,
                             int map_rows, int map_cols, int map_sides) {
    int32_t w[3];
    if (!gray_weights(channels, color_order, w)) return OVS_ERR_INVALID;
    const ovs_status st = size_status(rows, cols, max_rows, max_cols);
    if (st != OVS_OK) return st;
    if (src_stride < (size_t)cols * (size_t)channels) return OVS_ERR_INVALID;
    if (rectify && (map_rows == 0 || map_cols == 0 || map_rows != rows || map_cols != cols || sides > map_sides)) return OVS_ERR_INVALID;
    return OVS_OK;
}

// ---- I3 / I4: the float map of one camera ----
// iR = (P R)^-1 by the adjugate over the determinant; P = [fx 0 cx; 0 fy cy; 0 0 1], the products with its zeros are not formed
inline bool inverse_PR(const double R[9], const double P[4], double iR[9]) {
    double M[9];
    for (int j = 0; j < 3; ++j) {
        M[j] = P[0] * R[j] + P[2] * R[6 + j];
        M[3 + j] = P[1] * R[3 + j] + P[3] * R[6 + j];
        M[6 + j] = R[6 + j];
    }
    double c[9];
    c[0] = M[4] * M[8] - M[5] * M[7];
    c[1] = M[2] * M[7] - M[1] * M[8];
    c[2] = M[1] * M[5] - M[2] * M[4];
    c[3] = M[5] * M[6] - M[3] * M[8];
    c[4] = M[0] * M[8] - M[2] * M[6];
    c[5] = M[2] * M[3] - M[0] * M[5];
    c[6] = M[3] * M[7] - M[4] * M[6];
    c[7] = M[1] * M[6] - M[0] * M[7];
    c[8] = M[0] * M[4] - M[1] * M[3];
    const double det = M[0] * c[0] + M[1] * c[3] + M[2] * c[6];
    if (!std::isfinite(det) || det == 0.0) return false;
    for (int i = 0; i < 9; ++i) iR[i] = c[i] / det;
    return all_finite(iR, 9);
}

inline void map_point(const ovs_rectify_side& s, const double iR[9], const double k[8], double u, double v, float& mx, float& my) {
    const double X = iR[0] * u + iR[1] * v + iR[2];
    const double Y = iR[3] * u + iR[4] * v + iR[5];
    const double W = iR[6] * u + iR[7] * v + iR[8];
    const double x = X / W, y = Y / W;
    const double fxK = s.K[0], fyK = s.K[4], cxK = s.K[2], cyK = s.K[5];
    if (s.model == OVS_RECTIFY_PERSPECTIVE) {
        const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
        const double r2 = x * x + y * y;
        const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
        const double xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        mx = (float)(fxK * xd + cxK);
        my = (float)(fyK * yd + cyK);
    } else {
        const double r = ovs_dm::sqrt_d(x * x + y * y);
        const double th = ovs_det_atan(r);
        const double t2 = th * th;
        const double thd = th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
        const double scale = (r == 0.0) ? 1.0 : thd / r;
        mx = (float)(fxK * x * scale + cxK);
        my = (float)(fyK * y * scale + cyK);
    }
}

// the fixed map of one camera; false for what the ABI refuses (a bad side, a non-finite rectified camera, a singular P R)
inline bool build_fixed_map(const ovs_rectify_side* s, const double P[4], int rows, int cols, FixedMap& out) {
    if (!side_ok(s) || !P || !all_finite(P, 4)) return false;
    double iR[9];
    if (!inverse_PR(s->R, P, iR)) return false;
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < s->n_dist; ++i) k[i] = s->D[i];
    out.resize(rows, cols);
    for (int v = 0; v < rows; ++v)
        for (int u = 0; u < cols; ++u) {
            float mx, my;
            map_point(*s, iR, k, (double)u, (double)v, mx, my);
            fix_entry(mx, my, out.ixy[(size_t)v * out.pitch + u], out.fxy[(size_t)v * out.pitch + u]);
        }
    return true;
}

// ---- I7 (with I6's zero for a tap outside), the form both the kernel and the host loop evaluate ----
IMGPREP_FN int32_t blend(int32_t p00, int32_t p10, int32_t p01, int32_t p11, int32_t fx, int32_t fy) {
    return ((32 - fx) * (32 - fy) * p00 + fx * (32 - fy) * p10 + (32 - fx) * fy * p01 + fx * fy * p11 + 512) >> 10;
}
IMGPREP_FN int32_t gray_of(const int32_t* w, int32_t c0, int32_t c1, int32_t c2) { return (c0 * w[0] + c1 * w[1] + c2 * w[2] + 8192) >> 14; }

}   // namespace imgprep
