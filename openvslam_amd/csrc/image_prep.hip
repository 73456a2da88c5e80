// image_prep.hip -- the image front end on the device: gray conversion and stereo rectification in one launch, and the
// entries of the C ABI that own its handle. Replaces util::stereo_rectifier::rectify (two cv::remap calls) and util::convert_to_grayscale
// (cv::cvtColor) of upstream's frame constructors (expected: src/openvslam/util/stereo_rectifier.cc, image_converter.cc). The maps are built
// on the host by image_prep_plan.inc; the fused entries that write into the extractor's planes are in orb_api.hip.
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "image_prep_internal.inc"
#include "image_prep_plan.inc"

using namespace ovs;

namespace {

struct PrepArgs {
    const uint8_t* src[2];
    uint8_t* out[2];
    const uint32_t* ixy[2];
    const uint16_t* fxy[2];
    size_t src_stride, out_stride;
    int32_t rows, cols, map_pitch;
    int32_t w[3];       // rule I1's weights of channels 0, 1, 2
    int32_t src_dw;     // both source bases and the stride are multiples of 4: a lane's 4 pixels (no map) / a 4-channel tap load as dwords
    int32_t out_dw;     // the same for the outputs: a lane's 4 pixels are stored as one dword
};

// one tap of rule I6 for channel count CH: the bytes of the pixel at (x, y), or zeros outside -- the load itself always hits the source
// (offset 0 stands in for a tap outside; its value is dropped)
template <int CH>
__device__ __forceinline__ void tap(const uint8_t* __restrict__ src, const PrepArgs& a, int x, int y, int32_t c[3]) {
    const bool in = (unsigned)x < (unsigned)a.cols && (unsigned)y < (unsigned)a.rows;
    const uint8_t* q = src + (in ? (size_t)y * a.src_stride + (size_t)x * CH : (size_t)0);
    if constexpr (CH == 1) {
        c[0] = in ? (int32_t)q[0] : 0;
    } else {
        uint32_t v;
        if (CH == 4 && a.src_dw) v = *reinterpret_cast<const uint32_t*>(q);
        else v = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        v = in ? v : 0u;
        c[0] = (int32_t)(v & 0xffu);
        c[1] = (int32_t)((v >> 8) & 0xffu);
        c[2] = (int32_t)((v >> 16) & 0xffu);
    }
}

// rules I2, I6, I7 (and I1 for a colour source) for one output pixel with map entry (ix, iy, fx, fy)
template <int CH>
__device__ __forceinline__ uint32_t remap_pixel(const uint8_t* __restrict__ src, const PrepArgs& a, int ix, int iy, int fx, int fy) {
    constexpr int NC = CH == 1 ? 1 : 3;
    int32_t p00[3], p10[3], p01[3], p11[3];
    tap<CH>(src, a, ix, iy, p00);
    tap<CH>(src, a, ix + 1, iy, p10);
    tap<CH>(src, a, ix, iy + 1, p01);
    tap<CH>(src, a, ix + 1, iy + 1, p11);
    int32_t o[3];
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = imgprep::blend(p00[c], p10[c], p01[c], p11[c], fx, fy);
    if constexpr (CH == 1) return (uint32_t)o[0];
    else return (uint32_t)imgprep::gray_of(a.w, o[0], o[1], o[2]);
}

// A lane owns four consecutive pixels of a row; a workgroup 64 lanes x 4 rows; blockIdx.z is the side. RECT: through the resident map; otherwise
// rule I1 alone (CH == 1: a copy)
template <bool RECT, int CH>
__global__ __launch_bounds__(imgprep::kLanesX* imgprep::kRowsPerGroup) void k_image_prep(const PrepArgs a) {
    const int x0 = (int)(blockIdx.x * imgprep::kLanesX + threadIdx.x) * imgprep::kPixPerLane;
    const int y = (int)(blockIdx.y * imgprep::kRowsPerGroup + threadIdx.y);
    if (x0 >= a.cols || y >= a.rows) return;
    const bool right = blockIdx.z != 0;
    const uint8_t* __restrict__ src = right ? a.src[1] : a.src[0];
    uint8_t* __restrict__ out = (right ? a.out[1] : a.out[0]) + (size_t)y * a.out_stride + x0;
    const int n = min(imgprep::kPixPerLane, a.cols - x0);
    uint32_t px0 = 0, px1 = 0, px2 = 0, px3 = 0;
    if constexpr (RECT) {
        // the map's rows are padded to the lane's four entries (far outside), so the two wide loads are always inside it and aligned
        const size_t m = (size_t)y * a.map_pitch + x0;
        const uint4 e = *reinterpret_cast<const uint4*>((right ? a.ixy[1] : a.ixy[0]) + m);
        const uint2 f = *reinterpret_cast<const uint2*>((right ? a.fxy[1] : a.fxy[0]) + m);
        px0 = remap_pixel<CH>(src, a, (int)(int16_t)(e.x & 0xffffu), (int32_t)e.x >> 16, (int)(f.x & 0xffu), (int)((f.x >> 8) & 0xffu));
        px1 = remap_pixel<CH>(src, a, (int)(int16_t)(e.y & 0xffffu), (int32_t)e.y >> 16, (int)((f.x >> 16) & 0xffu), (int)(f.x >> 24));
        px2 = remap_pixel<CH>(src, a, (int)(int16_t)(e.z & 0xffffu), (int32_t)e.z >> 16, (int)(f.y & 0xffu), (int)((f.y >> 8) & 0xffu));
        px3 = remap_pixel<CH>(src, a, (int)(int16_t)(e.w & 0xffffu), (int32_t)e.w >> 16, (int)((f.y >> 16) & 0xffu), (int)(f.y >> 24));
    } else {
        const uint8_t* __restrict__ q = src + (size_t)y * a.src_stride + (size_t)x0 * CH;
        if (n == imgprep::kPixPerLane && a.src_dw) {   // x0 is a multiple of 4: the group starts on a dword for every CH
            const uint32_t* __restrict__ qd = reinterpret_cast<const uint32_t*>(q);
            if constexpr (CH == 1) {
                const uint32_t v = qd[0];
                px0 = v & 0xffu, px1 = (v >> 8) & 0xffu, px2 = (v >> 16) & 0xffu, px3 = v >> 24;
            } else if constexpr (CH == 3) {
                const uint32_t v0 = qd[0], v1 = qd[1], v2 = qd[2];   // c0 c1 c2 c0 | c1 c2 c0 c1 | c2 c0 c1 c2
                px0 = (uint32_t)imgprep::gray_of(a.w, v0 & 0xffu, (v0 >> 8) & 0xffu, (v0 >> 16) & 0xffu);
                px1 = (uint32_t)imgprep::gray_of(a.w, v0 >> 24, v1 & 0xffu, (v1 >> 8) & 0xffu);
                px2 = (uint32_t)imgprep::gray_of(a.w, (v1 >> 16) & 0xffu, v1 >> 24, v2 & 0xffu);
                px3 = (uint32_t)imgprep::gray_of(a.w, (v2 >> 8) & 0xffu, (v2 >> 16) & 0xffu, v2 >> 24);
            } else {
                const uint32_t v0 = qd[0], v1 = qd[1], v2 = qd[2], v3 = qd[3];   // (a row's base is only known to be 4-byte aligned)
                px0 = (uint32_t)imgprep::gray_of(a.w, v0 & 0xffu, (v0 >> 8) & 0xffu, (v0 >> 16) & 0xffu);
                px1 = (uint32_t)imgprep::gray_of(a.w, v1 & 0xffu, (v1 >> 8) & 0xffu, (v1 >> 16) & 0xffu);
                px2 = (uint32_t)imgprep::gray_of(a.w, v2 & 0xffu, (v2 >> 8) & 0xffu, (v2 >> 16) & 0xffu);
                px3 = (uint32_t)imgprep::gray_of(a.w, v3 & 0xffu, (v3 >> 8) & 0xffu, (v3 >> 16) & 0xffu);
            }
        } else {
            auto one = [&](int k) -> uint32_t {
                if (k >= n) return 0u;   // the tail of a row: nothing beyond its last pixel is read
                const uint8_t* t = q + k * CH;
                if constexpr (CH == 1) return (uint32_t)t[0];
                else return (uint32_t)imgprep::gray_of(a.w, (int32_t)t[0], (int32_t)t[1], (int32_t)t[2]);
            };
            px0 = one(0), px1 = one(1), px2 = one(2), px3 = one(3);
        }
    }
    if (n == imgprep::kPixPerLane && a.out_dw) {
        *reinterpret_cast<uint32_t*>(out) = px0 | (px1 << 8) | (px2 << 16) | (px3 << 24);
    } else {
        out[0] = (uint8_t)px0;
        if (n > 1) out[1] = (uint8_t)px1;
        if (n > 2) out[2] = (uint8_t)px2;
        if (n > 3) out[3] = (uint8_t)px3;
    }
}

template <bool RECT>
hipError_t launch_prep(const PrepArgs& a, int channels, int sides, hipStream_t s) {
    const imgprep::Launch g = imgprep::launch_for(a.rows, a.cols, sides);
    const dim3 grid(g.gx, g.gy, g.gz), block(g.bx, g.by);
    if (channels == 1) k_image_prep<RECT, 1><<<grid, block, 0, s>>>(a);
    else if (channels == 3) k_image_prep<RECT, 3><<<grid, block, 0, s>>>(a);
    else k_image_prep<RECT, 4><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

// both fixed maps of a handle replaced by `m` (side 1 may be empty); the handle's lock is held
ovs_status upload_maps(ovs_imgprep* p, const imgprep::FixedMap m[2], int sides) {
    OVS_HIP_TRY(hipSetDevice(p->device));
    OVS_HIP_TRY(hipStreamSynchronize(p->stream));   // a host-form run of the previous map has ended anyway; the _dev form is the caller's to order
    p->map_rows = p->map_cols = p->map_sides = 0;   // half-replaced maps are no maps
    for (int sd = 0; sd < sides; ++sd) {
        OVS_HIP_TRY(hipMemcpy(p->d_ixy[sd], m[sd].ixy.data(), m[sd].ixy.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        OVS_HIP_TRY(hipMemcpy(p->d_fxy[sd], m[sd].fxy.data(), m[sd].fxy.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    p->map_rows = m[0].rows, p->map_cols = m[0].cols, p->map_pitch = m[0].pitch, p->map_sides = sides;
    return OVS_OK;
}

}   // namespace

namespace ovs {

ovs_status imgprep_check(const ovs_imgprep* p, int rows, int cols, size_t src_stride, int channels, int color_order, int rectify, int sides) {
    return imgprep::run_status(rows, cols, src_stride, channels, color_order, rectify, sides, p->max_rows, p->max_cols, p->map_rows, p->map_cols, p->map_sides);
}

hipError_t imgprep_enqueue(const ovs_imgprep* p, const uint8_t* d_src_l, const uint8_t* d_src_r, int rows, int cols, size_t src_stride, int channels,
                           int color_order, int rectify, uint8_t* d_out_l, uint8_t* d_out_r, size_t out_stride, hipStream_t s) {
    PrepArgs a;
    a.src[0] = d_src_l, a.src[1] = d_src_r;
    a.out[0] = d_out_l, a.out[1] = d_out_r;
    a.ixy[0] = p->d_ixy[0], a.ixy[1] = p->d_ixy[1];
    a.fxy[0] = p->d_fxy[0], a.fxy[1] = p->d_fxy[1];
    a.src_stride = src_stride, a.out_stride = out_stride;
    a.rows = rows, a.cols = cols, a.map_pitch = p->map_pitch;
    imgprep::gray_weights(channels, color_order, a.w);
    a.src_dw = !(((uintptr_t)d_src_l | (uintptr_t)d_src_r | src_stride) & 3);
    a.out_dw = !(((uintptr_t)d_out_l | (uintptr_t)d_out_r | out_stride) & 3);
    const int sides = d_src_r ? 2 : 1;
    return rectify ? launch_prep<true>(a, channels, sides, s) : launch_prep<false>(a, channels, sides, s);
}

}   // namespace ovs

extern "C" {

ovs_status ovs_imgprep_create(int32_t device, int32_t max_rows, int32_t max_cols, ovs_imgprep** out) {
    if (!out || max_rows < 1 || max_cols < 1 || max_rows > imgprep::kMaxDim || max_cols > imgprep::kMaxDim) return OVS_ERR_INVALID;
    *out = nullptr;
    if (device < 0 || ovs_device_count() <= device) return OVS_ERR_NO_DEVICE;
    std::unique_ptr<ovs_imgprep> owner(new (std::nothrow) ovs_imgprep());
    ovs_imgprep* const p = owner.get();
    if (!p) return OVS_ERR_INVALID;
    p->device = device, p->max_rows = max_rows, p->max_cols = max_cols;
    OVS_HIP_TRY_RAW(hipSetDevice(device));
    OVS_HIP_TRY_RAW(p->res.stream(&p->stream));
    p->src_pitch = ((size_t)max_cols * 4 + 255) & ~(size_t)255;
    p->out_pitch = ((size_t)max_cols + 255) & ~(size_t)255;
    const size_t map_entries = (size_t)max_rows * (((size_t)max_cols + 3) & ~(size_t)3);
    for (int sd = 0; sd < 2; ++sd) {
        OVS_HIP_TRY_RAW(p->res.dev(&p->d_src[sd], p->src_pitch * max_rows));
        OVS_HIP_TRY_RAW(p->res.dev(&p->d_out[sd], p->out_pitch * max_rows));
        OVS_HIP_TRY_RAW(p->res.dev(&p->d_ixy[sd], map_entries * sizeof(uint32_t)));
        OVS_HIP_TRY_RAW(p->res.dev(&p->d_fxy[sd], map_entries * sizeof(uint16_t)));
    }
    *out = owner.release();
    return OVS_OK;
}

ovs_status ovs_imgprep_destroy(ovs_imgprep* p) {
    if (!p) return OVS_OK;
    (void)hipSetDevice(p->device);
    delete p;
    return OVS_OK;
}

ovs_status ovs_imgprep_set_rectifier(ovs_imgprep* p, int32_t rows, int32_t cols, const ovs_rectify_side* left, const ovs_rectify_side* right,
                                     const double* rect_fx_fy_cx_cy) {
    if (!p || !left || !rect_fx_fy_cx_cy || rows < 1 || cols < 1) return OVS_ERR_INVALID;
    if (!imgprep::side_ok(left) || (right && !imgprep::side_ok(right)) || !imgprep::all_finite(rect_fx_fy_cx_cy, 4)) return OVS_ERR_INVALID;
    double iR[9];
    if (!imgprep::inverse_PR(left->R, rect_fx_fy_cx_cy, iR) || (right && !imgprep::inverse_PR(right->R, rect_fx_fy_cx_cy, iR))) return OVS_ERR_INVALID;
    if (rows > p->max_rows || cols > p->max_cols) return OVS_ERR_CAPACITY;
    imgprep::FixedMap m[2];
    if (!imgprep::build_fixed_map(left, rect_fx_fy_cx_cy, rows, cols, m[0])) return OVS_ERR_INVALID;
    if (right && !imgprep::build_fixed_map(right, rect_fx_fy_cx_cy, rows, cols, m[1])) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    return upload_maps(p, m, right ? 2 : 1);
}

ovs_status ovs_imgprep_set_maps(ovs_imgprep* p, int32_t rows, int32_t cols, const float* map_x_left, const float* map_y_left,
                                const float* map_x_right, const float* map_y_right) {
    if (!p || !map_x_left || !map_y_left || (map_x_right == nullptr) != (map_y_right == nullptr) || rows < 1 || cols < 1) return OVS_ERR_INVALID;
    if (rows > p->max_rows || cols > p->max_cols) return OVS_ERR_CAPACITY;
    imgprep::FixedMap m[2];
    imgprep::fix_maps(map_x_left, map_y_left, rows, cols, (size_t)cols, m[0]);
    if (map_x_right) imgprep::fix_maps(map_x_right, map_y_right, rows, cols, (size_t)cols, m[1]);
    std::lock_guard<std::mutex> lock(p->mu);
    return upload_maps(p, m, map_x_right ? 2 : 1);
}

ovs_status ovs_imgprep_get_maps(ovs_imgprep* p, int32_t side, int16_t* ixy, uint8_t* fxy) {
    if (!p || side < 0 || side > 1) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    if (side >= p->map_sides || p->map_rows == 0) return OVS_ERR_INVALID;
    OVS_HIP_TRY(hipSetDevice(p->device));
    const size_t row = (size_t)p->map_cols, pitch = (size_t)p->map_pitch;
    if (ixy) OVS_HIP_TRY(hipMemcpy2D(ixy, row * 4, p->d_ixy[side], pitch * 4, row * 4, (size_t)p->map_rows, hipMemcpyDeviceToHost));
    if (fxy) OVS_HIP_TRY(hipMemcpy2D(fxy, row * 2, p->d_fxy[side], pitch * 2, row * 2, (size_t)p->map_rows, hipMemcpyDeviceToHost));
    return OVS_OK;
}

ovs_status ovs_imgprep_run(ovs_imgprep* p, const uint8_t* src_left, const uint8_t* src_right, int32_t rows, int32_t cols, size_t src_stride,
                           int32_t channels, int32_t color_order, int32_t rectify, uint8_t* out_left, uint8_t* out_right, size_t out_stride) {
    if (!p || !src_left || !out_left || (src_right == nullptr) != (out_right == nullptr)) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    const int sides = src_right ? 2 : 1;
    const ovs_status st = imgprep_check(p, rows, cols, src_stride, channels, color_order, rectify, sides);
    if (st != OVS_OK) return st;
    if (out_stride < (size_t)cols) return OVS_ERR_INVALID;
    if (rows == 0 || cols == 0) return OVS_OK;
    OVS_HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = p->stream;
    const uint8_t* const src[2] = {src_left, src_right};
    uint8_t* const out[2] = {out_left, out_right};
    for (int sd = 0; sd < sides; ++sd)
        OVS_HIP_TRY(hipMemcpy2DAsync(p->d_src[sd], p->src_pitch, src[sd], src_stride, (size_t)cols * channels, (size_t)rows, hipMemcpyHostToDevice, s));
    OVS_HIP_TRY(imgprep_enqueue(p, p->d_src[0], sides == 2 ? p->d_src[1] : nullptr, rows, cols, p->src_pitch, channels, color_order, rectify, p->d_out[0],
                                sides == 2 ? p->d_out[1] : nullptr, p->out_pitch, s));
    for (int sd = 0; sd < sides; ++sd)
        OVS_HIP_TRY(hipMemcpy2DAsync(out[sd], out_stride, p->d_out[sd], p->out_pitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, s));
    OVS_HIP_TRY(hipStreamSynchronize(s));
    return OVS_OK;
}

ovs_status ovs_imgprep_run_dev(ovs_imgprep* p, const uint8_t* d_src_left, const uint8_t* d_src_right, int32_t rows, int32_t cols, size_t src_stride,
                               int32_t channels, int32_t color_order, int32_t rectify, uint8_t* d_out_left, uint8_t* d_out_right, size_t out_stride,
                               void* stream) {
    if (!p || !d_src_left || !d_out_left || (d_src_right == nullptr) != (d_out_right == nullptr)) return OVS_ERR_INVALID;
    std::lock_guard<std::mutex> lock(p->mu);
    const ovs_status st = imgprep_check(p, rows, cols, src_stride, channels, color_order, rectify, d_src_right ? 2 : 1);
    if (st != OVS_OK) return st;
    if (out_stride < (size_t)cols) return OVS_ERR_INVALID;
    if (rows == 0 || cols == 0) return OVS_OK;
    OVS_HIP_TRY(hipSetDevice(p->device));
    OVS_HIP_TRY(imgprep_enqueue(p, d_src_left, d_src_right, rows, cols, src_stride, channels, color_order, rectify, d_out_left, d_out_right, out_stride,
                                (hipStream_t)stream));
    return OVS_OK;
}

}   // extern "C"
