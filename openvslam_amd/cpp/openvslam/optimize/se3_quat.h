// The two conversions the bundle adjusters (local_bundle_adjuster.cc, global_bundle_adjuster.cc) make between a keyframe's 4 x 4 pose and the
// 7-double SE3Quat record of the C ABI (translation, then the unit quaternion x, y, z, w).
#pragma once
#include <cmath>

#include "../data/frame_stub.h"

namespace openvslam {
namespace optimize {

// util::converter::to_g2o_SE3: rotation matrix -> unit quaternion (x, y, z, w) exactly as Eigen::Quaterniond(Matrix3d) does (the
// trace / largest-diagonal branches), then g2o::SE3Quat's normalisation with w >= 0
inline void pose_to_se3quat(const Mat44_t& T, double* p7) {
    double q[4];
    const double tr = (T(0, 0) + T(1, 1)) + T(2, 2);
    if (tr > 0.0) {
        double s = std::sqrt(tr + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (T(2, 1) - T(1, 2)) * s;
        q[1] = (T(0, 2) - T(2, 0)) * s;
        q[2] = (T(1, 0) - T(0, 1)) * s;
    } else {
        int i = 0;
        if (T(1, 1) > T(0, 0)) i = 1;
        if (T(2, 2) > T(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = std::sqrt(T(i, i) - T(j, j) - T(k, k) + 1.0);
        q[i] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (T(k, j) - T(j, k)) * s;
        q[j] = (T(j, i) + T(i, j)) * s;
        q[k] = (T(k, i) + T(i, k)) * s;
    }
    if (q[3] < 0.0)
        for (double& v : q) v = -v;
    const double n = std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    for (int a = 0; a < 3; ++a) p7[a] = T(a, 3);
    for (int a = 0; a < 4; ++a) p7[3 + a] = q[a] / n;
}

// shot_vertex::estimate() -> Mat44 (Eigen::Quaterniond::toRotationMatrix)
inline Mat44_t se3quat_to_pose(const double* p7) {
    const double x = p7[3], y = p7[4], z = p7[5], w = p7[6];
    Mat44_t T;
    T(0, 0) = 1 - 2 * (y * y + z * z);
    T(0, 1) = 2 * (x * y - z * w);
    T(0, 2) = 2 * (x * z + y * w);
    T(1, 0) = 2 * (x * y + z * w);
    T(1, 1) = 1 - 2 * (x * x + z * z);
    T(1, 2) = 2 * (y * z - x * w);
    T(2, 0) = 2 * (x * z - y * w);
    T(2, 1) = 2 * (y * z + x * w);
    T(2, 2) = 1 - 2 * (x * x + y * y);
    for (int a = 0; a < 3; ++a) T(a, 3) = p7[a];
    return T;
}

}   // namespace optimize
}   // namespace openvslam
