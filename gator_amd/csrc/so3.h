// Rotations in fp64, shared by train_batch.hip (the camera-frame root orientation) and smpl_fit.hip (the fit's pose update):
// exp is Rodrigues' formula; log goes through the quaternion of the matrix (Shepperd's choice of the largest of trace, m00, m11, m22
// as the pivot), angle = 2 atan2(|q_xyz|, q_w) with q_w >= 0: an angle in [0, pi], accurate at both ends, where acos of the trace
// loses half the digits.
#pragma once
#include <hip/hip_runtime.h>

namespace gator {

__device__ inline void rotvec_exp(const double r[3], double E[3][3]) {
    const double angle = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (angle == 0.0) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[i][j] = i == j ? 1.0 : 0.0;
        return;
    }
    const double x = r[0] / angle, y = r[1] / angle, z = r[2] / angle;
    const double s = sin(angle), c = cos(angle), C = 1.0 - c;
    E[0][0] = c + C * x * x;     E[0][1] = C * x * y - s * z; E[0][2] = C * x * z + s * y;
    E[1][0] = C * x * y + s * z; E[1][1] = c + C * y * y;     E[1][2] = C * y * z - s * x;
    E[2][0] = C * x * z - s * y; E[2][1] = C * y * z + s * x; E[2][2] = c + C * z * z;
}

// The rotation vector of M, angle in [0, pi].  q is 4 q_pivot times the unit quaternion: only its direction is used.
__device__ inline void rotmat_log(const double M[3][3], double rv[3]) {
    const double tr = M[0][0] + M[1][1] + M[2][2];
    double w, x, y, z;
    if (tr >= M[0][0] && tr >= M[1][1] && tr >= M[2][2]) {
        w = 1.0 + tr;              x = M[2][1] - M[1][2];                     y = M[0][2] - M[2][0];                     z = M[1][0] - M[0][1];
    } else if (M[0][0] >= M[1][1] && M[0][0] >= M[2][2]) {
        w = M[2][1] - M[1][2];     x = 1.0 + M[0][0] - M[1][1] - M[2][2];     y = M[0][1] + M[1][0];                     z = M[0][2] + M[2][0];
    } else if (M[1][1] >= M[2][2]) {
        w = M[0][2] - M[2][0];     x = M[0][1] + M[1][0];                     y = 1.0 + M[1][1] - M[0][0] - M[2][2];     z = M[1][2] + M[2][1];
    } else {
        w = M[1][0] - M[0][1];     x = M[0][2] + M[2][0];                     y = M[1][2] + M[2][1];                     z = 1.0 + M[2][2] - M[0][0] - M[1][1];
    }
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double n = sqrt(x * x + y * y + z * z);
    if (n == 0.0) { rv[0] = rv[1] = rv[2] = 0.0; return; }
    const double k = 2.0 * atan2(n, w) / n;
    rv[0] = x * k; rv[1] = y * k; rv[2] = z * k;
}

}  // namespace gator
