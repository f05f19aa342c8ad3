// The 2D joint chain, stated once: the steps that k_preprocess, k_preprocess_chain (caller_kernels.hip) and k_crop_joints (camera.hip)
// share.  One lane per sample, 64-lane blocks; a sample's joints are one COLUMN of a [kMaxJ][64] LDS image (run-time indexed private
// arrays would live in scratch).  Every piece keeps the reference's own mix of float32 and fp64, rounding for rounding: a caller is
// these calls in order plus what is its own (the aspect step, the box it writes, the flip).
#pragma once
#include <hip/hip_runtime.h>

#include "internal.h"

namespace gator {
namespace {

// element j of this lane's column of a [n][64] LDS image
template <class T> struct Col {
    T* base; int tid;
    __device__ __forceinline__ T& operator[](int j) const { return base[j * 64 + tid]; }
};

// The sample's jin joints (comps floats each, x and y first) into the columns; add_pn appends pelvis = (L_Hip + R_Hip) / 2 and
// neck = (L_Shoulder + R_Shoulder) / 2 of the COCO order (joints 11, 12 and 5, 6; demo/run.py:103-121).  Returns the joint count.
__device__ __forceinline__ int load_joints(const float* __restrict__ p, int jin, int comps, int add_pn, const Col<double>& x, const Col<double>& y) {
    for (int j = 0; j < jin; ++j) { x[j] = p[j * comps]; y[j] = p[j * comps + 1]; }
    if (add_pn) {
        x[jin] = (x[11] + x[12]) * 0.5;     y[jin] = (y[11] + y[12]) * 0.5;          // pelvis
        x[jin + 1] = (x[5] + x[6]) * 0.5;   y[jin + 1] = (y[5] + y[6]) * 0.5;        // neck
    }
    return jin + (add_pn ? 2 : 0);
}

// get_bbox (lib/coord_utils.py:21-39): the tight box as centre +- half extent in fp64, cast to float32 (x, y, w, h)
struct Box { float x, y, w, h; };
__device__ __forceinline__ Box tight_box(const Col<double>& x, const Col<double>& y, int J) {
    double xmin = x[0], xmax = x[0], ymin = y[0], ymax = y[0];
    for (int j = 1; j < J; ++j) { xmin = fmin(xmin, x[j]); xmax = fmax(xmax, x[j]); ymin = fmin(ymin, y[j]); ymax = fmax(ymax, y[j]); }
    const double xc = (xmin + xmax) / 2., bw0 = xmax - xmin, yc = (ymin + ymax) / 2., bh0 = ymax - ymin;
    const double bxmin = xc - 0.5 * bw0, bxmax = xc + 0.5 * bw0, bymin = yc - 0.5 * bh0, bymax = yc + 0.5 * bh0;
    return Box{(float)bxmin, (float)bymin, (float)(bxmax - bxmin), (float)(bymax - bymin)};
}

// process_bbox's sanitising (lib/coord_utils.py:42-66; float32 arithmetic on the float32 box, as numpy does): false where it REJECTS
// a box narrower or lower than one pixel (it returns None and the datasets drop the sample); else the box's extent (w, h) and centre.
__device__ __forceinline__ bool box_extent(const Box& b, float& w, float& h, float& cx, float& cy) {
    const float x2 = b.x + (b.w - 1.f), y2 = b.y + (b.h - 1.f);
    if (!((b.w * b.h > 0.f) && x2 >= b.x && y2 >= b.y)) return false;
    w = x2 - b.x; h = y2 - b.y;
    cx = b.x + w / 2.f; cy = b.y + h / 2.f;
    return true;
}

// process_bbox's aspect step (lib/coord_utils.py:56-61) grows the shorter side of the float32 extent to the wanted ratio.  Its two
// uses differ in precision, each as it was pinned against the reference's own results, and this is the one place that says so:
//   aspect_fp64: the datasets' input chain (data/PW3D/dataset.py:236-250).  The ratio is cfg.MODEL.input_shape[1] / [0], a python
//                float (fp64) against the float32 extents: compared and scaled in fp64, the result rounded back to float32;
//   aspect_f32 : the demo's crop (demo/run.py:124-127).  numpy 2 keeps `float32 op python float` in float32 (NEP 50): the ratio is
//                rounded to float32 and the step is float32 arithmetic throughout.
// (By value: written through references, the two branches' stores are merged into one store to a selected address before the
// callee is inlined, and the caller's w and h end up in scratch.)
struct Extent { float w, h; };
__device__ __forceinline__ Extent aspect_fp64(float w, float h, int res_w, int res_h) {
    const double ar = (double)res_w / (double)res_h;
    if ((double)w > ar * (double)h) h = (float)((double)w / ar);
    else if ((double)w < ar * (double)h) w = (float)((double)h * ar);
    return Extent{w, h};
}
__device__ __forceinline__ Extent aspect_f32(float w, float h, float aspect) {
    if (w > aspect * h) h = w / aspect;
    else if (w < aspect * h) w = h * aspect;
    return Extent{w, h};
}

// get_affine_transform (lib/aug_utils.py:140-173) for a box of centre (cen0, cen1) and width w, rotated by the angle whose sine and
// cosine are sn, cs, onto dst_w x dst_h pixels: three float32 point pairs -- the centre, the centre + get_dir([0, -w/2], rot) formed
// in fp64, get_3rd_point of the two -- solved for the 2x3 matrix as cv2.getAffineTransform does ([sx sy 1] T^T = [dx dy]; Cramer, fp64).
// With sn = 0.0, cs = 1.0 the second source point is (cen0 + 0.0, cen1 + (double)(w * -0.5f)), the unrotated form, bit for bit.
__device__ __forceinline__ void crop_affine(float cen0, float cen1, float w, double sn, double cs, int dst_w, int dst_h, double (&T)[2][3]) {
    const double p1 = (double)(w * -0.5f);
    const double sd0 = 0.0 * cs - p1 * sn, sd1 = 0.0 * sn + p1 * cs;                      // get_dir([0, -w/2], rot)
    float src[3][2], dst[3][2];
    src[0][0] = cen0; src[0][1] = cen1;
    src[1][0] = (float)((double)cen0 + sd0); src[1][1] = (float)((double)cen1 + sd1);
    dst[0][0] = dst_w * 0.5f; dst[0][1] = dst_h * 0.5f;
    dst[1][0] = (float)((double)(dst_w * 0.5) + 0.0); dst[1][1] = (float)((double)(dst_h * 0.5) + (double)(dst_w * -0.5f));
    for (int q = 0; q < 2; ++q) {
        float (*m)[2] = q ? dst : src;
        const float d0 = m[0][0] - m[1][0], d1 = m[0][1] - m[1][1];
        m[2][0] = m[1][0] + (-d1); m[2][1] = m[1][1] + d0;                                 // get_3rd_point
    }
    const double a0 = src[0][0], b0 = src[0][1], a1 = src[1][0], b1 = src[1][1], a2 = src[2][0], b2 = src[2][1];
    const double det = a0 * (b1 - b2) - b0 * (a1 - a2) + (a1 * b2 - a2 * b1);
    for (int r = 0; r < 2; ++r) {
        const double d0 = dst[0][r], d1 = dst[1][r], d2 = dst[2][r];
        T[r][0] = (d0 * (b1 - b2) - b0 * (d1 - d2) + (d1 * b2 - d2 * b1)) / det;
        T[r][1] = (a0 * (d1 - d2) - d0 * (a1 - a2) + (a1 * d2 - a2 * d1)) / det;
        T[r][2] = (a0 * (b1 * d2 - b2 * d1) - b0 * (a1 * d2 - a2 * d1) + d0 * (a1 * b2 - a2 * b1)) / det;
    }
}

// out = (xy - mean) / std per axis over the sample's J joints, population std (np.std), sums in fp64 whatever the columns hold;
// a degenerate axis gives inf/nan exactly as numpy does
template <class T> __device__ __forceinline__ void standardise(const Col<T>& x, const Col<T>& y, int J, float* __restrict__ o) {
    double mx = 0.0, my = 0.0;
    for (int j = 0; j < J; ++j) { mx += x[j]; my += y[j]; }
    mx /= J; my /= J;
    double vx = 0.0, vy = 0.0;
    for (int j = 0; j < J; ++j) { vx += (x[j] - mx) * (x[j] - mx); vy += (y[j] - my) * (y[j] - my); }
    const double sx = sqrt(vx / J), sy = sqrt(vy / J);
    for (int j = 0; j < J; ++j) { o[j * 2] = (float)((x[j] - mx) / sx); o[j * 2 + 1] = (float)((y[j] - my) / sy); }
}

}  // namespace
}  // namespace gator
