// The demo's camera step (demo/run.py:21-39,123-164, lib/models/project_net.py:6-17) on the device.
//   gator_crop_joints_f32 : raw 2D joints -> the fit's target in crop pixels, the crop box and its validity (demo/run.py:124-127)
//   gator_fit_camera_f32  : the 1500 Adam steps of the weak-perspective camera (s, tx, ty) against that target, and the camera in
//                           image coordinates (convert_crop_cam_to_orig_img), in one launch
// Both are per-sample problems: one lane per sample, sums in joint order, so a sample's result does not depend on its batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "internal.h"
#include "joints2d.h"

namespace gator {
namespace {

// get_bbox (lib/coord_utils.py:21-39) -> process_bbox(bbox, aspect, scale) (:42-66) -> j2d_processing(joints, (crop_w, crop_h), bbox1,
// rot 0, no flip) (lib/aug_utils.py:51-64,140-179), from the pieces of joints2d.h.  numpy 2 keeps `float32 op python float` in float32
// (NEP 50), so the box is float32 arithmetic throughout with aspect and scale rounded to float32; the joints, the centre of the tight
// box and the affine solve are fp64 as in the reference (its joints are float64, cv2 solves in double); the joints are rounded to
// float32 at the end (kp.astype).
__global__ __launch_bounds__(64) void k_crop_joints(const float* __restrict__ in, int B, int jin, int comps, int add_pn, float aspect,
                                                    float scale, int crop_w, int crop_h, float* __restrict__ xy, float* __restrict__ box,
                                                    int32_t* __restrict__ valid) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    __shared__ double xs_[kMaxJ * 64], ys_[kMaxJ * 64];
    const Col<double> x{xs_, (int)threadIdx.x}, y{ys_, (int)threadIdx.x};
    const int J = load_joints(in + (size_t)b * jin * comps, jin, comps, add_pn, x, y);
    float* o = xy + (size_t)b * J * 2;
    float w0, h0, cx, cy;
    const bool ok = box_extent(tight_box(x, y, J), w0, h0, cx, cy);
    valid[b] = ok ? 1 : 0;
    if (!ok) {                                              // process_bbox returns None: the sample has no crop
        for (int j = 0; j < 2 * J; ++j) o[j] = 0.f;
        for (int k = 0; k < 4; ++k) box[b * 4 + k] = 0.f;
        return;
    }
    const Extent e = aspect_f32(w0, h0, aspect);
    const float sw = e.w * scale, sh = e.h * scale;
    const float fx = cx - sw / 2.f, fy = cy - sh / 2.f;
    box[b * 4] = fx; box[b * 4 + 1] = fy; box[b * 4 + 2] = sw; box[b * 4 + 3] = sh;
    // get_center_scale, then the affine without a rotation
    double T[2][3];
    crop_affine(fx + sw * 0.5f, fy + sh * 0.5f, sw, 0.0, 1.0, crop_w, crop_h, T);
    for (int j = 0; j < J; ++j) {
        o[j * 2] = (float)(T[0][0] * x[j] + T[0][1] * y[j] + T[0][2]);
        o[j * 2 + 1] = (float)(T[1][0] * x[j] + T[1][1] * y[j] + T[1][2]);
    }
}

// torch.sign, except that NaN stays NaN (torch gives 0): a non-finite sample's camera becomes NaN instead of a fit of its other joints
__device__ __forceinline__ float sign_nan(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : (d == 0.f ? 0.f : d)); }

// one torch.optim.Adam step (single-tensor path, torch defaults) of one parameter; f = (step_size, sqrt(1 - beta2^t)) of this step
__device__ __forceinline__ void adam(float& p, float& m, float& v, float g, float2 f) {
    m = m + (g - m) * 0.1f;                       // exp_avg.lerp_(grad, 1 - beta1)
    v = v * 0.999f + 0.001f * (g * g);            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / f.y + 1e-8f;   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p + (-f.x * m) / denom;                   // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// the sample's n_fit x (px, py, target x, target y): registers when n_fit is the template argument, LDS columns otherwise
template <int NF> struct Joints {
    float v[4][NF];
    __device__ __forceinline__ float& at(int c, int k) { return v[c][k]; }
};
template <> struct Joints<0> {
    float* base; int tid;
    __device__ __forceinline__ float& at(int c, int k) { return base[(k * 4 + c) * 64 + tid]; }
};
template <int NF, class F> __device__ __forceinline__ void for_joints(int n, F&& f) {
    if constexpr (NF > 0) {
#pragma unroll
        for (int k = 0; k < NF; ++k) f(k);
    } else {
        for (int k = 0; k < n; ++k) f(k);
    }
}

// The fit of demo/run.py:150-157 for one sample per lane: per step the layer o = (p + t) * s * r + r (separate fp32 roundings), the
// L1 loss's gradient sign(o - target) / (2 n) back through it (sums in joint order), one Adam step per parameter.  tab[j] holds step
// j's two Adam factors, formed on the host in double as torch does.  Then the final mean L1 loss and, with box != NULL,
// convert_crop_cam_to_orig_img (demo/run.py:21-39) for an image of img_w x img_h pixels.
template <int NF>
__global__ __launch_bounds__(64) void k_fit_camera(const float* __restrict__ j3, int nj3, const float* __restrict__ tgt, int ntg, int n_fit,
                                                   const float* __restrict__ init, float r, int steps, const float2* __restrict__ tab,
                                                   const float* __restrict__ box, float img_w, float img_h, int B, float* __restrict__ cam,
                                                   float* __restrict__ loss, float* __restrict__ orig_cam) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int n = NF ? NF : n_fit;
    Joints<NF> q;
    if constexpr (NF == 0) {
        __shared__ float lds[kMaxJ * 4 * 64];
        q.base = lds;
        q.tid = threadIdx.x;
    }
    const float* pj = j3 + (size_t)b * nj3 * 3;
    const float* pt = tgt + (size_t)b * ntg * 2;
    for_joints<NF>(n, [&](int k) { q.at(0, k) = pj[k * 3]; q.at(1, k) = pj[k * 3 + 1]; q.at(2, k) = pt[k * 2]; q.at(3, k) = pt[k * 2 + 1]; });
    float s = init[b * 3], tx = init[b * 3 + 1], ty = init[b * 3 + 2];
    float ms = 0.f, mx = 0.f, my = 0.f, vs = 0.f, vx = 0.f, vy = 0.f;
    const float inv_n = 1.f / (float)(2 * n);         // the mean's backward: 1 / numel in fp32
    for (int j = 0; j < steps; ++j) {
        float gs = 0.f, gx = 0.f, gy = 0.f;
        for_joints<NF>(n, [&](int k) {
            const float ox = q.at(0, k) + tx, oy = q.at(1, k) + ty;
            const float dx = ox * s * r + r - q.at(2, k), dy = oy * s * r + r - q.at(3, k);
            const float grx = sign_nan(dx) * inv_n * r, gry = sign_nan(dy) * inv_n * r;
            gs = gs + grx * ox;
            gs = gs + gry * oy;
            gx = gx + grx * s;
            gy = gy + gry * s;
        });
        const float2 f = tab[j];
        adam(s, ms, vs, gs, f);
        adam(tx, mx, vx, gx, f);
        adam(ty, my, vy, gy, f);
    }
    cam[b * 3] = s; cam[b * 3 + 1] = tx; cam[b * 3 + 2] = ty;
    if (loss) {
        float acc = 0.f;
        for_joints<NF>(n, [&](int k) {
            acc = acc + fabsf((q.at(0, k) + tx) * s * r + r - q.at(2, k));
            acc = acc + fabsf((q.at(1, k) + ty) * s * r + r - q.at(3, k));
        });
        loss[b] = acc / (float)(2 * n);
    }
    if (box) {                                        // float32 throughout, as numpy does with the float32 camera and box
        const float bx = box[b * 4], by = box[b * 4 + 1], bw = box[b * 4 + 2], bh = box[b * 4 + 3];
        const float cx = bx + bw / 2.f, cy = by + bh / 2.f;
        const float hw = img_w / 2.f, hh = img_h / 2.f;
        const float sx = s * (1.f / (img_w / bh)), sy = s * (1.f / (img_h / bh));
        orig_cam[b * 4] = sx;
        orig_cam[b * 4 + 1] = sy;
        orig_cam[b * 4 + 2] = ((cx - hw) / hw / sx) + tx;
        orig_cam[b * 4 + 3] = ((cy - hh) / hh / sy) + ty;
    }
}

// Adam factor tables, one per (device, steps, schedule), uploaded once and kept for the life of the process: a schedule is a handful
// of numbers and callers reuse one (the demo's), so the fit itself enqueues nothing but its kernel.  Past kMaxTables distinct tables
// the device is synchronised and the cache emptied.
struct Table {
    int dev, steps;
    std::vector<double> key;
    float2* d;
};
constexpr size_t kMaxTables = 32;
std::mutex g_tab_mu;
std::vector<Table> g_tabs;

int adam_table(int steps, const int32_t* milestones, const double* lrs, int n_sched, const float2** out) {
    int dev = 0;
    GATOR_HIP_CHECK(hipGetDevice(&dev));
    std::vector<double> key;
    for (int i = 0; i < n_sched; ++i) { key.push_back((double)milestones[i]); key.push_back(lrs[i]); }
    std::lock_guard<std::mutex> lock(g_tab_mu);
    for (const Table& t : g_tabs)
        if (t.dev == dev && t.steps == steps && t.key == key) { *out = t.d; return GATOR_OK; }
    if (g_tabs.size() >= kMaxTables) {
        GATOR_HIP_CHECK(hipDeviceSynchronize());
        for (const Table& t : g_tabs) {
            int cur = 0;
            GATOR_HIP_CHECK(hipGetDevice(&cur));
            GATOR_HIP_CHECK(hipSetDevice(t.dev));
            GATOR_HIP_CHECK(hipFree(t.d));
            GATOR_HIP_CHECK(hipSetDevice(cur));
        }
        g_tabs.clear();
    }
    // torch (optim/adam.py, single-tensor path): step_size = lr / (1 - beta1 ** t), bias_correction2 ** 0.5, Python doubles;
    // the rate of 0-based step j is the last schedule entry whose milestone m satisfies j >= m + 1 (the first entry's from j = 0)
    std::vector<float2> h(steps);
    for (int j = 0; j < steps; ++j) {
        double lr = lrs[0];
        for (int i = 1; i < n_sched; ++i)
            if (j >= milestones[i] + 1) lr = lrs[i];
        const double t = (double)(j + 1);
        h[j].x = (float)(lr / (1.0 - std::pow(0.9, t)));
        h[j].y = (float)std::pow(1.0 - std::pow(0.999, t), 0.5);
    }
    float2* d = nullptr;
    GATOR_HIP_CHECK(hipMalloc(&d, sizeof(float2) * steps));
    const hipError_t e = hipMemcpy(d, h.data(), sizeof(float2) * steps, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(GATOR_EHIP, "hipMemcpy of the Adam table failed: %s", hipGetErrorString(e));
    }
    g_tabs.push_back(Table{dev, steps, key, d});
    *out = d;
    return GATOR_OK;
}
}  // namespace
}  // namespace gator

extern "C" int gator_crop_joints_f32(const float* joints, int32_t batch, int32_t num_joint_in, int32_t comps, int32_t add_pelvis_neck,
                                     float box_aspect, float box_scale, int32_t crop_w, int32_t crop_h, float* joints_crop, float* bbox,
                                     int32_t* valid, void* stream) {
    using namespace gator;
    if (!joints || !joints_crop || !bbox || !valid || batch <= 0 || num_joint_in <= 0 || comps < 2 || crop_w <= 0 || crop_h <= 0)
        return fail(GATOR_EINVAL, "gator_crop_joints_f32: bad arguments");
    if (!(box_aspect > 0.f) || !(box_scale > 0.f) || !std::isfinite(box_aspect) || !std::isfinite(box_scale))
        return fail(GATOR_EINVAL, "gator_crop_joints_f32: box_aspect and box_scale must be finite and positive");
    if (num_joint_in + (add_pelvis_neck ? 2 : 0) > kMaxJ) return fail(GATOR_EINVAL, "gator_crop_joints_f32: at most %d joints", kMaxJ);
    if (add_pelvis_neck && num_joint_in < 13) return fail(GATOR_EINVAL, "gator_crop_joints_f32: pelvis/neck need the COCO joint order (>= 13 joints)");
    k_crop_joints<<<(batch + 63) / 64, 64, 0, (hipStream_t)stream>>>(joints, batch, num_joint_in, comps, add_pelvis_neck ? 1 : 0, box_aspect,
                                                                   box_scale, crop_w, crop_h, joints_crop, bbox, valid);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

extern "C" int gator_fit_camera_f32(const float* joints3d, int32_t batch, int32_t n_joint_in, const float* target, int32_t n_target_in,
                                    int32_t n_fit, const float* init, int32_t crop_size, int32_t steps, const int32_t* milestones,
                                    const double* lrs, int32_t n_schedule, const float* bbox, float img_w, float img_h, float* cam,
                                    float* loss, float* orig_cam, void* stream) {
    using namespace gator;
    if (!joints3d || !target || !init || !cam || batch <= 0 || crop_size <= 0)
        return fail(GATOR_EINVAL, "gator_fit_camera_f32: bad arguments");
    if (n_fit < 1 || n_fit > kMaxJ || n_fit > n_joint_in || n_fit > n_target_in)
        return fail(GATOR_EINVAL, "gator_fit_camera_f32: n_fit must be 1..%d and at most the joints of both inputs", kMaxJ);
    if (steps < 0 || steps > (1 << 20)) return fail(GATOR_EINVAL, "gator_fit_camera_f32: steps must be 0..%d", 1 << 20);
    if (!milestones || !lrs || n_schedule < 1 || n_schedule > 8)
        return fail(GATOR_EINVAL, "gator_fit_camera_f32: the schedule needs 1..8 (milestone, lr) pairs");
    for (int i = 0; i < n_schedule; ++i) {
        if (!std::isfinite(lrs[i]) || lrs[i] < 0.0) return fail(GATOR_EINVAL, "gator_fit_camera_f32: learning rates must be finite and >= 0");
        if (i > 1 && milestones[i] <= milestones[i - 1]) return fail(GATOR_EINVAL, "gator_fit_camera_f32: milestones must increase");
        if (i > 0 && milestones[i] < 0) return fail(GATOR_EINVAL, "gator_fit_camera_f32: milestones must be >= 0");
    }
    if ((orig_cam != nullptr) != (bbox != nullptr)) return fail(GATOR_EINVAL, "gator_fit_camera_f32: orig_cam and bbox go together");
    if (orig_cam && (!(img_w > 0.f) || !(img_h > 0.f) || !std::isfinite(img_w) || !std::isfinite(img_h)))
        return fail(GATOR_EINVAL, "gator_fit_camera_f32: img_w and img_h must be finite and positive");
    const float2* tab = nullptr;
    if (steps > 0)
        if (int rc = adam_table(steps, milestones, lrs, n_schedule, &tab)) return rc;
    const float r = (float)(crop_size / 2.0);       // lib/models/project_net.py:11, a Python float rounded to the tensor's fp32
    const dim3 grid((batch + 63) / 64);
    hipStream_t st = (hipStream_t)stream;
    if (n_fit == 17)
        k_fit_camera<17><<<grid, 64, 0, st>>>(joints3d, n_joint_in, target, n_target_in, n_fit, init, r, steps, tab, bbox, img_w, img_h, batch, cam, loss, orig_cam);
    else
        k_fit_camera<0><<<grid, 64, 0, st>>>(joints3d, n_joint_in, target, n_target_in, n_fit, init, r, steps, tab, bbox, img_w, img_h, batch, cam, loss, orig_cam);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
