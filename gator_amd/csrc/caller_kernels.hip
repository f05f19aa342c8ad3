// "Next" rows of the scope table: the caller-side pieces either side of GATOR.forward, on the device.
//   gator_preprocess_pose2d_f32 : raw 2D joints -> model input (demo/run.py:103-121,127-134; data/PW3D/dataset.py:168-183,241-250)
//   gator_rigid_align_f32       : per-sample similarity (Procrustes) alignment (lib/coord_utils.py:127-149), the PA-MPJPE kernel
// Both are tiny per-sample problems (<= 19 joints, one 3x3 SVD): one thread per sample, fp64 arithmetic, fp32 in / out.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "joints2d.h"
#include "procrustes.h"

namespace gator {
namespace {

// With rot = 0 and flip = 0 (every evaluation path) the reference's bbox -> affine -> /[W,H] chain is a per-axis positive scale +
// shift, which cancels in the per-axis standardisation that follows it (checked on the demo input to 5e-8):
// out = (xy - mean) / std over the joints of the sample, population std (np.std).  COCO inputs first get pelvis = (L_Hip+R_Hip)/2
// and neck = (L_Shoulder+R_Shoulder)/2 appended (joints 11,12 and 5,6).
__global__ __launch_bounds__(64) void k_preprocess(const float* __restrict__ in, int B, int jin, int comps, int add_pn, float* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    __shared__ double xs_[kMaxJ * 64], ys_[kMaxJ * 64];
    const Col<double> x{xs_, (int)threadIdx.x}, y{ys_, (int)threadIdx.x};
    const int jout = load_joints(in + (size_t)b * jin * comps, jin, comps, add_pn, x, y);
    standardise(x, y, jout, out + (size_t)b * jout * 2);
}

// svd3 / rigid_fit (the 3x3 Jacobi SVD, the reflection fix, the LDS point sets, kMaxPts / kPtsLds): csrc/procrustes.h
__global__ void k_rigid_align(const float* __restrict__ A, const float* __restrict__ Bt, int nb, int n, float* __restrict__ out) {
    extern __shared__ double pts_lds[];                  // [2][kMaxPts][3][blockDim.x]
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const float* a = A + (size_t)b * n * 3;
    const float* t = Bt + (size_t)b * n * 3;
    const Pts pa{pts_lds, (int)threadIdx.x, (int)blockDim.x}, pt{pts_lds + (size_t)kMaxPts * 3 * blockDim.x, (int)threadIdx.x, (int)blockDim.x};
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) { pa(i, k) = a[i * 3 + k]; pt(i, k) = t[i * 3 + k]; }
    double c, R[3][3], tr[3];
    rigid_fit(pa, pt, n, c, R, tr);
    float* o = out + (size_t)b * n * 3;
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int r = 0; r < 3; ++r)
            o[i * 3 + r] = (float)(c * (R[r][0] * pa(i, 0) + R[r][1] * pa(i, 1) + R[r][2] * pa(i, 2)) + tr[r]);
}

// Per-sample evaluation errors in one launch (data/PW3D/dataset.py:273-286, 337-375): err[b][0] = mean distance of the root-aligned
// evaluation joints (MPJPE), err[b][1] = the same after the similarity alignment of the evaluation joints (PA-MPJPE).
__global__ void k_joint_errors(const float* __restrict__ P, const float* __restrict__ T, int nb, int nj, const int32_t* __restrict__ idx, int ne,
                               int root, float scale, float* __restrict__ err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    extern __shared__ double pts_lds[];                  // [2][kMaxPts][3][blockDim.x]
    const float* p = P + (size_t)b * nj * 3;
    const float* t = T + (size_t)b * nj * 3;
    const Pts pa{pts_lds, (int)threadIdx.x, (int)blockDim.x}, pt{pts_lds + (size_t)kMaxPts * 3 * blockDim.x, (int)threadIdx.x, (int)blockDim.x};
    double e0 = 0.0;
    for (int i = 0; i < ne; ++i) {
        const int j = idx ? idx[i] : i;
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            // float32 arithmetic where the reference has it: mesh * 1000, pred - pred[root], target - target[root], their difference
            const float pj = p[j * 3 + k] * scale, pr = p[root * 3 + k] * scale;
            const float dp = pj - pr, dt = t[j * 3 + k] - t[root * 3 + k];
            pa(i, k) = dp; pt(i, k) = dt;
            const float d = dp - dt;
            d2 += (double)d * (double)d;
        }
        e0 += sqrt(d2);
    }
    double c, R[3][3], tr[3];
    rigid_fit(pa, pt, ne, c, R, tr);
    const double e1 = aligned_error<true>(pa, pt, ne, c, R, tr);
    err[b * 2] = (float)(e0 / ne);
    err[b * 2 + 1] = (float)(e1 / ne);
}

}  // namespace
}  // namespace gator

using namespace gator;

namespace gator {
namespace {
// The GENERAL input chain (data/PW3D/dataset.py:236-250): tight bbox (lib/coord_utils.py:21-39) -> process_bbox (:42-66, which
// REJECTS a box narrower or lower than one pixel: valid = 0, the datasets drop such samples) -> get_affine_transform with rotation
// (lib/aug_utils.py:140-173: three float32 point pairs, solved as cv2.getAffineTransform does) -> affine per joint, optional
// flip_2d_joint (:31-38) -> float32 -> /[W,H] -> per-axis standardisation.  One thread per sample; float32 roundings where the
// reference has them (bbox, centre/scale, the point pairs, the transformed joints, the division), fp64 in between.
__global__ __launch_bounds__(64) void k_preprocess_chain(const float* __restrict__ in, int B, int jin, int comps, int add_pn,
                                                         const float* __restrict__ rot_deg, const int32_t* __restrict__ flip,
                                                         const int32_t* __restrict__ pairs, int n_pairs, int res_w, int res_h,
                                                         float* __restrict__ out, int32_t* __restrict__ valid) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    __shared__ double xs_[kMaxJ * 64], ys_[kMaxJ * 64];    // one column per thread (48 KB with the float32 images below: 64-thread blocks)
    __shared__ float fxs_[kMaxJ * 64], fys_[kMaxJ * 64];
    const Col<double> x{xs_, (int)threadIdx.x}, y{ys_, (int)threadIdx.x};
    const Col<float> fxn{fxs_, (int)threadIdx.x}, fyn{fys_, (int)threadIdx.x};
    const int J = load_joints(in + (size_t)b * jin * comps, jin, comps, add_pn, x, y);
    float* o = out + (size_t)b * J * 2;
    float w0, h0, cx, cy;
    const bool ok = box_extent(tight_box(x, y, J), w0, h0, cx, cy);
    if (valid) valid[b] = ok ? 1 : 0;
    if (!ok) {
        for (int j = 0; j < 2 * J; ++j) o[j] = 0.f;
        return;
    }
    const Extent e = aspect_fp64(w0, h0, res_w, res_h);
    const float w = e.w, h = e.h;
    const float fx = cx - w / 2.f, fy = cy - h / 2.f;
    // get_center_scale, then the affine with the sample's rotation
    const double rr = M_PI * (rot_deg ? (double)rot_deg[b] : 0.0) / 180.0, sn = sin(rr), cs = cos(rr);
    double T[2][3];
    crop_affine(fx + w * 0.5f, fy + h * 0.5f, w, sn, cs, res_w, res_h, T);
    for (int j = 0; j < J; ++j) {
        const double nx = T[0][0] * x[j] + T[0][1] * y[j] + T[0][2], ny = T[1][0] * x[j] + T[1][1] * y[j] + T[1][2];
        x[j] = nx; y[j] = ny;
    }
    if (flip && flip[b]) {
        for (int j = 0; j < J; ++j) x[j] = res_w - x[j] - 1;
        for (int q = 0; q < n_pairs; ++q) {
            const int u = pairs[2 * q], v = pairs[2 * q + 1];
            if (u < J && v < J) { const double tx = x[u], ty = y[u]; x[u] = x[v]; y[u] = y[v]; x[v] = tx; y[v] = ty; }
        }
    }
    for (int j = 0; j < J; ++j) { fxn[j] = (float)x[j] / (float)res_w; fyn[j] = (float)y[j] / (float)res_h; }   // astype(float32); /= [W,H]
    standardise(fxn, fyn, J, o);
}
}  // namespace
}  // namespace gator

extern "C" int gator_preprocess_chain_f32(const float* joints, int32_t batch, int32_t num_joint_in, int32_t comps, int32_t add_pelvis_neck,
                                          const float* rot_deg, const int32_t* flip, const int32_t* flip_pairs, int32_t n_pairs,
                                          int32_t res_w, int32_t res_h, float* pose2d, int32_t* valid, void* stream) {
    using namespace gator;
    if (!joints || !pose2d || batch <= 0 || num_joint_in <= 0 || comps < 2 || res_w <= 0 || res_h <= 0 || n_pairs < 0 || (n_pairs > 0 && !flip_pairs))
        return fail(GATOR_EINVAL, "gator_preprocess_chain_f32: bad arguments");
    if (num_joint_in + (add_pelvis_neck ? 2 : 0) > 32) return fail(GATOR_EINVAL, "gator_preprocess_chain_f32: at most 32 joints");
    if (add_pelvis_neck && num_joint_in < 13) return fail(GATOR_EINVAL, "gator_preprocess_chain_f32: pelvis/neck need the COCO joint order (>= 13 joints)");
    k_preprocess_chain<<<(batch + 63) / 64, 64, 0, (hipStream_t)stream>>>(joints, batch, num_joint_in, comps, add_pelvis_neck ? 1 : 0, rot_deg, flip,
                                                                       flip_pairs, n_pairs, res_w, res_h, pose2d, valid);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

extern "C" int gator_preprocess_pose2d_f32(const float* joints, int32_t batch, int32_t num_joint_in, int32_t comps,
                                           int32_t add_pelvis_neck, float* pose2d, void* stream) {
    if (!joints || !pose2d || batch <= 0 || num_joint_in <= 0 || num_joint_in + (add_pelvis_neck ? 2 : 0) > 32 || comps < 2)
        return fail(GATOR_EINVAL, "gator_preprocess_pose2d_f32: bad arguments");
    if (add_pelvis_neck && num_joint_in < 13) return fail(GATOR_EINVAL, "gator_preprocess_pose2d_f32: pelvis/neck need the COCO joint order (>= 13 joints)");
    k_preprocess<<<(batch + 63) / 64, 64, 0, (hipStream_t)stream>>>(joints, batch, num_joint_in, comps, add_pelvis_neck, pose2d);      // 64-thread blocks: the kernel's LDS images have 64 columns
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

extern "C" int gator_joint_errors_f32(const float* pred_joints, const float* target_joints, int32_t batch, int32_t n_joint,
                                      const int32_t* eval_joints, int32_t n_eval, int32_t root, float pred_scale, float* errors, void* stream) {
    using namespace gator;
    if (!pred_joints || !target_joints || !errors || batch <= 0 || n_joint <= 0 || root < 0 || root >= n_joint)
        return fail(GATOR_EINVAL, "gator_joint_errors_f32: bad arguments");
    const int ne = eval_joints ? n_eval : n_joint;
    if (ne < 3 || ne > 32) return fail(GATOR_EINVAL, "gator_joint_errors_f32: 3..32 evaluation joints");
    static bool lds_raised_[64] = {};
    if (int rc = raise_pts_lds((const void*)k_joint_errors, lds_raised_)) return rc;
    k_joint_errors<<<(batch + 63) / 64, 64, kPtsLds, (hipStream_t)stream>>>(pred_joints, target_joints, batch, n_joint, eval_joints, ne, root, pred_scale, errors);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

extern "C" int gator_rigid_align_f32(const float* a, const float* b, int32_t batch, int32_t n_points, float* aligned, void* stream) {
    if (!a || !b || !aligned || batch <= 0 || n_points < 3 || n_points > 32) return fail(GATOR_EINVAL, "gator_rigid_align_f32: bad arguments (3..32 points)");
    static bool lds_raised_[64] = {};
    if (int rc = raise_pts_lds((const void*)gator::k_rigid_align, lds_raised_)) return rc;
    k_rigid_align<<<(batch + 63) / 64, 64, kPtsLds, (hipStream_t)stream>>>(a, b, batch, n_points, aligned);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

// ---- measurement helper: the device-side traffic of this rank's share of an all-gather (include/gator_hip.h) ------------------------------
namespace gator {
typedef float tr_f4 __attribute__((ext_vector_type(4)));
// persistent-style: every workgroup walks the source in 4 KiB steps, strided by the grid, once per copy; 16 B per lane, non-temporal stores
// (the data is not read again on this device, like a receive buffer)
__global__ __launch_bounds__(256) void k_gather_traffic(const tr_f4* __restrict__ src, tr_f4* __restrict__ dst, long long n16, int copies) {
    for (int c = 0; c < copies; ++c) {
        tr_f4* d = dst + (size_t)c * n16;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256)
            __builtin_nontemporal_store(src[i], d + i);
    }
}
}  // namespace gator

extern "C" int gator_emulate_gather_traffic(const void* src, void* dst, int64_t bytes, int32_t copies, int32_t n_workgroups, void* stream) {
    using namespace gator;
    if (!src || !dst || bytes < 16 || (bytes & 15) || copies <= 0 || n_workgroups <= 0) return fail(GATOR_EINVAL, "gator_emulate_gather_traffic: bad arguments (bytes: a positive multiple of 16)");
    k_gather_traffic<<<n_workgroups, 256, 0, (hipStream_t)stream>>>((const tr_f4*)src, (tr_f4*)dst, (long long)(bytes / 16), copies);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
