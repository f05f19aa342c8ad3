// Whole-mesh evaluation on the device (data/PW3D/dataset.py:322-375, data/Human36M/dataset.py:515-600, compute_both_err :273-286):
//   gator_mesh_errors_f32 : per sample (MPJPE, PA-MPJPE, SMPL-joint MPJPE, MPVPE, PA-MPVPE) in ONE launch, from the two meshes.
// One 256-thread workgroup per sample.  The meshes are read from global memory (two fp32 meshes of 6890 vertices are 165 kB, more
// than the LDS) in THREE passes, each thread striding the vertices with fp64 partial sums:
//   1. the centroids, and the regressed joints (each joint summed by its own four lanes scanning the COO list);
//   2. the centred covariance and variance, and the MPVPE sum; then the joint columns and the two similarity fits;
//   3. the PA-MPVPE sum under the mesh's fit.
// Passes 1 and 2 are NOT folded into one pass over raw moments: the covariance is summed about the centroid, so a mesh 100 m from
// the origin loses nothing to cancellation.  Sums are reduced in a fixed order (xor butterfly inside a wave, then the four waves'
// values from LDS, first to last) and nothing is atomic: a sample's row is the same bits whatever the batch and its neighbours.
// Each scale is one float32 product per coordinate (lib/core/base.py:219 multiplies the float32 meshes); all after that is fp64.
#include <hip/hip_runtime.h>

#include "internal.h"
#include "procrustes.h"

namespace gator {
namespace {

constexpr int kMeshThreads = 256, kMeshWaves = kMeshThreads / 64;
constexpr int kMaxRegJoints = 64, kLanesPerJoint = kMeshThreads / kMaxRegJoints;      // the joint fit takes kMaxPts points (procrustes.h)

// v[k] := the sum of v[k] over the workgroup, in every thread, the same bits in each (wave_sum, then the four waves' values in a
// fixed order).  red: [kMeshWaves][K] doubles of LDS.
template <int K> __device__ void block_sum(double (&v)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();                                     // the readers of the previous sum are done with red
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
}

// joints[0 / 1][j][k] = sum over the entries of row j of val * (scaled pred / target vertex col), fp64.  Joint j belongs to lanes
// 4j .. 4j+3 of the workgroup; lane q takes entries q, q+4, ... in list order, the four partial sums are added in a fixed order.
// Entries may come in any order, duplicates add, a row outside [0, n_joint) matches no joint, a joint without entries is 0.
__device__ void regress(const gator_coo& g, const float* __restrict__ p, const float* __restrict__ t, float ps, float ts,
                        double (*joints)[kMaxRegJoints][3]) {
    const int j = threadIdx.x / kLanesPerJoint, q = threadIdx.x % kLanesPerJoint;
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int e = q; e < g.nnz; e += kLanesPerJoint)
        if (g.row[e] == j) {
            const double w = g.val[e];
            const size_t o = (size_t)g.col[e] * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[k] += w * (double)(p[o + k] * ps); a[3 + k] += w * (double)(t[o + k] * ts); }
        }
#pragma unroll
    for (int k = 0; k < 6; ++k) { a[k] += __shfl_xor(a[k], 1); a[k] += __shfl_xor(a[k], 2); }
    if (q == 0 && j < g.n_joint)
#pragma unroll
        for (int k = 0; k < 3; ++k) { joints[0][j][k] = a[k]; joints[1][j][k] = a[3 + k]; }
}

__device__ __forceinline__ float finite_or_nan(double x) { return isfinite(x) ? (float)x : __builtin_nanf(""); }

// err [B,5]; ev.nnz < 0 marks "no evaluation regressor" (columns 0 and 1 are NaN).  idx: n_eval joint indices or null for 0 .. n_eval-1.
__global__ __launch_bounds__(kMeshThreads) void k_mesh_errors(const float* __restrict__ P, const float* __restrict__ T, int n, float ps, float ts,
                                                              gator_coo rg, int root, gator_coo ev, int eroot,
                                                              const int32_t* __restrict__ idx, int ne, float* __restrict__ err) {
    __shared__ double red[kMeshWaves * 11];
    __shared__ double jr[2][kMaxRegJoints][3], je[2][kMaxRegJoints][3];      // regressed joints: [pred / target][joint][axis]
    __shared__ double pts[2 * kMaxPts * 3];                                   // the root-aligned evaluation joints of the joint fit
    __shared__ double fit[13];                                                // c, R, tr of the mesh
    const int tid = threadIdx.x;
    const float* p = P + (size_t)blockIdx.x * n * 3;
    const float* t = T + (size_t)blockIdx.x * n * 3;
    float* o = err + (size_t)blockIdx.x * 5;
    const bool has_eval = ev.nnz >= 0;

    // pass 1
    regress(rg, p, t, ps, ts, jr);
    if (has_eval) regress(ev, p, t, ps, ts, je);
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += kMeshThreads)
#pragma unroll
        for (int k = 0; k < 3; ++k) { s[k] += (double)(p[(size_t)i * 3 + k] * ps); s[3 + k] += (double)(t[(size_t)i * 3 + k] * ts); }
    block_sum(s, red);                                   // its barriers also publish jr / je
    double ca[3], cb[3], rp[3], rt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ca[k] = s[k] / n; cb[k] = s[3 + k] / n; rp[k] = jr[0][root][k]; rt[k] = jr[1][root][k]; }

    // pass 2: m[0..8] = the covariance, m[9] = the variance of the prediction, m[10] = the MPVPE sum
    double m[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += kMeshThreads) {
        double x[3], y[3], d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = (double)(p[(size_t)i * 3 + k] * ps); y[k] = (double)(t[(size_t)i * 3 + k] * ts);
            const double d = (x[k] - rp[k]) - (y[k] - rt[k]);
            d2 += d * d;
            x[k] -= ca[k]; y[k] -= cb[k];
            m[9] += x[k] * x[k];
        }
        m[10] += sqrt(d2);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) m[r * 3 + cc] += x[r] * y[cc];
    }
    block_sum(m, red);

    double c, R[3][3], tr[3];
    if (tid >> 6 == kMeshWaves - 1) {
        // the last wave: the joint columns, while the other waves fit the mesh
        double e2 = 0.0;
        if (tid - 64 * (kMeshWaves - 1) < rg.n_joint) {
            const int j = tid - 64 * (kMeshWaves - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double d = (jr[0][j][k] - rp[k]) - (jr[1][j][k] - rt[k]); e2 += d * d; }
            e2 = sqrt(e2);
        }
        e2 = wave_sum(e2);
        if ((tid & 63) == 0) {
            o[2] = finite_or_nan(e2 / rg.n_joint);
            if (!has_eval) { o[0] = o[1] = __builtin_nanf(""); }
            else {
                const Pts pa{pts, 0, 1}, pt{pts + kMaxPts * 3, 0, 1};
                double e0 = 0.0;
                for (int i = 0; i < ne; ++i) {
                    const int j = idx ? idx[i] : i;
                    double d2 = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        pa(i, k) = je[0][j][k] - je[0][eroot][k]; pt(i, k) = je[1][j][k] - je[1][eroot][k];
                        d2 += (pa(i, k) - pt(i, k)) * (pa(i, k) - pt(i, k));
                    }
                    e0 += sqrt(d2);
                }
                rigid_fit(pa, pt, ne, c, R, tr);
                o[0] = finite_or_nan(e0 / ne);
                o[1] = finite_or_nan(aligned_error<false>(pa, pt, ne, c, R, tr) / ne);
            }
        }
    } else {
        double H[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) H[r][cc] = m[r * 3 + cc] / n;
        similarity_from_moments(H, m[9] / n, ca, cb, c, R, tr);      // the same in every lane
        if (tid == 0) {
            fit[0] = c;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                fit[10 + r] = tr[r];
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) fit[1 + r * 3 + cc] = R[r][cc];
            }
        }
    }
    __syncthreads();
    c = fit[0];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        tr[r] = fit[10 + r];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) R[r][cc] = fit[1 + r * 3 + cc];
    }

    // pass 3
    double pa_sum[1] = {0.0};
    for (int i = tid; i < n; i += kMeshThreads) {
        double x[3], d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = (double)(p[(size_t)i * 3 + k] * ps);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double d = (c * (R[r][0] * x[0] + R[r][1] * x[1] + R[r][2] * x[2]) + tr[r]) - (double)(t[(size_t)i * 3 + r] * ts);
            d2 += d * d;
        }
        pa_sum[0] += sqrt(d2);
    }
    block_sum(pa_sum, red);
    if (tid == 0) {
        o[3] = finite_or_nan(m[10] / n);
        o[4] = finite_or_nan(pa_sum[0] / n);
    }
}

bool reg_ok(const gator_coo& g, int root) { return coo_ok(g) && g.n_joint <= kMaxRegJoints && root >= 0 && root < g.n_joint; }

}  // namespace
}  // namespace gator

extern "C" int gator_mesh_errors_f32(const float* pred, const float* target, int32_t batch, int32_t n_verts, float pred_scale,
                                     float target_scale, const gator_coo* root_regressor, int32_t root, const gator_coo* eval_regressor,
                                     int32_t eval_root, const int32_t* eval_joints, int32_t n_eval, float* errors, void* stream) {
    using namespace gator;
    if (!pred || !target || !errors || !root_regressor) return fail(GATOR_EINVAL, "gator_mesh_errors_f32: null mesh, output or root regressor");
    if (batch <= 0 || n_verts < 3) return fail(GATOR_EINVAL, "gator_mesh_errors_f32: batch %d, n_verts %d (batch >= 1, n_verts >= 3)", batch, n_verts);
    if (!reg_ok(*root_regressor, root))
        return fail(GATOR_EINVAL, "gator_mesh_errors_f32: root regressor (nnz >= 0 with its arrays, 1..64 joints, root inside them)");
    gator_coo ev = {nullptr, nullptr, nullptr, -1, 0};          // nnz < 0: the kernel's mark for "absent"
    const bool has_eval = eval_regressor && !(eval_regressor->nnz == 0 && !eval_regressor->row && !eval_regressor->col && !eval_regressor->val);
    int ne = 0;
    if (has_eval) {
        ev = *eval_regressor;
        if (!reg_ok(ev, eval_root))
            return fail(GATOR_EINVAL, "gator_mesh_errors_f32: evaluation regressor (nnz >= 0 with its arrays, 1..64 joints, root inside them)");
        ne = eval_joints ? n_eval : ev.n_joint;
        if (ne < 3 || ne > kMaxPts) return fail(GATOR_EINVAL, "gator_mesh_errors_f32: 3..32 evaluation joints");
    }
    k_mesh_errors<<<batch, kMeshThreads, 0, (hipStream_t)stream>>>(pred, target, n_verts, pred_scale, target_scale, *root_regressor, root, ev,
                                                                   eval_root, has_eval ? eval_joints : nullptr, ne, errors);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
