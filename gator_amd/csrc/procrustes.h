// Similarity (Procrustes) fit shared by the evaluation kernels: caller_kernels.hip (k_rigid_align, k_joint_errors) and temporal.hip
// (k_seq_errors): one sample per lane, <= kMaxPts points; mesh_eval.hip (k_mesh_errors): one workgroup per sample, the moments reduced
// over the whole mesh.  With it what those kernels share around the fit: the point-set bound and its LDS, the error under the fit,
// the wave's fp64 sum (train_batch.hip: k_camera_targets uses that too).
#pragma once
#include <hip/hip_runtime.h>

#include "internal.h"

namespace gator {
namespace {

constexpr int kMaxPts = 32;                                                       // points of a per-lane fit (3..32 evaluation joints)
constexpr size_t kPtsLds = (size_t)2 * kMaxPts * 3 * 64 * sizeof(double);         // 96 KB: the two point sets of a 64-thread block

// 96 KB of dynamic LDS > the 64 KB default: raised once PER DEVICE and per kernel, `done` being that kernel's table (the attribute
// belongs to the device's copy of the function; a process that evaluates on a second GPU, or whose first call failed transiently,
// must not inherit a cached answer)
inline int raise_pts_lds(const void* fn, bool (&done)[64]) {
    int dev = 0;
    GATOR_HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !done[dev]) {
        GATOR_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPtsLds));
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
    return GATOR_OK;
}

// A gator_coo as every entry point takes it: a count, and its three arrays unless it is empty.  The joint range is the caller's.
inline bool coo_ok(const gator_coo& g) { return g.nnz >= 0 && (g.nnz == 0 || (g.row && g.col && g.val)); }

// The sum of x over the 64 lanes of a wave, the same bits in every lane: a + b == b + a bit for bit, so after each xor step both
// partners hold one value.
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m);
    return x;
}

// 3x3 SVD by one-sided Jacobi (Hestenes) in fp64: G = H V is driven to orthogonal columns; s_i = |G_i|, U_i = G_i / s_i.
// V is a product of rotations and column swaps, orthogonal whatever the rank.  A column of G under 1e-14 s_0 is rounding noise:
// normalised it is a unit vector in no particular relation to the others, and R = V U^T would not be a rotation.  Such columns of U
// are therefore COMPLETED to an orthonormal basis: rank 2 (coplanar points) U_2 = U_0 x U_1; rank 1 (collinear points, e.g. a
// collapsed prediction) U_1 = a unit vector orthogonal to U_0, then U_2 = U_0 x U_1.  The completion spans the null space, so the
// optimum does not depend on it.  Rank 0 (H = 0) keeps U = 0: R = 0, c = 0 / var(a), aligned = the target centroid (NaN when
// var(a) = 0 too), as the reference's c = 0 gives.  The full-rank path is untouched.
__device__ void svd3(const double H[3][3], double U[3][3], double s[3], double V[3][3]) {
    double G[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { G[i][j] = H[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                double a = 0.0, bq = 0.0, c = 0.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) { a += G[i][p] * G[i][p]; bq += G[i][q] * G[i][q]; c += G[i][p] * G[i][q]; }
                off = fmax(off, fabs(c) / (sqrt(a * bq) + 1e-300));
                if (fabs(c) <= 1e-300) continue;
                const double zeta = (bq - a) / (2.0 * c);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double gp = G[i][p], gq = G[i][q];
                    G[i][p] = cs * gp - sn * gq;  G[i][q] = sn * gp + cs * gq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = cs * vp - sn * vq;  V[i][q] = sn * vp + cs * vq;
                }
            }
        if (off < 1e-15) break;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
    // sort descending (the reflection fix below must hit the SMALLEST singular value, as numpy's s[-1] does)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = i + 1; j < 3; ++j)
            if (s[j] > s[i]) {
                const double ts = s[i]; s[i] = s[j]; s[j] = ts;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double tg = G[r][i]; G[r][i] = G[r][j]; G[r][j] = tg;
                    const double tv = V[r][i]; V[r][i] = V[r][j]; V[r][j] = tv;
                }
            }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) U[i][j] = s[j] > 1e-300 ? G[i][j] / s[j] : 0.0;
    if (s[0] > 1e-300 && s[1] <= 1e-14 * s[0]) {      // rank-1 covariance (collinear points): U[:,1] = e x U[:,0], normalised
        const double u0 = U[0][0], u1 = U[1][0], u2 = U[2][0];
        const double m0 = fabs(u0), m1 = fabs(u1), m2 = fabs(u2);
        double w0, w1, w2;           // e = the coordinate axis on which U[:,0] is smallest: |e x U[:,0]| >= sqrt(2/3)
        if (m0 <= m1 && m0 <= m2) { w0 = 0.0; w1 = -u2; w2 = u1; }
        else if (m1 <= m2)        { w0 = u2;  w1 = 0.0; w2 = -u0; }
        else                      { w0 = -u1; w1 = u0;  w2 = 0.0; }
        const double wn = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
        U[0][1] = w0 / wn; U[1][1] = w1 / wn; U[2][1] = w2 / wn;
    }
    if (s[2] <= 1e-14 * s[0]) {      // rank-deficient covariance (coplanar or collinear points): complete U with the cross product
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    }
}

// rigid_transform_3D + rigid_align (lib/coord_utils.py:127-149): H = (A-ca)^T (B-cb) / n = U S V^T; R = V U^T, with the reflection
// fix (det R < 0: s3 := -s3, V[:,2] := -V[:,2]); c = sum(s) / sum_axis var(A); t = -(cR) ca + cb; out = cR A + t.
// The second half, from the moments: H = the covariance (A-ca)^T (B-cb) / n, var = sum_axis var(A), ca / cb = the centroids.
__device__ void similarity_from_moments(const double (&H)[3][3], double var, const double (&ca)[3], const double (&cb)[3], double& c,
                                        double (&R)[3][3], double (&tr)[3]) {
    double U[3][3], s[3], V[3][3];
    svd3(H, U, s, V);
    auto mkR = [&]() {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) R[r][cc] = V[r][0] * U[cc][0] + V[r][1] * U[cc][1] + V[r][2] * U[cc][2];
    };
    mkR();
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0.0) {
        s[2] = -s[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) V[r][2] = -V[r][2];
        mkR();
    }
    c = (s[0] + s[1] + s[2]) / var;
#pragma unroll
    for (int r = 0; r < 3; ++r) tr[r] = cb[r] - c * (R[r][0] * ca[0] + R[r][1] * ca[1] + R[r][2] * ca[2]);
}

// similarity (Procrustes) fit of n points a onto t, fp64: aligned = c R a + tr   (lib/coord_utils.py:127-142)
// The point sets live in LDS, one column per thread ([point][axis][thread]: conflict-free, no per-thread private arrays)
struct Pts {
    double* p; int tid, nt;
    __device__ double& operator()(int i, int k) const { return p[(size_t)(i * 3 + k) * nt + tid]; }
};
__device__ void rigid_fit(const Pts& a, const Pts& t, int n, double& c, double (&R)[3][3], double (&tr)[3]) {
    double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) { ca[k] += a(i, k); cb[k] += t(i, k); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { ca[k] /= n; cb[k] /= n; }
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var = 0.0;
    for (int i = 0; i < n; ++i) {
        double da[3], db[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { da[k] = a(i, k) - ca[k]; db[k] = t(i, k) - cb[k]; var += da[k] * da[k]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) H[r][cc] += da[r] * db[cc];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) H[r][cc] /= n;
    var /= n;
    similarity_from_moments(H, var, ca, cb, c, R, tr);
}

// The error under a fit: the sum over the n points of |c R a + tr - t|, fp64.  RoundF32: the aligned point is rounded to float32
// first, where the reference's aligned joints are float32 (k_joint_errors: data/PW3D/dataset.py:273-286).
template <bool RoundF32>
__device__ __forceinline__ double aligned_error(const Pts& a, const Pts& t, int n, double c, const double (&R)[3][3], const double (&tr)[3]) {
    double e = 0.0;
    for (int i = 0; i < n; ++i) {
        double d2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double v = c * (R[r][0] * a(i, 0) + R[r][1] * a(i, 1) + R[r][2] * a(i, 2)) + tr[r];
            const double al = RoundF32 ? (double)(float)v : v;
            d2 += (al - t(i, r)) * (al - t(i, r));
        }
        e += sqrt(d2);
    }
    return e;
}

}  // namespace
}  // namespace gator
