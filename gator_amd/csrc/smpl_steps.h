// The device steps that the SMPL kernels share, each stated once: the layer (smpl_lbs.hip), its backward (smpl_backward.hip) and the
// fit (smpl_fit.hip) recompute the same quantities and must get the same bits, so they call the same code.  The order of every
// floating-point operation here is part of the contract (-ffp-contract=off; every fmaf and every parenthesised sum as written).
#pragma once
#include <hip/hip_runtime.h>

#include "smpl_ctx.h"

namespace gator {

constexpr int kTS = 32;      // samples per tile: the M of one 32x32x2 MFMA
constexpr int kKU = 4;       // k-pairs per pipeline stage of the blend product: Kp is padded to two stages, 4 kKU
constexpr int kLd = 33;      // leading dimension of every [..][32 samples] LDS image: conflict-free along samples and along the other index

typedef float f32x16 __attribute__((ext_vector_type(16)));

// C/D map of the 32x32 MFMA: register r of lane (col, hi) holds row mfma32_row(r, hi) of column col
__device__ __forceinline__ int mfma32_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// The coefficient rows of the sample tile s0 .. s0 + ns, transposed into LDS: ct[k][sample], zero for the samples the batch lacks.
// 256 threads; the caller synchronises.
__device__ __forceinline__ void smpl_coef_tile(const float* __restrict__ coef, int s0, int ns, int Kp, float* ct) {
    for (int e = threadIdx.x; e < kTS * Kp; e += 256) {
        const int s = e / Kp, k = e - s * Kp;
        ct[k * kLd + s] = s < ns ? coef[(size_t)(s0 + s) * Kp + k] : 0.f;
    }
}

// The blend product of one wave: (ax, ay, az)[sample][vertex] += ct^T [32 x Kp] . basis [Kp x 3 x 32] on v_mfma_f32_32x32x2_f32 (exact
// fp32 products, one fixed fmaf chain over k), the three coordinate planes of the basis as three accumulators, so that a lane holds
// x, y, z of one vertex for 16 samples (rows mfma32_row).  ct: the transposed coefficient tile; bp: the basis at the lane's vertex
// (< NVp: the planes are padded to whole tiles).  A[i = sample][k], B[k][j = vertex]: lane (col, hi) feeds k + hi.  A stage is kKU
// k-pairs = twelve MFMAs; two register sets take turns, each loaded a whole stage (768 cycles of matrix work) before it is used.
__device__ __forceinline__ void smpl_blend(const float* ct, const float* __restrict__ bp, int NVp, int Kp, int col, int hi, f32x16& ax,
                                           f32x16& ay, f32x16& az) {
    const size_t plane = (size_t)Kp * NVp;
    float pa[kKU], px[kKU], py[kKU], pz[kKU], qa[kKU], qx[kKU], qy[kKU], qz[kKU];
    auto fetch = [&](int k, float (&a)[kKU], float (&x)[kKU], float (&y)[kKU], float (&z)[kKU]) {
#pragma unroll
        for (int u = 0; u < kKU; ++u) {
            const int kk = k + 2 * u + hi;
            const size_t o = (size_t)kk * NVp;
            a[u] = ct[kk * kLd + col];
            x[u] = bp[o]; y[u] = bp[o + plane]; z[u] = bp[o + 2 * plane];
        }
    };
    auto mma = [&](const float (&a)[kKU], const float (&x)[kKU], const float (&y)[kKU], const float (&z)[kKU]) {
#pragma unroll
        for (int u = 0; u < kKU; ++u) {
            ax = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], x[u], ax, 0, 0, 0);
            ay = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], y[u], ay, 0, 0, 0);
            az = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], z[u], az, 0, 0, 0);
        }
    };
    fetch(0, pa, px, py, pz);
    for (int k = 0; k < Kp; k += 4 * kKU) {                              // Kp is a multiple of two stages
        fetch(k + 2 * kKU, qa, qx, qy, qz);
        __builtin_amdgcn_sched_barrier(0);                              // keep the loads ahead of the stage they overlap
        mma(pa, px, py, pz);
        __builtin_amdgcn_sched_barrier(0);
        fetch(min(k + 4 * kKU, Kp - 2 * kKU), pa, px, py, pz);          // after the last stage: an in-bounds fetch nobody uses
        __builtin_amdgcn_sched_barrier(0);
        mma(qa, qx, qy, qz);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// o = A [p ; 1] for a 3x4 row-major A
__device__ __forceinline__ void smpl_affine(const float* A, float px, float py, float pz, float* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = fmaf(A[r * 4], px, fmaf(A[r * 4 + 1], py, fmaf(A[r * 4 + 2], pz, A[r * 4 + 3])));
}

// The kinematics of sample b in fp64, one wave per sample (lane t), R [NJ][9], J [NJ][3], G [NJ][12] in LDS: the layer's Rodrigues of
// every joint, the shaped rest joints from the regressor folded at create, and the chain G_0 = [R_0 | J_0], G_j = G_p [R_j | J_j - J_p],
// joint by joint (parents[j] < j).  All three are complete and visible to the wave on return.  pose_map, where given, receives the
// layer's pose map (R_j - I) for j >= 1 as floats, [NJ - 1][9].  Returns the lane's share of the sample's poison flag for the pose: 0,
// or NaN when an entry of its joint is not finite (x * 0 keeps NaN, turns Inf into NaN).
__device__ __forceinline__ double smpl_kinematics(const float* __restrict__ pose, const float* __restrict__ betas,
                                                  const double* __restrict__ jfold, const int32_t* __restrict__ parents, int b, int t, int NJ,
                                                  int NB, double* R, double* J, double* G, float* pose_map = nullptr) {
    double poison = 0.0;
    if (t < NJ) {
        const float* a = pose + ((size_t)b * NJ + t) * 3;
        const double ax = a[0], ay = a[1], az = a[2];
        poison = (ax + ay + az) * 0.0;
        double* r = R + t * 9;
        smpl_rodrigues(ax, ay, az, r);
        if (pose_map && t >= 1)
            for (int e = 0; e < 9; ++e) pose_map[(t - 1) * 9 + e] = (float)(r[e] - ((e & 3) == 0 ? 1.0 : 0.0));      // subtract_flat_id
        for (int c = 0; c < 3; ++c) {
            const double* f = jfold + (size_t)(t * 3 + c) * (1 + NB);
            double acc = f[0];
            if (betas)
                for (int k = 0; k < NB; ++k) acc += f[1 + k] * (double)betas[(size_t)b * NB + k];
            J[t * 3 + c] = acc;
        }
    }
    __syncthreads();
    const int row = (t & 15) >> 2, col = t & 3;                         // lane e < 12 owns entry (row, col) of the 3x4 global transform
    for (int j = 0; j < NJ; ++j) {
        if (t < 12) {
            if (j == 0) {
                G[t] = col < 3 ? R[row * 3 + col] : J[row];
            } else {
                const int p = parents[j];
                const double* gp = G + p * 12 + row * 4;
                double g = 0.0;
                for (int k = 0; k < 3; ++k) g += gp[k] * (col < 3 ? R[j * 9 + k * 3 + col] : J[j * 3 + k] - J[p * 3 + k]);
                G[j * 12 + t] = col < 3 ? g : g + gp[3];
            }
        }
        __syncthreads();
    }
    return poison;
}

}  // namespace gator
