// The backward pass of the SMPL layer (smpl_lbs.hip): the exact vector-Jacobian product
//   (grad_verts [B,NV,3], grad_joints [B,NJ,3])  ->  (grad_pose [B,3 NJ], grad_betas [B,NB], grad_trans [B,3])
// of gator_smpl_forward_f32 at (pose, betas, trans), recomputed from those inputs: the forward stores nothing per vertex.
//
// The mathematics, per sample.  Forward (smpl_lbs.hip): R_j the layer's Rodrigues of pose_j, m = (R_j - I)_{j >= 1} the pose map,
// coef = [betas ; m], p_v = v_posed = v_template_v + [shapedirs | posedirs]_v coef, J = jfold [1 ; betas] the shaped rest joints,
// G_0 = [R_0 | J_0], G_j = G_p [R_j | J_j - J_p] (p the parent), A_j = [A^R | A^t] = [G^R_j | G^t_j - G^R_j J_j],
// x_v = s (sum_j w_vj A_j [p_v ; 1] + off), q_j = s (G^t_j + off), s = out_scale, off = trans, or -G^t_c when centring, or 0.
// Backward, with gV, gJ the upstream gradients of x and q:
//   scale, offset   gx_v = s gV_v, gq_j = s gJ_j.  g_off = sum_v gx_v + sum_j gq_j is g_trans with trans, and is subtracted from gq_c
//                   when centring.
//   skinning        gA^R_j = sum_v w_vj gx_v p_v^T,  gA^t_j = sum_v w_vj gx_v,  gp_v = (sum_j w_vj A^R_j)^T gx_v.
//   blend shapes    g_coef = [shapedirs | posedirs]^T gp; its first NB entries go to g_betas, the rest is gR_j for j >= 1.
//   transforms      gG^R_j += gA^R_j - gA^t_j J_j^T,  gG^t_j += gA^t_j + gq_j,  gJ_j -= G^R_j^T gA^t_j.
//   chain           children before parents: gR_j += G^R_p^T gG^R_j,  gG^R_p += gG^R_j R_j^T + gG^t_j (J_j - J_p)^T,  gG^t_p += gG^t_j,
//                   gJ_j += G^R_p^T gG^t_j and gJ_p -= the same; the root takes gG_0 directly: gR_0 += gG^R_0, gJ_0 += gG^t_0.
//   rest joints     g_betas += jfold[:, 1:]^T gJ.
//   rotations       g_pose_j = (d R_j / d pose_j)^T gR_j through smpl_rodrigues (smpl_ctx.h): the matrix of the normalised quaternion,
//                   the normalisation, q = (cos h, (sin h / angle) a), h = angle / 2, angle = |a + 1e-8|.  angle >= 1.7e-8 at the
//                   all-zero pose, so every quotient is finite there, as in the forward.
//
// Kernels.
//   k_smpl_pose      (smpl_lbs.hip) at the inputs: the coefficient rows and the skinning transforms, as in the forward.
//   k_smpl_bwd_skin  the hot path, the transpose of k_smpl_skin.  A workgroup owns one (32-sample, 128-vertex) tile:
//                    1. p - v_template = [32 x K] . [K x 3 x 128]: smpl_coef_tile and smpl_blend (smpl_steps.h), the code k_smpl_skin
//                       runs, a lane holding x, y, z of one vertex for 16 samples;
//                    2. in registers gx = s gV, p, T^R = sum w A^R and gp = T^R^T gx; gx and p go to LDS as [coordinate][vertex][sample];
//                    3. gA as a matrix product over the tile's vertices in vertex order, D[joint][sample] += W^T[joint][v] . (gx_r p_c)[v][sample]
//                       with the dense [128 x 32] weight tile of the vertices in LDS (so any number of influences costs the same):
//                       wave c takes column c of [p ; 1] and the three rows r; wave 3 (the column of ones) also adds gx itself in fp64,
//                       the tile's share of g_off;
//                    4. gp replaces p in LDS and g_coef[k][sample] += basis^T[k][v] . gp[v][sample], 32 coefficients per wave and pass,
//                       one fmaf chain over (coordinate, vertex), the basis read from its transposed copy [3][NVp][Kq], which
//                       k_smpl_bwd_transpose makes on the first call that comes with grad_verts.
//                    Every result is a per-tile partial, written sample-minor to the workspace.  The chunk of the vertex sum is the tile:
//                    it depends on NV alone.
//   k_smpl_bwd_reduce adds the tiles' partials in tile order in fp64.
//   k_smpl_bwd_chain one wave per sample, fp64: smpl_kinematics (smpl_steps.h: rotations, rest joints, forward chain), then the transforms,
//                    the reverse chain, the rest joints and the Rodrigues derivative above; each output is rounded to float32 once.
// With grad_verts = NULL only k_smpl_bwd_chain runs (it recomputes its own rotations and joints): nothing per vertex is touched.
// Determinism: a sample is one MFMA column (steps 3, 4) or row (step 1) and one LDS column from end to end, every sum has a fixed order
// and nothing is atomic: row b is the same bits whatever the batch and from run to run.  A non-finite pose, beta, trans or upstream
// gradient of a sample makes its three gradient rows NaN (a 0 * x flag, as in the forward; grad_verts is seen through g_off) and changes
// no other row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "internal.h"
#include "smpl_ctx.h"
#include "smpl_steps.h"

namespace gator {
namespace {

constexpr int kSG = 16;      // k-steps per pipeline stage of the g_coef product

__host__ __device__ constexpr int bwd_pw(int Kq, int NJ) { return Kq + NJ * 12; }      // floats of one sample's partial: g_coef, gA
__host__ __device__ constexpr int bwd_sw(int Kq, int NJ) { return Kq + NJ * 12 + 4; }  // doubles of one sample's sums: g_coef, gA, g_off

// grid (NVp / kTV, sample tiles).  part: [sample tile][vertex tile][PW][32]; ptrans: [sample tile][vertex tile][3][32]
template <int MI_T>
__global__ __launch_bounds__(256) void k_smpl_bwd_skin(const float* __restrict__ basis, const float* __restrict__ basisT,
                                                       const float* __restrict__ vtempl, const int32_t* __restrict__ widx,
                                                       const float* __restrict__ wval, int MI, const float* __restrict__ coef,
                                                       const float* __restrict__ xform, const float* __restrict__ gverts, int B, int NV,
                                                       int NVp, int NJ, int Kp, int Kq, float out_scale, float* __restrict__ part,
                                                       double* __restrict__ ptrans) {
    extern __shared__ float lds[];
    float* gxL = lds;                          // [3][128][33] gx; before that the transposed coefficient tile [Kp][33]
    float* pL = gxL + 3 * kTV * kLd;           // [3][128][33] p, then gp
    float* WL = pL + 3 * kTV * kLd;            // [128][33]    the tile's skinning weights, dense
    float* xr = WL + kTV * kLd;                // [32][NJ][9]  A^R of the tile's samples
    const int s0 = blockIdx.y * kTS, v0 = blockIdx.x * kTV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const int ns = min(kTS, B - s0);
    smpl_coef_tile(coef, s0, ns, Kp, gxL);
    for (int e = threadIdx.x; e < kTV * kLd; e += 256) WL[e] = 0.f;
    for (int e = threadIdx.x; e < kTS * NJ * 9; e += 256) {
        const int s = e / (NJ * 9), q = e - s * (NJ * 9), j = q / 9, k = q - j * 9;
        xr[e] = s < ns ? xform[((size_t)(s0 + s) * NJ + j) * 12 + (k / 3) * 4 + (k % 3)] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < MI * kTV; e += 256) {                 // a vertex names a joint at most once: no two writes meet
        const int m = e / kTV, vl = e - m * kTV;
        const float w = wval[(size_t)m * NVp + v0 + vl];
        if (w != 0.f) WL[vl * kLd + widx[(size_t)m * NVp + v0 + vl]] = w;
    }
    const int vl = wave * 32 + col, v = v0 + vl;                        // < NVp: the planes are padded to whole tiles
    f32x16 ax = {0}, ay = {0}, az = {0};
    smpl_blend(gxL, basis + v, NVp, Kp, col, hi, ax, ay, az);           // step 1: p - v_template, by the forward's own code
    __syncthreads();                                                    // the coefficient tile is done with; the weight tile is complete
    // step 2
    const float tx = vtempl[v], ty = vtempl[NVp + v], tz = vtempl[2 * NVp + v];
    int ji[MI_T ? MI_T : 1];
    float jw[MI_T ? MI_T : 1];
    if constexpr (MI_T > 0) {
#pragma unroll
        for (int m = 0; m < MI_T; ++m) {
            ji[m] = m < MI ? widx[(size_t)m * NVp + v] * 9 : 0;
            jw[m] = m < MI ? wval[(size_t)m * NVp + v] : 0.f;
        }
    }
    const float* gbase = gverts + ((size_t)s0 * NV + min(v, NV - 1)) * 3;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = mfma32_row(r, hi);
        const float* xi = xr + i * NJ * 9;
        float T[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = 0.f;
        if constexpr (MI_T > 0) {
#pragma unroll
            for (int m = 0; m < MI_T; ++m) {
                const float* q = xi + ji[m];
#pragma unroll
                for (int e = 0; e < 9; ++e) T[e] = fmaf(jw[m], q[e], T[e]);
            }
        } else {
            for (int j = 0; j < NJ; ++j) {
                const float w = WL[vl * kLd + j];
                const float* q = xi + j * 9;
#pragma unroll
                for (int e = 0; e < 9; ++e) T[e] = fmaf(w, q[e], T[e]);
            }
        }
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (v < NV && i < ns) {
            const float* g = gbase + i * NV * 3;                        // < 2^31: NV <= 2^24, i < 32
            g0 = g[0] * out_scale; g1 = g[1] * out_scale; g2 = g[2] * out_scale;
        }
        gxL[vl * kLd + i] = g0;
        gxL[(kTV + vl) * kLd + i] = g1;
        gxL[(2 * kTV + vl) * kLd + i] = g2;
        pL[vl * kLd + i] = tx + ax[r];                                  // v_posed = v_template + blend offsets
        pL[(kTV + vl) * kLd + i] = ty + ay[r];
        pL[(2 * kTV + vl) * kLd + i] = tz + az[r];
        float h0 = fmaf(T[0], g0, fmaf(T[3], g1, T[6] * g2));           // gp = T^R^T gx
        float h1 = fmaf(T[1], g0, fmaf(T[4], g1, T[7] * g2));
        float h2 = fmaf(T[2], g0, fmaf(T[5], g1, T[8] * g2));
        asm volatile("" : "+v"(h0), "+v"(h1), "+v"(h2));                // computed here: sunk to its use in step 4, it keeps 36 LDS values per sample alive and spills
        ax[r] = h0; ay[r] = h1; az[r] = h2;
    }
    __syncthreads();
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    float* pt = part + tile * bwd_pw(Kq, NJ) * kTS;
    {   // step 3: A[i = joint][k = vertex] from the weight tile, B[k = vertex][j = sample] = gx_r p_c; lane (col, hi) feeds vertex 2 st + hi
        const int c = wave;
        f32x16 a0 = {0}, a1 = {0}, a2 = {0};
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll 4
        for (int st = 0; st < kTV / 2; ++st) {
            const int vv = 2 * st + hi;
            const float wv = WL[vv * kLd + col];
            const float pc = c < 3 ? pL[(c * kTV + vv) * kLd + col] : 1.f;
            const float g0 = gxL[vv * kLd + col], g1 = gxL[(kTV + vv) * kLd + col], g2 = gxL[(2 * kTV + vv) * kLd + col];
            a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, g0 * pc, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, g1 * pc, a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, g2 * pc, a2, 0, 0, 0);
            if (c == 3) { d0 += (double)g0; d1 += (double)g1; d2 += (double)g2; }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = mfma32_row(q, hi);
            if (j < NJ) {
                const int o = (Kq + j * 12 + c) * kTS + col;
                pt[o] = a0[q]; pt[o + 4 * kTS] = a1[q]; pt[o + 8 * kTS] = a2[q];
            }
        }
        if (c == 3) {                                                   // even vertices + odd vertices
            d0 += __shfl_xor(d0, 32); d1 += __shfl_xor(d1, 32); d2 += __shfl_xor(d2, 32);
            if (hi == 0) {
                double* o = ptrans + tile * 3 * kTS + col;
                o[0] = d0; o[kTS] = d1; o[2 * kTS] = d2;
            }
        }
    }
    __syncthreads();                                                    // p is done with: gp takes its place
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = mfma32_row(r, hi);
        pL[vl * kLd + i] = ax[r];
        pL[(kTV + vl) * kLd + i] = ay[r];
        pL[(2 * kTV + vl) * kLd + i] = az[r];
    }
    __syncthreads();
    // step 4: A[i = coefficient][k = vertex] from the transposed basis, B[k = vertex][j = sample] = gp.  The chain runs over the
    // coordinate, then the vertex: 192 steps in twelve stages of kSG; two register sets take turns, each loaded a whole stage
    // (1024 cycles of matrix work) before it is used, as in step 1.
    for (int cb = wave; cb < Kq / 32; cb += 4) {
        f32x16 acc = {0};
        const float* bt = basisT + (size_t)(v0 + hi) * Kq + cb * 32 + col;
        float pb[kSG], qb[kSG];
        auto fetch4 = [&](int s, float (&a)[kSG]) {                      // stage s: coordinate s / 4, vertices 32 (s % 4) ..
            const float* b = bt + ((size_t)(s >> 2) * NVp + 2 * kSG * (s & 3)) * Kq;
#pragma unroll
            for (int u = 0; u < kSG; ++u) a[u] = b[(size_t)(2 * u) * Kq];
        };
        auto mma4 = [&](int s, const float (&a)[kSG]) {
            const float* gp = pL + ((s >> 2) * kTV + 2 * kSG * (s & 3) + hi) * kLd + col;
#pragma unroll
            for (int u = 0; u < kSG; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], gp[2 * u * kLd], acc, 0, 0, 0);
        };
        constexpr int NS = 3 * kTV / (2 * kSG);
        fetch4(0, pb);
        for (int s = 0; s < NS; s += 2) {
            fetch4(s + 1, qb);
            __builtin_amdgcn_sched_barrier(0);
            mma4(s, pb);
            __builtin_amdgcn_sched_barrier(0);
            fetch4(min(s + 2, NS - 1), pb);                              // after the last stage: an in-bounds fetch nobody uses
            __builtin_amdgcn_sched_barrier(0);
            mma4(s + 1, qb);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = mfma32_row(q, hi);
            pt[(cb * 32 + k) * kTS + col] = acc[q];
        }
    }
}

// grid (ceil((PW + 3) / 8), sample tiles), 256 threads = 8 entries x 32 samples: sums[b][entry] = the tiles' partials, in tile order
__global__ __launch_bounds__(256) void k_smpl_bwd_reduce(const float* __restrict__ part, const double* __restrict__ ptrans, int B, int NT,
                                                         int PW, int SW, double* __restrict__ sums) {
    const int s = threadIdx.x & 31, e = blockIdx.x * 8 + (threadIdx.x >> 5), b = blockIdx.y * kTS + s;
    if (e >= PW + 3 || b >= B) return;
    double acc = 0.0;
    if (e < PW) {
        const float* src = part + ((size_t)blockIdx.y * NT * PW + e) * kTS + s;
        for (int t = 0; t < NT; ++t) acc += (double)src[(size_t)t * PW * kTS];
    } else {
        const double* src = ptrans + ((size_t)blockIdx.y * NT * 3 + (e - PW)) * kTS + s;
        for (int t = 0; t < NT; ++t) acc += src[(size_t)t * 3 * kTS];
    }
    sums[(size_t)b * SW + e] = acc;
}

// ga = (d R / d a)^T gR for R = smpl_rodrigues(a); g: 3x3 row-major
__device__ inline void smpl_rodrigues_vjp(double ax, double ay, double az, const double* g, double* ga) {
    const double ex = ax + 1e-8, ey = ay + 1e-8, ez = az + 1e-8;
    const double angle = sqrt(ex * ex + ey * ey + ez * ez);
    const double half = angle * 0.5, sn = sin(half), cs = cos(half), u = sn / angle;
    const double qw = cs, qx = u * ax, qy = u * ay, qz = u * az;
    const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    const double w = qw / qn, x = qx / qn, y = qy / qn, z = qz / qn;
    // the matrix of the unit quaternion (w, x, y, z)
    const double hw = 2.0 * (w * (g[0] + g[4] + g[8]) - z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
    const double hx = 2.0 * (x * (g[0] - g[4] - g[8]) + y * g[1] + z * g[2] + y * g[3] - w * g[5] + z * g[6] + w * g[7]);
    const double hy = 2.0 * (y * (g[4] - g[0] - g[8]) + x * g[1] + w * g[2] + x * g[3] + z * g[5] - w * g[6] + z * g[7]);
    const double hz = 2.0 * (z * (g[8] - g[0] - g[4]) - w * g[1] + x * g[2] + w * g[3] + y * g[5] + x * g[6] + y * g[7]);
    // the normalisation q / |q|
    const double dot = w * hw + x * hx + y * hy + z * hz;
    const double kw = (hw - w * dot) / qn, kx = (hx - x * dot) / qn, ky = (hy - y * dot) / qn, kz = (hz - z * dot) / qn;
    // q = (cos h, u a), u = sin h / angle, h = angle / 2
    const double gu = ax * kx + ay * ky + az * kz;
    const double gh = -sn * kw + (cs / angle) * gu;
    const double gangle = 0.5 * gh - (u / angle) * gu;
    const double k = gangle / angle;                                    // angle = |a + 1e-8|
    ga[0] = u * kx + k * ex; ga[1] = u * ky + k * ey; ga[2] = u * kz + k * ez;
}

// One wave per sample, fp64.  sums: the reduced [B][SW] of the hot kernel, or NULL without grad_verts.
__global__ __launch_bounds__(64) void k_smpl_bwd_chain(const float* __restrict__ pose, const float* __restrict__ betas,
                                                       const float* __restrict__ trans, const float* __restrict__ gjoints,
                                                       const double* __restrict__ jfold, const int32_t* __restrict__ parents, int NJ, int NB,
                                                       int Kq, int SW, int center, double out_scale, const double* __restrict__ sums,
                                                       float* __restrict__ gpose, float* __restrict__ gbetas, float* __restrict__ gtrans) {
    __shared__ double R[kSmplMaxJ * 9], J[kSmplMaxJ * 3], G[kSmplMaxJ * 12], gG[kSmplMaxJ * 12], gR[kSmplMaxJ * 9], gJ[kSmplMaxJ * 3];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* sm = sums ? sums + (size_t)b * SW : nullptr;
    const int PW = bwd_pw(Kq, NJ);
    double poison = 0.0;                 // 0, or NaN when an input or an upstream gradient of the sample is not finite
    if (betas)
        for (int k = t; k < NB; k += 64) poison += (double)betas[(size_t)b * NB + k] * 0.0;
    if (trans && t < 3) poison += (double)trans[(size_t)b * 3 + t] * 0.0;
    if (sm && t < 3) poison += sm[PW + t] * 0.0;                        // a non-finite grad_verts entry shows in its sum
    poison += smpl_kinematics(pose, betas, jfold, parents, b, t, NJ, NB, R, J, G);
    // scale and offset, skinning transforms -> gG, gJ; blend shapes -> gR
    double gq[3] = {0.0, 0.0, 0.0};
    if (t < NJ) {
        double gA[12];
        for (int e = 0; e < 12; ++e) gA[e] = sm ? sm[Kq + t * 12 + e] : 0.0;
        if (gjoints)
            for (int c = 0; c < 3; ++c) gq[c] = (double)gjoints[((size_t)b * NJ + t) * 3 + c] * out_scale;
        poison += (gq[0] + gq[1] + gq[2]) * 0.0;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) gG[t * 12 + r * 4 + c] = gA[r * 4 + c] - gA[r * 4 + 3] * J[t * 3 + c];
            gG[t * 12 + r * 4 + 3] = gA[r * 4 + 3] + gq[r];
        }
        for (int c = 0; c < 3; ++c)
            gJ[t * 3 + c] = -((G[t * 12 + c] * gA[3] + G[t * 12 + 4 + c] * gA[7]) + G[t * 12 + 8 + c] * gA[11]);
        for (int e = 0; e < 9; ++e) gR[t * 9 + e] = (sm && t >= 1) ? sm[NB + (t - 1) * 9 + e] : 0.0;
    }
    double goff[3];
    for (int c = 0; c < 3; ++c) {
        double x = gq[c];
        for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
        goff[c] = x + (sm ? sm[PW + c] : 0.0);
    }
    for (int d = 32; d > 0; d >>= 1) poison += __shfl_xor(poison, d);
    __syncthreads();
    if (center >= 0 && t < 3) gG[center * 12 + t * 4 + 3] -= goff[t];
    __syncthreads();
    // the reverse chain: joint j's gG is final when its turn comes (parents[j] < j)
    for (int j = NJ - 1; j >= 1; --j) {
        const int p = parents[j];
        const double* gj = gG + j * 12;
        const double* Gp = G + p * 12;
        if (t < 9) {
            const int r = t / 3, c = t - r * 3;
            gR[j * 9 + t] += (Gp[r] * gj[c] + Gp[4 + r] * gj[4 + c]) + Gp[8 + r] * gj[8 + c];
            const double* Rj = R + j * 9 + c * 3;
            gG[p * 12 + r * 4 + c] += ((gj[r * 4] * Rj[0] + gj[r * 4 + 1] * Rj[1]) + gj[r * 4 + 2] * Rj[2])
                                      + gj[r * 4 + 3] * (J[j * 3 + c] - J[p * 3 + c]);
        } else if (t < 12) {
            const int c = t - 9;
            const double gd = (Gp[c] * gj[3] + Gp[4 + c] * gj[7]) + Gp[8 + c] * gj[11];
            gJ[j * 3 + c] += gd;
            gJ[p * 3 + c] -= gd;
            gG[p * 12 + c * 4 + 3] += gj[c * 4 + 3];
        }
        __syncthreads();
    }
    if (t < 9) gR[t] += gG[(t / 3) * 4 + t % 3];
    else if (t < 12) gJ[t - 9] += gG[(t - 9) * 4 + 3];
    __syncthreads();
    if (gbetas)
        for (int k = t; k < NB; k += 64) {
            double acc = sm ? sm[k] : 0.0;
            for (int e = 0; e < NJ * 3; ++e) acc += jfold[(size_t)e * (1 + NB) + 1 + k] * gJ[e];
            gbetas[(size_t)b * NB + k] = (float)(acc + poison);
        }
    if (gpose && t < NJ) {
        const float* a = pose + ((size_t)b * NJ + t) * 3;
        double ga[3];
        smpl_rodrigues_vjp((double)a[0], (double)a[1], (double)a[2], gR + t * 9, ga);
        for (int c = 0; c < 3; ++c) gpose[((size_t)b * NJ + t) * 3 + c] = (float)(ga[c] + poison);
    }
    if (gtrans && t < 3) gtrans[(size_t)b * 3 + t] = (float)(goff[t] + poison);
}

// basisT[x][v][k] = basis[x][k][v], zero for k >= Kp: 32 x 32 tiles through LDS, both sides in 128-byte rows.  grid (NVp / 32, Kq / 32, 3)
__global__ __launch_bounds__(256) void k_smpl_bwd_transpose(const float* __restrict__ basis, int Kp, int Kq, int NVp, float* __restrict__ basisT) {
    __shared__ float tile[32][33];
    const int v0 = blockIdx.x * 32, k0 = blockIdx.y * 32, x = blockIdx.z, a = threadIdx.x & 31, b = threadIdx.x >> 5;
    for (int r = b; r < 32; r += 8) tile[r][a] = k0 + r < Kp ? basis[((size_t)x * Kp + k0 + r) * NVp + v0 + a] : 0.f;
    __syncthreads();
    for (int r = b; r < 32; r += 8) basisT[((size_t)x * NVp + v0 + r) * Kq + k0 + a] = tile[a][r];
}

size_t bwd_lds_bytes(int NJ) { return sizeof(float) * ((size_t)7 * kTV * kLd + (size_t)kTS * NJ * 9); }

// The transposed basis is made by the first call that needs it, so a ctx that never differentiates holds one copy of the basis.
// That call allocates and waits for its stream once, like a growth of the workspace: it cannot be the one that is captured.
int bwd_basis(gator_smpl* c, hipStream_t st) {
    const size_t need = (size_t)3 * c->NVp * c->Kq;
    if (c->basisT.cap >= need) return GATOR_OK;
    GATOR_TRY(c->grow(c->basisT, need));
    k_smpl_bwd_transpose<<<dim3(c->NVp / 32, c->Kq / 32, 3), 256, 0, st>>>(c->basis, c->Kp, c->Kq, c->NVp, c->basisT);
    GATOR_HIP_CHECK(hipGetLastError());
    GATOR_HIP_CHECK(hipStreamSynchronize(st));                          // a call on another stream may follow at once
    return GATOR_OK;
}

}  // namespace

int smpl_backward_build(gator_smpl* c, const gator_smpl_model*) {
    c->Kq = (c->Kp + 31) / 32 * 32;
    // One value for every ctx of the process, whatever its joint count: the kernels are shared, and a later, smaller model must not
    // lower the limit of an earlier one.  155 136 bytes at kSmplMaxJ; SMPL's launches ask for 145 920: one workgroup per CU either way.
    const int lds = (int)bwd_lds_bytes(kSmplMaxJ);
    GATOR_HIP_CHECK(hipFuncSetAttribute((const void*)k_smpl_bwd_skin<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    GATOR_HIP_CHECK(hipFuncSetAttribute((const void*)k_smpl_bwd_skin<0>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return GATOR_OK;
}
}  // namespace gator

extern "C" int gator_smpl_workspace_bytes(const gator_smpl* ctx, int64_t* bytes, int64_t* allocations) {
    return gator::handle_workspace(ctx, "gator_smpl_workspace_bytes", bytes, allocations);
}

extern "C" int gator_smpl_backward_f32(gator_smpl* ctx, const float* pose, const float* betas, const float* trans, int32_t batch,
                                       int32_t center_idx, float out_scale, const float* grad_verts, const float* grad_joints,
                                       float* grad_pose, float* grad_betas, float* grad_trans, void* stream) {
    using namespace gator;
    const char* who = "gator_smpl_backward_f32";
    GATOR_TRY(smpl_check_layer_call(who, ctx, pose, trans, batch, center_idx, out_scale));
    if (!grad_verts && !grad_joints) return fail(GATOR_EINVAL, "%s: grad_verts and grad_joints are both NULL, there is nothing to propagate", who);
    if (batch == 0 || (!grad_pose && !grad_betas && !grad_trans)) return GATOR_OK;
    if (!ctx->NB) grad_betas = nullptr;
    const int tiles = (batch + kTS - 1) / kTS, NT = ctx->NVp / kTV, PW = bwd_pw(ctx->Kq, ctx->NJ), SW = bwd_sw(ctx->Kq, ctx->NJ);
    GATOR_TRY(smpl_reserve(ctx, batch));
    hipStream_t st = (hipStream_t)stream;
    if (grad_verts) {
        GATOR_TRY(bwd_basis(ctx, st));
        GATOR_TRY(ctx->grow(ctx->bpart, (size_t)tiles * NT * PW * kTS));
        GATOR_TRY(ctx->grow(ctx->btrans, (size_t)tiles * NT * 3 * kTS));
        GATOR_TRY(ctx->grow(ctx->bsum, (size_t)batch * SW));
        GATOR_TRY(smpl_pose_stage(ctx, pose, betas, nullptr, batch, -1, 1.0, nullptr, st));
        GATOR_TRY(launch_by_influences(ctx, k_smpl_bwd_skin<4>, k_smpl_bwd_skin<0>, dim3(NT, tiles), bwd_lds_bytes(ctx->NJ), st, ctx->basis,
                                       ctx->basisT, ctx->vtempl, ctx->widx, ctx->wval, ctx->MI, ctx->coef, ctx->xform, grad_verts, batch, ctx->NV,
                                       ctx->NVp, ctx->NJ, ctx->Kp, ctx->Kq, out_scale, ctx->bpart, ctx->btrans));
        k_smpl_bwd_reduce<<<dim3((PW + 3 + 7) / 8, tiles), 256, 0, st>>>(ctx->bpart, ctx->btrans, batch, NT, PW, SW, ctx->bsum);
        GATOR_HIP_CHECK(hipGetLastError());
    }
    k_smpl_bwd_chain<<<batch, 64, 0, st>>>(pose, ctx->NB ? betas : nullptr, trans, grad_joints, ctx->jfold, ctx->parents, ctx->NJ, ctx->NB, ctx->Kq,
                                           SW, center_idx < 0 ? -1 : center_idx, (double)out_scale, grad_verts ? ctx->bsum.get() : nullptr,
                                           grad_pose, grad_betas, grad_trans);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
