// The inverse of the SMPL layer on the device: a batched Levenberg-Marquardt fit of (pose [B,3 NJ], betas [B,NB], trans [B,3]) to target
// vertices [B,NV,3], owned by the gator_smpl handle.  No priors, no joint limits, no per-vertex weights: the unconstrained least-squares
// fit in vertex space, for models with at most four influences per vertex (the layer's MI_T = 4 form: SMPL, MANO).
//
// The iteration.  Unknowns P = 3 NJ + NB + 3: a world-frame rotation increment delta_k per joint, the betas, the translation.  The state
// is the float32 (pose, betas, trans) the layer takes, so the answer is what the caller feeds back to gator_smpl_forward_f32.
//   forward      k_smpl_pose at the candidate (smpl_lbs.hip): the coefficient row, the skinning transforms A_j, the posed joints p_j;
//                the kernels here recompute v_posed = v_template + basis . coef and apply A_j with the layer's smpl_affine (smpl_steps.h).
//   residual     r_v = verts_v + trans - target_v, verts_v = sum_j w_vj x_vj, x_vj = A_j [v_posed_v ; 1] (joint j's image of the vertex)
//   rotation     d verts_v / d delta_k = -[c_vk]x,  c_vk = sum_{j in subtree(k)} w_vj (x_vj - p_k): the per-joint images, not the blended
//                vertex (that simpler form stalls in local minima on small meshes).  The subtree test is a bit mask of ancestors per
//                influence, folded at create.  The pose blend shapes' dependence on the rotation is left out; the residual is exact, so
//                on a target that some parameters reproduce the fixed point is unaffected (on a noisy one it is J^T r = 0 with this J).
//   shape        d verts_v / d beta_b = (sum_j w_vj Rg_j) S_v[:, b]; the joints' movement with beta is left out as well.
//   translation  identity.
//   normal eq.   r is appended to J as column P and the width padded to N = 32 ceil((P + 1) / 32) (96 for SMPL, at most 128):
//                M = [J | r]^T [J | r] holds H = J^T J, g = J^T r and the squared error r^T r = M[P][P].
//   step         accept the candidate iff its error is smaller than the current one (the initial state is the first candidate: it is
//                accepted when its error is finite and leaves lambda alone; otherwise the sample is bad and its outputs are NaN).
//                accept: the candidate and its M become current, lambda = max(lambda / 4, 1e-9); reject: lambda = min(8 lambda, 1e6).
//                Solve (H + lambda diag H + 1e-12 I) d = -g by Cholesky in fp64; a non-positive pivot is one more rejection
//                (lambda times 8 again, d = 0).  R_k <- exp(Rg_parent(k)^T d_k) R_k (Rg_parent = I for the root), pose_k = the
//                axis-angle whose LAYER rotation is R_k: log R_k (so3.h) corrected for the layer's `+ 1e-8` (layer_axisang below);
//                betas += d_beta, trans += d_trans.  lambda_0 = 1e-2.
//   schedule     `iters` steps, iters + 1 evaluations, no early exit, no host read: every launch is decided by the arguments.
//
// Kernels.
//   k_smpl_fit_init    the default start (zero pose, zero betas, trans = centroid(target) - centroid(v_template), fp64 sums in a
//                      fixed order) or a copy of the caller's; lambda_0.
//   k_smpl_fit_normal  the hot path.  A workgroup owns one sample and one 512-vertex chunk and walks it in tiles of 64 vertices: v_posed,
//                      the four images, then the tile's 192 rows of [J | r] into LDS (row c 64 + v, leading dimension N + 1), then
//                      M += rows^T rows on v_mfma_f32_32x32x2_f32 (exact fp32 products, a fixed chain over the rows): wave w takes rows
//                      48 w .. 48 w + 47 into the upper 32x32 tiles of M, held in registers over the whole chunk.  The four waves'
//                      sums are added in order through LDS.
//   k_smpl_fit_reduce  adds the chunks' partial tiles in order into M [B,N,N] (the upper tiles; the rest is not written).
//   k_smpl_fit_solve   one wave per sample, fp64: the step above.
// Determinism: the chunking depends on NV alone, every sum has a fixed order and nothing is atomic, so row b is the same bits whatever
// the batch and from run to run.  No index is computed from device data: a non-finite target or start makes that sample's own outputs
// NaN (through its error, M[P][P]) and touches no other sample.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "internal.h"
#include "smpl_ctx.h"
#include "smpl_steps.h"
#include "so3.h"

namespace gator {
namespace {

constexpr int kFV = 64;             // vertices per tile
constexpr int kFC = 512;            // vertices per chunk: a multiple of the layer's vertex padding kTV
constexpr int kFRows = 3 * kFV;     // rows of [J | r] per tile, 48 per wave
constexpr int kFitMaxBatch = 65535;
constexpr double kLambda0 = 1e-2, kLambdaMin = 1e-9, kLambdaMax = 1e6, kRidge = 1e-12;

__host__ __device__ constexpr int fit_pairs(int nt) { return nt * (nt + 1) / 2; }

struct FitState {          // three arrays of one state, [B][3 NJ], [B][NB], [B][3]
    float *pose, *betas, *trans;
};

__global__ __launch_bounds__(256) void k_smpl_fit_init(const float* __restrict__ target, const float* __restrict__ ipose,
                                                       const float* __restrict__ ibetas, const float* __restrict__ itrans, int NV, int NJ,
                                                       int NB, double cx, double cy, double cz, FitState cand, double* __restrict__ scal) {
    __shared__ double red[256 * 3];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t == 0) { scal[(size_t)b * 4] = kLambda0; scal[(size_t)b * 4 + 1] = INFINITY; scal[(size_t)b * 4 + 2] = 0.0; scal[(size_t)b * 4 + 3] = 0.0; }
    if (ipose) {
        for (int i = t; i < NJ * 3; i += 256) cand.pose[(size_t)b * NJ * 3 + i] = ipose[(size_t)b * NJ * 3 + i];
        for (int i = t; i < NB; i += 256) cand.betas[(size_t)b * NB + i] = ibetas[(size_t)b * NB + i];
        if (t < 3) cand.trans[(size_t)b * 3 + t] = itrans[(size_t)b * 3 + t];
        return;
    }
    double s[3] = {0.0, 0.0, 0.0};
    const float* tg = target + (size_t)b * NV * 3;
    for (int v = t; v < NV; v += 256)
        for (int c = 0; c < 3; ++c) s[c] += (double)tg[(size_t)v * 3 + c];
    for (int c = 0; c < 3; ++c) red[c * 256 + t] = s[c];
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d)
            for (int c = 0; c < 3; ++c) red[c * 256 + t] += red[c * 256 + t + d];
        __syncthreads();
    }
    for (int i = t; i < NJ * 3; i += 256) cand.pose[(size_t)b * NJ * 3 + i] = 0.f;
    for (int i = t; i < NB; i += 256) cand.betas[(size_t)b * NB + i] = 0.f;
    if (t < 3) cand.trans[(size_t)b * 3 + t] = (float)(red[t * 256] / (double)NV - (t == 0 ? cx : t == 1 ? cy : cz));
}

// grid (S chunks, B samples).  part: [B][S][pairs][32][32], pair (ta <= tb) in the order (0,0) (0,1) .. (0,NT-1) (1,1) ..
template <int NT>
__global__ __launch_bounds__(256) void k_smpl_fit_normal(const float* __restrict__ basis, const float* __restrict__ vtempl,
                                                         const int32_t* __restrict__ widx, const float* __restrict__ wval,
                                                         const uint32_t* __restrict__ amask, int MI, const float* __restrict__ coef,
                                                         const float* __restrict__ xform, const float* __restrict__ joints,
                                                         const float* __restrict__ offs, const float* __restrict__ trans,
                                                         const float* __restrict__ target, int NV, int NVp, int NJ, int NB, int Kp, int P,
                                                         float* __restrict__ part) {
    constexpr int N = 32 * NT, ld = N + 1, NP = fit_pairs(NT);
    extern __shared__ float lds[];
    float* Jt = lds;                        // [192][ld]; after the chunk: the four waves' tiles [4][32][32]
    float* vpart = Jt;                      // [4][64][3]: the blend sum's quarters live in the rows' place until the rows are written
    float* xf = Jt + kFRows * ld;           // [NJ][12]
    float* pj = xf + NJ * 12;               // [NJ][3]
    float* cf = pj + NJ * 3;                // [Kp]
    float* img = cf + Kp;                   // [64][4][3]
    const int b = blockIdx.y, chunk = blockIdx.x, S = gridDim.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, col = lane & 31, hi = lane >> 5;
    for (int e = tid; e < NJ * 12; e += 256) xf[e] = xform[(size_t)b * NJ * 12 + e];
    for (int e = tid; e < NJ * 3; e += 256) pj[e] = joints[(size_t)b * NJ * 3 + e];
    for (int e = tid; e < Kp; e += 256) cf[e] = coef[(size_t)b * Kp + e];
    const float t0 = trans[(size_t)b * 3], t1 = trans[(size_t)b * 3 + 1], t2 = trans[(size_t)b * 3 + 2];
    const float o0 = offs[(size_t)b * 4], o1 = offs[(size_t)b * 4 + 1], o2 = offs[(size_t)b * 4 + 2];      // 0, or NaN for a non-finite pose / beta
    const size_t plane = (size_t)Kp * NVp;
    f32x16 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = f32x16{0};
    __syncthreads();
    const int items = kFV * (NJ + NB + 1);
    for (int tile = 0; tile < kFC / kFV; ++tile) {
        const int v0 = chunk * kFC + tile * kFV;           // < NVp whenever < NV: the planes are padded to kTV, which kFV and kFC divide
        if (v0 >= NV) break;
        const int vl = lane, v = v0 + vl;
        {   // a quarter of the blend sum per wave
            const int kq = Kp / 4;                          // Kp is a multiple of 16
            const float* bp = basis + (size_t)(wave * kq) * NVp + v;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int k = 0; k < kq; ++k) {
                const float c = cf[wave * kq + k];
                s0 = fmaf(c, bp[(size_t)k * NVp], s0);
                s1 = fmaf(c, bp[(size_t)k * NVp + plane], s1);
                s2 = fmaf(c, bp[(size_t)k * NVp + 2 * plane], s2);
            }
            float* o = vpart + (wave * kFV + vl) * 3;
            o[0] = s0; o[1] = s1; o[2] = s2;
        }
        __syncthreads();
        {   // wave m: influence m's image of every vertex of the tile
            float vp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                vp[c] = vtempl[(size_t)c * NVp + v] + (((vpart[vl * 3 + c] + vpart[(kFV + vl) * 3 + c]) + vpart[(2 * kFV + vl) * 3 + c]) + vpart[(3 * kFV + vl) * 3 + c]);
            const int m = wave;
            const float* A = xf + (m < MI ? widx[(size_t)m * NVp + v] : 0) * 12;
            smpl_affine(A, vp[0], vp[1], vp[2], img + (vl * 4 + m) * 3);
        }
        __syncthreads();
        for (int it = tid; it < items; it += 256) {         // 64 consecutive items share the column group c: uniform in a wave
            const int c = it >> 6;
            const bool valid = v < NV;
            float w[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) w[m] = m < MI ? wval[(size_t)m * NVp + v] : 0.f;
            const float* im = img + vl * 12;
            float* row0 = Jt + vl * ld;
            float* row1 = row0 + kFV * ld;
            float* row2 = row1 + kFV * ld;
            if (c < NJ) {
                const float px = pj[c * 3], py = pj[c * 3 + 1], pz = pj[c * 3 + 2];
                float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint32_t mask = m < MI ? amask[(size_t)m * NVp + v] : 0u;
                    if ((mask >> c) & 1u) {
                        cx = fmaf(w[m], im[m * 3] - px, cx);
                        cy = fmaf(w[m], im[m * 3 + 1] - py, cy);
                        cz = fmaf(w[m], im[m * 3 + 2] - pz, cz);
                    }
                }
                if (!valid) cx = cy = cz = 0.f;
                const int q = c * 3;                         // -[c]x
                row0[q] = 0.f;  row0[q + 1] = cz;  row0[q + 2] = -cy;
                row1[q] = -cz;  row1[q + 1] = 0.f; row1[q + 2] = cx;
                row2[q] = cy;   row2[q + 1] = -cx; row2[q + 2] = 0.f;
            } else if (c < NJ + NB) {
                const int bi = c - NJ;
                float Rb[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) Rb[e] = 0.f;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float* A = xf + (m < MI ? widx[(size_t)m * NVp + v] : 0) * 12;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int k = 0; k < 3; ++k) Rb[r * 3 + k] = fmaf(w[m], A[r * 4 + k], Rb[r * 3 + k]);
                }
                const float* sp = basis + (size_t)bi * NVp + v;
                const float s0 = sp[0], s1 = sp[plane], s2 = sp[2 * plane];
                const int q = NJ * 3 + bi;
                row0[q] = valid ? fmaf(Rb[0], s0, fmaf(Rb[1], s1, Rb[2] * s2)) : 0.f;
                row1[q] = valid ? fmaf(Rb[3], s0, fmaf(Rb[4], s1, Rb[5] * s2)) : 0.f;
                row2[q] = valid ? fmaf(Rb[6], s0, fmaf(Rb[7], s1, Rb[8] * s2)) : 0.f;
            } else {                                          // translation, the residual, the padding
                const int q = NJ * 3 + NB;
                const float one = valid ? 1.f : 0.f;
                row0[q] = one; row0[q + 1] = 0.f; row0[q + 2] = 0.f;
                row1[q] = 0.f; row1[q + 1] = one; row1[q + 2] = 0.f;
                row2[q] = 0.f; row2[q + 1] = 0.f; row2[q + 2] = one;
                float x[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) x[r] = fmaf(w[3], im[9 + r], fmaf(w[2], im[6 + r], fmaf(w[1], im[3 + r], w[0] * im[r])));
                const float* tg = target + ((size_t)b * NV + (valid ? v : 0)) * 3;
                row0[P] = valid ? ((x[0] + t0) - tg[0]) + o0 : 0.f;
                row1[P] = valid ? ((x[1] + t1) - tg[1]) + o1 : 0.f;
                row2[P] = valid ? ((x[2] + t2) - tg[2]) + o2 : 0.f;
                for (int k = P + 1; k < N; ++k) { row0[k] = 0.f; row1[k] = 0.f; row2[k] = 0.f; }
            }
        }
        __syncthreads();
        const float* rp = Jt + (wave * (kFRows / 4) + hi) * ld + col;
#pragma unroll 4
        for (int ks = 0; ks < kFRows / 8; ++ks) {            // two rows per MFMA: lane (col, hi) feeds row 2 ks + hi
            float val[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) val[t] = rp[ks * 2 * ld + t * 32];
            int p = 0;
#pragma unroll
            for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                for (int tb = ta; tb < NT; ++tb, ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(val[ta], val[tb], acc[p], 0, 0, 0);
        }
        __syncthreads();                                     // the next tile's blend quarters overwrite the rows
    }
    float* out = part + ((size_t)b * S + chunk) * NP * 1024;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            Jt[wave * 1024 + mfma32_row(r, hi) * 32 + col] = acc[p][r];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            out[(size_t)p * 1024 + e] = ((Jt[e] + Jt[1024 + e]) + Jt[2048 + e]) + Jt[3072 + e];
        }
        __syncthreads();
    }
}

// grid (pairs, B), 256 threads: M[b][32 ta + i][32 tb + j] = sum over the chunks, in order
__global__ __launch_bounds__(256) void k_smpl_fit_reduce(const float* __restrict__ part, int S, int NT, float* __restrict__ M) {
    const int b = blockIdx.y, p = blockIdx.x, NP = gridDim.x, N = NT * 32;
    int ta = 0, rest = p;
    while (rest >= NT - ta) { rest -= NT - ta; ++ta; }
    const int tb = ta + rest;
    for (int e = threadIdx.x; e < 1024; e += 256) {
        const float* src = part + ((size_t)b * S * NP + p) * 1024 + e;
        float s = src[0];
        for (int c = 1; c < S; ++c) s += src[(size_t)c * NP * 1024];
        M[((size_t)b * N + ta * 32 + (e >> 5)) * N + tb * 32 + (e & 31)] = s;
    }
}

// The axis-angle a whose LAYER rotation is exp(rho).  The layer takes the angle as |a + 1e-8| and normalises the quaternion
// (cos h, sin h . a / |a + 1e-8|), h = |a + 1e-8| / 2: its rotation of a has a's axis and the angle
// theta(a) = 2 atan2(sin h |a| / |a + 1e-8|, cos h), off |a| by up to ~1e-8.  One fixed-point step, a = rho (2 |rho| - theta(rho)) / |rho|,
// leaves an error of the order 1e-16; without it every step would carry 1e-8 rad into the next evaluation.
__device__ void layer_axisang(const double rho[3], double a[3]) {
    const double n = sqrt(rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2]);
    if (n == 0.0) { a[0] = a[1] = a[2] = 0.0; return; }
    const double ex = rho[0] + 1e-8, ey = rho[1] + 1e-8, ez = rho[2] + 1e-8;
    const double al = sqrt(ex * ex + ey * ey + ez * ez);
    const double theta = 2.0 * atan2(sin(al * 0.5) * n / al, cos(al * 0.5));
    const double k = (2.0 * n - theta) / n;
    a[0] = rho[0] * k; a[1] = rho[1] * k; a[2] = rho[2] * k;
}

// One wave per sample.  LDS (dynamic): the packed lower triangle of the damped H / its Cholesky factor, the right-hand side,
// the local and the global rotations of the current state.
__global__ __launch_bounds__(64) void k_smpl_fit_solve(const float* __restrict__ Mcand, float* __restrict__ Mcur, FitState cand, FitState cur,
                                                       double* __restrict__ scal, const int32_t* __restrict__ parents, int NV, int NJ, int NB,
                                                       int P, int N, int first, int last, float* __restrict__ out_pose,
                                                       float* __restrict__ out_betas, float* __restrict__ out_trans, float* __restrict__ out_rms) {
    extern __shared__ double sm[];
    double* L = sm;                                  // [P (P + 1) / 2], row i at i (i + 1) / 2
    double* rhs = L + P * (P + 1) / 2;               // [P]
    double* R = rhs + P;                             // [NJ][9]
    double* Rg = R + NJ * 9;                         // [NJ][9]
    const int b = blockIdx.x, t = threadIdx.x, NP3 = NJ * 3;
    const float* Mc = Mcand + (size_t)b * N * N;
    float* Mu = Mcur + (size_t)b * N * N;
    float* cp = cand.pose + (size_t)b * NP3;  float* cb = cand.betas + (size_t)b * NB;  float* ct = cand.trans + (size_t)b * 3;
    float* up = cur.pose + (size_t)b * NP3;   float* ub = cur.betas + (size_t)b * NB;   float* ut = cur.trans + (size_t)b * 3;
    double lam = scal[(size_t)b * 4], err = scal[(size_t)b * 4 + 1];
    bool bad = scal[(size_t)b * 4 + 2] != 0.0;
    const double e = (double)Mc[(size_t)P * N + P];
    bool accept;
    if (first) {
        bad = !isfinite(e);
        accept = true;
    } else {
        accept = e < err;
        lam = accept ? fmax(lam * 0.25, kLambdaMin) : fmin(lam * 8.0, kLambdaMax);
    }
    if (accept) {
        err = e;
        for (int i = t; i < NP3; i += 64) up[i] = cp[i];
        for (int i = t; i < NB; i += 64) ub[i] = cb[i];
        if (t < 3) ut[t] = ct[t];
        for (int i = t; i < (P + 1) * N; i += 64) Mu[i] = Mc[i];          // rows 0 .. P hold H, g and the error
    }
    __syncthreads();
    if (last) {
        const float nan = __builtin_nanf("");
        for (int i = t; i < NP3; i += 64) out_pose[(size_t)b * NP3 + i] = bad ? nan : up[i];
        for (int i = t; i < NB; i += 64) out_betas[(size_t)b * NB + i] = bad ? nan : ub[i];
        if (t < 3) out_trans[(size_t)b * 3 + t] = bad ? nan : ut[t];
        if (t == 0) out_rms[b] = bad ? nan : (float)sqrt(err / (double)NV);
        return;
    }
    // the damped system from the upper triangle of the current M: H[i][j] = M[j][i] for j <= i
    for (int e = t; e < P * N; e += 64) {            // rows of M in order: coalesced, independent loads
        const int j = e / N, i = e - j * N;
        if (i < j || i >= P) continue;
        const double h = (double)Mu[e];
        L[i * (i + 1) / 2 + j] = j == i ? (h + lam * h) + kRidge : h;
    }
    for (int i = t; i < P; i += 64) rhs[i] = -(double)Mu[(size_t)i * N + P];
    __syncthreads();
    bool fail = bad;
    for (int j = 0; j < P && !fail; ++j) {           // left-looking Cholesky, column by column
        const double* Lj = L + j * (j + 1) / 2;
        for (int i = j + t; i < P; i += 64) {
            double* Li = L + i * (i + 1) / 2;
            double s = Li[j];
#pragma unroll 8
            for (int k = 0; k < j; ++k) s -= Li[k] * Lj[k];      // one chain in k order; unrolled so that the LDS reads run ahead of it
            Li[j] = s;
        }
        __syncthreads();
        const double d = Lj[j];
        __syncthreads();
        if (!(d > 0.0) || !isfinite(d)) { fail = true; break; }           // uniform: every lane reads the same pivot
        const double sd = sqrt(d);
        for (int i = j + t; i < P; i += 64) {
            double* Li = L + i * (i + 1) / 2;
            Li[j] = i == j ? sd : Li[j] / sd;
        }
        __syncthreads();
    }
    if (fail) {
        lam = fmin(lam * 8.0, kLambdaMax);
        for (int i = t; i < P; i += 64) rhs[i] = 0.0;
        __syncthreads();
    } else {
        for (int i = 0; i < P; ++i) {                // L y = rhs, column-oriented
            const double y = rhs[i] / L[i * (i + 1) / 2 + i];
            __syncthreads();
            for (int k = i + 1 + t; k < P; k += 64) rhs[k] -= L[k * (k + 1) / 2 + i] * y;
            if (t == 0) rhs[i] = y;
            __syncthreads();
        }
        for (int i = P - 1; i >= 0; --i) {           // L^T d = y
            const double* Li = L + i * (i + 1) / 2;
            const double x = rhs[i] / Li[i];
            __syncthreads();
            for (int k = t; k < i; k += 64) rhs[k] -= Li[k] * x;
            if (t == 0) rhs[i] = x;
            __syncthreads();
        }
    }
    // the rotations of the current state, then the candidate
    if (t < NJ) smpl_rodrigues((double)up[t * 3], (double)up[t * 3 + 1], (double)up[t * 3 + 2], R + t * 9);
    __syncthreads();
    for (int j = 0; j < NJ; ++j) {                   // parents[j] < j
        if (t < 9) {
            if (j == 0) {
                Rg[t] = R[t];
            } else {
                const double* gp = Rg + parents[j] * 9 + (t / 3) * 3;
                const double* rj = R + j * 9 + (t % 3);
                Rg[j * 9 + t] = (gp[0] * rj[0] + gp[1] * rj[3]) + gp[2] * rj[6];
            }
        }
        __syncthreads();
    }
    if (t < NJ) {
        double dl[3], E[3][3], Rn[3][3], rho[3], a[3];
        const double* d = rhs + t * 3;
        if (t == 0) {
            dl[0] = d[0]; dl[1] = d[1]; dl[2] = d[2];
        } else {
            const double* gp = Rg + parents[t] * 9;
#pragma unroll
            for (int c = 0; c < 3; ++c) dl[c] = (gp[c] * d[0] + gp[3 + c] * d[1]) + gp[6 + c] * d[2];      // Rg_parent^T d
        }
        rotvec_exp(dl, E);
        const double* r = R + t * 9;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rn[i][j] = (E[i][0] * r[j] + E[i][1] * r[3 + j]) + E[i][2] * r[6 + j];
        rotmat_log(Rn, rho);
        layer_axisang(rho, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) cp[t * 3 + c] = (float)a[c];
    }
    for (int i = t; i < NB; i += 64) cb[i] = (float)((double)ub[i] + rhs[NP3 + i]);
    if (t < 3) ct[t] = (float)((double)ut[t] + rhs[NP3 + NB + t]);
    if (t == 0) { scal[(size_t)b * 4] = lam; scal[(size_t)b * 4 + 1] = err; scal[(size_t)b * 4 + 2] = bad ? 1.0 : 0.0; }
}

size_t normal_lds_bytes(const gator_smpl* c, int NT) {
    return sizeof(float) * ((size_t)kFRows * (32 * NT + 1) + (size_t)c->NJ * 15 + c->Kp + kFV * 12);      // SMPL: 79 904 bytes, two workgroups per CU
}

// P unknowns, NT = N / 32 column tiles of [J | r], S chunks of the vertex range
void fit_sizes(const gator_smpl* c, int* P, int* NT, int* S) {
    *P = 3 * c->NJ + c->NB + 3;
    *NT = (*P + 1 + 31) / 32;
    *S = (c->NV + kFC - 1) / kFC;
}

FitState fit_state(const gator_smpl* c, int which) {
    int P, NT, S;
    fit_sizes(c, &P, &NT, &S);
    float* base = c->fstate.get() + (size_t)which * c->fcap * P;
    return FitState{base, base + (size_t)c->fcap * c->NJ * 3, base + (size_t)c->fcap * (c->NJ * 3 + c->NB)};
}

int fit_reserve(gator_smpl* c, int B) {
    GATOR_TRY(smpl_reserve(c, B));
    if (B <= c->fcap) return GATOR_OK;
    c->fcap = 0;
    int P, NT, S;
    fit_sizes(c, &P, &NT, &S);
    const size_t N = 32 * (size_t)NT;
    GATOR_TRY(c->grow(c->fjoints, (size_t)B * c->NJ * 3));
    GATOR_TRY(c->grow(c->fstate, 2 * (size_t)B * P));
    GATOR_TRY(c->grow(c->fscal, (size_t)B * 4));
    GATOR_TRY(c->grow(c->fpart, (size_t)B * S * fit_pairs(NT) * 1024));
    GATOR_TRY(c->grow(c->fM, 2 * (size_t)B * N * N));
    c->fcap = B;
    return GATOR_OK;
}

template <int NT>
int launch_normal(gator_smpl* c, const float* trans, const float* target, int batch, int S, int P, hipStream_t st) {
    k_smpl_fit_normal<NT><<<dim3(S, batch), 256, normal_lds_bytes(c, NT), st>>>(c->basis, c->vtempl, c->widx, c->wval, c->amask, c->MI, c->coef, c->xform,
                                                                                 c->fjoints, c->offs, trans, target, c->NV, c->NVp, c->NJ, c->NB,
                                                                                 c->Kp, P, c->fpart);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

// the candidate's M: the pose stage, the chunks' partial tiles, their sum
int fit_normal(gator_smpl* c, const float* pose, const float* betas, const float* trans, const float* target, int batch, float* M, hipStream_t st) {
    int P, NT, S;
    fit_sizes(c, &P, &NT, &S);
    GATOR_TRY(smpl_pose_stage(c, pose, betas, nullptr, batch, -1, 1.0, c->fjoints, st));
    switch (NT) {
        case 1: GATOR_TRY(launch_normal<1>(c, trans, target, batch, S, P, st)); break;
        case 2: GATOR_TRY(launch_normal<2>(c, trans, target, batch, S, P, st)); break;
        case 3: GATOR_TRY(launch_normal<3>(c, trans, target, batch, S, P, st)); break;
        default: GATOR_TRY(launch_normal<4>(c, trans, target, batch, S, P, st)); break;
    }
    k_smpl_fit_reduce<<<dim3(fit_pairs(NT), batch), 256, 0, st>>>(c->fpart, S, NT, M);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

int fit_common_checks(const char* who, gator_smpl* ctx, int batch) {
    GATOR_TRY(smpl_check_batch(who, ctx, batch, kFitMaxBatch));
    if (ctx->MI > 4)
        return fail(GATOR_EUNSUPPORTED, "%s: the model has up to %d influences per vertex, the fit supports at most 4", who, ctx->MI);
    return GATOR_OK;
}
}  // namespace

int smpl_fit_build(gator_smpl* c, const gator_smpl_model* m) {
    const int NV = c->NV, NJ = c->NJ, NVp = c->NVp;
    double s[3] = {0.0, 0.0, 0.0};
    for (int v = 0; v < NV; ++v)
        for (int x = 0; x < 3; ++x) s[x] += (double)m->v_template[(size_t)v * 3 + x];
    for (int x = 0; x < 3; ++x) c->tcen[x] = s[x] / NV;
    if (c->MI > 4) return GATOR_OK;                             // the fit refuses such a model; the layer takes it
    std::vector<uint32_t> anc(NJ, 0u);                          // bit k of anc[j]: k is j or an ancestor of j
    for (int j = 0; j < NJ; ++j) anc[j] = (1u << j) | (j ? anc[m->parents[j]] : 0u);
    std::vector<uint32_t> am((size_t)c->MI * NVp, 0u);
    for (int v = 0; v < NV; ++v) {
        int n = 0;
        for (int j = 0; j < NJ; ++j)
            if (m->weights[(size_t)v * NJ + j] != 0.f) am[(size_t)(n++) * NVp + v] = anc[j];      // the order of widx / wval
    }
    GATOR_TRY(upload(c->amask, am));
    int P, NT, S;
    fit_sizes(c, &P, &NT, &S);
    const int lds = (int)normal_lds_bytes(c, NT);
    const void* fn = NT == 1 ? (const void*)k_smpl_fit_normal<1> : NT == 2 ? (const void*)k_smpl_fit_normal<2>
                   : NT == 3 ? (const void*)k_smpl_fit_normal<3> : (const void*)k_smpl_fit_normal<4>;
    GATOR_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return GATOR_OK;
}
}  // namespace gator

extern "C" int gator_smpl_fit_width(const gator_smpl* ctx, int32_t* P, int32_t* N) {
    using namespace gator;
    if (!ctx) return fail(GATOR_EINVAL, "gator_smpl_fit_width: null ctx");
    int p, nt, s;
    fit_sizes(ctx, &p, &nt, &s);
    if (P) *P = p;
    if (N) *N = 32 * nt;
    return GATOR_OK;
}

extern "C" int gator_smpl_fit_normal_f32(gator_smpl* ctx, const float* pose, const float* betas, const float* trans, const float* target_verts,
                                         int32_t batch, float* out_M, void* stream) {
    using namespace gator;
    GATOR_TRY(fit_common_checks("gator_smpl_fit_normal_f32", ctx, batch));
    if (!pose || !trans || !target_verts || !out_M || (ctx->NB > 0 && !betas))
        return fail(GATOR_EINVAL, "gator_smpl_fit_normal_f32: pose, betas, trans, target_verts and out_M must not be NULL");
    if (batch == 0) return GATOR_OK;
    GATOR_TRY(fit_reserve(ctx, batch));
    return fit_normal(ctx, pose, betas, trans, target_verts, batch, out_M, (hipStream_t)stream);
}

extern "C" int gator_smpl_fit_f32(gator_smpl* ctx, const float* target_verts, const float* init_pose, const float* init_betas,
                                  const float* init_trans, int32_t batch, int32_t iters, float* out_pose, float* out_betas, float* out_trans,
                                  float* out_rms, void* stream) {
    using namespace gator;
    GATOR_TRY(fit_common_checks("gator_smpl_fit_f32", ctx, batch));
    if (!target_verts || !out_pose || !out_trans || !out_rms || (ctx->NB > 0 && !out_betas))
        return fail(GATOR_EINVAL, "gator_smpl_fit_f32: target_verts, out_pose, out_betas, out_trans and out_rms must not be NULL");
    if (iters < 1 || iters > 256) return fail(GATOR_EINVAL, "gator_smpl_fit_f32: iters %d outside 1..256", iters);
    const bool any = init_pose || init_trans || (ctx->NB > 0 && init_betas);
    const bool all = init_pose && init_trans && (ctx->NB == 0 || init_betas);
    if (any && !all) return fail(GATOR_EINVAL, "gator_smpl_fit_f32: init_pose, init_betas and init_trans are NULL together or set together");
    if (batch == 0) return GATOR_OK;
    GATOR_TRY(fit_reserve(ctx, batch));
    hipStream_t st = (hipStream_t)stream;
    int P, NT, S;
    fit_sizes(ctx, &P, &NT, &S);
    const int N = 32 * NT;
    const FitState cand = fit_state(ctx, 0), cur = fit_state(ctx, 1);
    float* Mcand = ctx->fM.get();
    float* Mcur = Mcand + (size_t)ctx->fcap * N * N;
    k_smpl_fit_init<<<batch, 256, 0, st>>>(target_verts, all ? init_pose : nullptr, init_betas, init_trans, ctx->NV, ctx->NJ, ctx->NB, ctx->tcen[0],
                                           ctx->tcen[1], ctx->tcen[2], cand, ctx->fscal);
    GATOR_HIP_CHECK(hipGetLastError());
    const size_t lds = sizeof(double) * ((size_t)P * (P + 1) / 2 + P + (size_t)ctx->NJ * 18);
    for (int i = 0; i <= iters; ++i) {
        GATOR_TRY(fit_normal(ctx, cand.pose, cand.betas, cand.trans, target_verts, batch, Mcand, st));
        k_smpl_fit_solve<<<batch, 64, lds, st>>>(Mcand, Mcur, cand, cur, ctx->fscal, ctx->parents, ctx->NV, ctx->NJ, ctx->NB, P, N, i == 0, i == iters,
                                                 out_pose, out_betas, out_trans, out_rms);
        GATOR_HIP_CHECK(hipGetLastError());
    }
    return GATOR_OK;
}
