// The SMPL body-model layer (smplpytorch/pytorch/smpl_layer.py:65-158, rodrigues_layer.py:13-52) on the device, batched:
//   (pose [B,NJ*3], betas [B,NB], trans [B,3]) -> (verts [B,NV,3], joints [B,NJ,3])
// in two launches and without the layer's per-vertex intermediates (th_T [B,4,4,NV], v_shaped, v_posed never exist in memory).
//   k_smpl_pose : one wave per sample, fp64.  Rodrigues with the reference's `+ 1e-8` inside the norm and its normalised quaternion,
//                 the pose map R[1:] - I, the shaped rest joints from the regressor folded at create, the kinematic chain; writes the
//                 sample's coefficient row [betas ; pose map], its NJ skinning transforms (3x4, fp32), its offset and the joints.
//   k_smpl_skin : the hot path.  Per (32-sample, 128-vertex) tile the blend offsets [32 x K] . [K x 3 x 128] on the fp32-input MFMA
//                 (v_mfma_f32_32x32x2_f32: exact fp32 products, a fixed fmaf chain over k), the three coordinate planes of the basis as
//                 three accumulators, so that a lane holds x, y, z of one vertex for 16 samples; then, in registers, T = sum w A over the
//                 vertex's (index, weight) list with the tile's transforms in LDS, T . [v_posed ; 1], offset, scale, store.
// A sample is one MFMA row and one LDS row from end to end: its result depends on no other sample of the batch, and a non-finite
// pose or beta makes every output of its own sample non-finite and touches no other.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "internal.h"
#include "smpl_ctx.h"

namespace gator {
namespace {

constexpr int kTS = 32;      // samples per tile: the M of one 32x32x2 MFMA
constexpr int kKU = 4;      // k-pairs per pipeline stage of the blend GEMM: K is padded to two stages, 4 kKU
constexpr int kCoefLd = 33;  // LDS leading dimension of the transposed coefficient tile (conflict-free both ways)

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(64) void k_smpl_pose(const float* __restrict__ pose, const float* __restrict__ betas, const float* __restrict__ trans,
                                                  const double* __restrict__ jfold, const int32_t* __restrict__ parents, int NJ, int NB, int K,
                                                  int Kp, int center, double out_scale, float* __restrict__ coef, float* __restrict__ xform,
                                                  float* __restrict__ offs, float* __restrict__ joints) {
    __shared__ double R[kSmplMaxJ * 9], J[kSmplMaxJ * 3], G[kSmplMaxJ * 12];
    const int b = blockIdx.x, t = threadIdx.x;
    float* cf = coef + (size_t)b * Kp;
    double poison = 0.0;                 // 0, or NaN when any pose or beta entry of the sample is not finite (x * 0 keeps NaN, turns Inf into NaN)
    for (int k = t; k < NB; k += 64) {
        cf[k] = betas ? betas[(size_t)b * NB + k] : 0.f;
        poison += (double)cf[k] * 0.0;
    }
    for (int k = K + t; k < Kp; k += 64) cf[k] = 0.f;
    if (t < NJ) {
        const float* a = pose + ((size_t)b * NJ + t) * 3;
        const double ax = a[0], ay = a[1], az = a[2];
        poison += (ax + ay + az) * 0.0;
        double* r = R + t * 9;
        smpl_rodrigues(ax, ay, az, r);
        if (t >= 1)
            for (int e = 0; e < 9; ++e) cf[NB + (t - 1) * 9 + e] = (float)(r[e] - ((e & 3) == 0 ? 1.0 : 0.0));      // subtract_flat_id
        for (int c = 0; c < 3; ++c) {
            const double* f = jfold + (size_t)(t * 3 + c) * (1 + NB);
            double acc = f[0];
            if (betas)
                for (int k = 0; k < NB; ++k) acc += f[1 + k] * (double)betas[(size_t)b * NB + k];
            J[t * 3 + c] = acc;
        }
    }
    __syncthreads();
    // the chain, joint by joint (parents[j] < j); lane e < 12 owns entry (row, col) of the 3x4 global transform
    const int row = (t & 15) >> 2, col = t & 3;
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
    // A non-finite root rotation leaves the root joint finite and a non-finite elbow its ancestors (the reference's behaviour); here the
    // whole sample is marked instead: the flag, summed over the wave, rides on the offset that every joint and vertex receives.
    for (int d = 32; d > 0; d >>= 1) poison += __shfl_xor(poison, d);
    double off[3];
    for (int c = 0; c < 3; ++c) off[c] = poison + (trans ? (double)trans[(size_t)b * 3 + c] : 0.0) - (center >= 0 ? G[center * 12 + c * 4 + 3] : 0.0);
    if (t < 4) offs[(size_t)b * 4 + t] = (float)(t == 0 ? off[0] : t == 1 ? off[1] : t == 2 ? off[2] : 0.0);
    if (t < NJ) {
        const double* g = G + t * 12;
        float* o = xform + ((size_t)b * NJ + t) * 12;
        for (int r = 0; r < 3; ++r) {
            double tr = g[r * 4 + 3];
            if (joints) joints[((size_t)b * NJ + t) * 3 + r] = (float)((tr + off[r]) * out_scale);
            for (int c = 0; c < 3; ++c) { o[r * 4 + c] = (float)g[r * 4 + c]; tr -= g[r * 4 + c] * J[t * 3 + c]; }
            o[r * 4 + 3] = (float)tr;                                                // G.t - G.R . J
        }
    }
}

// MI_T = 4: at most four influences per vertex (SMPL, MANO), held in registers; MI_T = 0: any number, read per sample from the lists
template <int MI_T>
__global__ __launch_bounds__(256) void k_smpl_skin(const float* __restrict__ basis, const float* __restrict__ vtempl, const int32_t* __restrict__ widx,
                                                   const float* __restrict__ wval, int MI, const float* __restrict__ coef,
                                                   const float* __restrict__ xform, const float* __restrict__ offs, int B, int NV, int NVp,
                                                   int NJ, int Kp, float out_scale, float* __restrict__ verts) {
    extern __shared__ float lds[];
    const int s0 = blockIdx.y * kTS, v0 = blockIdx.x * kTV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, hi = lane >> 5;
    const int ns = min(kTS, B - s0);
    for (int e = threadIdx.x; e < kTS * Kp; e += 256) {                 // the tile's coefficient rows, transposed: lds[k][sample]
        const int s = e / Kp, k = e - s * Kp;
        lds[k * kCoefLd + s] = s < ns ? coef[(size_t)(s0 + s) * Kp + k] : 0.f;
    }
    __syncthreads();
    const int v = v0 + wave * 32 + col;                                 // < NVp: the planes are padded to whole tiles
    const size_t plane = (size_t)Kp * NVp;
    const float* bp = basis + v;
    f32x16 ax = {0}, ay = {0}, az = {0};
    // A[i = sample][k], B[k][j = vertex]: lane (col, hi) feeds k + hi.  A stage is kKU k-pairs = twelve MFMAs; two register sets
    // take turns, each loaded a whole stage (768 cycles of matrix work) before it is used.
    float pa[kKU], px_[kKU], py_[kKU], pz_[kKU], qa[kKU], qx[kKU], qy[kKU], qz[kKU];
    auto fetch = [&](int k, float (&a)[kKU], float (&x)[kKU], float (&y)[kKU], float (&z)[kKU]) {
#pragma unroll
        for (int u = 0; u < kKU; ++u) {
            const int kk = k + 2 * u + hi;
            const size_t o = (size_t)kk * NVp;
            a[u] = lds[kk * kCoefLd + col];
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
    fetch(0, pa, px_, py_, pz_);
    for (int k = 0; k < Kp; k += 4 * kKU) {                              // Kp is a multiple of two stages
        fetch(k + 2 * kKU, qa, qx, qy, qz);
        __builtin_amdgcn_sched_barrier(0);                              // keep the loads ahead of the stage they overlap
        mma(pa, px_, py_, pz_);
        __builtin_amdgcn_sched_barrier(0);
        fetch(min(k + 4 * kKU, Kp - 2 * kKU), pa, px_, py_, pz_);       // after the last stage: an in-bounds fetch nobody uses
        __builtin_amdgcn_sched_barrier(0);
        mma(qa, qx, qy, qz);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                                    // the coefficient tile is done with: the transforms take its place
    const int nxf = ns * NJ * 12;
    const float* xs = xform + (size_t)s0 * NJ * 12;
    for (int e = threadIdx.x; e < nxf; e += 256) lds[e] = xs[e];
    float* lo = lds + kTS * NJ * 12;
    if (threadIdx.x < kTS * 4) lo[threadIdx.x] = (int)threadIdx.x < ns * 4 ? offs[(size_t)s0 * 4 + threadIdx.x] : 0.f;
    __syncthreads();
    if (v >= NV) return;
    const float tx = vtempl[v], ty = vtempl[NVp + v], tz = vtempl[2 * NVp + v];
    int ji[MI_T ? MI_T : 1];
    float jw[MI_T ? MI_T : 1];
    if constexpr (MI_T > 0) {
#pragma unroll
        for (int m = 0; m < MI_T; ++m) {
            ji[m] = m < MI ? widx[(size_t)m * NVp + v] * 12 : 0;
            jw[m] = m < MI ? wval[(size_t)m * NVp + v] : 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;                  // C/D map of the 32x32 MFMA: register r of lane (col, hi) is row i
        if (i >= ns) continue;
        const float* xi = lds + i * NJ * 12;
        float T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = 0.f;
        if constexpr (MI_T > 0) {
#pragma unroll
            for (int m = 0; m < MI_T; ++m) {
                const float4* q = reinterpret_cast<const float4*>(xi + ji[m]);
                const float4 q0 = q[0], q1 = q[1], q2 = q[2];
                const float qq[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
                for (int e = 0; e < 12; ++e) T[e] = fmaf(jw[m], qq[e], T[e]);
            }
        } else {
            for (int m = 0; m < MI; ++m) {
                const float w = wval[(size_t)m * NVp + v];
                const float4* q = reinterpret_cast<const float4*>(xi + widx[(size_t)m * NVp + v] * 12);
                const float4 q0 = q[0], q1 = q[1], q2 = q[2];
                const float qq[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
                for (int e = 0; e < 12; ++e) T[e] = fmaf(w, qq[e], T[e]);
            }
        }
        const float px = tx + ax[r], py = ty + ay[r], pz = tz + az[r];   // v_posed = v_template + blend offsets
        const float x = fmaf(T[0], px, fmaf(T[1], py, fmaf(T[2], pz, T[3])));
        const float y = fmaf(T[4], px, fmaf(T[5], py, fmaf(T[6], pz, T[7])));
        const float z = fmaf(T[8], px, fmaf(T[9], py, fmaf(T[10], pz, T[11])));
        float* o = verts + ((size_t)(s0 + i) * NV + v) * 3;             // 32 lanes x 12 bytes: 384 contiguous bytes per sample
        o[0] = (x + lo[i * 4]) * out_scale;
        o[1] = (y + lo[i * 4 + 1]) * out_scale;
        o[2] = (z + lo[i * 4 + 2]) * out_scale;
    }
}

size_t skin_lds_bytes(const gator_smpl* c) {
    const size_t a = (size_t)c->Kp * kCoefLd, b = (size_t)kTS * c->NJ * 12 + kTS * 4;
    return sizeof(float) * (a > b ? a : b);
}

template <class T> int upload(DevBuf<T>& d, const std::vector<T>& h) {
    GATOR_TRY(d.alloc(sizeof(T) * (h.empty() ? 1 : h.size())));
    if (!h.empty()) GATOR_HIP_CHECK(hipMemcpy(d.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return GATOR_OK;
}

int smpl_build(gator_smpl* c, const gator_smpl_model* m) {
    const int NV = c->NV, NJ = c->NJ, NB = c->NB, NP = (NJ - 1) * 9, Kp = c->Kp, NVp = c->NVp;
    std::vector<float> basis((size_t)3 * Kp * NVp, 0.f), vt((size_t)3 * NVp, 0.f);
    for (int v = 0; v < NV; ++v)
        for (int x = 0; x < 3; ++x) {
            vt[(size_t)x * NVp + v] = m->v_template[(size_t)v * 3 + x];
            float* b = basis.data() + (size_t)x * Kp * NVp + v;
            for (int k = 0; k < NB; ++k) b[(size_t)k * NVp] = m->shapedirs[((size_t)v * 3 + x) * NB + k];
            for (int k = 0; k < NP; ++k) b[(size_t)(NB + k) * NVp] = m->posedirs[((size_t)v * 3 + x) * NP + k];
        }
    int MI = 1;
    for (int v = 0; v < NV; ++v) {
        int n = 0;
        for (int j = 0; j < NJ; ++j) n += m->weights[(size_t)v * NJ + j] != 0.f;
        MI = n > MI ? n : MI;
    }
    c->MI = MI;
    std::vector<int32_t> wi((size_t)MI * NVp, 0);
    std::vector<float> ww((size_t)MI * NVp, 0.f);
    for (int v = 0; v < NV; ++v) {
        int n = 0;
        for (int j = 0; j < NJ; ++j) {
            const float w = m->weights[(size_t)v * NJ + j];
            if (w != 0.f) { wi[(size_t)n * NVp + v] = j; ww[(size_t)n * NVp + v] = w; ++n; }
        }
    }
    // J = J_regressor . (v_template + shapedirs . betas) is linear in betas: fold the regressor into both terms once, in fp64
    std::vector<double> jf((size_t)NJ * 3 * (1 + NB), 0.0);
    for (int j = 0; j < NJ; ++j)
        for (int v = 0; v < NV; ++v) {
            const double r = m->j_regressor[(size_t)j * NV + v];
            if (r == 0.0) continue;
            for (int x = 0; x < 3; ++x) {
                double* f = jf.data() + (size_t)(j * 3 + x) * (1 + NB);
                f[0] += r * (double)m->v_template[(size_t)v * 3 + x];
                for (int k = 0; k < NB; ++k) f[1 + k] += r * (double)m->shapedirs[((size_t)v * 3 + x) * NB + k];
            }
        }
    std::vector<int32_t> par(m->parents, m->parents + NJ);
    par[0] = 0;
    GATOR_TRY(upload(c->basis, basis));
    GATOR_TRY(upload(c->vtempl, vt));
    GATOR_TRY(upload(c->widx, wi));
    GATOR_TRY(upload(c->wval, ww));
    GATOR_TRY(upload(c->jfold, jf));
    GATOR_TRY(upload(c->parents, par));
    return GATOR_OK;
}

}  // namespace

int smpl_reserve(gator_smpl* c, int B) {
    if (B <= c->cap) return GATOR_OK;
    c->cap = 0;
    GATOR_TRY(c->grow(c->coef, (size_t)B * c->Kp));
    GATOR_TRY(c->grow(c->xform, (size_t)B * c->NJ * 12));
    GATOR_TRY(c->grow(c->offs, (size_t)B * 4));
    c->cap = B;
    return GATOR_OK;
}

int smpl_pose_stage(gator_smpl* c, const float* pose, const float* betas, const float* trans, int batch, int center, double out_scale,
                    float* joints, hipStream_t st) {
    k_smpl_pose<<<batch, 64, 0, st>>>(pose, c->NB ? betas : nullptr, trans, c->jfold, c->parents, c->NJ, c->NB, c->K, c->Kp, center < 0 ? -1 : center,
                                      out_scale, c->coef, c->xform, c->offs, joints);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
}  // namespace gator

extern "C" int gator_smpl_create(const gator_smpl_model* m, gator_smpl** out) {
    using namespace gator;
    if (!m || !out) return fail(GATOR_EINVAL, "gator_smpl_create: null argument");
    *out = nullptr;
    GATOR_TRY(check_struct_size("gator_smpl_create", "gator_smpl_model", m->struct_size, sizeof(gator_smpl_model)));
    if (m->n_verts < 1 || m->n_verts > (1 << 24)) return fail(GATOR_EINVAL, "gator_smpl_create: n_verts %d outside 1..%d", m->n_verts, 1 << 24);
    if (m->n_joints < 2 || m->n_joints > kSmplMaxJ) return fail(GATOR_EINVAL, "gator_smpl_create: n_joints %d outside 2..%d", m->n_joints, kSmplMaxJ);
    if (m->n_betas < 0 || m->n_betas > kSmplMaxB) return fail(GATOR_EINVAL, "gator_smpl_create: n_betas %d outside 0..%d", m->n_betas, kSmplMaxB);
    if (!m->v_template || !m->posedirs || !m->weights || !m->j_regressor || !m->parents || (m->n_betas > 0 && !m->shapedirs))
        return fail(GATOR_EINVAL, "gator_smpl_create: a model array is NULL");
    for (int j = 1; j < m->n_joints; ++j)
        if (m->parents[j] < 0 || m->parents[j] >= j)
            return fail(GATOR_EINVAL, "gator_smpl_create: parents[%d] = %d, a parent must precede its joint", j, m->parents[j]);
    return create_handle(out, [&](gator_smpl* c) -> int {
        c->NV = m->n_verts; c->NJ = m->n_joints; c->NB = m->n_betas;
        c->K = c->NB + (c->NJ - 1) * 9;
        c->Kp = (c->K + 4 * kKU - 1) / (4 * kKU) * (4 * kKU);
        c->NVp = (c->NV + kTV - 1) / kTV * kTV;
        GATOR_TRY(smpl_build(c, m));
        GATOR_TRY(smpl_fit_build(c, m));
        return smpl_backward_build(c, m);
    });
}

extern "C" int gator_smpl_destroy(gator_smpl* ctx) { return gator::destroy_handle(ctx); }

extern "C" int gator_smpl_workspace(const gator_smpl* ctx, const void** base, int64_t* capacity) {
    using namespace gator;
    if (!ctx) return fail(GATOR_EINVAL, "gator_smpl_workspace: null ctx");
    if (base) *base = ctx->coef.get();
    if (capacity) *capacity = ctx->cap;
    return GATOR_OK;
}

extern "C" int gator_smpl_forward_f32(gator_smpl* ctx, const float* pose, const float* betas, const float* trans, int32_t batch,
                                      int32_t center_idx, float out_scale, float* verts, float* joints, void* stream) {
    using namespace gator;
    if (center_idx >= 0 && trans) return fail(GATOR_EINVAL, "gator_smpl_forward_f32: center_idx goes with trans = NULL (the layer centres only an untranslated batch)");
    GATOR_TRY(check_handle(ctx, "gator_smpl_forward_f32", "ctx"));
    if (batch < 0 || (batch > 0 && !pose)) return fail(GATOR_EINVAL, "gator_smpl_forward_f32: bad pose / batch");
    if (center_idx >= ctx->NJ) return fail(GATOR_EINVAL, "gator_smpl_forward_f32: center_idx %d, the model has %d joints", center_idx, ctx->NJ);
    if (!std::isfinite(out_scale)) return fail(GATOR_EINVAL, "gator_smpl_forward_f32: out_scale must be finite");
    const int tiles = (batch + kTS - 1) / kTS;
    if (tiles > 65535) return fail(GATOR_EINVAL, "gator_smpl_forward_f32: batch %d above %d", batch, 65535 * kTS);
    if (batch == 0) return GATOR_OK;
    GATOR_TRY(smpl_reserve(ctx, batch));
    hipStream_t st = (hipStream_t)stream;
    GATOR_TRY(smpl_pose_stage(ctx, pose, betas, trans, batch, center_idx, (double)out_scale, joints, st));
    if (verts) {
        const dim3 grid(ctx->NVp / kTV, tiles);
        const size_t lds = skin_lds_bytes(ctx);
        if (ctx->MI <= 4)
            k_smpl_skin<4><<<grid, 256, lds, st>>>(ctx->basis, ctx->vtempl, ctx->widx, ctx->wval, ctx->MI, ctx->coef, ctx->xform, ctx->offs,
                                                   batch, ctx->NV, ctx->NVp, ctx->NJ, ctx->Kp, out_scale, verts);
        else
            k_smpl_skin<0><<<grid, 256, lds, st>>>(ctx->basis, ctx->vtempl, ctx->widx, ctx->wval, ctx->MI, ctx->coef, ctx->xform, ctx->offs,
                                                   batch, ctx->NV, ctx->NVp, ctx->NJ, ctx->Kp, out_scale, verts);
        GATOR_HIP_CHECK(hipGetLastError());
    }
    return GATOR_OK;
}
