// The SMPL body-model layer (smplpytorch/pytorch/smpl_layer.py:65-158, rodrigues_layer.py:13-52) on the device, batched:
//   (pose [B,NJ*3], betas [B,NB], trans [B,3]) -> (verts [B,NV,3], joints [B,NJ,3])
// in two launches and without the layer's per-vertex intermediates (th_T [B,4,4,NV], v_shaped, v_posed never exist in memory).
// The steps that the backward and the fit run as well (kinematics, coefficient tile, blend product, affine apply) are in smpl_steps.h.
//   k_smpl_pose : one wave per sample, fp64.  Rodrigues with the reference's `+ 1e-8` inside the norm and its normalised quaternion,
//                 the pose map R[1:] - I, the shaped rest joints from the regressor folded at create, the kinematic chain (all four:
//                 smpl_kinematics); writes the sample's coefficient row [betas ; pose map], its NJ skinning transforms (3x4, fp32), its
//                 offset and the joints.
//   k_smpl_skin : the hot path.  Per (32-sample, 128-vertex) tile the blend offsets [32 x K] . [K x 3 x 128] on the fp32-input MFMA
//                 (smpl_blend; v_mfma_f32_32x32x2_f32: exact fp32 products, a fixed fmaf chain over k), the three coordinate planes of the
//                 basis as three accumulators, so that a lane holds x, y, z of one vertex for 16 samples; then, in registers, T = sum w A
//                 over the vertex's (index, weight) list with the tile's transforms in LDS, T . [v_posed ; 1], offset, scale, store.
// A sample is one MFMA row and one LDS row from end to end: its result depends on no other sample of the batch, and a non-finite
// pose or beta makes every output of its own sample non-finite and touches no other.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "internal.h"
#include "smpl_ctx.h"
#include "smpl_steps.h"

namespace gator {
namespace {

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
    poison += smpl_kinematics(pose, betas, jfold, parents, b, t, NJ, NB, R, J, G, cf + NB);
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
    smpl_coef_tile(coef, s0, ns, Kp, lds);
    __syncthreads();
    const int v = v0 + wave * 32 + col;                                 // < NVp: the planes are padded to whole tiles
    f32x16 ax = {0}, ay = {0}, az = {0};
    smpl_blend(lds, basis + v, NVp, Kp, col, hi, ax, ay, az);
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
        const int i = mfma32_row(r, hi);
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
        float x[3];
        smpl_affine(T, tx + ax[r], ty + ay[r], tz + az[r], x);          // v_posed = v_template + blend offsets
        float* o = verts + ((size_t)(s0 + i) * NV + v) * 3;             // 32 lanes x 12 bytes: 384 contiguous bytes per sample
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (x[c] + lo[i * 4 + c]) * out_scale;
    }
}

size_t skin_lds_bytes(const gator_smpl* c) {
    const size_t a = (size_t)c->Kp * kLd, b = (size_t)kTS * c->NJ * 12 + kTS * 4;
    return sizeof(float) * (a > b ? a : b);
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

int smpl_check_batch(const char* who, const gator_smpl* ctx, int batch, int max_batch) {
    GATOR_TRY(check_handle(ctx, who, "ctx"));
    if (batch < 0 || batch > max_batch) return fail(GATOR_EINVAL, "%s: batch %d outside 0..%d", who, batch, max_batch);
    return GATOR_OK;
}

int smpl_check_layer_call(const char* who, const gator_smpl* ctx, const float* pose, const float* trans, int batch, int center_idx,
                          float out_scale) {
    if (center_idx >= 0 && trans) return fail(GATOR_EINVAL, "%s: center_idx goes with trans = NULL (the layer centres only an untranslated batch)", who);
    GATOR_TRY(smpl_check_batch(who, ctx, batch, 65535 * kTS));          // the sample tiles are the grid's y
    if (batch > 0 && !pose) return fail(GATOR_EINVAL, "%s: pose is NULL", who);
    if (center_idx >= ctx->NJ) return fail(GATOR_EINVAL, "%s: center_idx %d, the model has %d joints", who, center_idx, ctx->NJ);
    if (!std::isfinite(out_scale)) return fail(GATOR_EINVAL, "%s: out_scale must be finite", who);
    return GATOR_OK;
}

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
    GATOR_TRY(smpl_check_layer_call("gator_smpl_forward_f32", ctx, pose, trans, batch, center_idx, out_scale));
    if (batch == 0) return GATOR_OK;
    GATOR_TRY(smpl_reserve(ctx, batch));
    hipStream_t st = (hipStream_t)stream;
    GATOR_TRY(smpl_pose_stage(ctx, pose, betas, trans, batch, center_idx, (double)out_scale, joints, st));
    if (verts)
        GATOR_TRY(launch_by_influences(ctx, k_smpl_skin<4>, k_smpl_skin<0>, dim3(ctx->NVp / kTV, (batch + kTS - 1) / kTS), skin_lds_bytes(ctx), st,
                                       ctx->basis, ctx->vtempl, ctx->widx, ctx->wval, ctx->MI, ctx->coef, ctx->xform, ctx->offs, batch, ctx->NV,
                                       ctx->NVp, ctx->NJ, ctx->Kp, out_scale, verts));
    return GATOR_OK;
}
