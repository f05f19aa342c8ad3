// Vertex regressor: upsample_conv (Conv1d 431->6890, k=3, p=1 over the 3-long xyz axis) + bias + template add,
// lib/models/MDR.py:122,167-168.   out[b][o][l] = bias[o] + tpl[o][l] + sum_c sum_k w[o][c][k] * vc[b][c][l+k-1]
//
// Formulated as three accumulators (l = 0,1,2) per (32 samples x 32 vertices) wave tile that SHARE the weight operands:
// tap k of the weights meets input column l' = l+k-1, so each loaded weight fragment w[.][c][k] feeds up to three fp32
// MFMAs (7 per (c-step) instead of 9: the zero-padding taps are never multiplied -> 41.6 of the dense 53.45 MFLOP/mesh) and
// the 35.6 MB weight is streamed once per 128 samples.  A = packed vert431 (rows = samples), B = packed weights
// (cols = output vertices)  ->  accumulator: vertex on the lane, samples in registers, so each lane stores the 3
// contiguous floats out[b][o][0..2] and a wave row covers 384 contiguous bytes.
#include "upsample_common.h"

namespace gator {
namespace {

// NT = 32-sample tiles per wave that share each weight fragment.  NT = 2 (64 samples x 32 vertices x 3 coords) halves the
// weight traffic and, at B=256, gives 864 waves - at most one per SIMD, so no co-resident partner competes for the MFMA pipe
// (142 -> 107 us); NT = 1 keeps small batches spread over the chip.
template <int NT>
__global__ __launch_bounds__(256, 1) void k_upsample(const float* __restrict__ vcp, const float* __restrict__ wp,
                                                     const float* __restrict__ bias, const float* __restrict__ tpl,
                                                     float* __restrict__ out, int B, int MT, int nwg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int MP = (MT + NT - 1) / NT, mgroups = (MP + 3) >> 2;
    const int ob = wg / mgroups, mp = (wg % mgroups) * 4 + wave;
    if (mp >= MP) return;
    int mt[NT], nt = 0;
    const f32x4* a_base[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        if (NT * mp + m < MT) nt = m + 1;
        mt[m] = NT * mp + m < MT ? NT * mp + m : NT * mp;        // ragged tail: repeat the first tile (its result is not stored)
        a_base[m] = reinterpret_cast<const f32x4*>(vcp) + ((size_t)mt[m] * 3 * kCB * 4) * 64 + lane;
    }
    const f32x4* w_base = reinterpret_cast<const f32x4*>(wp) + ((size_t)ob * kCB * 4) * 64 + lane;
    const size_t w_tap = (size_t)kOB * kCB * 4 * 64, a_lp = (size_t)kCB * 4 * 64;
    f32x16 acc[NT][3], tot[NT][3];
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int l = 0; l < 3; ++l) { acc[m][l] = zero16(); tot[m][l] = zero16(); }
    // software pipeline over the 56 (cb,g) steps: the operand fragments of step s+1 are requested before the MFMAs of step s
    // are queued (the fence keeps that order), so their L2 latency hides behind 28*NT MFMAs
    f32x4 x[NT][3], w[3];
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int l = 0; l < 3; ++l) x[m][l] = a_base[m][l * a_lp];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = w_base[k * w_tap];
#pragma unroll 1
    for (int cb = 0; cb < kCB; ++cb) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int sn = cb * 4 + g + 1 < kCB * 4 ? cb * 4 + g + 1 : cb * 4 + g;     // next step (last one re-loads itself)
            const size_t o = (size_t)sn * 64;
            f32x4 nx[NT][3], nw[3];
#pragma unroll
            for (int m = 0; m < NT; ++m)
#pragma unroll
                for (int l = 0; l < 3; ++l) nx[m][l] = a_base[m][l * a_lp + o];
#pragma unroll
            for (int k = 0; k < 3; ++k) nw[k] = w_base[k * w_tap + o];
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // the tap list (regressor_slots.h: kRegTaps) written out in another issue order: consecutive MFMAs never write
                // the same accumulator
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[m][0] = GATOR_MFMA(x[m][0][j], w[1][j], acc[m][0]);
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[m][1] = GATOR_MFMA(x[m][0][j], w[0][j], acc[m][1]);
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[m][2] = GATOR_MFMA(x[m][1][j], w[0][j], acc[m][2]);
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[m][0] = GATOR_MFMA(x[m][1][j], w[2][j], acc[m][0]);
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[m][1] = GATOR_MFMA(x[m][1][j], w[1][j], acc[m][1]);
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[m][2] = GATOR_MFMA(x[m][2][j], w[1][j], acc[m][2]);
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[m][1] = GATOR_MFMA(x[m][2][j], w[2][j], acc[m][1]);
            }
#pragma unroll
            for (int m = 0; m < NT; ++m)
#pragma unroll
                for (int l = 0; l < 3; ++l) x[m][l] = nx[m][l];
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = nw[k];
        }
        // two-level summation: chains of <= 96 products per 32-vertex block, then 14 partial sums (fp32 accuracy)
#pragma unroll
        for (int m = 0; m < NT; ++m)
#pragma unroll
            for (int l = 0; l < 3; ++l) { tot[m][l] += acc[m][l]; acc[m][l] = zero16(); }
    }
    regress_finish<false>(ob, mt, nt, true, lane, B, bias, tpl, out, JregEpi{}, [&](int m, int l, int r) { return tot[m][l][r]; });
}

}  // namespace

int launch_upsample_f32(const FusedState* f, const gator_ctx* c, const FusedWs& ws, int B, float* verts, void* stream) {
    const int MT = (B + 31) / 32;
    if (MT >= 8) {          // >= 225 samples: two tiles per wave
        const int MP = (MT + 1) / 2, nwg = kOB * ((MP + 3) / 4);
        k_upsample<2><<<nwg, 256, 0, (hipStream_t)stream>>>(ws.vcp, f->up_w, c->w.up_b, c->w.v6890, verts, B, MT, nwg);
        GATOR_HIP_CHECK(hipGetLastError());
        return GATOR_OK;
    }
    const int nwg = kOB * ((MT + 3) / 4);
    k_upsample<1><<<nwg, 256, 0, (hipStream_t)stream>>>(ws.vcp, f->up_w, c->w.up_b, c->w.v6890, verts, B, MT, nwg);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

// ---- the row's entries: every form of the packed operands and of the launch, chosen by the plan (forward_plan.h) -------------------------
// upsample_conv.weight [6890][431][3] -> the form's packed weights; *unscale: what undoes the two-plane form's operand scalings.  (The
// fp32 form's weights are fused_pack_linear's tile grids, one per tap.)
int pack_upsample_any(Regressor form, const float* up_w, void* dst, float* unscale, void* stream) {
    if (form == Regressor::X2) return pack_upsample_x2(up_w, dst, unscale, stream);
    if (form == Regressor::X3) return pack_operand<__bf16, 3, false, w_slot_b16>(up_w, kNV, 32 * kOB, dst, upsample_x3_weight_elems() / 3, 1.f, stream);
    if (form == Regressor::BF16) return pack_operand<__bf16, 1, false, w_slot_b16>(up_w, kNV, 32 * kOB, dst, 0, 1.f, stream);
    return fail(GATOR_EINVAL, "pack_upsample_any: no packed weight form");
}

// vc [B][431][3] -> the A operand of the plan's kernel in ws.  The three-plane form's planes are strided by the workspace capacity, so
// padding written once stays valid for every smaller batch
int launch_pack_vc_any(const RegressorPlan& r, const float* vc, int B, const FusedWs& ws, void* stream) {
    const int pad32 = (B + 31) / 32 * 32;
    switch (r.form) {
    case Regressor::FP32: return pack_operand<float, 1, false, act_slot_f32>(vc, B, pad32, ws.vcp, 0, 1.f, stream);
    case Regressor::X3: return pack_operand<__bf16, 3, false, act_slot_b16>(vc, B, pad32, ws.vcp3, upsample_x3_vcp_elems(ws.cap) / 3, 1.f, stream);
    case Regressor::X2: return pack_operand<_Float16, 2, true, act_slot_x2>(vc, B, (B + 127) / 128 * 128, ws.vcp3, kX2Plane, (float)(1 << kActShift), stream);
    case Regressor::BF16: return pack_operand<__bf16, 1, false, act_slot_b16>(vc, B, pad32, ws.vcp16.get(), 0, 1.f, stream);
    default: return fail(GATOR_EINVAL, "launch_pack_vc_any: no regressor planned");
    }
}

int launch_upsample_any(const FusedState* f, const gator_ctx* c, const FusedWs& ws, const RegressorPlan& r, int B, float* verts, void* stream) {
    switch (r.form) {
    case Regressor::FP32: return launch_upsample_f32(f, c, ws, B, verts, stream);
    case Regressor::X3: return launch_upsample_x3(f, c, ws, B, verts, stream, r.with_joints);
    case Regressor::X2: return launch_upsample_x2(f, c, ws, B, verts, stream, r.with_joints, r.w1);
    case Regressor::BF16: return launch_upsample_bf16(f, c, ws, B, verts, stream);
    default: return fail(GATOR_EINVAL, "launch_upsample_any: no regressor planned");
    }
}

}  // namespace gator
