// bf16 variant of the vertex regressor (BASELINE config 3: "full GATOR forward bf16, MFMA vertex regressor"): the
// upsample_conv GEMM (lib/models/MDR.py:122,167-168) on v_mfma_f32_32x32x16_bf16 -- bf16 operands, fp32 accumulate, fp32
// bias/template epilogue and fp32 output.  Everything upstream stays fp32, so parity is MPJPE-level (bf16 rounding of the
// 431x3 coarse vertices and of the weights: ~0.2 mm rms on a vertex), not the 1e-3 mm of the fp32 path.
//
// Same tap-sharing formulation as upsample_fused.hip (7 MFMAs per loaded k-step, padding taps never multiplied) with
// K = 16 coarse vertices per MFMA.  At 16x the fp32 MFMA rate the kernel is bound by operand traffic, so one wave owns TWO
// 32-sample tiles per weight fragment (64 samples x 32 vertices x 3 coords).
#include "upsample_common.h"

namespace gator {
namespace {

__global__ __launch_bounds__(256) void k_upsample_bf16(const __bf16* __restrict__ vcp, const __bf16* __restrict__ wp,
                                                       const float* __restrict__ bias, const float* __restrict__ tpl,
                                                       float* __restrict__ out, int B, int MT, int nwg) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int MP = (MT + 1) >> 1, mgroups = (MP + 3) >> 2;
    const int ob = wg / mgroups, mp = (wg % mgroups) * 4 + wave;          // mp: pair of 32-sample tiles
    if (mp >= MP) return;
    const int mt0 = 2 * mp, mt1 = (2 * mp + 1 < MT) ? 2 * mp + 1 : 2 * mp;   // odd tile count: the last pair repeats its tile
    const bf16x8* a0p = reinterpret_cast<const bf16x8*>(vcp) + ((size_t)mt0 * 3 * kS16) * 64 + lane;
    const bf16x8* a1p = reinterpret_cast<const bf16x8*>(vcp) + ((size_t)mt1 * 3 * kS16) * 64 + lane;
    const bf16x8* wq = reinterpret_cast<const bf16x8*>(wp) + ((size_t)ob * kS16) * 64 + lane;
    const size_t w_tap = (size_t)kOB * kS16 * 64, a_lp = (size_t)kS16 * 64;
    f32x16 acc[2][3];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int l = 0; l < 3; ++l) acc[m][l] = zero16();
#pragma unroll 2
    for (int s = 0; s < kS16; ++s) {
        const size_t o = (size_t)s * 64;
        const bf16x8 w0 = wq[o], w1 = wq[w_tap + o], w2 = wq[2 * w_tap + o];
        const bf16x8 x0 = a0p[o], x1 = a0p[a_lp + o], x2 = a0p[2 * a_lp + o];
        const bf16x8 y0 = a1p[o], y1 = a1p[a_lp + o], y2 = a1p[2 * a_lp + o];
        // the tap list (regressor_slots.h: kRegTaps) written out, two sample tiles interleaved; A = samples (rows), B = vertices (cols)
        acc[0][0] = GATOR_MFMA_BF16(x0, w1, acc[0][0]);
        acc[1][0] = GATOR_MFMA_BF16(y0, w1, acc[1][0]);
        acc[0][1] = GATOR_MFMA_BF16(x0, w0, acc[0][1]);
        acc[1][1] = GATOR_MFMA_BF16(y0, w0, acc[1][1]);
        acc[0][2] = GATOR_MFMA_BF16(x1, w0, acc[0][2]);
        acc[1][2] = GATOR_MFMA_BF16(y1, w0, acc[1][2]);
        acc[0][0] = GATOR_MFMA_BF16(x1, w2, acc[0][0]);
        acc[1][0] = GATOR_MFMA_BF16(y1, w2, acc[1][0]);
        acc[0][1] = GATOR_MFMA_BF16(x1, w1, acc[0][1]);
        acc[1][1] = GATOR_MFMA_BF16(y1, w1, acc[1][1]);
        acc[0][2] = GATOR_MFMA_BF16(x2, w1, acc[0][2]);
        acc[1][2] = GATOR_MFMA_BF16(y2, w1, acc[1][2]);
        acc[0][1] = GATOR_MFMA_BF16(x2, w2, acc[0][1]);
        acc[1][1] = GATOR_MFMA_BF16(y2, w2, acc[1][1]);
    }
    const int mts[2] = {mt0, mt1};
    regress_finish<false>(ob, mts, mt1 == mt0 ? 1 : 2, true, lane, B, bias, tpl, out, JregEpi{}, [&](int m, int l, int r) { return acc[m][l][r]; });
}

}  // namespace

int launch_upsample_bf16(const FusedState* f, const gator_ctx* c, const FusedWs& ws, int B, float* verts, void* stream) {
    const int MT = (B + 31) / 32;
    const int MP = (MT + 1) / 2;
    const int nwg = kOB * ((MP + 3) / 4);
    k_upsample_bf16<<<nwg, 256, 0, (hipStream_t)stream>>>((const __bf16*)ws.vcp16.get(), (const __bf16*)f->up_w16.get(), c->w.up_b, c->w.v6890,
                                                         verts, B, MT, nwg);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

}  // namespace gator
