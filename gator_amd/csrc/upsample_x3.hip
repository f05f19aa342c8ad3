// fp32-accurate vertex regressor (upsample_conv + template, MDR.py:167-168) on the bf16 MFMA by split precision.
//
// Every fp32 operand is split EXACTLY into three bf16 planes, x = hi + mid + lo (8+8+8 significand bits; each remainder is
// exactly representable, so nothing is lost).  A product a*w is then the sum of nine exact partial products; the six largest
// (hi*hi | hi*mid, mid*hi | mid*mid, hi*lo, lo*hi) are computed on v_mfma_f32_32x32x16_bf16 -- 6 x 32 cycles per 16-deep
// k-step against 8 x 64 cycles for the fp32-input MFMA (2.7x) -- and the dropped terms are below 2^-23 of the product.
// hi*hi goes to one accumulator, the five small-magnitude terms to another, so they are not rounded away against the big sum.
#include "upsample_common.h"

namespace gator {
namespace {

// One workgroup = one 32-vertex output tile x up to 8 sample tiles (one per compute wave) + ONE LOADER WAVE.
// The 9 weight fragments of a k-step (3 taps x 3 planes, 9 KiB; the 54 MB weight stream comes from HBM) are fetched by
// the loader wave four k-steps ahead into a register ring and handed to the compute waves through a double-buffered LDS
// stage: its vmcnt queue is its own, so the compute waves' (L2-resident) activation prefetch never queues behind an
// HBM miss (vmcnt retires in order).  Each compute wave register-prefetches its 9 activation fragments one step ahead.
// The finished vertex and the joint-regression epilogue: upsample_common.h (regress_finish).
constexpr int kX3Waves = 8, kX3Ring = 4;
__global__ __launch_bounds__(64 * (kX3Waves + 1), 1) void k_upsample_x3(const __bf16* __restrict__ vcp, const __bf16* __restrict__ wp,
                                                                       const float* __restrict__ bias, const float* __restrict__ tpl,
                                                                       float* __restrict__ out, int B, int MT, int nwg, int64_t a_plane,
                                                                       int64_t w_plane, const JregEpi jr) {
    __shared__ bf16x8 wl[2][9][64];
    __shared__ f32x4 tot[kX3Waves][12][64];       // running totals of the hi*hi chains, see the flush below (96 KiB)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int mgroups = (MT + kX3Waves - 1) / kX3Waves;
    const int ob = wg / mgroups;
    // wave-uniform base (scalar registers) + one per-lane offset: nine 64-bit per-lane pointers would cost the loader 18 VGPRs
    const bf16x8* wu = reinterpret_cast<const bf16x8*>(wp) + ((size_t)ob * kS16) * 64;
    const size_t w_tap = (size_t)kOB * kS16 * 64, wpl = (size_t)w_plane / 8;
#define W_AT(e, step) wu[(size_t)((e) % 3) * wpl + (size_t)((e) / 3) * w_tap + (size_t)(step) * 64 + lane]
    static_assert(kS16 % kX3Ring == 0, "k-steps must be a multiple of the ring depth");
    if (wave == kX3Waves) {
        bf16x8 ring[kX3Ring][9];
#pragma unroll
        for (int j = 0; j < kX3Ring; ++j)
#pragma unroll
            for (int e = 0; e < 9; ++e) ring[j][e] = W_AT(e, j);
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            wl[0][e][lane] = ring[0][e];
            ring[0][e] = W_AT(e, kX3Ring);
        }
        __syncthreads();
#pragma unroll 1
        for (int s0 = 0; s0 < kS16; s0 += kX3Ring) {
#pragma unroll
            for (int j = 0; j < kX3Ring; ++j) {
                const int s = s0 + j, slot = (j + 1) % kX3Ring;
                const int nxt = s + 1 + kX3Ring < kS16 ? s + 1 + kX3Ring : kS16 - 1;
#pragma unroll
                for (int e = 0; e < 9; ++e) {
                    wl[(s + 1) & 1][e][lane] = ring[slot][e];                   // W(s+1), issued three steps ago
                    ring[slot][e] = W_AT(e, nxt);
                }
                __syncthreads();
            }
        }
        return;
    }
    const int mt_raw = (wg % mgroups) * kX3Waves + wave;
    const bool live = mt_raw < MT;
    const int mt = live ? mt_raw : MT - 1;             // idle waves shadow the last tile (they must keep the barriers)
    const bf16x8* ab = reinterpret_cast<const bf16x8*>(vcp) + ((size_t)__builtin_amdgcn_readfirstlane(mt) * 3 * kS16) * 64 + lane;
    const size_t a_lp = (size_t)kS16 * 64, ap = (size_t)a_plane / 8;
    f32x16 big[3], sm[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) { big[l] = zero16(); sm[l] = zero16(); }
    // Activation fragments x[lp][plane] are reloaded ROLLING: the MFMAs run grouped by input position lp (for a fixed output l
    // that is still tap order k = 0,1,2, so every accumulator sees the same sequence of products as a tap-major loop), and as
    // soon as the group of lp has been queued its three fragments are re-requested for the next k-step -- the loads fly behind
    // the remaining groups and the barrier, at no extra registers (a second prefetch set would cost 36 VGPRs and spill: nine
    // waves per workgroup leave 168).
    bf16x8 x[3][3];
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int p = 0; p < 3; ++p) x[l][p] = ab[p * ap + l * a_lp];
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < kS16; ++s) {
        const int cur = s & 1;
        const size_t on = (size_t)(s + 1 < kS16 ? s + 1 : s) * 64;
#pragma unroll
        for (int lp = 0; lp < 3; ++lp) {
#pragma unroll
            for (int t = 0; t < 7; ++t) {              // this input position's taps of the list (regressor_slots.h: kRegTaps); accumulators are independent
                if (kRegTaps[t].lp != lp) continue;
                const int k = kRegTaps[t].k, l = kRegTaps[t].l;
                const bf16x8 w0 = wl[cur][3 * k + 0][lane], w1 = wl[cur][3 * k + 1][lane], w2 = wl[cur][3 * k + 2][lane];
                big[l] = GATOR_MFMA_BF16(x[lp][0], w0, big[l]);      // hi*hi
                sm[l] = GATOR_MFMA_BF16(x[lp][0], w1, sm[l]);        // hi*mid
                sm[l] = GATOR_MFMA_BF16(x[lp][1], w0, sm[l]);        // mid*hi
                sm[l] = GATOR_MFMA_BF16(x[lp][1], w1, sm[l]);        // mid*mid
                sm[l] = GATOR_MFMA_BF16(x[lp][0], w2, sm[l]);        // hi*lo
                sm[l] = GATOR_MFMA_BF16(x[lp][2], w0, sm[l]);        // lo*hi
            }
            asm volatile("" ::: "memory");             // keep the reload below behind this group's MFMAs (and its LDS reads above it)
#pragma unroll
            for (int p = 0; p < 3; ++p) x[lp][p] = ab[p * ap + lp * a_lp + on];
        }
        // Every 7 k-steps the hi*hi chain is flushed into an LDS-resident total and restarted from zero: the chain's
        // partial sums stay small (their roundings scale with their magnitude) and only 4 additions happen at full
        // magnitude -- the two-level summation of the fp32 kernel, with LDS instead of 48 more accumulator registers.
        if (s % 7 == 6 && s != kS16 - 1) {
#pragma unroll
            for (int l = 0; l < 3; ++l)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v4[j] = big[l][4 * g + j];
                    if (s != 6) v4 += tot[wave][l * 4 + g][lane];
                    tot[wave][l * 4 + g][lane] = v4;
                }
#pragma unroll
            for (int l = 0; l < 3; ++l) big[l] = zero16();
        }
        __syncthreads();
    }
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v4 = tot[wave][l * 4 + g][lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) big[l][4 * g + j] += v4[j];
        }
    const int mts[1] = {mt};
    regress_finish<true>(ob, mts, 1, live, lane, B, bias, tpl, out, jr, [&](int, int l, int r) { return big[l][r] + sm[l][r]; });
}

// joints[b][j][c] = sum of joint j's entries of P[b], ascending vertex order, accumulated in fp64
__global__ void k_jreg_reduce(const float* __restrict__ P, const int* __restrict__ row_ptr, int nnz, int nj, int B, float* __restrict__ joints) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * nj * 3) return;
    const int c = (int)(i % 3), j = (int)((i / 3) % nj);
    const int64_t b = i / (3 * nj);
    double acc = 0.0;
    for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e) acc += (double)P[(b * nnz + e) * 3 + c];
    joints[i] = (float)acc;
}

}  // namespace

int launch_jreg_reduce(const FusedState* f, int B, float* joints, void* stream) {
    const int64_t n = (int64_t)B * f->jr_nj * 3;
    k_jreg_reduce<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(f->jr_P.get(), f->jr_rowptr.get(), f->jr_nnz, f->jr_nj, B, joints);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

// verts == nullptr: vertices are not stored (joint regression only); with_joints: also fill f->jr_P for launch_jreg_reduce
int launch_upsample_x3(const FusedState* f, const gator_ctx* c, const FusedWs& ws, int B, float* verts, void* stream, bool with_joints) {
    const int MT = (B + 31) / 32;
    const JregEpi jr = jreg_epi(f, with_joints);
    const int64_t w_plane = (int64_t)upsample_x3_weight_elems() / 3, a_plane = (int64_t)upsample_x3_vcp_elems(ws.cap) / 3;
    const int nwg = kOB * ((MT + kX3Waves - 1) / kX3Waves);
    k_upsample_x3<<<nwg, 64 * (kX3Waves + 1), 0, (hipStream_t)stream>>>((const __bf16*)ws.vcp3, (const __bf16*)f->up_w3.get(), c->w.up_b,
                                                                       c->w.v6890, verts, B, MT, nwg, a_plane, w_plane, jr);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

}  // namespace gator
