// Device code shared by the MDR kernels (mdr_fused.hip: tile, layer and persistent kernels; mdr_head.hip: joint tokens and head): the row-wise
// helpers over a token's 64 channels, the four flash-attention loops, the weight streams and the operand policy TokOp<XA> that says what
// each arithmetic form is.  Everything here is inlined into its callers.
#pragma once
#include "fused_common.h"
#include "fused_state.h"
#include "x3_common.h"

#include <type_traits>

// (the diagnostic build of mdr_fused.hip defines these before it includes this file: GATOR_MDR_CUT)
#ifndef MDR_WIDX
#define MDR_WIDX(i) (i)
#define MDR_KVIDX(i) (i)
#endif

namespace gator {
namespace {


// ---- row-wise helpers over the 64 channels (2 blocks) of a token (lane pair l, l^32) -------------------------------
// nn.LayerNorm(64), eps inside the sqrt
__device__ __forceinline__ void layernorm64(const f32x16 (&x)[2], const float* __restrict__ w, const float* __restrict__ b,
                                            int h, f32x16 (&y)[2]) {
    f32x16 d0 = x[0], d1 = x[1];
    const float rstd = ln_center64(d0, d1);
    y[0] = d0 * rstd * load_chanvec_S(w, 0, h) + load_chanvec_S(b, 0, h);
    y[1] = d1 * rstd * load_chanvec_S(w, 32, h) + load_chanvec_S(b, 32, h);
}

// sum of squares of the 64 channel deviations of a token: four FMA chains per block instead of 32 products + 32 adds (and each term
// rounded once instead of twice)
__device__ __forceinline__ float row_sumsq64(const f32x16& a, const f32x16& b) {
    float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r & 3] = __builtin_fmaf(a[r], a[r], p[r & 3]);
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r & 3] = __builtin_fmaf(b[r], b[r], p[r & 3]);
    const float s = (p[0] + p[1]) + (p[2] + p[3]);
    return s + xhalf(s);
}
// nn.LayerNorm(64) with the affine part as one FMA per value: (d * rstd) * w + b.  w and b come from the workgroup's LDS table; when
// the result only feeds 4-product linears the table holds 16 w and 16 b (mdr_stage_vectors), so the result IS the operand scale.
__device__ __forceinline__ void layernorm64_L(const f32x16 (&x)[2], const float* w, const float* b, int h, f32x16 (&y)[2]) {
    const float mean = row_sum(x[0], x[1]) * (1.0f / 64.0f);
    f32x16 d0 = x[0] - mean, d1 = x[1] - mean;
    const float var = row_sumsq64(d0, d1) * (1.0f / 64.0f);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    y[0] = __builtin_elementwise_fma(d0 * rstd, chanvec_lds(w, 0, h), chanvec_lds(b, 0, h));
    y[1] = __builtin_elementwise_fma(d1 * rstd, chanvec_lds(w, 32, h), chanvec_lds(b, 32, h));
}
__device__ __forceinline__ void custom_ln64_L(f32x16 (&x)[2], const float* a2, const float* b2, int h) {
    const float mean = row_sum(x[0], x[1]) * (1.0f / 64.0f);
    f32x16 d0 = x[0] - mean, d1 = x[1] - mean;
    const float std = sqrtf(row_sumsq64(d0, d1) * (1.0f / 63.0f));
    const float inv = 1.0f / (std + 1e-6f);
    x[0] = __builtin_elementwise_fma(chanvec_lds(a2, 0, h) * d0, f32x16(inv), chanvec_lds(b2, 0, h));
    x[1] = __builtin_elementwise_fma(chanvec_lds(a2, 32, h) * d1, f32x16(inv), chanvec_lds(b2, 32, h));
}

// Annotated-Transformer LayerNorm: a_2 * (x - mean) / (std_unbiased + 1e-6) + b_2
__device__ __forceinline__ void custom_ln64(f32x16 (&x)[2], const float* __restrict__ a2, const float* __restrict__ b2, int h) {
    const float mean = row_sum(x[0], x[1]) * (1.0f / 64.0f);
    f32x16 d0 = x[0] - mean, d1 = x[1] - mean;
    const float std = sqrtf(row_sum(d0 * d0, d1 * d1) * (1.0f / 63.0f));
    const float inv = 1.0f / (std + 1e-6f);
    x[0] = load_chanvec_S(a2, 0, h) * d0 * inv + load_chanvec_S(b2, 0, h);
    x[1] = load_chanvec_S(a2, 32, h) * d1 * inv + load_chanvec_S(b2, 32, h);
}

// Two waves share a SIMD.  A wave whose next instruction is an MFMA that cannot issue yet (matrix pipe busy) still wins the issue
// arbitration against a younger partner and starves the partner's VALU work (tools/microbench/helper_valu.hip: a VALU wave beside
// a wave of back-to-back MFMAs makes NO progress at equal priority, full speed at priority 1 - and the MFMAs still issue every 32
// cycles).  So a wave raises its priority while it runs VALU sections (softmax, splits, LayerNorm, GELU) and drops it for its
// MFMA bursts: whoever has vector work gets the issue slots, the matrix pipe is fed from the gaps.
#define MDR_PRIO_VALU() __builtin_amdgcn_s_setprio(1)
#define MDR_PRIO_MFMA() __builtin_amdgcn_s_setprio(0)
#define MDR_PIN()                            \
    do {                                     \
        asm volatile("" ::: "memory");       \
        __builtin_amdgcn_sched_barrier(0);   \
    } while (0)

// one 32-key tile of the flash attention: scores, online softmax, P.V into accumulator OACC
#define ATTN_TILE(KT, KB, VB, OACC, OACB)                                                                       \
    {                                                                                                       \
        f32x16 S = dot16(KB, qv, zero16());   /* S^T[key][query], two interleaved 8-step chains */            \
        float bm = -1e30f;                                                                                  \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                    \
            float sc = S[r] * c;                                                                            \
            if ((KT) == kVT - 1 && kap(r) + 4 * h >= kV - 32 * (kVT - 1)) sc = -1e30f; /* keys 431..447 do not exist */ \
            S[r] = sc;                                                                                      \
            bm = fmaxf(bm, sc);                                                                             \
        }                                                                                                   \
        bm = fmaxf(bm, xhalf(bm));                                                                          \
        if (!__all(bm <= m + 8.0f)) { /* lazy rescale (wave-uniform): P stays <= 2^8, exact in fp32 */      \
            const float mn = fmaxf(m, bm);                                                                  \
            const float al = __builtin_amdgcn_exp2f(m - mn);                                                \
            O = O * al;                                                                                     \
            O2 = O2 * al;                                                                                   \
            O3 = O3 * al;                                                                                   \
            O4 = O4 * al;                                                                                   \
            l *= al;                                                                                        \
            m = mn;                                                                                         \
        }                                                                                                   \
        float ps = 0.f;                                                                                     \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                    \
            const float pe = __builtin_amdgcn_exp2f(S[r] - m);                                              \
            S[r] = pe;                                                                                      \
            ps += pe;                                                                                       \
        }                                                                                                   \
        l += ps;                                                                                            \
        /* O^T[d][query] += V^T[d][key] P^T[key][query] */                                                  \
        _Pragma("unroll") for (int r = 0; r < 16; r += 2) {                                                 \
            OACC = GATOR_MFMA(VB[r], S[r], OACC);                                                           \
            OACB = GATOR_MFMA(VB[r + 1], S[r + 1], OACB);                                                   \
        }                                                                                                   \
    }

// ---- flash attention of one 32-query tile against the 431 keys of its sample, one head --------------------------------
// Even key tiles accumulate into chains O/O2 (even/odd key of the tile), odd tiles into O3/O4: four fp32 chains of ~110 products,
// and no two consecutive MFMAs write the same accumulator.  (Explicit K/V double buffering was measured:
// no gain -- the co-resident wave already covers the tile loads -- and it costs 32 VGPRs.)
__device__ __forceinline__ f32x16 self_attention_head(const float* __restrict__ qt, const float* __restrict__ kbase,
                                                      const float* __restrict__ vbase, int lane) {
    const int h = lane >> 5;
    const f32x16 qv = load_block(qt, lane);
    f32x16 O = zero16(), O2 = zero16(), O3 = zero16(), O4 = zero16();
    float m = -1e30f, l = 0.f;
    const float c = kLog2e * 0.17677669529663688110f;      // log2(e) / sqrt(d_k): scores kept in the exp2 domain
#pragma unroll 1
    for (int kt = 0; kt < kVT - 2; kt += 4) {               // 12 tiles in 3 trips of 4 (chain kt&3), then the last two
        {
            const f32x16 kb = load_block(kbase + (size_t)kt * 2 * kTile, lane), vb = load_block(vbase + (size_t)kt * 2 * kTile, lane);
            ATTN_TILE(kt, kb, vb, O, O2)
        }
        {
            const f32x16 kb = load_block(kbase + (size_t)(kt + 1) * 2 * kTile, lane), vb = load_block(vbase + (size_t)(kt + 1) * 2 * kTile, lane);
            ATTN_TILE(kt + 1, kb, vb, O3, O4)
        }
        {
            const f32x16 kb = load_block(kbase + (size_t)(kt + 2) * 2 * kTile, lane), vb = load_block(vbase + (size_t)(kt + 2) * 2 * kTile, lane);
            ATTN_TILE(kt + 2, kb, vb, O, O2)
        }
        {
            const f32x16 kb = load_block(kbase + (size_t)(kt + 3) * 2 * kTile, lane), vb = load_block(vbase + (size_t)(kt + 3) * 2 * kTile, lane);
            ATTN_TILE(kt + 3, kb, vb, O3, O4)
        }
    }
    {
        const f32x16 kb = load_block(kbase + (size_t)(kVT - 2) * 2 * kTile, lane), vb = load_block(vbase + (size_t)(kVT - 2) * 2 * kTile, lane);
        ATTN_TILE(kVT - 2, kb, vb, O, O2)
    }
    {
        const f32x16 kb = load_block(kbase + (size_t)(kVT - 1) * 2 * kTile, lane), vb = load_block(vbase + (size_t)(kVT - 1) * 2 * kTile, lane);
        ATTN_TILE(kVT - 1, kb, vb, O3, O4)
    }
    l += xhalf(l);
    return ((O + O2) + (O3 + O4)) * (1.0f / l);
}

// ---- the same on split-precision operands (x3_common.h): Q, K, V arrive as X3 tiles, S^T = K Q^T and O^T += V^T P^T are 12
// bf16 MFMAs each (768 cycles per key tile against 2048), the probabilities are split in registers.  The bf16 MFMA sums
// 16 products internally and its dependent chain issues back to back, so two accumulators (even / odd key tiles) suffice.
#define ATTN_TILE_X3(KT, KB, VB, OACC)                                                                      \
    {                                                                                                       \
        f32x16 S = x3_mma(KB, qx, zero16());  /* S^T[key][query] */                                         \
        float bm = -1e30f;                                                                                  \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {   /* Q arrives pre-scaled by log2(e)/sqrt(d_k) */ \
            float sc = S[r];                                                                                \
            if ((KT) == kVT - 1 && kap(r) + 4 * h >= kV - 32 * (kVT - 1)) sc = -1e30f;                      \
            S[r] = sc;                                                                                      \
            bm = fmaxf(bm, sc);                                                                             \
        }                                                                                                   \
        bm = fmaxf(bm, xhalf(bm));                                                                          \
        if (!__all(bm <= m + 8.0f)) {                                                                       \
            const float mn = fmaxf(m, bm);                                                                  \
            const float al = __builtin_amdgcn_exp2f(m - mn);                                                \
            O = O * al;                                                                                     \
            O2 = O2 * al;                                                                                   \
            l *= al;                                                                                        \
            m = mn;                                                                                         \
        }                                                                                                   \
        float ps = 0.f;                                                                                     \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                    \
            const float pe = __builtin_amdgcn_exp2f(S[r] - m);                                              \
            S[r] = pe;                                                                                      \
            ps += pe;                                                                                       \
        }                                                                                                   \
        l += ps;                                                                                            \
        OACC = x3_mma(VB, x3_split(S), OACC);   /* O^T[d][query] += V^T[d][key] P^T[key][query] */          \
    }
__device__ __forceinline__ f32x16 self_attention_head_x3(const float* __restrict__ qt, const float* __restrict__ kbase,
                                                         const float* __restrict__ vbase, int lane) {
    const int h = lane >> 5;
    const X3 qx = x3_load(qt, lane);
    f32x16 O = zero16(), O2 = zero16();
    float m = -1e30f, l = 0.f;
    X3 kb = x3_load(kbase, lane), vb = x3_load(vbase, lane);
#pragma unroll 1
    for (int kt = 0; kt < kVT; kt += 2) {                   // tiles kt (-> O) and kt + 1 (-> O2); the next tile's K/V in flight
        X3 kn = x3_load(kbase + (size_t)(kt + 1) * 2 * kTileX3, lane), vn = x3_load(vbase + (size_t)(kt + 1) * 2 * kTileX3, lane);
        ATTN_TILE_X3(kt, kb, vb, O)
        const int k2 = kt + 2 < kVT ? kt + 2 : kt;
        kb = x3_load(kbase + (size_t)k2 * 2 * kTileX3, lane);
        vb = x3_load(vbase + (size_t)k2 * 2 * kTileX3, lane);
        ATTN_TILE_X3(kt + 1, kn, vn, O2)
    }
    l += xhalf(l);
    return (O + O2) * (1.0f / l);
}

// ---- the same on two-plane fp16 operands (x3_common.h, "X2"): 6 MFMAs per product instead of 12, 3 VALU ops per split value
// instead of 5.5, 4 KiB tiles instead of 6.  Q and K arrive scaled by 16 (Q also by log2(e)/sqrt(d_k)), so the accumulator holds
// 256 x the score: the running maximum is kept in that domain and the 2^-8 rides on the FMA that forms the exponent.  V arrives
// scaled by 16 and the probabilities carry an extra 2^6 (so that their low plane stays a normal fp16 number); both cancel in
// O / (16 l).
constexpr float kX2QK = 16.0f, kX2V = 16.0f;
#define ATTN_PV(VB, PX) { O2 = x2_mma_small(VB, PX, O2); O = x2_mma_main(VB, PX, O); }
#define ATTN_TILE_X2(KT, KB, VB)                                                                            \
    {                                                                                                       \
        MDR_PRIO_MFMA();                                                                                    \
        f32x16 S = x2_mma(KB, qx, zero16());  /* 256 x S^T[key][query] */                                   \
        MDR_PRIO_VALU();                                                                                    \
        float bm = -1e30f;                                                                                  \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                    \
            float sc = S[r];                                                                                \
            if ((KT) == kVT - 1 && kap(r) + 4 * h >= kV - 32 * (kVT - 1)) sc = -1e30f;                      \
            S[r] = sc;                                                                                      \
            bm = fmaxf(bm, sc);                                                                             \
        }                                                                                                   \
        bm = fmaxf(bm, xhalf(bm));                                                                          \
        if (!__all(bm <= m + 2048.0f)) {      /* lazy rescale: P stays <= 2^8 (x 2^6 below) */               \
            const float mn = fmaxf(m, bm);                                                                  \
            const float al = __builtin_amdgcn_exp2f((m - mn) * 0.00390625f);                                \
            O = O * al;                                                                                     \
            O2 = O2 * al;                                                                                   \
            l *= al;                                                                                        \
            m = mn;                                                                                         \
        }                                                                                                   \
        const float off = 6.0f - m * 0.00390625f;                                                           \
        float ps = 0.f;                                                                                     \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                    \
            const float pe = __builtin_amdgcn_exp2f(fmaf(S[r], 0.00390625f, off));                          \
            S[r] = pe;                                                                                      \
            ps += pe;                                                                                       \
        }                                                                                                   \
        l += ps;                                                                                            \
        const X2 px_ = x2_split(S);                                                                         \
        MDR_PRIO_MFMA();                                                                                    \
        /* O^T[d][query] += V^T[d][key] P^T[key][query]: the hi*hi products of every key tile into O, the cross products (2^-11 of    \
           it) into O2 -- O is rounded 28 times at full magnitude over the 14 tiles instead of 42 times for each of two equal halves.   \
           (Measured and not taken: a third accumulator for the odd tiles' hi*hi products spills; the same split for the MLP's fc2      \
           accumulators fits in exactly 256 registers, makes the launch 8 % slower and moves the error by nothing.) */                   \
        ATTN_PV(VB, px_)                                                                                    \
    }
template <bool kActScale16>
__device__ __forceinline__ f32x16 self_attention_head_x2(const float* __restrict__ qt, const float* __restrict__ kbase,
                                                         const float* __restrict__ vbase, int lane) {
    const int h = lane >> 5;
    const X2 qx = x2_load(qt, lane);
    f32x16 O = zero16(), O2 = zero16();
    float m = -1e30f, l = 0.f;
    X2 kb = x2_load(kbase, lane), vb = x2_load(vbase, lane);
    // tiles kt and kt + 1 per trip, the next tile's K/V in flight.  The last pair is peeled so that the mask of the 17 keys that
    // do not exist (431 = 13 x 32 + 15) is compile-time there and absent from the loop (it cost 5 selects per tile as a runtime test).
    // (Round 4, measured and dropped: tiles after the first WITHOUT the row maximum -- probabilities against the running reference,
    // only their row sums inspected (a lane's 16 probabilities are below their sum, so "sum <= 2^14" proves the fp16 range), the
    // whole tile redone the long way where that fails.  14 of ~120 VALU instructions fewer per tile, same results to rounding, the
    // large-logit test green -- and the launch 12 us SLOWER.)
#pragma unroll 1
    for (int kt = 0; kt < kVT - 2; kt += 2) {
        X2 kn = x2_load(kbase + (size_t)MDR_KVIDX(kt + 1) * 2 * kTile, lane), vn = x2_load(vbase + (size_t)MDR_KVIDX(kt + 1) * 2 * kTile, lane);
        ATTN_TILE_X2(0, kb, vb)
        kb = x2_load(kbase + (size_t)MDR_KVIDX(kt + 2) * 2 * kTile, lane);
        vb = x2_load(vbase + (size_t)MDR_KVIDX(kt + 2) * 2 * kTile, lane);
        ATTN_TILE_X2(0, kn, vn)
    }
    {
        X2 kn = x2_load(kbase + (size_t)MDR_KVIDX(kVT - 1) * 2 * kTile, lane), vn = x2_load(vbase + (size_t)MDR_KVIDX(kVT - 1) * 2 * kTile, lane);
        ATTN_TILE_X2(kVT - 2, kb, vb)
        ATTN_TILE_X2(kVT - 1, kn, vn)
    }
    l += xhalf(l);
    return (O + O2) * (((kActScale16 ? 16.0f : 1.0f) / kX2V) / l);      // kActScale16: 16 x the head's output, the operand scale of the out-projection
}


// ---- ONE fp16 plane ("X1", BASELINE config 3: the MDR layers in 16-bit operand mode, XA == 3) --------------------------------------------
// Activations, Q, K, V and the probabilities are ONE fp16 plane of 16 x value (64 x for P): no split, 2 KiB tiles, 2 MFMAs per 32-deep
// product in the attention cores (against 6) and 4 per token-wise product (weights on their two leading fp16 planes, 22 bits: against
// 8); accumulation, softmax, norms, GELU and the residual stream stay fp32.  What that costs in accuracy is the activation rounding
// (2^-12 relative per operand element): tools/emulate_16bit.py, profiles/r05_emulate_16bit.txt (sub-millimetre vertices).
constexpr int kTileX1 = kTile / 2;
// One key tile (the step of self_attention_head_x1).  The VALU work per tile is what bounds this form (4 MFMAs against ~50 vector
// instructions), so the softmax is cut to exp2 + row sum + one conversion per pair:
//   * Q arrives scaled by log2(e) / sqrt(d_k) and K unscaled, so the MFMA delivers the score in the exp2 domain, and the running
//     reference is one add per value (ci = 6 - m: the 2^6 keeps P's fp16 image normal);
//   * no row maximum: the probabilities are non-negative, so "the lane's row sum < 2^15" proves every one of them is inside fp16's range;
//     where that fails (first tile, a tile whose scores jump by 2^9, anything non-finite) the tile is redone the long way: raw scores,
//     maximum, rescale of O and l, new reference.  Wave-uniform and rare.
template <bool kActScale16>
__device__ __forceinline__ f32x16 self_attention_head_x1(const float* __restrict__ qt, const float* __restrict__ kbase,
                                                         const float* __restrict__ vbase, int lane) {
    const int h = lane >> 5;
    const X1 qx = x1_load(qt, lane);
    f32x16 O = zero16();
    float m = -1e30f, l = 0.f;
    // Software-pipelined by one key tile (unrolled by two: fixed register names): the RAW scores of tile kt + 1 are issued before the
    // exponentials of tile kt, so the MFMAs run under the vector work of the same wave.  (The reference is added per value -- one
    // v_add more than carrying it on the accumulator's initial value, which needs a 16-register tile per head on top of the two score
    // tiles and spills; this form is bound by latency, not by its vector instruction count.)
    X1 kA = x1_load(kbase, lane), vA = x1_load(vbase, lane);
    X1 kB = x1_load(kbase + (size_t)MDR_KVIDX(1) * 2 * kTileX1, lane), vB = x1_load(vbase + (size_t)MDR_KVIDX(1) * 2 * kTileX1, lane);
    f32x16 SA = x1_mma(kA, qx, zero16()), SB;
    float ci = 1e30f;                           // 6 - m; an empty history overflows the first tile's row sums: it takes the long way
    auto step = [&](auto last_, const int kt, f32x16& Sc, f32x16& Sn, X1& Kc, const X1& Kn, X1& Vc) {
        constexpr int KT = decltype(last_)::value;      // kVT - 1 for the last tile (compile-time mask), else 0
        if (KT != kVT - 1) Sn = x1_mma(Kn, qx, zero16());     // raw scores of tile kt + 1: independent of everything below
        if (KT == kVT - 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) if (kap(r) + 4 * h >= kV - 32 * (kVT - 1)) Sc[r] = -1e30f;     // keys 431..447 do not exist
        }
        float ps = 0.f;
        if (__all(ci < 1e29f)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float pe = __builtin_amdgcn_exp2f(Sc[r] + ci); ps += pe; Sc[r] = pe; }
        } else ps = 1e30f;
        if (!__all(ps < 32768.0f)) {            // (the raw scores are gone where the fast way ran: back from K)
            f32x16 R = x1_mma(Kc, qx, zero16());
            float bm = -1e30f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (KT == kVT - 1 && kap(r) + 4 * h >= kV - 32 * (kVT - 1)) R[r] = -1e30f;
                bm = fmaxf(bm, R[r]);
            }
            bm = fmaxf(bm, xhalf(bm));
            const float mn = fmaxf(m, bm);
            const float al = __builtin_amdgcn_exp2f(m - mn);
            O = O * al;
            l *= al;
            m = mn;
            ci = 6.0f - m;
            ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { Sc[r] = __builtin_amdgcn_exp2f(R[r] + ci); ps += Sc[r]; }
        }
        l += ps;
        O = x1_mma(Vc, x1_cvt(Sc), O);
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 2 < kVT) {                             // tile kt + 2 into the buffers tile kt has just left
            Kc = x1_load(kbase + (size_t)MDR_KVIDX(kt + 2) * 2 * kTileX1, lane);
            Vc = x1_load(vbase + (size_t)MDR_KVIDX(kt + 2) * 2 * kTileX1, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll 1
    for (int kt = 0; kt < kVT - 2; kt += 2) {
        step(std::integral_constant<int, 0>(), kt, SA, SB, kA, kB, vA);
        step(std::integral_constant<int, 0>(), kt + 1, SB, SA, kB, kA, vB);
    }
    step(std::integral_constant<int, 0>(), kVT - 2, SA, SB, kA, kB, vA);
    step(std::integral_constant<int, kVT - 1>(), kVT - 1, SB, SA, kB, kA, vB);
    l += xhalf(l);
    return O * (((kActScale16 ? 16.0f : 1.0f) / kX2V) / l);
}

// ---- weight stream of the tokenwise part: two buffers of one tile pair each (2 x 32 VGPRs).  The pair for the NEXT
// product is requested right after the current product's MFMAs are queued, so its L2 latency hides behind them and
// behind the co-resident wave.  MDR_PIN keeps the order (memory ops and scheduler).
struct W2 { WTile t[2]; };
__device__ __forceinline__ W2 ldw2(const float* __restrict__ Wp, int i0, int i1, int lane) {
    W2 w;
    w.t[0] = load_wtile(Wp, i0, lane);
    w.t[1] = load_wtile(Wp, i1, lane);
    return w;
}
// 64-term contraction as two independent 32-term chains (one per k-block)
__device__ __forceinline__ f32x16 lin2_T(const W2& w, const f32x16 (&x)[2], f32x16 init) {
    f32x16 a1 = zero16();
    mma2_T(w.t[0], x[0], init, w.t[1], x[1], a1);
    return init + a1;
}
__device__ __forceinline__ f32x16 lin2_C(const W2& w, const f32x16 (&x)[2]) {
    f32x16 a0 = zero16(), a1 = zero16();
    mma2_C(w.t[0], x[0], a0, w.t[1], x[1], a1);
    return a0 + a1;
}

// X: self-attention on split-precision operands (q/k/v tiles are X3 tiles, 1.5x the size, same tile indices)
// split-precision forms: the weight pair is two X3 tiles (48 VGPRs), activations are split once per linear input, one chain
struct W2X { X3 t[2]; };
__device__ __forceinline__ W2X ldw2x(const float* __restrict__ Wx, int i0, int i1, int lane) {
    W2X w;
    w.t[0] = x3_load(Wx + (size_t)i0 * kTileX3, lane);
    w.t[1] = x3_load(Wx + (size_t)i1 * kTileX3, lane);
    return w;
}
__device__ __forceinline__ f32x16 lin2_T(const W2X& w, const X3 (&x)[2], f32x16 init) { return x3_mma(w.t[1], x[1], x3_mma(w.t[0], x[0], init)); }
__device__ __forceinline__ f32x16 lin2_C(const W2X& w, const X3 (&x)[2]) { return x3_mma(x[1], w.t[1], x3_mma(x[0], w.t[0], zero16())); }
// XA == 2: weights as two H3 tiles (three exact fp16 planes, 48 VGPRs), activations as X2 (two fp16 planes of 16 x value)
constexpr float kActScale = 16.0f;
struct W2H { H3 t[2]; };
__device__ __forceinline__ W2H ldw2h(const float* __restrict__ Wx, int i0, int i1, int lane) {
    W2H w;
    w.t[0] = h3_load(Wx + (size_t)i0 * kTileX3, lane);
    w.t[1] = h3_load(Wx + (size_t)i1 * kTileX3, lane);
    return w;
}
// a 64-deep product: the twelve cross products of both tiles first (accumulator still at bias magnitude), the four hi*hi products last
__device__ __forceinline__ f32x16 lin2_T(const W2H& w, const X2 (&x)[2], f32x16 init) {
    return h3_mma_wa_main(w.t[1], x[1], h3_mma_wa_main(w.t[0], x[0], h3_mma_wa_small(w.t[1], x[1], h3_mma_wa_small(w.t[0], x[0], init))));
}
__device__ __forceinline__ f32x16 lin2_C(const W2H& w, const X2 (&x)[2]) {
    return h3_mma_aw_main(x[1], w.t[1], h3_mma_aw_main(x[0], w.t[0], h3_mma_aw_small(x[1], w.t[1], h3_mma_aw_small(x[0], w.t[0], zero16()))));
}

// XA == 3: weights as the two leading fp16 planes (hi, mid: 22 bits) of two H3 tiles (32 VGPRs), activations as X1
struct W2G { G2 t[2]; };
__device__ __forceinline__ W2G ldw2g(const float* __restrict__ Wx, int i0, int i1, int lane) {
    W2G w;
    w.t[0] = g2_load(Wx + (size_t)i0 * kTileX3, lane);
    w.t[1] = g2_load(Wx + (size_t)i1 * kTileX3, lane);
    return w;
}
__device__ __forceinline__ f32x16 lin2_T(const W2G& w, const X1 (&x)[2], f32x16 init) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) init = GATOR_MFMA_F16(w.t[t].mid[s], x[t].p[s], init);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) init = GATOR_MFMA_F16(w.t[t].hi[s], x[t].p[s], init);
    return init;
}
__device__ __forceinline__ f32x16 lin2_C(const W2G& w, const X1 (&x)[2]) {
    f32x16 acc = zero16();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = GATOR_MFMA_F16(x[t].p[s], w.t[t].mid[s], acc);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc = GATOR_MFMA_F16(x[t].p[s], w.t[t].hi[s], acc);
    return acc;
}

// ---- the operand policy: what an arithmetic form XA of the tile kernels IS, said once ------------------------------------------------------
// XA   0: everything on the fp32-input MFMA ; 1: split precision (exact bf16 x 3, six partial products) everywhere ; 2 (the default):
//         token-wise linears on four partial products (weights exact on three fp16 planes, activations on two: x3_common.h), the
//         431x431 self-attention and the J-joint cross-attention on two fp16 planes ; 3 (config 3): the same on ONE fp16 activation plane
// A form names its weight pair W and the loader ldw, its activation operand A, how an accumulator tile becomes one (from / from_scaled),
// the Q/K/V tiles it stores (store; kTileQ floats each) and attends over (attend), and the operands JOp of the J-joint cross-attention.
//
// JOp: the joint K/V tiles, q and the probabilities.  fp32 blocks for XA 0 and 1; for XA >= 2 the tiles arrive as fp16 planes of kScale x value
// (k_gat_joint / k_mdr_joint), q goes in at kScale and the probabilities at kPScale x value (their low plane stays a normal fp16 number):
// 24 fp16 MFMAs of 32 cycles per tile instead of 64 fp32-input MFMAs of 64 cycles.  Like the 431x431 attention that rounds the operands to
// 22 bits (one plane, XA 3: the hi planes of the same tiles, q and the probabilities rounded once); a softmax average over 17 joints.
struct JointF32 {
    typedef f32x16 KV;
    static constexpr float kScale = 1.0f, kPScale = 1.0f;
    static __device__ __forceinline__ KV load(const float* __restrict__ p, int lane) { return load_block(p, lane); }
    static __device__ __forceinline__ f32x16 mma(const KV& kv, const f32x16& x) { return dot16(kv, x, zero16()); }
};
struct JointX2 {
    typedef X2 KV;
    static constexpr float kScale = 16.0f, kPScale = 64.0f;
    static __device__ __forceinline__ KV load(const float* __restrict__ p, int lane) { return x2_load(p, lane); }
    static __device__ __forceinline__ f32x16 mma(const KV& kv, const f32x16& x) { return x2_mma(kv, x2_split(x), zero16()); }
};
struct JointX1 {
    typedef X1 KV;
    static constexpr float kScale = 16.0f, kPScale = 64.0f;
    static __device__ __forceinline__ KV load(const float* __restrict__ p, int lane) { return x1_load(p, lane); }
    static __device__ __forceinline__ f32x16 mma(const KV& kv, const f32x16& x) { return x1_mma(kv, x1_cvt(x), zero16()); }
};

template <int XA> struct TokOp;
template <> struct TokOp<0> {
    typedef W2 W; typedef f32x16 A; typedef JointF32 JOp;
    static constexpr int kTileQ = kTile;
    static __device__ __forceinline__ W ldw(const float* __restrict__ Wp, int i0, int i1, int lane) { return ldw2(Wp, MDR_WIDX(i0), MDR_WIDX(i1), lane); }
    static __device__ __forceinline__ A from_scaled(const f32x16& v) { return v; }
    static __device__ __forceinline__ A from(const f32x16& v, float pre = 1.0f) { return v; }
    static __device__ __forceinline__ void store(float* p, int lane, const f32x16& v) { store_block(p, lane, v); }
    static __device__ __forceinline__ f32x16 attend(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int lane) { return self_attention_head(q, k, v, lane); }
};
template <> struct TokOp<1> {
    typedef W2X W; typedef X3 A; typedef JointF32 JOp;
    static constexpr int kTileQ = kTileX3;
    static __device__ __forceinline__ W ldw(const float* __restrict__ Wp, int i0, int i1, int lane) { return ldw2x(Wp, MDR_WIDX(i0), MDR_WIDX(i1), lane); }
    static __device__ __forceinline__ A from_scaled(const f32x16& v) { return x3_split(v); }
    static __device__ __forceinline__ A from(const f32x16& v, float pre = 1.0f) { return x3_split(v); }
    static __device__ __forceinline__ void store(float* p, int lane, const f32x16& v) { x3_store(p, lane, x3_split(v)); }
    static __device__ __forceinline__ f32x16 attend(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int lane) { return self_attention_head_x3(q, k, v, lane); }
};
// XA >= 2: the operands are fp16 planes of kActScale x value.  from_scaled takes a tile that already carries that scale (a LayerNorm whose staged
// affine part does, an attention head's output), from a tile holding `pre` x its value (pre = 1, or 1 / lin_s for a 4-product linear's raw output)
template <> struct TokOp<2> {
    typedef W2H W; typedef X2 A; typedef JointX2 JOp;
    static constexpr int kTileQ = kTile;
    static __device__ __forceinline__ W ldw(const float* __restrict__ Wp, int i0, int i1, int lane) { return ldw2h(Wp, MDR_WIDX(i0), MDR_WIDX(i1), lane); }
    static __device__ __forceinline__ A from_scaled(const f32x16& v) { return x2_split(v); }
    static __device__ __forceinline__ A from(const f32x16& v, float pre = 1.0f) { return x2_split(v * (kActScale * pre)); }
    static __device__ __forceinline__ void store(float* p, int lane, const f32x16& v) { x2_store(p, lane, x2_split(v)); }
    static __device__ __forceinline__ f32x16 attend(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int lane) { return self_attention_head_x2<true>(q, k, v, lane); }
};
template <> struct TokOp<3> {
    typedef W2G W; typedef X1 A; typedef JointX1 JOp;
    static constexpr int kTileQ = kTileX1;
    static __device__ __forceinline__ W ldw(const float* __restrict__ Wp, int i0, int i1, int lane) { return ldw2g(Wp, MDR_WIDX(i0), MDR_WIDX(i1), lane); }
    static __device__ __forceinline__ A from_scaled(const f32x16& v) { return x1_cvt(v); }
    static __device__ __forceinline__ A from(const f32x16& v, float pre = 1.0f) { return x1_cvt(v * (kActScale * pre)); }
    static __device__ __forceinline__ void store(float* p, int lane, const f32x16& v) { x1_store(p, lane, x1_cvt(v)); }
    static __device__ __forceinline__ f32x16 attend(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int lane) { return self_attention_head_x1<true>(q, k, v, lane); }
};
// floats of a Q/K/V tile per form, for the host side (launch_mdr: strides of the tile sets)
constexpr int kTileQ[4] = {TokOp<0>::kTileQ, TokOp<1>::kTileQ, TokOp<2>::kTileQ, TokOp<3>::kTileQ};

// ---- cross-attention over the J joint tokens (keys/values precomputed per sample by k_mdr_joint / k_gat_joint), one head: a masked softmax over
// at most 32 keys.  qscale: kScale / (the factor qh carries).  Returns kScale x the head's output: the operand scale of the projection that follows
template <int XA>
__device__ __forceinline__ f32x16 cross_attention_head(const float* __restrict__ kj, const float* __restrict__ vjp, const f32x16& qh, float qscale, int J, int lane) {
    typedef typename TokOp<XA>::JOp JOp;
    constexpr bool kPlanes = JOp::kScale != 1.0f;
    const int h = lane >> 5;
    const typename JOp::KV kx = JOp::load(kj, lane);
    f32x16 S;                                                              // kScale^2 x S^T[joint][token]
    if constexpr (kPlanes) S = JOp::mma(kx, qh * qscale); else S = JOp::mma(kx, qh);
    typename JOp::KV vx;
    if constexpr (kPlanes) vx = JOp::load(vjp, lane);                      // in flight during the softmax
    const float c = kLog2e * 0.17677669529663688110f * (1.0f / (JOp::kScale * JOp::kScale));    // head_dim ** -0.5 (MDR.py:25), exp2 domain
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float s = (kap(r) + 4 * h < J) ? S[r] * c : -1e30f;
        S[r] = s;
        mx = fmaxf(mx, s);
    }
    mx = fmaxf(mx, xhalf(mx));
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(S[r] - mx);
        S[r] = p;
        sum += p;
    }
    sum += xhalf(sum);
    const float inv = JOp::kPScale / sum;
    if constexpr (!kPlanes) vx = JOp::load(vjp, lane);
    const f32x16 o = JOp::mma(vx, S * inv);
    if constexpr (kPlanes) return o * (1.0f / JOp::kPScale); else return o;
}

// bias_norm (BatchNorm1d(431) over the vertex axis in eval mode, or LayerNorm(3) in the alpha variant) + GELU of a token's three bias features (MDR.py:159-160)
__device__ __forceinline__ void head_bias_act(bool alpha, const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, int v, float (&x)[3]) {
    if (alpha) {      // LayerNorm(3)
        const float m = (x[0] + x[1] + x[2]) / 3.0f;
        const float qq = ((x[0] - m) * (x[0] - m) + (x[1] - m) * (x[1] - m) + (x[2] - m) * (x[2] - m)) / 3.0f;
        const float rs = 1.0f / sqrtf(qq + 1e-5f);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = (x[c] - m) * rs * bn_w[c] + bn_b[c];
    } else {          // BatchNorm1d(431) eval: channel = vertex
        const float rs = 1.0f / sqrtf(bn_var[v] + 1e-5f);
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = (x[c] - bn_mean[v]) * rs * bn_w[v] + bn_b[v];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = gelu_f(x[c]);
}

}  // namespace
}  // namespace gator
