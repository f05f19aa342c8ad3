// GAT graph-aware transformer encoder (lib/models/GAT.py:133-152, GATBlock :33-43), six blocks in ONE launch, one workgroup per
// sample -- the form for one sample per CU (batches up to one round of the chip), built around what bounds that case.
//
// What bounds it (tools/microbench/wstream.hip, profiles/r03_microbench_weight_stream.txt).  A sample walks 1 560 operand tiles of
// split-precision weights (9.4 MB) that nobody else on its CU can share.  Streamed alone they take 85 us (54 B/clk through the
// CU's vector L1); with their 12 MFMAs each issued by the same four waves 101 us, provided those waves do nothing else.  k_gat
// (gat_fused.hip) has each of its four waves alternate between that stream, the J x J attention, LayerNorms, GELUs and operand
// splits, so the stream stops whenever the wave does anything else: 226 us.
//
// Two roles, eight waves (two per SIMD):
//   waves 0-3  "product waves": ONLY the weight stream (five tiles in flight in registers, one contiguous per-wave stream in
//              consumption order, packed at create), the bf16 MFMAs of the token-wise linears with the activation operand read
//              from LDS, and the raw fp32 accumulator parked in LDS.  Wave w owns channel block w of every 128-wide layer.
//   waves 4-7  "helper waves": everything else.  Helper w picks up product wave w's raw tile one step later and does bias,
//              residual, LayerNorm, the J x J attention of heads 2w / 2w+1 (fp32-input MFMA, scores and probabilities in
//              registers), the MGCN adjacency product, the hop-1 / hop-2 aggregations, GELU and the exact hi/mid/lo split into
//              the next operand tile.
// (Round 4, measured and not kept: s_setprio 1 / 2 / 3 on the helpers only inside their long steps -- scores + softmax, P.V, the four
// GELU steps -- moves k_gat8 by less than 1 us; round 3 had the static form making the sum worse.  The GELU as plain instead of
// packed FMAs, the file without packed fp32 or without SLP vectorisation: no change either.  With the diagnostic library:
// GATOR_GAT8_DBG=16 (helpers keep only the barriers and the L2 warm-up) 128 us against 167 for the whole kernel on one box -- the
// helpers cost 39 us, and their steps are latency (LDS round trips, barrier skew), not instruction count: 40 % fewer VALU
// instructions in the GELU steps bought 2.5 us.)
// One workgroup barrier per step, 22 steps per block; in 16 of them a product wave streams one 4-tile unit (a 32-channel output
// block over K = 128) while the helper finishes the previous unit, six are helper-only (SB, the hop aggregations, residual +
// LayerNorm twice).  Both roles live in disjoint branches of one kernel so that neither pays the other's registers; the barriers
// are numbered GAT8_BAR(n) in both and tests/test_host_cpu.py checks that the two sequences are identical.
//
// LDS (149 KiB): A = 4 operand tiles (Y = LN1(x) | Y2 = LN2(x) | hidden blocks 4w+3), B = 12 operand tiles (AT | SB | FB, later
// hidden blocks 4w+j, j < 3), R0 / R1 = 2 x 4 raw tiles (product wave w writes R[step & 1][w], helper w reads it in the next
// step), X = 4 fp32 tiles: the embedding's output (first LayerNorm), then the four partial hop-2 linears; ST = per-wave LayerNorm
// statistics.  k_gat8<false, 16>: arithmetic and operand formats are k_gat's (x3_common.h: exact three-way bf16 split, six partial
// products, fp32 accumulation); it agrees with k_gat to fp32 rounding (the MLP's four partial sums group the hidden blocks
// differently, the LayerNorm variance is combined from per-wave statistics), not bit for bit.  k_gat8<true, LR> (default): the
// token-wise products on four partial products, the J x J attention and the hop aggregations on fp16 planes; LR = the
// registers of a rows-over-tokens tile that hold tokens which exist (10 for J <= 18, 12 for J <= 20): the helpers skip the others, and
// the MLP's hidden tiles go through a C-layout GELU (hid_store) -- bitwise the results of the all-rows form.
#include "fused_common.h"
#include "fused_state.h"
#include "x3_common.h"
#include "gat8_forms.h"
#include "gat8_rows.h"
#include "gat8_tail.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace gator {
namespace {

struct Gat8Blk { const float *back32, *mc, *mdT, *aoffT, *f1b, *vecs; };
struct Gat8Args {
    int B, J;
    const float* pose2d;
    const float *gl0_W, *gl0_b, *gn_w, *gn_b, *gl3_p, *gl3_b, *posT;
    const float *biasT, *m1T, *m2T;
    const float *norm_w, *norm_b;
    const float* wstream;            // [4 product waves][390 tiles][kTileX3] (+ kNT tiles of slack behind the last wave)
    Gat8Blk blk[kDepth];
    float* feat;
    int tapB;
    float* blk_tap;
    float lin_inv;                   // H4 form: 1 / (16 x 2^weight shift), the factor every raw product tile carries
    Gat8Tail tl;                     // k_gat8<..., TAIL = true>: the lifter and the MDR joint tokens as the kernel's epilogue
    int pf_n, pf_loads;              // L2 warm-up of the next block's weights: workgroups per XCD that share it, 8 KiB touches per helper wave (0: off)
#ifdef GATOR_DIAG
    unsigned long long* stamps;      // [2 roles][kDepth][23 steps][work, wait]
    int dbg;                         // GATOR_GAT8_DBG: 1 = helpers only keep the barriers (what do the product waves cost alone?)
#endif
};

#ifdef GATOR_DIAG
// diagnostic library only (python -m gator_amd.build --diag; GATOR_GAT_STAMPS=1): per role, block and step the cycles spent working
// (from leaving the previous barrier to arriving at this one) and waiting in the barrier, of workgroup 0's waves 0 and 4; written to
// LDS, copied out by GAT8_STAMPS_OUT when the role is done
#define GAT8_BAR(n)                                                                                      \
    do {                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        const unsigned long long t_arr_ = __builtin_amdgcn_s_memtime();                                  \
        __syncthreads();                                                                                 \
        const unsigned long long t_go_ = __builtin_amdgcn_s_memtime();                                   \
        if (st_out) { st_out[((size_t)bi_ * 23 + (n)) * 2] = t_arr_ - st_last; st_out[((size_t)bi_ * 23 + (n)) * 2 + 1] = t_go_ - t_arr_; } \
        st_last = t_go_;                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
    } while (0)
#define GAT8_STAMPS_OUT(n0, n1)                                                                          \
    do { if (st_out) for (int i_ = (n0); i_ < (n1); ++i_) a.stamps[i_] = st_lds[i_]; } while (0)
#define GAT8_SUB(k)                                                                                     \
    do {                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        if (st_out) st_out[(size_t)kDepth * 23 * 2 + bi_ * 8 + (k)] = __builtin_amdgcn_s_memtime() - st_last;              \
        __builtin_amdgcn_sched_barrier(0);                                                               \
    } while (0)
#else
#define GAT8_BAR(n) __syncthreads()
#define GAT8_SUB(k)
#define GAT8_STAMPS_OUT(n0, n1)
#endif

// A helper wave is alone with its own dependency chains (its SIMD partner issues MFMAs, nobody fills its latency slots), so the
// reductions are trees of independent partial sums and the GELU walks its polynomial level by level (fused_common.h: gelu_pairs).
__device__ __forceinline__ float rsum128(const f32x16 (&x)[4]) {
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        p[q] = 0.f;
#pragma unroll
        for (int r = 4 * q; r < 4 * q + 4; ++r) p[q] += (x[0][r] + x[1][r]) + (x[2][r] + x[3][r]);
    }
    const float s = (p[0] + p[1]) + (p[2] + p[3]);
    return s + xhalf(s);
}

// nn.LayerNorm(128) of the residual stream X (4 fp32 tiles in LDS): statistics over all four tiles, result for this wave's own
// channel block only (xw = its registers, the same values as X[w]); same operation order as k_gat's layernorm128
__device__ __forceinline__ f32x16 ln_own(const float* X, const f32x16& xw, const f32x16& wv, const f32x16& bv, int lane) {
    f32x16 x[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) x[kb] = load_block(X + kb * kTile, lane);
    const float mean = rsum128(x) * (1.0f / 128.0f);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) { x[kb] = x[kb] - mean; x[kb] = x[kb] * x[kb]; }
    const float rstd = 1.0f / sqrtf(rsum128(x) * (1.0f / 128.0f) + 1e-5f);
    return (xw - mean) * rstd * wv + bv;
}

// LayerNorm(128) inside the block loop without a second pass over the residual stream: the wave that updates its 32 channels of a
// token leaves their (mean, sum of squared deviations) in LDS, and the four pairs of a token are combined exactly (Chan et al.):
// M2 = sum M2_w + 32 sum (mean_w - mean)^2.  ln_own re-read all four tiles and reduced twice in a step the product waves wait through.
__device__ __forceinline__ void tile_stats(const f32x16& xw, float* st_w, int lane) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) s += (xw[4 * q] + xw[4 * q + 1]) + (xw[4 * q + 2] + xw[4 * q + 3]);
    s += xhalf(s);
    const float m = s * (1.0f / 32.0f);
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        p[q] = 0.f;
#pragma unroll
        for (int r = 4 * q; r < 4 * q + 4; ++r) { const float d = xw[r] - m; p[q] += d * d; }
    }
    float m2 = (p[0] + p[1]) + (p[2] + p[3]);
    m2 += xhalf(m2);
    if (lane < 32) { st_w[2 * lane] = m; st_w[2 * lane + 1] = m2; }
}
__device__ __forceinline__ f32x16 ln_stats(const float* ST, const f32x16& xw, const f32x16& wv, const f32x16& bv, int lane) {
    const int tok = lane & 31;
    float m[4], q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] = ST[i * 64 + 2 * tok]; q[i] = ST[i * 64 + 2 * tok + 1]; }
    const float mean = ((m[0] + m[1]) + (m[2] + m[3])) * 0.25f;
    float dev = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float d = m[i] - mean; dev += d * d; }
    const float m2 = ((q[0] + q[1]) + (q[2] + q[3])) + 32.0f * dev;
    const float rstd = 1.0f / sqrtf(m2 * (1.0f / 128.0f) + 1e-5f);
    return (xw - mean) * rstd * wv + bv;
}

// one k-step of the two-plane product (x3_common.h: x2_mma does both): lo*hi | hi*lo | hi*hi
__device__ __forceinline__ f32x16 x2_mma_step(const X2& A, const X2& B, int s, f32x16 acc) {
    acc = GATOR_MFMA_F16(A.p[1][s], B.p[0][s], acc);
    acc = GATOR_MFMA_F16(A.p[0][s], B.p[1][s], acc);
    return GATOR_MFMA_F16(A.p[0][s], B.p[0][s], acc);
}

// H4: the token-wise products on four partial products (weights H3, operands X2; raw tiles carry 1 / a.lin_inv) instead of six
template <bool H4, int LR, bool H2 = false, bool LB = false, bool TAIL = false>
__global__ __launch_bounds__(512, 2) void k_gat8(const Gat8Args a) {
    static_assert(H4 || !TAIL, "the fused tail writes two-plane K / V tiles: four-product forms only");
    using F = Gat8Stream<H4, H2, LB>;                           // the form of the weight stream (gat8_forms.h)
    constexpr int kWF = F::kTileFloats;                         // floats per tile of the weight stream
    const float inv = H4 ? a.lin_inv : 1.0f;
    // operand tile of a true-scale register tile; pick-up of a raw product tile with what is added to it
    // Token lanes that do not exist (15 of a tile's 32 at J = 17) store ZERO operands: no live value changes (a token's row never
    // meets another token's except through the masked J x J operators), but the MFMAs stop toggling on 47 % of their columns and
    // the chip holds a higher clock -- k_gat8 163.7 -> 159.7 us on one box, bit-identical results (DESIGN.md 4c on why data matters).
    const float op16 = ((threadIdx.x & 31) < a.J) ? 16.0f : 0.0f;
    auto st_opnd = [&](float* dst, int lane_, const f32x16& v) {
        if constexpr (H4) x2_store(dst, lane_, x2_split(v * op16)); else x3_store(dst, lane_, x3_split(v));
    };
    auto pick = [&](const float* raw, int lane_, const f32x16& add) {
        if constexpr (H4) return fma16(load_block(raw, lane_), inv, add); else return load_block(raw, lane_) + add;
    };
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* A = lds + kA;
    float* Bq = lds + kBq;
    float* X = lds + kXo;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, h = lane >> 5, J = a.J;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool is_prod = wave < 4;
    const int w = wave & 3;                              // channel block of this wave (either role).  Waves i and i + 4 share a SIMD: every
                                                         // SIMD hosts one product and one helper wave (both product waves of a pair on one
                                                         // SIMD, helpers on the other two: 180 us instead of 162, measured in round 4)
    float* R0w = lds + kR + w * kTile;
    float* R1w = lds + kR + (4 + w) * kTile;
    if constexpr (TAIL) {      // the persistent MDR launch's counter blocks (tickets, error flag, completion counts), dealt over the workgroups:
        if (a.tl.mdr_ctr)      // the previous forward's launches are complete (stream order), this forward's start after this kernel
            for (size_t i = (size_t)b * 512 + t; i < mdr_ctr_words(a.tl.ctr_B); i += (size_t)a.B * 512) a.tl.mdr_ctr[i] = 0u;
    }

    // ---------------- embedding: GraphLinear(2->64) . GroupNorm(4,64) . GELU . GraphLinear(64->128) + pos (GAT.py:135-144)
    {
        float* hbuf = Bq;                 // [64][32]
        float* gt = Bq + 2 * kTile;       // 2 T-layout tiles
        float* stat = Bq + 4 * kTile;     // [4][2]
        const float* p = a.pose2d + (size_t)b * J * 2;
        for (int e = t; e < 64 * 32; e += 512) {
            const int c = e >> 5, j = e & 31;
            hbuf[e] = j < J ? a.gl0_W[c * 2] * p[j * 2] + a.gl0_W[c * 2 + 1] * p[j * 2 + 1] + a.gl0_b[c] : 0.f;
        }
        __syncthreads();
        if (!is_prod) {   // helper w -> GroupNorm group w (16 channels x J tokens), two-pass
            float s = 0.f;
            for (int e = lane; e < 16 * 32; e += 64) s += ((e & 31) < J) ? hbuf[w * 512 + e] : 0.f;
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const float mean = s / (16.0f * J);
            float q = 0.f;
            for (int e = lane; e < 16 * 32; e += 64) {
                const float d = hbuf[w * 512 + e] - mean;
                q += ((e & 31) < J) ? d * d : 0.f;
            }
            for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
            if (lane == 0) { stat[w * 2] = mean; stat[w * 2 + 1] = 1.0f / sqrtf(q / (16.0f * J) + 1e-5f); }
        }
        __syncthreads();
        // GroupNorm affine + GELU as two T-layout operand tiles gt[kb][g][lane][j] <-> token lane&31, channel 32kb+8g+4h+j
        for (int e = t; e < 2 * kTile; e += 512) {
            const int j4 = e & 3, ln = (e >> 2) & 63, g = (e >> 8) & 3, kb = e >> 10;
            const int tok = ln & 31, c = 32 * kb + 8 * g + 4 * (ln >> 5) + j4;
            gt[e] = tok < J ? gelu_f((hbuf[c * 32 + tok] - stat[(c >> 4) * 2]) * stat[(c >> 4) * 2 + 1] * a.gn_w[c] + a.gn_b[c]) : 0.f;
        }
        __syncthreads();
        if (!is_prod) {   // GraphLinear(64->128) on the fp32-input MFMA: helper w -> channel block w; + folded position tiles
            f32x16 acc = load_chanvec_T(a.gl3_b, 32 * w, h) + load_block(a.posT + (size_t)w * kTile, lane), ac1 = zero16();
            mma2_T(load_wtile(a.gl3_p, w * 2 + 0, lane), load_block(gt, lane), acc, load_wtile(a.gl3_p, w * 2 + 1, lane),
                   load_block(gt + kTile, lane), ac1);
            store_block(X + w * kTile, lane, acc + ac1);
        }
        __syncthreads();
    }

    // From here on the two roles run in DISJOINT branches and meet only at workgroup barriers: s_barrier counts arrivals, it does not
    // care which branch a wave arrives from, so this is well defined exactly as long as both branches execute the SAME NUMBER of
    // barriers in the same order -- barrier 0, then 1 .. 22 per block, each written with the numbered macro.  tests/test_host_cpu.py parses this file and fails if the
    // two sequences differ (a barrier only one role executes hangs the GPU); keep that test in the CPU suite.
    if (is_prod) {
        // =========================================== product waves ===========================================================
        typename F::W W[kNT];                                                          // the head of the weight stream (held back until here: five tiles
        const float* __restrict__ wp = a.wstream + (size_t)w * kWaveTiles * kWF;         // live across the embedding would spill)
#pragma unroll
        for (int s = 0; s < kNT; ++s) { W[s] = F::load(wp, lane); wp += kWF; }
        asm volatile("" ::: "memory");
#ifdef GATOR_DIAG
        unsigned long long* st_lds = reinterpret_cast<unsigned long long*>(lds + kGat8LdsFloats);
        unsigned long long* st_out = (a.stamps && b == 0 && w == 0 && lane == 0) ? st_lds : nullptr;
        if (st_out) for (int i_ = 0; i_ < kDepth * 23 * 2; ++i_) st_lds[i_] = 0;
        unsigned long long st_last = __builtin_amdgcn_s_memtime();
        int bi_ = 0;
#endif
        GAT8_BAR(0);                                                        // helpers: Y = LN1(x) of block 0
#pragma unroll 1
        for (int bi = 0; bi < kDepth; ++bi) {
#ifdef GATOR_DIAG
            bi_ = bi;
#endif
            const float *Y0 = A, *Y1 = A + kTileX3, *Y2 = A + 2 * kTileX3, *Y3 = A + 3 * kTileX3;
            typename F::O pre;
            pre = F::load_opnd(Y0, lane);
            unit4<F, gat8_slot(U_Q), false>(W, wp, pre, Y1, Y2, Y3, R0w, lane);             // q  (T)
            pre = F::load_opnd(Y0, lane);
            GAT8_BAR(1);
            unit4<F, gat8_slot(U_K), false>(W, wp, pre, Y1, Y2, Y3, R1w, lane);             // k  (T)
            pre = F::load_opnd(Y0, lane);
            GAT8_BAR(2);
            unit4<F, gat8_slot(U_V), true>(W, wp, pre, Y1, Y2, Y3, R0w, lane);              // v  (C)
            pre = F::load_opnd(Y0, lane);
            GAT8_BAR(3);
            unit4<F, gat8_slot(U_H0), false>(W, wp, pre, Y1, Y2, Y3, R1w, lane);             // h0 = y W[0]  (T: its MGCN term is token-wise)
            pre = F::load_opnd(Y0, lane);
            GAT8_BAR(4);
            unit4<F, gat8_slot(U_H1), true>(W, wp, pre, Y1, Y2, Y3, R0w, lane);              // h1 = y W[1]  (C)
            GAT8_BAR(5);
            pre = F::load_opnd(Bq, lane);
            unit4<F, gat8_slot(U_PROJ), false>(W, wp, pre, Bq + kTileX3, Bq + 2 * kTileX3, Bq + 3 * kTileX3, R1w, lane);                   // proj(AT)
            GAT8_BAR(6);
            GAT8_BAR(7);                                                    // helpers: SB = proj + attention bias + MGCN
            pre = F::load_opnd(Bq + 4 * kTileX3, lane);
            unit4<F, gat8_slot(U_LIN0), true>(W, wp, pre, Bq + 5 * kTileX3, Bq + 6 * kTileX3, Bq + 7 * kTileX3, R0w, lane);                // linears[0](SB)  (C)
            unit1<F, gat8_slot(U_LIN1)>(W, wp, Bq + (4 + w) * kTileX3, X + w * kTile, lane);                                              // linears[1], k block w
            GAT8_BAR(8);
            GAT8_BAR(9);                                                    // helpers: hop aggregations -> FB
            pre = F::load_opnd(Bq + 8 * kTileX3, lane);
            unit4<F, gat8_slot(U_BACK), false>(W, wp, pre, Bq + 9 * kTileX3, Bq + 10 * kTileX3, Bq + 11 * kTileX3, R1w, lane);             // linearback(FB), k < 128
            GAT8_BAR(10);
            GAT8_BAR(11);                                                   // helpers: residual
            GAT8_BAR(12);                                                   // helpers: Y2 = LN2(x)
            pre = F::load_opnd(Y0, lane);
            unit4<F, gat8_slot(U_FC1, 0), H4>(W, wp, pre, Y1, Y2, Y3, R0w, lane);             // fc1, hidden block 4w
            pre = F::load_opnd(Y0, lane);
            GAT8_BAR(13);
            unit4<F, gat8_slot(U_FC1, 4), H4>(W, wp, pre, Y1, Y2, Y3, R1w, lane);             //      4w + 1
            pre = F::load_opnd(Y0, lane);
            GAT8_BAR(14);
            unit4<F, gat8_slot(U_FC1, 8), H4>(W, wp, pre, Y1, Y2, Y3, R0w, lane);             //      4w + 2
            pre = F::load_opnd(Y0, lane);
            GAT8_BAR(15);
            unit4<F, gat8_slot(U_FC1, 12), H4>(W, wp, pre, Y1, Y2, Y3, R1w, lane);             //      4w + 3
            pre = F::template load_opnd<H4>(Bq, lane);                                    // (hidden blocks 4w' were complete at barrier 14)
            GAT8_BAR(16);
            // fc2: unit u contracts over hidden blocks {4w' + u}: tiles 3w' + u of B for u < 3, tile w' of A for u = 3
            unit4<F, gat8_slot(U_FC2, 0), false, H4>(W, wp, pre, Bq + 3 * kTileX3, Bq + 6 * kTileX3, Bq + 9 * kTileX3, R0w, lane);
            pre = F::template load_opnd<H4>(Bq + 1 * kTileX3, lane);
            GAT8_BAR(17);
            unit4<F, gat8_slot(U_FC2, 4), false, H4>(W, wp, pre, Bq + 4 * kTileX3, Bq + 7 * kTileX3, Bq + 10 * kTileX3, R1w, lane);
            pre = F::template load_opnd<H4>(Bq + 2 * kTileX3, lane);
            GAT8_BAR(18);
            unit4<F, gat8_slot(U_FC2, 8), false, H4>(W, wp, pre, Bq + 5 * kTileX3, Bq + 8 * kTileX3, Bq + 11 * kTileX3, R0w, lane);
            pre = F::template load_opnd<H4>(Y0, lane);                                    // (hidden blocks 4w' + 3, complete at barrier 17)
            GAT8_BAR(19);
            unit4<F, gat8_slot(U_FC2, 12), false, H4>(W, wp, pre, Y1, Y2, Y3, R1w, lane);
            skip_pad<F, gat8_slot(U_COUNT)>(W, wp, lane);                          // the block's dummy tiles: refill their slots, no product
            GAT8_BAR(20);
            if constexpr (TAIL) {
                if (bi + 1 == kDepth) {      // idle from here on: stage the epilogue's vectors and pos_j tiles (the operand tiles are dead), fetch the first lifter rows
                    if (a.tl.jkv) {
                        const Gat8Tail& tl = a.tl;
                        if (t < VJ_TOTAL / 4) joint_stage_vecs(tl, lds + kTVJ, t);
                        for (int e = t; e < 2 * kTile / 4; e += 256)
                            reinterpret_cast<f32x4*>(lds + kTPosj)[e] = reinterpret_cast<const f32x4*>(tl.posj_T)[e];
                    }
                }
            }
            GAT8_BAR(21);                                                   // helpers: residual
            GAT8_BAR(22);                                                   // helpers: Y = LN1(x) of the next block | final norm
        }
        GAT8_STAMPS_OUT(0, kDepth * 23 * 2);
        if constexpr (TAIL) gat8_tail<LR, false>(a.tl, a.pose2d, lds, b, J, w, lane);
        return;
    }

    // =============================================== helper waves ===============================================================
    const int tok = lane & 31;
    const HidAddr hid = hid_addr(lane);
#ifdef GATOR_DIAG
    if (a.dbg & 1) {
        for (int n = 0; n < 1 + 22 * kDepth; ++n) __syncthreads();
        return;
    }
    if (a.dbg & 16) {      // barriers + the L2 warm-up of the weight streams only: what the product waves cost with warm weights
        __syncthreads();       // (warm_weights of the block loop, written again: shared as a function it moves every form's instructions)
        for (int bi = 0; bi < kDepth; ++bi)
            for (int n = 1; n <= 22; ++n) {
                if ((n == 2 || n == 19) && bi + 1 < kDepth && a.pf_loads > 0) {
                    const char* wsrc = reinterpret_cast<const char*>(a.wstream + ((size_t)w * kWaveTiles + (size_t)(bi + 1) * kBlkTiles) * kWF);
                    const int share = a.pf_loads * 8192, first = ((b >> 3) % a.pf_n) * share, lim = kBlkTiles * kWF * 4 - 128;
                    const int i0 = n == 2 ? 0 : (a.pf_loads + 1) / 2, i1 = n == 2 ? (a.pf_loads + 1) / 2 : a.pf_loads;
                    for (int i = i0; i < i1; ++i)
                        glds<4>(reinterpret_cast<const float*>(wsrc + min(first + i * 8192 + lane * 128, lim)), lds + kDummy + w * 256);
                }
                __syncthreads();
            }
        return;
    }
    unsigned long long* st_lds = reinterpret_cast<unsigned long long*>(lds + kGat8LdsFloats);
    unsigned long long* st_out = (a.stamps && b == 0 && w == 0 && lane == 0) ? st_lds + (size_t)kDepth * 23 * 2 : nullptr;
    if (st_out) for (int i_ = 0; i_ < kDepth * 23 * 2 + kDepth * 8; ++i_) st_out[i_] = 0;
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
    int bi_ = 0;
#endif
    f32x16 xw = load_block(X + w * kTile, lane);          // this wave's channel block of the residual stream
    {
        const float* vec = a.blk[0].vecs;
        const f32x16 y = ln_own(X, xw, load_chanvec_T(vec, V_N1W + 32 * w, h), load_chanvec_T(vec, V_N1B + 32 * w, h), lane);
        st_opnd(A + w * kTileX3, lane, y);
    }
    GAT8_BAR(0);
#pragma unroll 1
    for (int bi = 0; bi < kDepth; ++bi) {
#ifdef GATOR_DIAG
        bi_ = bi;
#endif
        const Gat8Blk& kb = a.blk[bi];
        const float* vec = kb.vecs;
        // L2 warm-up.  Between two launches of this kernel the rest of the forward moves ~1 GB, so the weights start in HBM; all
        // workgroups of an XCD walk them in step, so every tile would be an HBM-latency miss for all of them at once (175 -> 195 us
        // without it).  Each workgroup pulls its 1/n-th of the NEXT block's four streams into its XCD's L2 one block ahead, and this
        // helper's share of that block's tables.  One dword per 128-byte line: a wave instruction touches 64 lines = 8 KiB and costs the
        // issuing wave ~350 cycles, so the touches sit in the steps where the helper has slack against its product wave (2 and 18).
        const bool warm = bi + 1 < kDepth && a.pf_loads > 0;
        const float* dummy = lds + kDummy + w * 256;
        const Gat8Blk& nx = a.blk[bi + 1 < kDepth ? bi + 1 : bi];
        auto warm_weights = [&](int i0, int i1) {
            const char* wsrc = reinterpret_cast<const char*>(a.wstream + ((size_t)w * kWaveTiles + (size_t)(bi + 1) * kBlkTiles) * kWF);
            const int share = a.pf_loads * 8192, first = ((b >> 3) % a.pf_n) * share, lim = kBlkTiles * kWF * 4 - 128;
            for (int i = i0; i < i1; ++i)
                glds<4>(reinterpret_cast<const float*>(wsrc + min(first + i * 8192 + lane * 128, lim)), dummy);
        };
        // ---- step 1: constants of the attention (nothing to pick up yet)
        const f32x16 bq = load_chanvec_T(vec, V_QKVB + 32 * w, h), bk = load_chanvec_T(vec, V_QKVB + 128 + 32 * w, h);
        const float vb = vec[V_QKVB + 256 + 32 * w + tok];
        const f32x16 ba = load_block(a.biasT + (size_t)(2 * w) * kTile, lane), bb = load_block(a.biasT + (size_t)(2 * w + 1) * kTile, lane);
        GAT8_BAR(1);
        // ---- step 2: q
        const f32x16 q = pick(R0w, lane, bq);
        X2 qx;                                                 // H4: q on two planes already here (the helper has slack in this step)
        if constexpr (H4) qx = x2_split(q * op16);            // (op16: zero for the token lanes that do not exist)
        if (warm) warm_weights(0, (a.pf_loads + 1) / 2);
        if constexpr (TAIL) {
            // The epilogue's weights are HBM-cold like the streams (the lifter's 444 KB at J = 17, the joint-token linear's and the three
            // layers' wk / wv H3 tiles): every workgroup of the XCD would miss on them together.  One block ahead -- the last block has no
            // next block to warm -- this helper pulls its share of each region into the XCD's L2, one dword per 128-byte line.
            if (bi + 1 == kDepth && a.tl.warm_n > 0) {
                const int idx = ((b >> 3) % a.tl.warm_n) * 4 + w, parts = a.tl.warm_n * 4;
                auto touch = [&](const float* base, int bytes) {
                    const int share = ((bytes / parts + 127) / 128) * 128;
                    for (int off = lane * 128; off < share; off += 8192)
                        glds<4>(reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + min(idx * share + off, bytes - 128)), dummy);
                };
                touch(a.tl.lifter_w, 3 * J * kC * J * 4);
                if (a.tl.jkv) {
                    touch(a.tl.jf_h3, 8 * kTileX3 * 4);
#pragma unroll 1
                    for (int li = 0; li < 3; ++li) touch(a.tl.j_wk_h3[li], 8 * kTileX3 * 4);      // wk | wv: eight contiguous tiles of the layer's grid
                }
            }
        }
        GAT8_BAR(2);
        // ---- step 3: k; scores and softmax of heads 2w, 2w+1 (modules.py:121-133): S^T[key][query], query on the lane
        f32x16 sa = zero16(), sb = zero16();
        {
            const f32x16 k = pick(R1w, lane, bk);
            float sscale = 0.25f;
            if constexpr (H4) {      // q, k on two fp16 planes of 16 x value: a head's 16 channels are exactly one k-step (registers 0..7 | 8..15)
                const X2 kx = x2_split(k * op16);
                sa = GATOR_MFMA_F16(kx.p[1][0], qx.p[0][0], sa);
                sb = GATOR_MFMA_F16(kx.p[1][1], qx.p[0][1], sb);
                sa = GATOR_MFMA_F16(kx.p[0][0], qx.p[1][0], sa);
                sb = GATOR_MFMA_F16(kx.p[0][1], qx.p[1][1], sb);
                sa = GATOR_MFMA_F16(kx.p[0][0], qx.p[0][0], sa);
                sb = GATOR_MFMA_F16(kx.p[0][1], qx.p[0][1], sb);
                sscale = 0.25f / 256.0f;
            } else {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    sa = GATOR_MFMA(k[r], q[r], sa);                                // head 2w:   channels 0..15 of the block
                    sb = GATOR_MFMA(k[r + 8], q[r + 8], sb);                        // head 2w+1: channels 16..31
                }
            }
            // rows = keys: only registers r < LR can hold a key that exists (the others' probability is exactly 0)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (r < LR) {
                    const bool ok = kap(r) + 4 * h < J;
                    sa[r] = ok ? (sa[r] * sscale + ba[r]) * kLog2e : -1e30f;        // q k^T * head_dim**-0.5 + hop/path bias
                    sb[r] = ok ? (sb[r] * sscale + bb[r]) * kLog2e : -1e30f;
                } else {
                    sa[r] = 0.f;
                    sb[r] = 0.f;
                }
            }
            float ma = sa[0], mb = sb[0], la, lb;
            {   // row maxima; sums as trees (four independent partials each)
#pragma unroll
                for (int r = 1; r < LR; ++r) { ma = fmaxf(ma, sa[r]); mb = fmaxf(mb, sb[r]); }
                ma = fmaxf(ma, xhalf(ma));
                mb = fmaxf(mb, xhalf(mb));
#pragma unroll
                for (int r = 0; r < LR; ++r) {
                    sa[r] = __builtin_amdgcn_exp2f(sa[r] - ma);
                    sb[r] = __builtin_amdgcn_exp2f(sb[r] - mb);
                }
                float pa[4], pb[4];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    pa[q4] = tree4<LR>(q4, [&](int r) { return sa[r]; });
                    pb[q4] = tree4<LR>(q4, [&](int r) { return sb[r]; });
                }
                la = LR > 12 ? (pa[0] + pa[1]) + (pa[2] + pa[3]) : LR > 8 ? (pa[0] + pa[1]) + pa[2] : pa[0] + pa[1];
                lb = LR > 12 ? (pb[0] + pb[1]) + (pb[2] + pb[3]) : LR > 8 ? (pb[0] + pb[1]) + pb[2] : pb[0] + pb[1];
            }
            la += xhalf(la);
            lb += xhalf(lb);
            const float ia = 1.0f / la, ib = 1.0f / lb;
#pragma unroll
            for (int r = 0; r < LR; ++r) { sa[r] = sa[r] * ia; sb[r] = sb[r] * ib; }
        }
        GAT8_BAR(3);
        // ---- steps 4, 5: v; P.V (both heads, rows 0..15 <- head 2w, rows 16..31 <- head 2w+1); pick up h0 in between
        f32x16 O = zero16(), Ob = zero16();
        const bool lo = tok < 16;
        {
            f32x16 v = load_block(R0w, lane);
            if constexpr (H4) v = v * inv;
            X2 va, vbx, pa, pb;      // H4: V of head 2w (channel lanes 0..15) / head 2w+1 (16..31) and the two probability tiles on two planes
            if constexpr (H4) {
                const X2 vx = x2_split_rows<LR>((v + vb) * 16.0f);      // rows = keys
                const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) { va.p[pl][ks] = lo ? vx.p[pl][ks] : z; vbx.p[pl][ks] = lo ? z : vx.p[pl][ks]; }
                pa = x2_split_rows<LR>(sa * (4.0f * op16));          // x 64, or zero for a query lane that does not exist
                pb = x2_split_rows<LR>(sb * (4.0f * op16));
                O = x2_mma_step(va, pa, 0, O);
                Ob = x2_mma_step(vbx, pb, 0, Ob);
            } else {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const float vv = v[r] + vb;
                    O = GATOR_MFMA(lo ? vv : 0.f, sa[r], O);
                    Ob = GATOR_MFMA(lo ? 0.f : vv, sb[r], Ob);
                }
            }
            GAT8_BAR(4);
            const f32x16 mdt = load_block(kb.mdT + (size_t)w * kTile, lane);        // (constants are requested about one step before their use)
            f32x16 h0 = load_block(R1w, lane);
            if constexpr (H4) h0 = h0 * inv;
            if constexpr (H4) {
                O = x2_mma_step(va, pa, 1, O);
                Ob = x2_mma_step(vbx, pb, 1, Ob);
                x2_store(Bq + w * kTileX3, lane, x2_split((O + Ob) * (op16 * (1.0f / 1024.0f))));      // AT[w]: O carries 16 x 64
            } else {
#pragma unroll
                for (int r = 8; r < 16; ++r) {
                    const float vv = v[r] + vb;
                    O = GATOR_MFMA(lo ? vv : 0.f, sa[r], O);
                    Ob = GATOR_MFMA(lo ? 0.f : vv, sb[r], Ob);
                }
                st_opnd(Bq + w * kTileX3, lane, O + Ob);                            // AT[w]
            }
            O = h0 * mdt;                                                          // diag(A)[t] * M[t][n] * h0[t][n]  (O re-used)
        }
        const f32x16 mct = load_block(kb.mc + (size_t)w * kTile, lane), aoff = load_block(kb.aoffT, lane);
        const f32x16 bg = load_chanvec_T(vec, V_GCNB + 32 * w, h);
        GAT8_BAR(5);
        // ---- step 6: h1; MGCN (modules.py:243-255): sum_j (M.h1)[j][n] Aoff[t][j] as one MFMA product + the token-wise term
        f32x16 g_out;
        {
            f32x16 h1 = load_block(R0w, lane);
            if constexpr (H4) h1 = h1 * inv;
            h1 = h1 * mct;
            g_out = dot16_rows<LR>(h1, aoff, bg) + O;          // k = token j: Aoff[t][j] is zero for the rows that do not exist
        }
        const f32x16 bp = load_chanvec_T(vec, V_PROJB + 32 * w, h);
        GAT8_BAR(6);
        // ---- step 7: SB = proj(attention) + bias + MGCN
        {
            const f32x16 acc = pick(R1w, lane, bp);
            st_opnd(Bq + (4 + w) * kTileX3, lane, acc + g_out);
        }
        GAT8_BAR(7);
        // constants of the X_Feat steps
        const f32x16 m1 = load_block(a.m1T, lane), m2 = load_block(a.m2T, lane);
        const float b0 = vec[V_LIN0B + 32 * w + tok];
        f32x16 f1 = load_block(kb.f1b, lane);                                      // rowsum(m2)[t] * linears[1].bias[n]
        GAT8_BAR(8);
        // ---- step 9: X_Feat (modules.py:158-177): hop<=1 aggregation of linears[0], hop==2 aggregation of linears[1]
        {
            const f32x16 u0 = pick(R0w, lane, f32x16(b0));
            f32x16 u1 = (load_block(X, lane) + load_block(X + kTile, lane)) + (load_block(X + 2 * kTile, lane) + load_block(X + 3 * kTile, lane));
            if constexpr (H4) {
                // the hop masks are 0 / 1: one exact fp16 plane; the aggregated tiles on two planes like every other operand of this
                // form -> 2 x 4 fp16 MFMAs (256 cycles) instead of 32 fp32-input ones (2 048) in a step the product waves wait through
                const X2 u0x = x2_split_rows<LR>(u0 * 16.0f), u1x = x2_split_rows<LR>(u1 * (16.0f * inv));      // rows = the aggregated token
                f32x16 f0 = zero16(), f1a = zero16();
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    f16x8 m1h, m2h;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const bool live = 8 * s + j < LR;
                        m1h[j] = live ? (_Float16)m1[8 * s + j] : (_Float16)0.f;
                        m2h[j] = live ? (_Float16)m2[8 * s + j] : (_Float16)0.f;
                    }
                    f0 = GATOR_MFMA_F16(u0x.p[1][s], m1h, f0);
                    f1a = GATOR_MFMA_F16(u1x.p[1][s], m2h, f1a);
                    f0 = GATOR_MFMA_F16(u0x.p[0][s], m1h, f0);
                    f1a = GATOR_MFMA_F16(u1x.p[0][s], m2h, f1a);
                }
                x2_store(Bq + (8 + w) * kTileX3, lane, x2_split(f0));              // FB[w]: f0 already carries the operand scale 16
                f1 = fma16(f1a, 1.0f / 16.0f, f1);
            } else {
                f32x16 f0 = zero16(), f1a = zero16();
                dot16x2(u0, m1, f0, u1, m2, f1a);
                st_opnd(Bq + (8 + w) * kTileX3, lane, f0);                        // FB[w]
                f1 += f1a;
            }
        }
        const f32x16 bback = load_chanvec_T(vec, V_BACKB + 32 * w, h);
        f32x4 wb40, wb41;                                                          // linearback's k block 4 (fp32 tile): only k < 16 is live
        {
            const f32x4* p = reinterpret_cast<const f32x4*>(kb.back32) + ((size_t)(w * 5 + 4) * 4) * 64 + lane;
            wb40 = p[0];
            wb41 = p[64];
        }
        GAT8_BAR(9);
        // ---- step 10: linearback's k tail (channels 128..143 <- the hop-2 features), exact fp32 products
        f32x16 tl = bback, tl2 = zero16();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tl = GATOR_MFMA(wb40[j], f1[j], tl);
            tl2 = GATOR_MFMA(wb41[j], f1[4 + j], tl2);
        }
        const f32x16 n2w = load_chanvec_T(vec, V_N2W + 32 * w, h), n2b = load_chanvec_T(vec, V_N2B + 32 * w, h);
        GAT8_BAR(10);
        // ---- step 11: residual
        xw += pick(R1w, lane, tl) + tl2;
        tile_stats(xw, lds + kStat + w * 64, lane);
        GAT8_BAR(11);
        // ---- step 12: Y2 = LN2(x)
        st_opnd(A + w * kTileX3, lane, ln_stats(lds + kStat, xw, n2w, n2b, lane));
        GAT8_BAR(12);
        // ---- steps 13-17: MLP hidden blocks 4w + j: bias, GELU, split (modules.py:188-196).  H4: the raw tile is in C layout (channel
        // on the lane: ONE bias value per lane; token rows r < LR in the registers), see hid_store; else T layout, all 16 registers.
        struct FcBias { float s; f32x16 v; };
        auto fc1_bias = [&](int j) {
            FcBias o;
            if constexpr (H4) {
                o.v = zero16();
#ifdef GATOR_DIAG
                if (a.dbg & 8) { o.s = 0.f; return o; }
#endif
                o.s = vec[V_FC1B + 32 * (4 * w + j) + (lane & 31)];
            }
            else { o.s = 0.f; o.v = load_chanvec_T(vec, V_FC1B + 32 * (4 * w + j), h); }
            return o;
        };
        auto hidden = [&](const float* raw, float* dst, const FcBias& fb) {
            if constexpr (H4) {
                f32x16 hd = fma16(load_block_rows<LR>(raw, lane), inv, f32x16(fb.s));
                GAT8_SUB(0);
#ifdef GATOR_DIAG
                if (!(a.dbg & 2))
#endif
                gelu_pairs<LR / 2>(hd);
                GAT8_SUB(1);
#ifdef GATOR_DIAG
                if (!(a.dbg & 4))
#endif
                hid_store<LR>(dst, hid, hd);
                GAT8_SUB(3);
            } else {
                f32x16 hd = pick(raw, lane, fb.v);
                gelu_pairs<8>(hd);
                st_opnd(dst, lane, hd);
            }
        };
        FcBias fb0 = fc1_bias(0), fb1 = fc1_bias(1);
        GAT8_BAR(13);
        hidden(R0w, Bq + (3 * w + 0) * kTileX3, fb0);
        fb0 = fc1_bias(2);
        GAT8_BAR(14);
        hidden(R1w, Bq + (3 * w + 1) * kTileX3, fb1);
        fb1 = fc1_bias(3);
        GAT8_BAR(15);
        hidden(R0w, Bq + (3 * w + 2) * kTileX3, fb0);
        GAT8_BAR(16);
        hidden(R1w, A + w * kTileX3, fb1);                                             // (Y2 is dead: fc1 finished before barrier 16)
        const f32x16 bfc2 = load_chanvec_T(vec, V_FC2B + 32 * w, h);
        GAT8_BAR(17);
        // ---- steps 18-21: the four partial sums of fc2, residual
        f32x16 c01 = pick(R0w, lane, bfc2);
        GAT8_BAR(18);
        c01 = pick(R1w, lane, c01);
        if (warm) warm_weights((a.pf_loads + 1) / 2, a.pf_loads);
        if (warm) {                                  // this helper's share of the next block's tables and vectors, one lane per line
            const int l32 = lane & 31;
            glds<4>(h == 0 ? nx.mdT + (size_t)w * kTile + l32 * 32 : nx.mc + (size_t)w * kTile + l32 * 32, dummy);
            if (w == 0) glds<4>(nx.vecs + lane * 32, dummy);
            if (w == 1) glds<4>(h == 0 ? nx.aoffT + l32 * 32 : nx.f1b + l32 * 32, dummy);
            glds<4>(nx.back32 + (size_t)(w * 5 + 4) * kTile + (lane & 15) * 32, dummy);
        }
        GAT8_BAR(19);
        f32x16 c23 = load_block(R0w, lane);
        if constexpr (H4) c23 = c23 * inv;
        // LayerNorm weights of what follows: the next block's norm1, or the encoder's final norm
        const bool last = bi + 1 == kDepth;
        const float* nvec = last ? a.norm_w : a.blk[bi + 1 < kDepth ? bi + 1 : bi].vecs + V_N1W;
        const float* nvecb = last ? a.norm_b : a.blk[bi + 1 < kDepth ? bi + 1 : bi].vecs + V_N1B;
        const f32x16 nw = load_chanvec_T(nvec, 32 * w, h), nb = load_chanvec_T(nvecb, 32 * w, h);
        GAT8_BAR(20);
        c23 = pick(R1w, lane, c23);
        xw += c01 + c23;
        tile_stats(xw, lds + kStat + w * 64, lane);
        if (a.blk_tap && tok < J) {          // debug tap (off in timed runs): this wave's channel block of the block output
            store_row_block(a.blk_tap + (((size_t)bi * a.tapB + b) * J + tok) * kC + 32 * w, h, xw);
        }
        GAT8_BAR(21);
        // ---- step 22: Y = LN1(x) for the next block; after the last block LN -> GELU -> feat (GAT.py:148-150)
        {
            f32x16 y = ln_stats(lds + kStat, xw, nw, nb, lane);
            if (!last) {
                st_opnd(A + w * kTileX3, lane, y);
            } else {
                gelu_pairs<8>(y);
                if (tok < J) store_row_block(a.feat + ((size_t)b * J + tok) * kC + 32 * w, h, y);
                if constexpr (TAIL) {        // feat stays on chip for the epilogue: channel block w as a T-layout tile (X is free since step 9);
                    if (tok >= J) y = zero16();      // zero for the token lanes that do not exist (they are operand columns of the joint-token linear)
                    store_block(X + w * kTile, lane, y);
                }
            }
        }
        GAT8_BAR(22);
    }
    GAT8_STAMPS_OUT(kDepth * 23 * 2, 2 * kDepth * 23 * 2 + kDepth * 8);
    if constexpr (TAIL) gat8_tail<LR, true>(a.tl, a.pose2d, lds, b, J, w, lane);
}

}  // namespace

constexpr size_t kGat8Lds = (size_t)(kGat8LdsFloats + kDiagLdsFloats) * sizeof(float);

// The eleven forms of k_gat8, named once with what the host needs to know of their weight stream (gat8_forms.h): the dynamic-LDS
// opt-in and the launch both read this table
using Gat8Kernel = void (*)(const Gat8Args);
struct Gat8Entry { Gat8Form form; Gat8Kernel kernel; int tile_floats; bool byte_lo; };
template <bool H4, int LR, bool H2 = false, bool LB = false, bool TAIL = false>
constexpr Gat8Entry gat8_entry() {
    using F = Gat8Stream<H4, H2, LB>;
    return {{H4, LR, H2, LB, TAIL}, k_gat8<H4, LR, H2, LB, TAIL>, F::kTileFloats, F::kByteLo};
}
const Gat8Entry kGat8Kernels[] = {
    gat8_entry<false, 16>(), gat8_entry<true, 10>(), gat8_entry<true, 12>(), gat8_entry<true, 10, true>(), gat8_entry<true, 12, true>(),
    gat8_entry<true, 10, false, true>(), gat8_entry<true, 12, false, true>(), gat8_entry<true, 10, true, false, true>(),
    gat8_entry<true, 12, true, false, true>(), gat8_entry<true, 10, false, true, true>(), gat8_entry<true, 12, false, true, true>()};

int gat8_prepare_device() {
    for (const auto& e : kGat8Kernels)
        GATOR_HIP_CHECK(hipFuncSetAttribute((const void*)e.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGat8Lds));
    return GATOR_OK;
}

// The per-wave weight streams: the X3 tile grids of fused_create_gat (gxbuf, tile-for-tile image of gbuf from gblk[0].qkv on)
// re-ordered into the order product wave w consumes them, block after block.
#ifdef GATOR_DIAG
// GATOR_GAT_STAMPS: the stamp buffers of one launch, zeroed before it, read back (synchronously) and printed behind it
constexpr int kGat8Stamps = 2 * kDepth * 23 * 2 + kDepth * 8;
struct Gat8Diag { DevBuf<unsigned long long> stamps, tstamps; };

static int gat8_diag_setup(const FusedState* f, bool tail, Gat8Args& a, Gat8Diag& d) {
    a.stamps = nullptr;
    a.dbg = f->opt.gat8_dbg;
    a.tl.tstamps = nullptr;
    if (!f->opt.gat_stamps) return GATOR_OK;
    GATOR_TRY(d.stamps.alloc(kGat8Stamps * sizeof(unsigned long long)));
    a.stamps = d.stamps.get();
    GATOR_HIP_CHECK(hipMemset(a.stamps, 0, kGat8Stamps * sizeof(unsigned long long)));
    if (tail) {
        GATOR_TRY(d.tstamps.alloc(64 * sizeof(unsigned long long)));
        a.tl.tstamps = d.tstamps.get();
        GATOR_HIP_CHECK(hipMemset(a.tl.tstamps, 0, 64 * sizeof(unsigned long long)));
    }
    return GATOR_OK;
}

static int gat8_diag_report(Gat8Diag& d, int B) {
    if (d.tstamps) {
        unsigned long long ts[64];
        GATOR_HIP_CHECK(hipMemcpy(ts, d.tstamps, sizeof(ts), hipMemcpyDeviceToHost));
        d.tstamps.reset();
        fprintf(stderr, "[k_gat8 tail stamps, one workgroup, B=%d] s_memtime cycles since wave 0 entered: entry | loads issued + joint-token MFMAs | lifter done | at barrier | past barrier | jf + LN done | job 1 | job 2\n", B);
        for (int v = 0; v < 8; ++v) {
            fprintf(stderr, "  wave %d:", v);
            for (int k = 0; k < 8; ++k) fprintf(stderr, " %6lld", ts[v * 8 + k] ? (long long)(ts[v * 8 + k] - ts[0]) : -1LL);
            fprintf(stderr, "\n");
        }
    }
    if (d.stamps) {     // blocks 1..5 averaged (block 0 carries the cold start)
        std::vector<unsigned long long> hs(kGat8Stamps);
        GATOR_HIP_CHECK(hipMemcpy(hs.data(), d.stamps, kGat8Stamps * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        d.stamps.reset();
        double tot[2] = {0, 0};
        fprintf(stderr, "[k_gat8 stamps, wg0, B=%d] cycles per step, mean of blocks 1-5: step | product work wait | helper work wait\n", B);
        for (int n = 0; n < 23; ++n) {
            double v[4] = {0, 0, 0, 0};
            for (int role = 0; role < 2; ++role)
                for (int bi = 1; bi < kDepth; ++bi)
                    for (int k = 0; k < 2; ++k) v[role * 2 + k] += (double)hs[(((size_t)role * kDepth + bi) * 23 + n) * 2 + k] / (kDepth - 1);
            fprintf(stderr, "  %2d | %7.0f %7.0f | %7.0f %7.0f\n", n, v[0], v[1], v[2], v[3]);
            tot[0] += v[0] + v[1]; tot[1] += v[2] + v[3];
        }
        fprintf(stderr, "  per block: product %.0f, helper %.0f cycles\n", tot[0], tot[1]);
        fprintf(stderr, "  helper sub-stamps of step 15 (block 1), cycles since the barrier:");
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %llu", hs[(size_t)2 * kDepth * 23 * 2 + 1 * 8 + k]);
        fprintf(stderr, "\n");
    }
    return GATOR_OK;
}
#endif

int launch_gat8(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pose2d, int B_total, float* pose3d, void* stream) {
    const Gat8Entry* e = nullptr;
    for (const auto& k : kGat8Kernels)
        if (k.form == p.gat8) e = &k;
    if (!e) return fail(GATOR_EINVAL, "k_gat8: no such form");
    const int row0 = p.n_tiled, B = B_total - row0;      // this launch's samples start at row row0 of the batch
    const size_t o = (size_t)row0 * c->J;
    Gat8Args a;
    const Weights& w = c->w;
    a.B = B; a.J = c->J; a.pose2d = pose2d + o * 2;
    a.gl0_W = w.gl0_W; a.gl0_b = w.gl0_b; a.gn_w = w.gn_w; a.gn_b = w.gn_b; a.gl3_p = f->g_gl3; a.gl3_b = w.gl3_b; a.posT = f->g_posT;
    a.biasT = f->g_biasT; a.m1T = f->g_m1T; a.m2T = f->g_m2T;
    a.norm_w = w.norm_w; a.norm_b = w.norm_b;
    a.wstream = e->byte_lo ? f->g8stream_b.get() : f->g8stream.get();      // the byte-lo stream, or the H3 stream (the one-plane form reads its hi and mid)
    for (int i = 0; i < kDepth; ++i) {
        const GatBlockPk& b = f->gblk[i];
        a.blk[i] = Gat8Blk{b.back, b.mc, b.mdT, b.aoffT, b.f1b, f->g_vecs + (size_t)i * V_TOTAL};
    }
    a.feat = ws.feat + o * kC;
    a.tl = Gat8Tail{};
    const bool tail = p.gat8.tail;
    if (tail) {      // the lifter (x_out [B,3J] IS pose3d [B,J,3]) and the MDR joint tokens / K / V tiles of ITS samples as the kernel's epilogue
        Gat8Tail& tl = a.tl;
        tl.lifter_w = w.lifter_w; tl.lifter_b = w.lifter_b; tl.x_out = pose3d + o * 3; tl.jkv = ws.jkv + (size_t)row0 * 12 * kTile;
        if (p.ctr_zero == CtrZero::GAT8_TAIL) { tl.mdr_ctr = ws.mdr_ctr; tl.ctr_B = B_total; }      // ... and the zeroing of the whole forward's MDR counters
        tl.jf5 = f->jfeat5; tl.jf_h3 = f->jf128_h3; tl.jf_b = w.jfeat_b; tl.posj_T = f->posj_T;
        auto h3_of = [&](const float* t) { return f->wxbuf + (size_t)(t - f->lay[0].wq) / kTile * kTileX3; };      // the MDR layers' H3 image mirrors wbuf tile for tile
        for (int i = 0; i < 3; ++i) { tl.j_n1w[i] = w.lay[i].n1w; tl.j_n1b[i] = w.lay[i].n1b; tl.j_wk_h3[i] = h3_of(f->lay[i].wk); tl.j_wv_h3[i] = h3_of(f->lay[i].wv); }
        tl.jf_inv = std::ldexp(1.0f, -(4 + f->jf128_wshift));
        tl.kv_inv = std::ldexp(1.0f, -(4 + f->mdr_wshift));
    }
    a.blk_tap = nullptr;
    a.tapB = B;
    if (c->block_taps) {
        GATOR_TRY(gat_ensure_blk_tap(c, f, B_total));
        a.blk_tap = f->blk_tap + (size_t)row0 * c->J * kC; a.tapB = B_total;
    }
    // L2 warm-up: each workgroup touches its share of the next block's weight stream
    a.pf_n = std::min(32, (B + 7) / 8);                  // workgroups b and b + 8 share an XCD (round-robin dispatch; speed only)
    a.pf_loads = (kBlkTiles * e->tile_floats * 4 / a.pf_n + 8191) / 8192;       // 8 KiB (64 lines) per instruction
    if (a.pf_loads > 6) a.pf_loads = 0;      // fewer than ~8 workgroups per XCD (B < 64): a share is so large that touching it costs more than it hides
    a.tl.warm_n = (tail && a.pf_n >= 8) ? a.pf_n : 0;      // (fewer than 8 workgroups per XCD: a share is too large to be worth touching)
    a.lin_inv = std::ldexp(1.0f, -(4 + f->gat8_wshift));
#ifdef GATOR_DIAG
    Gat8Diag diag;
    GATOR_TRY(gat8_diag_setup(f, tail, a, diag));
#endif
    e->kernel<<<B, 512, kGat8Lds, (hipStream_t)stream>>>(a);
    GATOR_HIP_CHECK(hipGetLastError());
#ifdef GATOR_DIAG
    GATOR_TRY(gat8_diag_report(diag, B));
#endif
    return GATOR_OK;
}

}  // namespace gator
