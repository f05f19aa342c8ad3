// k_gat8 (gat_roles.hip): the kernel's LDS map and its epilogue (TAIL): the lifter and the MDR joint tokens of the workgroup's sample.
#pragma once
#include "fused_common.h"
#include "fused_state.h"
#include "x3_common.h"
#include "joint_tokens.h"

namespace gator {
namespace {

// LDS map (floats)
constexpr int kA = 0;                                   // 4 operand tiles
constexpr int kBq = kA + 4 * kTileX3;                   // 12 operand tiles
constexpr int kR = kBq + 12 * kTileX3;                  // R0 (4 raw tiles) | R1 (4 raw tiles)
constexpr int kXo = kR + 8 * kTile;                     // 4 fp32 tiles
constexpr int kDummy = kXo + 4 * kTile;                 // 4 x 1 KiB landing window of the L2 warm-up (never read)
constexpr int kStat = kDummy + 1024;                     // [4 helper waves][32 tokens][mean, M2] of the wave's 32 channels (LayerNorm statistics)
constexpr int kGat8LdsFloats = kStat + 256;             // 149 KiB
#ifdef GATOR_DIAG
constexpr int kDiagStamps = 2 * kDepth * 23 * 2 + kDepth * 8;      // u64 cycle stamps, kept in LDS while the kernel runs (a global
constexpr int kDiagLdsFloats = 2 * kDiagStamps;                    // store waits ~0.5k cycles behind the product waves' stream and
#else                                                               // would be measured as work of the step it sits in)
constexpr int kDiagLdsFloats = 0;
#endif

// Epilogue of k_gat8<..., TAIL = true> (round 6): what gat_tail.hip's two launches do for the batch, done by the workgroup that owns
// the sample and has its feat on chip.
struct Gat8Tail {
    const float *lifter_w, *lifter_b;       // lifter.weight [3J][128J] as the reference stores it, bias [3J]  (GAT.py:151-152)
    float* x_out;                           // [B][3J] = pose3d [B][J][3] (mm)
    float* jkv;                             // nullptr: lifter only (stand-alone GAT entry point)
    unsigned* mdr_ctr;                      // non-null: zero k_mdr_persist's tickets / completion counts of the forward (as k_gat_joint does)
    int ctr_B;                              //           ... of a forward of ctr_B samples (mdr_ctr_words)
    const float *jf5, *jf_h3, *jf_b, *posj_T;      // get_joint_feature: columns 0..4 as [5][64], columns 5..132 as H3 tiles [2][4], bias; pos_j tiles
    const float *j_n1w[3], *j_n1b[3], *j_wk_h3[3], *j_wv_h3[3];      // per LBF layer: norm1, wk / wv as H3 tiles [2][2] (the MDR layers' own weight image)
    float jf_inv, kv_inv;                          // 1 / (16 x 2^weight shift) of the two H3 weight sets (x3_common.h: four-product linears)
#ifdef GATOR_DIAG
    unsigned long long* tstamps;                   // [8 waves][8] s_memtime stamps of workgroup B/2's epilogue (GATOR_GAT_STAMPS)
#endif
    int warm_n;                                    // L2 warm-up of the epilogue's weights: workgroups per XCD that share it (0: off)
};

// ---- epilogue (TAIL): lifter Linear(128J -> 3J) (GAT.py:151-152), MDR joint tokens and the three layers' cross-attention K / V
// operand tiles (MDR.py:130-134,37-38,65) -- formerly k_gat_lifter + k_gat_joint (gat_tail.hip: 5.7 + 16.4 us and two launch
// boundaries at B = 256, with ~2 MFLOP per sample between them; those launches stay for the sample-tiled encoder).  This workgroup owns
// the sample and ends with its feat on chip:
//   lifter       a 3J x 128J matrix-vector product: 444 KB (J = 17) of fp32 weights per sample that nobody on the CU can share, i.e.
//                a stream like the rest of this kernel.  All eight waves walk rows o = wave + 8 r as coalesced 1 KiB loads (lane l owns
//                k = 256 i + 4 l), exact fp32 FMAs against feat held in registers (read once from the T-layout tiles in X), one DPP
//                reduction per row.  (The product waves idle from barrier 20 of the last block on, but rows fetched ahead there would live beside the five
//                weight-stream tiles the block loop carries: 140 - 430 B per lane of scratch.  They stage the small operands instead.)  Fixed order: results do not depend on the batch.
//   joint tokens jf = Linear(133 -> 64)(cat(pose2d, pose3d / 1000, feat)) + pos_j: the 128 feat columns do not need pose3d, so product waves
//                0 / 1 (whose share of the rows is the smaller one) contract them behind their last rows; the five other columns are FMAs
//                once pose3d is known.  Then LayerNorm per layer and the 12 (layer, K | V, channel block) jobs, two on each of the other
//                six waves, their weight tiles requested behind the last lifter rows (same operand tiles out as k_gat_joint: two fp16
//                planes of 16 x value).  These token-wise linears run as every other one of the
//                default arithmetic does -- weights exact on three fp16 planes, activations on two, four partial products -- instead of
//                k_gat_joint's fp32-input MFMAs: measured with the MFMAs cut out, the 32-MFMA fp32 chains of the K / V jobs
//                alone were 6.5 us of the epilogue's 15.
// LDS: the operand tiles A | Bq are dead after barrier 20 of the last block.
constexpr int kTP = kA;                                 // the joint tokens without their pose3d columns (2 channel blocks, token on the lane)
constexpr int kTPosj = kTP + 2 * kTile;                 // pos_j tiles (2)
constexpr int kTVJ = kTPosj + 2 * kTile;                // per-channel vectors
constexpr int kTXO = kTVJ + VJ_TOTAL;                        // pose3d of the sample (3J <= 64 floats)
static_assert(kTXO + 64 <= kR, "the epilogue's LDS lives in the dead operand tiles");

__device__ __forceinline__ float dpp_add(float s, int ctrl_tag) {
    const int u = __builtin_bit_cast(int, s);
    int m;
    if (ctrl_tag == 0) m = __builtin_amdgcn_update_dpp(u, u, 0xB1, 0xf, 0xf, false);            // quad_perm [1,0,3,2]
    else if (ctrl_tag == 1) m = __builtin_amdgcn_update_dpp(u, u, 0x4E, 0xf, 0xf, false);       // quad_perm [2,3,0,1]
    else if (ctrl_tag == 2) m = __builtin_amdgcn_update_dpp(u, u, 0x141, 0xf, 0xf, false);      // row_half_mirror
    else m = __builtin_amdgcn_update_dpp(u, u, 0x140, 0xf, 0xf, false);                         // row_mirror
    return s + __builtin_bit_cast(float, m);
}
// sum over the 64 lanes, the same value (and the same association) in every lane
__device__ __forceinline__ float wave_sum64(float s) {
    s = dpp_add(s, 0); s = dpp_add(s, 1); s = dpp_add(s, 2); s = dpp_add(s, 3);      // every lane: the total of its row of 16
    const int u = __builtin_bit_cast(int, s);
    const float t0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 0)), t1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 16)),
                t2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 32)), t3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 48));
    return (t0 + t1) + (t2 + t3);
}
// one row of the lifter weight: NI - 1 full 1 KiB chunks and a half chunk (K = 128 J = 256 (NI - 1) + 128 for J = 17, 19)
template <int NI>
struct LiftRow { f32x4 w[NI]; };
template <int NI>
__device__ __forceinline__ void lift_load(LiftRow<NI>& r, const float* __restrict__ wrow, int lane, bool live) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NI; ++i) r.w[i] = (live && (i < NI - 1 || lane < 32)) ? *reinterpret_cast<const f32x4*>(wrow + 256 * i + 4 * lane) : z;
}
template <int NI>
__device__ __forceinline__ float lift_dot(const LiftRow<NI>& r, const f32x4 (&f)[NI]) {
    f32x2 acc = {0.f, 0.f};                               // two chains of packed FMAs (components 0, 2 | 1, 3), fixed order
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        acc = pk_fma(f32x2{r.w[i][0], r.w[i][1]}, f32x2{f[i][0], f[i][1]}, acc);
        acc = pk_fma(f32x2{r.w[i][2], r.w[i][3]}, f32x2{f[i][2], f[i][3]}, acc);
    }
    return wave_sum64(acc[0] + acc[1]);
}
constexpr int kLiftPre = 2;          // rows per batch; two batches in registers (one being multiplied, one in flight)

#ifdef GATOR_DIAG
#define GAT8_TSTAMP(k) do { __builtin_amdgcn_sched_barrier(0); if (tl.tstamps && b == 32 && lane == 0) tl.tstamps[v8 * 8 + (k)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define GAT8_TSTAMP(k)
#endif
// HELPER: the calling wave is helper w (holds channel block w of feat in `y`); else product wave w.
template <int LR, bool HELPER>
__device__ __forceinline__ void gat8_tail(const Gat8Tail& tl, const float* pose2d, float* lds, int b, int J, int w, int lane) {
    constexpr int NI = LR == 10 ? 9 : 10;
    const int h = lane >> 5, tok = lane & 31, tkj = tok < J ? tok : 0;
    const int v8 = HELPER ? w : 4 + w;                        // row phase of this wave (phases 0 .. 2 own one row more: the helpers', who have nothing else here)
    const int K = kC * J, R = 3 * J;
    const float* X = lds + kXo;                               // feat as four T-layout tiles, zero for the tokens that do not exist (stored before barrier 22)
    float* P = lds + kTP;
    const float* VJ = lds + kTVJ;
    float* XO = lds + kTXO;
    const bool joint = tl.jkv != nullptr;
    // who does what besides its lifter rows: product waves 0 / 1 the feat columns of the joint-token linear (channel block w, all of K = 128);
    // the other six waves two K / V jobs each
    const bool jf_wave = !HELPER && w < 2 && joint;
    // K / V jobs (layer li, k | v, channel block nb) = 2 pair + nb, pair = 2 li + kv: helper w both blocks of pair w, product wave w block
    // w & 1 of pair 4 + (w >> 1) -- three jobs on every SIMD, and a wave's jobs share their operand (one layer's LayerNorm)
    const int pair = HELPER ? w : 4 + (w >> 1), li = pair >> 1, kv = pair & 1;
    const int job0 = HELPER ? 2 * w : 8 + w, njob = HELPER ? 2 : 1;
    GAT8_TSTAMP(0);
    const float bias_r = (lane < 8 && v8 + 8 * lane < R) ? tl.lifter_b[v8 + 8 * lane] : 0.f;      // lane r: the bias of row v8 + 8 r
    const float* wbase = tl.lifter_w + (size_t)v8 * K;
    // rows r = 0 .. 7 of this wave in batches of kLiftPre, the next batch in flight while the current one is multiplied
    constexpr int NB = 8 / kLiftPre;
    LiftRow<NI> cur[kLiftPre], nxt[kLiftPre];
#pragma unroll
    for (int q = 0; q < kLiftPre; ++q) lift_load(cur[q], wbase + (size_t)(8 * q) * K, lane, v8 + 8 * q < R);
    GAT8_TSTAMP(1);
    f32x4 f[NI];                                              // feat[k], k = 256 i + 4 lane: token 2 i + (lane >> 5), channels 4 (lane & 31) ..
    {
        const int c = 4 * (lane & 31);
        const float* fx = X + (c >> 5) * kTile + (((c & 31) >> 3) * 64 + 32 * ((c >> 2) & 1)) * 4;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = 2 * i + (lane >> 5);
            f[i] = *reinterpret_cast<const f32x4*>(fx + (j < J ? j : 0) * 4);
        }
    }
    auto job_tile = [&](int job, int i) {
        const int li = job >> 2, kv = (job >> 1) & 1, nb = job & 1;
        return h3_load((kv ? tl.j_wv_h3[li] : tl.j_wk_h3[li]) + (size_t)(nb * 2 + i) * kTileX3, lane);
    };
    // the weights of what follows the lifter are requested behind the last batch of rows, so that they ride in the same stream
    H3 wt[4];                                                 // jf wave: its channel block's four k tiles; K / V wave: [job][k block]
    float p2x = 0.f, p2y = 0.f;
    float res = 0.f;
#pragma unroll
    for (int bt = 0; bt < NB; ++bt) {
        if (bt + 1 < NB) {
#pragma unroll
            for (int q = 0; q < kLiftPre; ++q) {
                const int r = (bt + 1) * kLiftPre + q;
                lift_load(nxt[q], wbase + (size_t)(8 * r) * K, lane, v8 + 8 * r < R);
            }
        }
        auto tail_tiles = [&](int i0) {       // two of the four weight tiles of what follows (requested while the last rows are multiplied)
            if (jf_wave) {
#pragma unroll
                for (int kb = i0; kb < i0 + 2; ++kb) wt[kb] = h3_load(tl.jf_h3 + (size_t)(w * 4 + kb) * kTileX3, lane);
            } else if (i0 < 2 * njob) {
#pragma unroll
                for (int i = i0; i < i0 + 2; ++i) wt[i] = job_tile(job0 + (i >> 1), i & 1);
            }
        };
        if (bt + 1 == NB && joint) {
            tail_tiles(0);
            p2x = pose2d[((size_t)b * J + tkj) * 2];
            p2y = pose2d[((size_t)b * J + tkj) * 2 + 1];
        }
#pragma unroll
        for (int q = 0; q < kLiftPre; ++q) {
            const int r = bt * kLiftPre + q;
            const float tot = lift_dot(cur[q], f);
            res = lane == r ? tot : res;
            if (bt + 1 == NB && q == 0 && joint) { __builtin_amdgcn_sched_barrier(0); tail_tiles(2); }      // (this row's registers are free now)
        }
        if (bt + 1 < NB) {
#pragma unroll
            for (int q = 0; q < kLiftPre; ++q) cur[q] = nxt[q];
        }
    }
    GAT8_TSTAMP(2);
    // x_out[o] = bias[o] + sum_k W[o][k] feat[k]
    if (lane < 8 && v8 + 8 * lane < R) {
        const float xo = res + bias_r;
        tl.x_out[(size_t)b * R + v8 + 8 * lane] = xo;
        XO[v8 + 8 * lane] = xo;
    }
    if (!joint) return;
    if (jf_wave) {
        // jf without its pose3d columns: bias + pos_j + feat columns (GATOR.py:19, MDR.py:130-134), channel block w, token on the lane
        f32x16 acc = zero16(), acs = zero16();
        const f32x16 init = chanvec_lds(VJ, VJ_JFB + 32 * w, h) + load_block(lds + kTPosj + w * kTile, lane);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const X2 fx2 = x2_split(load_block(X + kb * kTile, lane) * 16.0f);
            acs = h3_mma_wa_small(wt[kb], fx2, acs);
            acc = h3_mma_wa_main(wt[kb], fx2, acc);
        }
        store_block(P + w * kTile, lane, fma16(acc + acs, tl.jf_inv, init));
        wt[0] = job_tile(job0, 0);                             // (its own K / V job's tiles, in flight across the barrier)
        wt[1] = job_tile(job0, 1);
    }
    GAT8_TSTAMP(3);
    __syncthreads();
    GAT8_TSTAMP(4);
    // jf = that + columns 0..4 (pose2d, pose3d / 1000)
    f32x16 jf[2];
    {
        const float pin[5] = {p2x, p2y, XO[tkj * 3] / 1000.f, XO[tkj * 3 + 1] / 1000.f, XO[tkj * 3 + 2] / 1000.f};
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x16 acc = load_block(P + nb * kTile, lane);
#pragma unroll
            for (int i = 0; i < 5; ++i) acc += chanvec_lds(VJ, VJ_JF5 + i * 64 + 32 * nb, h) * pin[i];
            jf[nb] = acc;
        }
    }
    f32x16 d0 = jf[0], d1 = jf[1];
    const float rstd = ln_center64(d0, d1);
    GAT8_TSTAMP(5);
    // per LBF layer: k = wk(LN1(jf)), v = wv(LN1(jf)) as MFMA operand tiles (two fp16 planes of 16 x value: mdr_ops.h, cross_attention_head / JointX2)
    f32x16 fz0, fz1;
    joint_norm1(d0, d1, rstd, VJ, li, h, fz0, fz1);
    const X2 z0 = x2_split(fz0 * 16.0f), z1 = x2_split(fz1 * 16.0f);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (q >= njob) break;
        const int nb = (job0 + q) & 1;
        float* out = tl.jkv + (((size_t)b * 3 + li) * 4 + kv * 2 + nb) * kTile;
        const H3 &k0 = wt[2 * q], &k1 = wt[2 * q + 1];
        f32x16 r0 = zero16(), r1 = zero16();                   // r1: the cross products of both k blocks, r0: the hi x hi ones (x3_common.h on the order)
        if (kv == 0) {
            r1 = h3_mma_wa_small(k1, z1, h3_mma_wa_small(k0, z0, r1));
            r0 = h3_mma_wa_main(k1, z1, h3_mma_wa_main(k0, z0, r0));
            r0 += r1;
            if (tok >= J) r0 = zero16();                       // joints >= J: zero rows (masked in the softmax anyway)
        } else {
            r1 = h3_mma_aw_small(z1, k1, h3_mma_aw_small(z0, k0, r1));
            r0 = h3_mma_aw_main(z1, k1, h3_mma_aw_main(z0, k0, r0));
            r0 += r1;
#pragma unroll
            for (int r = 0; r < 16; ++r) r0[r] = (kap(r) + 4 * h < J) ? r0[r] : 0.f;
        }
        x2_store(out, lane, x2_split(r0 * (16.0f * tl.kv_inv)));
        GAT8_TSTAMP(6 + q);
    }
}

}  // namespace
}  // namespace gator
