// k_gat8 (gat_roles.hip), product waves: the order of the weight stream and the four forms its tiles come in.  Shared with
// gat8_stream.hip, which builds the streams in exactly this order and these tile formats.
#pragma once
#include "fused_common.h"
#include "fused_state.h"
#include "x3_common.h"
#include "gat8_rows.h"

namespace gator {
namespace {

constexpr int kNT = 5;                                  // weight tiles in flight per product wave.  6 (one dummy tile per block, +28 VGPRs) was measured:
                                                        // no change (188 - 192 us either way on one box), so the stream is not short of bytes in flight
// The units of a block in the order a product wave consumes them: (tile grid of the block, tiles per product wave).  A unit is the
// K = 128 contraction of one 32-channel output block (4 tiles); linears[1] is one tile, fc1 / fc2 four units each.  The kernel's slot
// indices (gat8_slot) and the stream builder's tile order (gat8_build_stream) both come from this list.
enum Gat8UnitId { U_Q, U_K, U_V, U_H0, U_H1, U_PROJ, U_LIN0, U_LIN1, U_BACK, U_FC1, U_FC2, U_COUNT };
struct Gat8Unit { const float* GatBlockPk::*grid; int tiles; };
constexpr Gat8Unit kGat8Units[U_COUNT] = {
    {&GatBlockPk::qkv, 4}, {&GatBlockPk::qkv, 4}, {&GatBlockPk::qkv, 4}, {&GatBlockPk::w0, 4}, {&GatBlockPk::w1, 4}, {&GatBlockPk::proj, 4},
    {&GatBlockPk::lin0, 4}, {&GatBlockPk::lin1, 1}, {&GatBlockPk::back, 4}, {&GatBlockPk::fc1, 16}, {&GatBlockPk::fc2, 16}};
// tile offset of unit u inside a block (U_COUNT: the tiles of a block)
constexpr int gat8_off(int u) {
    int o = 0;
    for (int i = 0; i < u; ++i) o += kGat8Units[i].tiles;
    return o;
}
// tile i of unit u, for product wave w (= channel block w), as an index into the unit's [NB][KB] grid
constexpr int gat8_unit_tile(int u, int w, int i) {
    return u == U_K ? (4 + w) * 4 + i          // qkv rows 128 .. 255
         : u == U_V ? (8 + w) * 4 + i          //          256 .. 383
         : u == U_LIN1 ? w                     // linears[1] (128 -> 16): k block w
         : u == U_BACK ? w * 5 + i             // linearback, k < 128 (its fifth k block is the helpers' fp32 tile)
         : u == U_FC1 ? w * 16 + i             // hidden blocks 4w + i / 4, k block i % 4
         : u == U_FC2 ? w * 16 + 4 * (i & 3) + (i >> 2)      // unit i / 4 contracts over hidden blocks {4w' + i / 4}, w' = i % 4
         : w * 4 + i;
}
constexpr int kUseTiles = gat8_off(U_COUNT);                   // 65
constexpr int kPadTiles = (kNT - kUseTiles % kNT) % kNT;       // dummy tiles behind a block so that every block starts at slot 0
constexpr int kBlkTiles = kUseTiles + kPadTiles;
constexpr int kWaveTiles = kBlkTiles * kDepth;                 // per product wave
constexpr int kStreamTiles = 4 * kWaveTiles + kNT;             // four product waves + kNT tiles of slack behind the last one
// slot (compile-time) of tile i of unit u: its offset inside the block, mod kNT
constexpr int gat8_slot(int u, int i = 0) { return (gat8_off(u) + i) % kNT; }

// ---- the four forms of a stream tile.  Each says: the register tile W and the operand tile O it multiplies, floats from one tile of
// a wave's stream to the next, which of FusedState's two streams holds it, the load of a whole tile, the operand load, the schedule of
// one tile product with the refill of its slot woven in, and whether that product leaves its small terms in a second accumulator
// that the unit adds once.  Gat8Stream<H4, H2, LB> picks the form from k_gat8's template parameters; a combination that has no
// form does not compile.
//
// mma_refill<CL>: CL = false: weights as A operand -> T-layout accumulator (token on the lane); CL = true: activations as A -> C-layout.
// A plane's load (tile kNT positions further down the stream) is issued right behind the LAST MFMA that reads that plane, so it
// issues in the shadow of the next MFMA.  Issued as a burst behind the twelve MFMAs (k_gat's form) the six 1 KiB loads hold the
// in-order wave at the memory pipeline's issue rate while the matrix pipe idles: measured here as 3.2k cycles per 4-tile unit against
// 1.5k of MFMA time.  sched_barrier pins the order.
template <bool H4, bool H2, bool LB> struct Gat8Stream;

// The exact six-product form (GATOR_GAT8_H4=0): three bf16 planes of weights and activations (x3_common.h), one accumulator.
template <> struct Gat8Stream<false, false, false> {
    typedef X3 W;
    typedef X3 O;
    static constexpr int kTileFloats = kTileX3;
    static constexpr bool kByteLo = false, kFoldSmall = false;
    static __device__ __forceinline__ W load(const float* p, int lane) { return x3_load(p, lane); }
    template <bool SWZ = false> static __device__ __forceinline__ O load_opnd(const float* p, int lane) { return x3_load(p, lane); }
    template <bool CL>
    static __device__ __forceinline__ void mma_refill(W& w, const O& b, f32x16& acc, f32x16&, const float* __restrict__ wp, int lane) {
        const bf16x8* q = reinterpret_cast<const bf16x8*>(wp) + lane;
#define GAT8_MM(wpl, bpl, s) acc = CL ? GATOR_MFMA_BF16(b.p[bpl][s], w.p[wpl][s], acc) : GATOR_MFMA_BF16(w.p[wpl][s], b.p[bpl][s], acc)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            GAT8_MM(2, 0, s);                                  // lo*hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[2][s] = q[(2 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
            GAT8_MM(0, 2, s);                                  // hi*lo
            GAT8_MM(1, 1, s);                                  // mid*mid
            GAT8_MM(1, 0, s);                                  // mid*hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[1][s] = q[(1 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
            GAT8_MM(0, 1, s);                                  // hi*mid
            GAT8_MM(0, 0, s);                                  // hi*hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[0][s] = q[(0 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
#undef GAT8_MM
    }
};

// what the three fp16 forms share: activations on two fp16 planes (the fc2 units read the hidden tiles swizzled, gat8_rows.h), and
// the cross products in their OWN accumulator `acs` (2^-11 of the result: its roundings do not matter), so the main one is rounded
// twice per tile instead of eight times -- every MFMA rounds its accumulator at the accumulator's magnitude, and in-product
// accumulation is where the path's fp32 noise comes from (x3_common.h, x2_mma).  The unit adds the two once, in the product wave's
// idle vector slots.
struct Gat8StreamF16 {
    typedef X2 O;
    static constexpr bool kFoldSmall = true;
    template <bool SWZ = false> static __device__ __forceinline__ O load_opnd(const float* p, int lane) { return SWZ ? x2_load_swz(p, lane) : x2_load(p, lane); }
};

// The four-product form (x3_common.h: weights exact on three fp16 planes, activations on two; GATOR_GAT8_LOBYTE=0): w_hi a_lo |
// w_lo a_hi, w_mid a_hi, w_hi a_hi -- 8 MFMAs per tile; the refill of a plane still follows the last MFMA that reads it.
template <> struct Gat8Stream<true, false, false> : Gat8StreamF16 {
    typedef H3 W;
    static constexpr int kTileFloats = kTileX3;
    static constexpr bool kByteLo = false;
    static __device__ __forceinline__ W load(const float* p, int lane) { return h3_load(p, lane); }
    template <bool CL>
    static __device__ __forceinline__ void mma_refill(W& w, const O& b, f32x16& acc, f32x16& acs, const float* __restrict__ wp, int lane) {
        const f16x8* q = reinterpret_cast<const f16x8*>(wp) + lane;
#define GAT8_MM(wpl, bpl, s, AC) AC = CL ? GATOR_MFMA_F16(b.p[bpl][s], w.p[wpl][s], AC) : GATOR_MFMA_F16(w.p[wpl][s], b.p[bpl][s], AC)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            GAT8_MM(0, 1, s, acs);                             // w hi  * a lo
            GAT8_MM(2, 0, s, acs);                             // w lo  * a hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[2][s] = q[(2 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
            GAT8_MM(1, 0, s, acs);                             // w mid * a hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[1][s] = q[(1 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
            GAT8_MM(0, 0, s, acc);                             // w hi  * a hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[0][s] = q[(0 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
#undef GAT8_MM
    }
};

// The one-plane form (BASELINE config 3, the 16-bit operand mode: DESIGN.md 4e): activations on their hi plane only, weights on their
// hi and mid planes (x3_common.h: G2) -- w_mid a_hi | w_hi a_hi, four MFMAs per tile, and the lo plane of the weight stream (a third of
// its bytes) is never loaded.  Same tile geometry, same stream as the four-product form.
template <> struct Gat8Stream<true, true, false> : Gat8StreamF16 {
    typedef G2 W;
    static constexpr int kTileFloats = kTileX3;
    static constexpr bool kByteLo = false;
    static __device__ __forceinline__ W load(const float* p, int lane) {      // g2_load's two planes, requested plane by plane like the refills
        const f16x8* q = reinterpret_cast<const f16x8*>(p) + lane;
        W o;
#pragma unroll
        for (int s = 0; s < 2; ++s) o.hi[s] = q[s * 64];
#pragma unroll
        for (int s = 0; s < 2; ++s) o.mid[s] = q[(2 + s) * 64];
        return o;
    }
    template <bool CL>
    static __device__ __forceinline__ void mma_refill(W& w, const O& b, f32x16& acc, f32x16& acs, const float* __restrict__ wp, int lane) {
        const f16x8* q = reinterpret_cast<const f16x8*>(wp) + lane;
#define GAT8_MM(wv, s, AC) AC = CL ? GATOR_MFMA_F16(b.p[0][s], (wv), AC) : GATOR_MFMA_F16((wv), b.p[0][s], AC)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            GAT8_MM(w.mid[s], s, acs);                         // w mid * a hi
            __builtin_amdgcn_sched_barrier(0);
            w.mid[s] = q[(1 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
            GAT8_MM(w.hi[s], s, acc);                          // w hi  * a hi
            __builtin_amdgcn_sched_barrier(0);
            w.hi[s] = q[(0 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
#undef GAT8_MM
    }
};

// The byte-lo form of the four-product stream (round 5; default): the same three fp16 planes, but the lo plane travels as ONE BYTE
// per weight.  lo = fp16(w - hi - mid) is zero or a single power of two between 2^-24 and 2^-10 (the residual of two 11-bit
// roundings of a 24-bit significand is at most one unit of w's last place), so the top byte of fp16(2^24 lo) -- sign, five exponent
// bits, two mantissa bits -- holds it exactly; the product wave rebuilds the fp16 value with two v_perm_b32 and two v_pk_mul_f16
// (x 2^-24, exact: fp16 denormals are on) per four weights in the shadow of the MFMA before, and multiplies the SAME bits in the SAME
// order: results are bit for bit those of the H3 stream (tests/test_gpu_digest.py), a sixth of the stream's bytes never crosses the
// L2 -> CU path that bounds this kernel.  gat8_build_stream checks on the device, with this very expansion, that every
// weight's lo survives the round trip, and keeps the H3 stream if one does not.
constexpr int kTileH3B = 2 * 512 + 256;      // floats of a byte-lo tile: hi and mid planes as in H3 (1 KiB per k-step each), lo as one byte per weight
struct H3B { f16x8 p[2][2]; uint4 lo; };     // [plane hi/mid][k-step] + 16 lo bytes (k-step 0: x y, k-step 1: z w): 20 VGPRs
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f16x8 lo_expand(unsigned d0, unsigned d1) {
    const f16x2_t sc = {(_Float16)5.9604644775390625e-08f, (_Float16)5.9604644775390625e-08f};      // 2^-24
    union { unsigned u[4]; f16x2_t h[4]; f16x8 v; } o;
    o.u[0] = __builtin_amdgcn_perm(d0, d0, 0x010c000cu);      // (byte 0, byte 1) -> the high bytes of two halves
    o.u[1] = __builtin_amdgcn_perm(d0, d0, 0x030c020cu);
    o.u[2] = __builtin_amdgcn_perm(d1, d1, 0x010c000cu);
    o.u[3] = __builtin_amdgcn_perm(d1, d1, 0x030c020cu);
#pragma unroll
    for (int i = 0; i < 4; ++i) o.h[i] = o.h[i] * sc;
    return o.v;
}
template <> struct Gat8Stream<true, false, true> : Gat8StreamF16 {
    typedef H3B W;
    static constexpr int kTileFloats = kTileH3B;
    static constexpr bool kByteLo = true;
    static __device__ __forceinline__ W load(const float* p, int lane) {
        const f16x8* q = reinterpret_cast<const f16x8*>(p) + lane;
        W o;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) o.p[pl][s2] = q[(pl * 2 + s2) * 64];
        o.lo = reinterpret_cast<const uint4*>(p + 1024)[lane];
        return o;
    }
    template <bool CL>
    static __device__ __forceinline__ void mma_refill(W& w, const O& b, f32x16& acc, f32x16& acs, const float* __restrict__ wp, int lane) {
        const f16x8* q = reinterpret_cast<const f16x8*>(wp) + lane;
#define GAT8_MM(wv, bpl, s, AC) AC = CL ? GATOR_MFMA_F16(b.p[bpl][s], (wv), AC) : GATOR_MFMA_F16((wv), b.p[bpl][s], AC)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            GAT8_MM(w.p[0][s], 1, s, acs);                     // w hi  * a lo
            const f16x8 lo = lo_expand(s == 0 ? w.lo.x : w.lo.z, s == 0 ? w.lo.y : w.lo.w);
            GAT8_MM(lo, 0, s, acs);                            // w lo  * a hi
            __builtin_amdgcn_sched_barrier(0);
            if (s == 1) w.lo = reinterpret_cast<const uint4*>(wp + 1024)[lane];
            __builtin_amdgcn_sched_barrier(0);
            GAT8_MM(w.p[1][s], 0, s, acs);                     // w mid * a hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[1][s] = q[(1 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
            GAT8_MM(w.p[0][s], 0, s, acc);                     // w hi  * a hi
            __builtin_amdgcn_sched_barrier(0);
            w.p[0][s] = q[(0 * 2 + s) * 64];
            __builtin_amdgcn_sched_barrier(0);
        }
#undef GAT8_MM
    }
};

// ---- product wave: one unit = the K = 128 contraction of one 32-channel output block (4 weight tiles) --------------------------
// Slot indices are compile-time (S0 = gat8_slot of the unit); every slot is refilled with the tile kNT positions further down the
// wave's stream right after the MFMAs that read it are queued.
// `b` = the unit's first operand tile, already requested: where that tile was complete two barriers ago (Y for k / v / h0 / h1, Y2
// for the later fc1 units, the hidden blocks for fc2) the caller reads it BEFORE the barrier that opens the step, so the matrix
// pipe does not idle through an LDS round trip after every barrier.
template <class F, int S0, bool CL, bool SWZ = false>
__device__ __forceinline__ void unit4(typename F::W (&W)[kNT], const float* __restrict__& wp, typename F::O b, const float* o1, const float* o2,
                                      const float* o3, float* raw, int lane) {
    const float* ops[4] = {o1, o1, o2, o3};
    f32x16 acc = zero16(), acs = zero16();
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        typename F::O bn = b;
        if (kb < 3) bn = F::template load_opnd<SWZ>(ops[kb + 1], lane);
        F::template mma_refill<CL>(W[(S0 + kb) % kNT], b, acc, acs, wp, lane);
        wp += F::kTileFloats;
        b = bn;
    }
    if constexpr (F::kFoldSmall) acc = acc + acs;
    store_block(raw, lane, acc);
}
// one tile: partial hop-2 linear (linears[1], 128 -> 16) over k block `w` of SB; C-layout
template <class F, int S0>
__device__ __forceinline__ void unit1(typename F::W (&W)[kNT], const float* __restrict__& wp, const float* o0, float* raw, int lane) {
    f32x16 acc = zero16(), acs = zero16();
    const typename F::O b = F::load_opnd(o0, lane);
    F::template mma_refill<true>(W[S0 % kNT], b, acc, acs, wp, lane);
    wp += F::kTileFloats;
    if constexpr (F::kFoldSmall) acc = acc + acs;
    store_block(raw, lane, acc);
}
// consume the kPadTiles dummy tiles behind a block: their slots get the tiles kNT positions further down (the next block's)
template <class F, int S0>
__device__ __forceinline__ void skip_pad(typename F::W (&W)[kNT], const float* __restrict__& wp, int lane) {
#pragma unroll
    for (int i = 0; i < kPadTiles; ++i) {
        W[(S0 + i) % kNT] = F::load(wp, lane);
        wp += F::kTileFloats;
    }
}

}  // namespace
}  // namespace gator
