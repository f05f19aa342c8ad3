// k_gat8 (gat_roles.hip), helper waves: the token rows that do not exist, and the MLP's hidden operand tiles that skip them.
#pragma once
#include "fused_common.h"
#include "x3_common.h"

namespace gator {
namespace {

// ---- token rows that do not exist.  A tile whose REGISTERS run over tokens (C layout: v[r] <-> token kap(r) + 4h; S^T and P^T with
// the key on the row) has live data only in registers r < LR: tokens 0 .. J-1 with J = 17 / 19 sit in r <= 8 / 10.  The rows behind
// them hold products against zero operand rows or masked scores (probability exactly 0): every instruction spent on them is wasted,
// and the helper waves are the long side of most steps.  LR (even: 10 for J <= 18, 12 for J <= 20; 16 = every row, the six-product form) is a template
// parameter of the kernel; skipping dead rows changes no bit of a live value (sums lose terms that are exactly +0).
template <int LR>
__device__ __forceinline__ X2 x2_split_rows(const f32x16& v) {     // x2_split with zero halves for the dead rows
    X2 o;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (8 * s + j < LR) {
                const float x = v[8 * s + j];
                const _Float16 hh = (_Float16)x;
                o.p[0][s][j] = hh;
                o.p[1][s][j] = (_Float16)(x - (float)hh);
            } else {
                o.p[0][s][j] = (_Float16)0.f;
                o.p[1][s][j] = (_Float16)0.f;
            }
        }
    return o;
}
// (a + b) + (c + d) over the live registers of group q, the association of the full tree (a dead term is an exact +0)
template <int LR, class F>
__device__ __forceinline__ float tree4(int q, F f) {
    const int n = LR - 4 * q;          // live registers in this group
    if (n <= 0) return 0.f;
    if (n == 1) return f(4 * q);
    if (n == 2) return f(4 * q) + f(4 * q + 1);
    if (n == 3) return (f(4 * q) + f(4 * q + 1)) + f(4 * q + 2);
    return (f(4 * q) + f(4 * q + 1)) + (f(4 * q + 2) + f(4 * q + 3));
}
// dot16 (fused_common.h) over the live k rows only: the same two chains (even / odd registers)
template <int LR>
__device__ __forceinline__ f32x16 dot16_rows(const f32x16& A, const f32x16& B, f32x16 init) {
    f32x16 e = init, o = zero16();
#pragma unroll
    for (int r = 0; r < LR; r += 2) {
        e = GATOR_MFMA(A[r], B[r], e);
        o = GATOR_MFMA(A[r + 1], B[r + 1], o);
    }
    return e + o;
}

// The MLP's hidden tiles in the four-product form.  fc1 leaves its accumulator in C layout (channel on the lane, token rows in the
// registers), so the GELU and the split run over the LR registers that hold tokens instead of all 16 -- in T layout 15 of a tile's
// 32 token lanes are padding at J = 17 and every instruction pays for them.  fc2 wants the hidden activations as an operand with k =
// channel, i.e. the transpose of what a C-layout lane holds, and the operand goes through LDS anyway: lane (c, h) writes its value of
// token t as ONE half into chunk (plane, s = c >> 4, lane' = t + 32 ((c >> 2) & 1)), element 4 ((c >> 3) & 1) + (c & 3).  The chunk
// index is XOR-ed with s + 2 (lane' >> 5) so that the 64 lanes of one such store hit 32 different banks (unswizzled: 8); the fc2
// units read the tile with the same XOR (x2_load_swz).  Token rows that do not exist are not written: their halves keep whatever
// finite operand the tile held before, which only ever reaches the same padding token's outputs.
__device__ __forceinline__ X2 x2_load_swz(const float* __restrict__ tile, int lane) {
    const f16x8* q = reinterpret_cast<const f16x8*>(tile);
    X2 o;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int s = 0; s < 2; ++s) o.p[pl][s] = q[(pl * 2 + s) * 64 + (lane ^ (s + 2 * (lane >> 5)))];
    return o;
}
struct HidAddr { int base, off[4]; };                  // byte offsets of a C-layout lane into a hidden operand tile
__device__ __forceinline__ HidAddr hid_addr(int lane) {
    const int c = lane & 31, hh = lane >> 5, s = c >> 4, kh = (c >> 2) & 1, jj = 4 * ((c >> 3) & 1) + (c & 3), swz = s + 2 * kh;
    HidAddr a;
    a.base = s * 1024 + (4 * hh + 32 * kh) * 16 + jj * 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) a.off[q] = (q ^ swz) * 16;
    return a;
}
// two planes of 16 x v[r] for the token rows r < LR, scattered into the operand tile
template <int LR>
__device__ __forceinline__ void hid_store(float* tile, const HidAddr& ha, const f32x16& v) {
    char* lb = reinterpret_cast<char*>(tile) + ha.base;
#pragma unroll
    for (int r = 0; r < LR; ++r) {
        const float x = v[r] * 16.0f;
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        char* pr = lb + ha.off[r & 3] + (r >> 2) * 128;
        *reinterpret_cast<_Float16*>(pr) = hi;
        *reinterpret_cast<_Float16*>(pr + 2048) = lo;
    }
}
// the first ceil(LR / 4) register groups of a block
template <int LR>
__device__ __forceinline__ f32x16 load_block_rows(const float* __restrict__ p, int lane) {
    const f32x4* q = reinterpret_cast<const f32x4*>(p) + lane;
    f32x16 v = zero16();
#pragma unroll
    for (int g = 0; g < (LR + 3) / 4; ++g) {
        const f32x4 t = q[g * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * g + j] = t[j];
    }
    return v;
}

}  // namespace
}  // namespace gator
