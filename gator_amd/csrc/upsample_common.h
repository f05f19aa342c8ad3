// The vertex regressor's one statement.  Its four kernels (upsample_fused.hip fp32-input MFMA, upsample_x3.hip three bf16 planes,
// upsample_x2.hip two fp16 planes, upsample_bf16.hip one bf16 plane) differ in how they form the conv sums; everything around the sums
// is here or in regressor_slots.h: where an operand element lives and the tap list (regressor_slots.h), the one pack kernel that writes
// every packed operand through those slots, the finished vertex with the joint-regression epilogue (regress_finish; k_upsample_x2
// keeps it written out, see there), and the row's launch and pack entries.  The plane splits are x3_common.h's split2 / split3, the LDS-DMA helpers fused_common.h's.
#pragma once
#include "fused_state.h"
#include "x3_common.h"      // bf16x8 / f16x8, GATOR_MFMA_BF16 / GATOR_MFMA_F16, split2 / split3

namespace gator {

constexpr int kActShift = 4;      // the two-plane form carries its activations x 2^4 (upsample_x2.hip)

struct __attribute__((packed)) F3 { float x, y, z; };      // one vertex: a 12-byte store

// Joint-regression epilogue (lib/core/base.py:221, demo/run.py:142: joints = J_regressor @ mesh, a 107-nnz matrix): a wave that
// has just formed vertex v of its samples also writes w_e * v for every regressor entry e = (joint, v, w_e) of its 32-vertex
// block into P[sample][e][xyz]; k_jreg_reduce sums each joint's entries in a fixed order.  No atomics, no second pass over the
// 82 kB/mesh of vertices -- and with `out` == nullptr the vertices are never written at all (evaluation needs the joints only).
struct JregEpi {
    const int2* blk;            // [kOB] (first entry, entry count) of every 32-vertex block, entries sorted by vertex
    const int2* ent;            // (vertex, slot in P) per entry
    const float* w;             // weight per entry
    float* P;                   // [B][nnz][3]; nullptr: no joint regression
    int nnz;
};
inline JregEpi jreg_epi(const FusedState* f, bool with_joints) {
    JregEpi jr{};
    if (with_joints) { jr.blk = (const int2*)f->jr_blk.get(); jr.ent = (const int2*)f->jr_ent.get(); jr.w = f->jr_w.get(); jr.P = f->jr_P.get(); jr.nnz = f->jr_nnz; }
    return jr;
}

// The finished vertices of a wave's NT accumulator tiles of 32 vertices x 32 samples (vertex block ob on the lanes, sample tiles mt[]
// in the registers; tiles nt.. repeat an earlier one and are not stored): (sum + bias) + template -- the conv output first, then the
// template add, MDR.py:167-168 -- as one 12-byte store per (sample, vertex), and with JREG its regressor entries.  sum(m, l, r) is the
// finished conv sum of tile m, coordinate l, register r; a wave that is not `live` stores nothing.
template <bool JREG, int NT, class Sum>
__device__ __forceinline__ void regress_finish(int ob, const int (&mt)[NT], int nt, bool live, int lane, int B, const float* __restrict__ bias,
                                               const float* __restrict__ tpl, float* __restrict__ out, const JregEpi& jr, Sum sum) {
    const int ov = 32 * ob + (lane & 31), h = lane >> 5;
    if (ov >= kNV || !live) return;
    const float bo = bias[ov];
    const float t0 = tpl[ov * 3], t1 = tpl[ov * 3 + 1], t2 = tpl[ov * 3 + 2];
    int2 jb{0, 0};
    if constexpr (JREG) jb = jr.P ? jr.blk[ob] : int2{0, 0};      // regressor entries of this vertex block (most blocks have none)
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        if (m > 0 && m >= nt) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int smp = 32 * mt[m] + kap(r) + 4 * h;
            if (smp >= B) continue;
            F3 v;
            v.x = (sum(m, 0, r) + bo) + t0;
            v.y = (sum(m, 1, r) + bo) + t1;
            v.z = (sum(m, 2, r) + bo) + t2;
            if (!JREG || out) *reinterpret_cast<F3*>(out + ((int64_t)smp * kNV + ov) * 3) = v;
            if constexpr (JREG)
                for (int e = jb.x; e < jb.x + jb.y; ++e) {
                    const int2 en = jr.ent[e];
                    if (en.x == ov) {
                        const float we = jr.w[e];
                        F3 q;
                        q.x = we * v.x; q.y = we * v.y; q.z = we * v.z;
                        *reinterpret_cast<F3*>(jr.P + ((int64_t)smp * jr.nnz + en.y) * 3) = q;
                    }
                }
        }
    }
}

// The pack kernel of every operand of the row: activations vc[b][431][3] and weights w[o][431][3] alike are [row][coarse vertex][t]
// arrays (t = input position | tap).  A thread takes one padded coordinate triple, rounds or splits SCALE * value (zero in the padding)
// into the form's PLANES planes of T and writes them through SLOT (regressor_slots.h), `plane` elements apart.  Threads are numbered in
// the order every layout's fragments share -- 8 k indices, 32 rows, the k half, then k-step, t and row block -- so a wave writes whole fragments.
template <class T, int PLANES, bool SCALED, size_t (*SLOT)(int, int, int)>
__global__ void k_pack_operand(const float* __restrict__ src, int rows, int rows_pad, T* __restrict__ dst, size_t plane, float scale) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)rows_pad * kRegK * 3) return;
    int64_t q = e >> 9;
    const int s = (int)(q % kS16); q /= kS16;
    const int t = (int)(q % 3), row = 32 * (int)(q / 3) + (int)((e >> 3) & 31), c = 16 * s + (int)((e >> 5) & 8) + (int)(e & 7);
    float x = (row < rows && c < kV) ? src[((int64_t)row * kV + c) * 3 + t] : 0.f;
    if constexpr (SCALED) x *= scale;
    T* d = dst + SLOT(row, c, t);
    if constexpr (PLANES == 1) d[0] = (T)x;
    else if constexpr (PLANES == 2) { const Split2<T> p = split2<T>(x); d[0] = p.h; d[plane] = p.l(); }
    else { const Split3<T> p = split3<T>(x); d[0] = p.h; d[plane] = p.m; d[2 * plane] = p.l(); }
}
template <class T, int PLANES, bool SCALED, size_t (*SLOT)(int, int, int)>
inline int pack_operand(const float* src, int rows, int rows_pad, void* dst, size_t plane, float scale, void* stream) {
    const int64_t n = (int64_t)rows_pad * kRegK * 3;
    k_pack_operand<T, PLANES, SCALED, SLOT><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(src, rows, rows_pad, (T*)dst, plane, scale);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

// the four kernels' launchers, behind launch_upsample_any (upsample_fused.hip).  verts == nullptr: vertices are not stored (joint
// regression only); with_joints: also fill f->jr_P for launch_jreg_reduce
int launch_upsample_f32(const FusedState* f, const gator_ctx* c, const FusedWs& ws, int B, float* verts, void* stream);
int launch_upsample_bf16(const FusedState* f, const gator_ctx* c, const FusedWs& ws, int B, float* verts, void* stream);
int launch_upsample_x3(const FusedState* f, const gator_ctx* c, const FusedWs& ws, int B, float* verts, void* stream, bool with_joints);
int launch_upsample_x2(const FusedState* f, const gator_ctx* c, const FusedWs& ws, int B, float* verts, void* stream, bool with_joints, bool w1);
int pack_upsample_x2(const float* up_w, void* dst, float* unscale, void* stream);      // chooses the weights' power-of-two scale

}  // namespace gator
