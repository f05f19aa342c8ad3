// What the four forms of the vertex regressor (upsample_fused.hip, upsample_bf16.hip, upsample_x3.hip, upsample_x2.hip) share:
// the 16-deep k-step count, the 12-byte vertex store and the tables of the joint-regression epilogue.
#pragma once
#include "fused_state.h"
#include "x3_common.h"      // bf16x8 / f16x8, GATOR_MFMA_BF16 / GATOR_MFMA_F16

namespace gator {

constexpr int kS16 = 28;      // 16-deep k-steps over the 431 (-> 448) coarse vertices

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

}  // namespace gator
