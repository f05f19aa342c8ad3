// The MDR joint tokens and their cross-attention K / V tiles (lib/models/GATOR.py:19, MDR.py:130-134,37-38,65): what k_gat_joint
// (gat_tail.hip) and k_gat8's fused tail (gat8_tail.h) share -- the vector table and its staging, the job decode, LN1's affine step.
// (The 64-channel statistics are fused_common.h's ln_center64, which k_mdr_joint's layernorm64 uses too; k_gat<., true> ends with
// the lifter and builds no joint tokens.)  The token-wise products differ per kernel (fp32 WTile, or the H3 four-product form) and
// stay with their kernels; so do the five pose columns and the two masks of joints >= J, which as shared functions moved the
// instructions of all three kernels (profiles/refactor_encoder_forms.txt).
//   jf = Linear(133 -> 64)(cat(pose2d, pose3d / 1000, feat)) + pos_j;  per LBF layer li: k = wk(LN1(jf)), v = wv(LN1(jf))
//   K tile [hd][g][lane=(joint,h)][j] = k[joint][32hd+8g+4h+j]  (T-layout block hd)
//   V tile [hd][g][lane=(d,h)][j]     = v[joint=8g+4h+j][32hd+d] (C-layout block hd)
#pragma once
#include "fused_common.h"

namespace gator {
namespace {

// every per-channel vector of the joint-token part as one LDS table: jf bias | jf columns 0..4 [5][64] | norm1 w / b [3 layers][64]
enum { VJ_JFB = 0, VJ_JF5 = 64, VJ_N1W = 384, VJ_N1B = 576, VJ_TOTAL = 768 };
// thread t < VJ_TOTAL / 4 stages one float4 of the table.  ARGS: jf_b, jf5, j_n1w[3], j_n1b[3]
template <class ARGS>
__device__ __forceinline__ void joint_stage_vecs(const ARGS& a, float* VJ, int t) {
    const int off = 4 * t;
    const float* src = off < VJ_JF5 ? a.jf_b + off : off < VJ_N1W ? a.jf5 + (off - VJ_JF5)
                       : off < VJ_N1B ? a.j_n1w[(off - VJ_N1W) >> 6] + (off & 63) : a.j_n1b[(off - VJ_N1B) >> 6] + (off & 63);
    reinterpret_cast<f32x4*>(VJ)[t] = *reinterpret_cast<const f32x4*>(src);
}
// the 12 K / V jobs of a sample: job = (layer li, k | v, channel block nb)
struct JointJob { int li, kv, nb; };
__device__ __forceinline__ JointJob joint_job(int job) { return JointJob{job >> 2, (job >> 1) & 1, job & 1}; }
// LN1 of layer li from the centred tokens d0, d1 and their rstd (fused_common.h: ln_center64)
__device__ __forceinline__ void joint_norm1(const f32x16& d0, const f32x16& d1, float rstd, const float* VJ, int li, int h, f32x16& fz0, f32x16& fz1) {
    fz0 = d0 * rstd * chanvec_lds(VJ, VJ_N1W + 64 * li, h) + chanvec_lds(VJ, VJ_N1B + 64 * li, h);
    fz1 = d1 * rstd * chanvec_lds(VJ, VJ_N1W + 64 * li + 32, h) + chanvec_lds(VJ, VJ_N1B + 64 * li + 32, h);
}

}  // namespace
}  // namespace gator
