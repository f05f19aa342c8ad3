// MDR head, the parts beside the tiles (mdr_fused.hip): the joint tokens' K/V tiles in front of the layers (k_mdr_joint) and, behind them, the coarse vertices
// from the per-token head features (MDR.py:156-166) -- k_mdr_head_finish on the tiles' conv partial sums, or the whole head in k_mdr_head (A/B form).
#include "mdr_ops.h"

#include <cmath>

namespace gator {
namespace {

struct HeadArgs {
    const float *hf, *bn_w, *bn_b, *bn_mean, *bn_var, *bconv_w, *bconv_b;
    float *vc, *vcp;
    __bf16* vcp3;           // non-null: write the hi/mid/lo bf16 planes of the split-precision vertex GEMM instead of vcp
    size_t vcp3_plane;
    _Float16* vcp2;         // non-null: write the scaled hi/lo fp16 planes of the two-plane vertex GEMM (upsample_x2.hip) instead
    const unsigned* persist_ctr;   // non-null: the counter blocks of the forward's persistent launches.  The sample's launch must not have tripped its
    MdrChunkPlan plan;             // hang guard and must have counted all 14 last-stage tiles of the sample; else its vertices are NaN (loud, not silent)
    unsigned* status;              // the ctx's sticky device status words, one per DeviceStatus reason (host-mapped; internal.h), read by the next API call
    const float* pose2d;           // the forward's input poses [B][J][2] (non-null on the whole-forward path): a bad sample whose own input is not
    int J;                         // finite reports DEV_INPUT_NONFINITE -- the reference returns NaN for it too -- instead of DEV_NONFINITE
    int alpha;
};

// A wave whose tokens of sample b hold a bad coarse vertex reports why: its persistent launch did not finish the sample (1), the sample's own
// input pose is not finite (3), else a non-finite activation or the operand range (2).  Each reason has its own status word, set by a plain
// store, so the reports of one forward never overwrite each other whatever the order of their waves.  The input is only read when bad.
__device__ __forceinline__ void head_report(const HeadArgs& a, int b, bool bad, bool poisoned) {
    if (!a.status || !__any(bad)) return;
    const int lane = threadIdx.x & 63;
    bool in_bad = false;
    if (a.pose2d && !poisoned) {
        for (int i = lane; i < 2 * a.J; i += 64) in_bad = in_bad || !__builtin_isfinite(a.pose2d[(size_t)b * 2 * a.J + i]);
        in_bad = __any(in_bad);
    }
    if (lane == 0)      // sticky, host-visible: the next API call on the ctx (or gator_device_status) reports it
        __hip_atomic_store(a.status + (poisoned ? DEV_PERSIST_INCOMPLETE : in_bad ? DEV_INPUT_NONFINITE : DEV_NONFINITE), 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// where a coarse vertex coordinate goes: the reference layout (tap / stage API) and the packed A operand of whichever vertex GEMM the ctx runs.
// The three layouts are regressor_slots.h's act_slot_x2 / act_slot_b16 / act_slot_f32 and the splits x3_common.h's split2 / split3, restated:
// written with those functions k_mdr_head_finish and both k_mdr_head<512, .> compile to other listings (profiles/refactor_regressor.txt)
__device__ __forceinline__ void head_store(const HeadArgs& a, int b, int v, int c, float val) {
    const int mt = b >> 5, sl = b & 31;
    a.vc[((size_t)b * kV + v) * 3 + c] = val;
    if (a.vcp2) {       // two fp16 planes of 2^4 * val, in k_upsample_x2's operand order [mt/4][v/16][mt%4][l'][plane][lane][v%8]
        const float sv = val * 16.0f;
        const _Float16 hi = (_Float16)sv;
        const _Float16 lo = (_Float16)(sv - (float)hi);
        const size_t pair = ((((size_t)(mt >> 2) * 28 + (v >> 4)) * 4 + (mt & 3)) * 3 + c) * 2;
        const size_t e = (size_t)(((v >> 3) & 1) * 32 + sl) * 8 + (v & 7);
        a.vcp2[pair * 512 + e] = hi; a.vcp2[(pair + 1) * 512 + e] = lo;
    } else if (a.vcp3) {       // exact three-way bf16 split, in k_upsample_x3's operand order [plane][mt][l'][v/16][lane][v%8]
        const __bf16 hi = (__bf16)val;
        const float r1 = val - (float)hi;
        const __bf16 mid = (__bf16)r1;
        const __bf16 lo = (__bf16)(r1 - (float)mid);
        const size_t e = ((((size_t)mt * 3 + c) * 28 + (v >> 4)) * 64 + ((v >> 3) & 1) * 32 + sl) * 8 + (v & 7);
        a.vcp3[e] = hi; a.vcp3[a.vcp3_plane + e] = mid; a.vcp3[2 * a.vcp3_plane + e] = lo;
    } else {
        const int cb = v >> 5, g = (v & 31) >> 3, hh = (v & 7) >> 2, j = v & 3;
        a.vcp[(((((size_t)mt * 3 + c) * kCB + cb) * 4 + g) * 64 + hh * 32 + sl) * 4 + j] = val;
    }
}

// |vert431| must stay below 4 094 m for the two-plane vertex regressor (16 x value in an fp16 plane); any non-finite value -- e.g. an activation
// beyond +-4 094 that overflowed an fp16 operand plane somewhere upstream -- ends up at the test against this limit as NaN too
__device__ __forceinline__ float head_limit(const HeadArgs& a) { return a.vcp2 ? 4094.0f : 3.0e38f; }

// ---- the head behind the tiles' conv partials (round 6): bias_conv1d's result = bias + the 14 partials in tile order; then per token the softmax-mix
// of MDR.py:161-166.  One sample; `bc`: 60 floats of LDS; called by every thread of a workgroup of NT threads (k_mdr_head_finish).
// Light by construction: no conv, no cross-lane sums.
template <int NT>
__device__ __forceinline__ void head_finish(const HeadArgs& a, const double* __restrict__ hpart_b, int b, bool poisoned, float (*bc)[3]) {
    const int t = threadIdx.x;
    const float* hf = a.hf + (size_t)b * kV * 32;
    constexpr int NR = (kV + NT - 1) / NT;
    // every global read up front: this thread's tokens' head features, and (threads 0..59) the partials of output (row, position) t
    f32x4 row[NR][5], tail[NR], cc[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int v = t + NT * i;
        const float* r = hf + (v < kV ? v : 0) * 32;
#pragma unroll
        for (int g = 0; g < 5; ++g) row[i][g] = *reinterpret_cast<const f32x4*>(r + 4 * g);
        tail[i] = *reinterpret_cast<const f32x4*>(r + 24);
        cc[i] = *reinterpret_cast<const f32x4*>(r + 28);
    }
    if (t < 60) {
        double pv[kVT];
#pragma unroll
        for (int k = 0; k < kVT; ++k) pv[k] = hpart_b[k * 64 + t];
        double s = pv[0];
#pragma unroll
        for (int k = 1; k < kVT; ++k) s += pv[k];
        bc[t / 3][t % 3] = (float)(s + (double)a.bconv_b[t / 3]);
    }
    __syncthreads();
    const float limit = head_limit(a);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int v = t + NT * i;
        if (v < kV) {
            float av[20];
#pragma unroll
            for (int g = 0; g < 5; ++g) { av[4 * g] = row[i][g][0]; av[4 * g + 1] = row[i][g][1]; av[4 * g + 2] = row[i][g][2]; av[4 * g + 3] = row[i][g][3]; }
            float mx = -1e30f, p[20], l = 0.f;
            for (int m = 0; m < 20; ++m) mx = fmaxf(mx, av[m]);
            for (int m = 0; m < 20; ++m) {
                p[m] = __builtin_amdgcn_exp2f((av[m] - mx) * kLog2e);
                l += p[m];
            }
            const float il = 1.0f / l;
            // alpha = 1.1 ** scale_linear(x)  (MDR.py:162): powf via double exp keeps it exact to fp32 rounding; once per token
            const float sc = a.alpha ? (float)exp((double)tail[i][3] * 0.09531017980432493) : 1.0f;
            for (int c = 0; c < 3; ++c) {
                float o = 0.f;
                for (int m = 0; m < 20; ++m) o += (p[m] * il) * bc[m][c];
                float val = sc * o + cc[i][c];
                if (poisoned) val = __builtin_nanf("");
                bad = bad || !(fabsf(val) < limit);
                head_store(a, b, v, c, val);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    head_report(a, b, bad, poisoned);
}

// Joint tokens: jf = Linear(133->64)(pose_combine) + pos_j (MDR.py:130-134); per layer k = wk(LN1(jf)), v = wv(LN1(jf))
// (MDR.py:37-38 with norm1 applied to the concatenated tokens, :65).  jf does not change across the three layers.
// One workgroup (2 waves) per sample; wave w owns channel block w (= head w).  Output in MFMA operand order:
//   K tile [hd][g][lane=(joint,h)][j] = k[joint][32hd+8g+4h+j]  (T-layout block hd)
//   V tile [hd][g][lane=(d,h)][j]     = v[joint=8g+4h+j][32hd+d] (C-layout block hd)
struct JointArgs {
    const float *pc, *jw_p, *jb, *posj_T;       // jw_p: packed [2 nb][5 kb]; posj_T: [2] T-layout tiles of pos_j[1..J]
    const float *n1w[3], *n1b[3], *wk_p[3], *wv_p[3];
    float* jkv;
    int J;
    unsigned* mdr_ctr;      // non-null: zero k_mdr_persist's tickets and completion counts (B = gridDim.x)
    int x2;                 // K/V tiles as two fp16 planes of 16 x value (mdr_ops.h: JointX2) instead of fp32 blocks
};
__global__ __launch_bounds__(128) void k_mdr_joint(const JointArgs a) {
    __shared__ __attribute__((aligned(16))) float PCt[5 * kTile];
    __shared__ __attribute__((aligned(16))) float JF[2 * kTile];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, h = lane >> 5, J = a.J;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    if (a.mdr_ctr) {
        // every launch's counter block (tickets, error flag, completion counts): the whole region, dealt over the workgroups
        for (size_t i = (size_t)b * 128 + t; i < mdr_ctr_words((int)gridDim.x); i += (size_t)gridDim.x * 128) a.mdr_ctr[i] = 0u;
    }
    for (int e = t; e < 5 * kTile; e += 128) {
        const int j4 = e & 3, ln = (e >> 2) & 63, g = (e >> 8) & 3, kb = e >> 10;
        const int tok = ln & 31, k = 32 * kb + 8 * g + 4 * (ln >> 5) + j4;
        PCt[e] = (tok < J && k < 133) ? a.pc[((size_t)b * J + tok) * 133 + k] : 0.f;
    }
    __syncthreads();
    {
        f32x16 a0 = load_chanvec_S(a.jb, 32 * wave, h) + load_block(a.posj_T + wave * kTile, lane), a1 = zero16();
#pragma unroll
        for (int kb = 0; kb < 5; ++kb) {
            if (kb & 1) a1 = mma_T(load_wtile(a.jw_p, wave * 5 + kb, lane), load_block(PCt + kb * kTile, lane), a1);
            else a0 = mma_T(load_wtile(a.jw_p, wave * 5 + kb, lane), load_block(PCt + kb * kTile, lane), a0);
        }
        store_block(JF + wave * kTile, lane, a0 + a1);
    }
    __syncthreads();
    f32x16 jf[2];
    jf[0] = load_block(JF, lane);
    jf[1] = load_block(JF + kTile, lane);
    const bool tok_ok = (lane & 31) < J;
#pragma unroll 1
    for (int li = 0; li < 3; ++li) {
        f32x16 fz[2];
        layernorm64(jf, a.n1w[li], a.n1b[li], h, fz);
        float* out = a.jkv + (((size_t)b * 3 + li) * 4) * kTile;
        f32x16 kt, k1 = zero16();
        kt = zero16();
        mma2_T(load_wtile(a.wk_p[li], wave * 2 + 0, lane), fz[0], kt, load_wtile(a.wk_p[li], wave * 2 + 1, lane), fz[1], k1);
        kt += k1;
        if (!tok_ok) kt = zero16();             // joints >= J: zero rows (masked in the softmax anyway)
        if (a.x2) x2_store(out + wave * kTile, lane, x2_split(kt * 16.0f)); else store_block(out + wave * kTile, lane, kt);
        f32x16 vt = zero16(), v1 = zero16();
        mma2_C(load_wtile(a.wv_p[li], wave * 2 + 0, lane), fz[0], vt, load_wtile(a.wv_p[li], wave * 2 + 1, lane), fz[1], v1);
        vt += v1;
#pragma unroll
        for (int r = 0; r < 16; ++r) vt[r] = (kap(r) + 4 * h < J) ? vt[r] : 0.f;
        if (a.x2) x2_store(out + (2 + wave) * kTile, lane, x2_split(vt * 16.0f)); else store_block(out + (2 + wave) * kTile, lane, vt);
    }
}

// sum of a double over the 64 lanes on DPP row operations (quad swaps, half-row and row mirrors: every lane ends with its row's total) and four
// v_readlane per half -- 12 cross-lane moves in registers instead of the 12 ds_bpermute round trips of a __shfl_xor butterfly; fixed association
__device__ __forceinline__ double dpp_mov_f64(double v, int which) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    int lo = (int)(unsigned)u, hi = (int)(unsigned)(u >> 32);
    if (which == 0) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xf, 0xf, false); }             // quad_perm [1,0,3,2]
    else if (which == 1) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xf, 0xf, false); }        // quad_perm [2,3,0,1]
    else if (which == 2) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xf, 0xf, false); }      // row_half_mirror
    else { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xf, 0xf, false); }                      // row_mirror
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_sum64_f64(double s) {
    s += dpp_mov_f64(s, 0); s += dpp_mov_f64(s, 1); s += dpp_mov_f64(s, 2); s += dpp_mov_f64(s, 3);
    const unsigned long long u = __builtin_bit_cast(unsigned long long, s);
    const int lo = (int)(unsigned)u, hi = (int)(unsigned)(u >> 32);
    double t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned l2 = (unsigned)__builtin_amdgcn_readlane(lo, 16 * r), h2 = (unsigned)__builtin_amdgcn_readlane(hi, 16 * r);
        t[r] = __builtin_bit_cast(double, ((unsigned long long)h2 << 32) | l2);
    }
    return (t[0] + t[1]) + (t[2] + t[3]);
}

// MDR head (MDR.py:156-166) from the per-token head features hf[b][v][32]:
//   ch 0..19 = mat_A, 24..26 = bias_linear out, 27 = scale_linear out, 28..30 = mat_C   (our own packing order)
// Writes vert431 both in the reference layout (tap / stage API) and as the packed A operand of the vertex GEMM.
// One workgroup per sample, three short phases with a barrier between them.  The kernel is a LATENCY chain, not a throughput one
// (18.7 us at B = 64, 24 us at B = 256, round-3 sweep): with HOIST every global read it will ever need -- this lane's 63 conv
// weights, its token's 32 head features -- is issued before the first phase, and the phases run on registers and LDS only
// (16 / 13 us).  That costs 196 VGPRs, one workgroup per CU: batches of more than two workgroups per CU take the rolled form
// (same arithmetic in the same order, 2 workgroups per CU), which is the faster one there.
template <int NT, bool HOIST>
__global__ __launch_bounds__(NT, HOIST ? 2 : 4) void k_mdr_head(const HeadArgs a) {
    static_assert(NT >= kV, "one token per thread");
    __shared__ float bn[kV][5];      // [0 | x y z | 0]: the conv's zero padding of the xyz axis as stored zeros (unconditional reads in the loop)
    __shared__ float bc[20][3];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* hf = a.hf + (size_t)b * kV * 32;
    const int v = t;
    const bool tok = v < kV;
    constexpr int NW = NT / 64, NIT = (kV * 3 + 63) / 64;
    // ---- all global reads up front
    f32x4 row[5], tail = {0.f, 0.f, 0.f, 0.f}, cc = tail;
    auto load_rows = [&]() {
        const float* r = hf + v * 32;
#pragma unroll
        for (int g = 0; g < 5; ++g) row[g] = *reinterpret_cast<const f32x4*>(r + 4 * g);
        cc = *reinterpret_cast<const f32x4*>(r + 28);
    };
    if (tok) {
        tail = *reinterpret_cast<const f32x4*>(hf + v * 32 + 24);
        if (HOIST) load_rows();
    }
    // Conv1d(431->20,k3,p1) weight of row m = wave + 8 q at e = lane + 64 it
    auto conv_w = [&](int q, int it) {
        const int e = lane + 64 * it, m = wave + NW * q;
        return e < kV * 3 ? a.bconv_w[(m < 20 ? m : 0) * (kV * 3) + e] : 0.f;
    };
    float wreg[3][HOIST ? NIT : 1];
    if (HOIST) {
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int q = 0; q < 3; ++q) wreg[q][HOIST ? it : 0] = conv_w(q, it);
    }
    if (tok) {
        float x[3] = {tail[0], tail[1], tail[2]};      // (mdr_ops.h: head_bias_act, written out -- the call timed slower than the A/B bound allows, profiles/refactor_mdr_forms.txt)
        if (a.alpha) {      // LayerNorm(3)
            const float m = (x[0] + x[1] + x[2]) / 3.0f;
            const float qq = ((x[0] - m) * (x[0] - m) + (x[1] - m) * (x[1] - m) + (x[2] - m) * (x[2] - m)) / 3.0f;
            const float rs = 1.0f / sqrtf(qq + 1e-5f);
            for (int c = 0; c < 3; ++c) x[c] = (x[c] - m) * rs * a.bn_w[c] + a.bn_b[c];
        } else {            // BatchNorm1d(431) eval: channel = vertex
            const float rs = 1.0f / sqrtf(a.bn_var[v] + 1e-5f);
            for (int c = 0; c < 3; ++c) x[c] = (x[c] - a.bn_mean[v]) * rs * a.bn_w[v] + a.bn_b[v];
        }
        bn[v][0] = 0.f; bn[v][4] = 0.f;
        for (int c = 0; c < 3; ++c) bn[v][1 + c] = gelu_f(x[c]);
    }
    __syncthreads();
    {   // Conv1d(431->20,k3,p1) over the xyz axis.  Wave w owns output rows m = w, w+8, w+16 and walks the whole (c,k) axis:
        // 9 accumulators and 9 wave reductions per wave.
        float acc[3][3];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.f;
        // Round 6 (the conv loop was 6.5 of the launch's 17 us, the nine double-precision butterflies through LDS 2.6, by timing cuts): the walk
        // e = lane + 64 it advances (channel c, tap k) by (21, +1) instead of dividing; the padding is stored zeros, not conditions; the
        // products are fused multiply-adds; the wave sums run on DPP row operations (still in double: bc feeds every coarse vertex).
        int cch = lane / 3, ktap = lane - 3 * cch;
#pragma unroll(HOIST ? NIT : 1)
        for (int it = 0; it < NIT; ++it) {
            const int e = lane + 64 * it;
            if (e < kV * 3) {
                // tap k of channel c meets input position l + k - 1 (zero padding outside 0..2 = the stored zeros)
                const float in0 = bn[cch][ktap], in1 = bn[cch][ktap + 1], in2 = bn[cch][ktap + 2];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float w = HOIST ? wreg[q][HOIST ? it : 0] : conv_w(q, it);
                    acc[q][0] = fmaf(w, in0, acc[q][0]);
                    acc[q][1] = fmaf(w, in1, acc[q][1]);
                    acc[q][2] = fmaf(w, in2, acc[q][2]);
                }
            }
            cch += ktap == 2 ? 22 : 21;          // e + 64 = 3 (c + 21) + (k + 1)
            ktap = ktap == 2 ? 0 : ktap + 1;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const double s = wave_sum64_f64((double)acc[q][l]);
                const int m = wave + NW * q;
                if (lane == 0 && m < 20) bc[m][l] = (float)(s + (double)a.bconv_b[m]);
            }
    }
    __syncthreads();
    const int mt = b >> 5, sl = b & 31;
    bool poisoned = false;
    if (a.persist_ctr) {      // (the lookup of k_mdr_head_finish, written out: as a shared function it timed slower here, profiles/refactor_mdr_forms.txt)
        int ch, b0, n;
        a.plan.locate(b, ch, b0, n);
        const unsigned* blk = a.persist_ctr + a.plan.block(ch);
        poisoned = blk[kCtrError] != 0u || blk[kCtrDone + (size_t)3 * n + (b - b0)] != (unsigned)kVT;
    }
    const float limit = head_limit(a);
    bool bad = false;
    if (tok) {
        if (!HOIST) load_rows();
        // (the softmax-mix and the store below are head_finish's, and stay written out here: as functions shared with head_finish they change
        // k_mdr_head_finish's instructions -- head_store's second caller alone does, profiles/refactor_mdr_forms.txt.  The layouts below are
        // regressor_slots.h's, restated as in head_store.)
        float av[20];
#pragma unroll
        for (int g = 0; g < 5; ++g) { av[4 * g] = row[g][0]; av[4 * g + 1] = row[g][1]; av[4 * g + 2] = row[g][2]; av[4 * g + 3] = row[g][3]; }
        float mx = -1e30f, p[20], l = 0.f;
        for (int m = 0; m < 20; ++m) mx = fmaxf(mx, av[m]);
        for (int m = 0; m < 20; ++m) {
            p[m] = __builtin_amdgcn_exp2f((av[m] - mx) * kLog2e);
            l += p[m];
        }
        const float il = 1.0f / l;
        // alpha = 1.1 ** scale_linear(x)  (MDR.py:162): powf via double exp keeps it exact to fp32 rounding; once per token
        const float sc = a.alpha ? (float)exp((double)tail[3] * 0.09531017980432493) : 1.0f;
        const int cb = v >> 5, g = (v & 31) >> 3, hh = (v & 7) >> 2, j = v & 3;
        for (int c = 0; c < 3; ++c) {
            float o = 0.f;
            for (int m = 0; m < 20; ++m) o += (p[m] * il) * bc[m][c];
            float val = sc * o + cc[c];
            if (poisoned) val = __builtin_nanf("");
            bad = bad || !(fabsf(val) < limit);
            a.vc[((size_t)b * kV + v) * 3 + c] = val;
            if (a.vcp2) {       // two fp16 planes of 2^4 * val, in k_upsample_x2's operand order [mt/4][v/16][mt%4][l'][plane][lane][v%8]
                const float sv = val * 16.0f;
                const _Float16 hi = (_Float16)sv;
                const _Float16 lo = (_Float16)(sv - (float)hi);
                const size_t pair = ((((size_t)(mt >> 2) * 28 + (v >> 4)) * 4 + (mt & 3)) * 3 + c) * 2;
                const size_t e = (size_t)(((v >> 3) & 1) * 32 + sl) * 8 + (v & 7);
                a.vcp2[pair * 512 + e] = hi; a.vcp2[(pair + 1) * 512 + e] = lo;
            } else if (a.vcp3) {       // exact three-way bf16 split, in k_upsample_x3's operand order [plane][mt][l'][v/16][lane][v%8]
                const __bf16 hi = (__bf16)val;
                const float r1 = val - (float)hi;
                const __bf16 mid = (__bf16)r1;
                const __bf16 lo = (__bf16)(r1 - (float)mid);
                const size_t e = ((((size_t)mt * 3 + c) * 28 + (v >> 4)) * 64 + ((v >> 3) & 1) * 32 + sl) * 8 + (v & 7);
                a.vcp3[e] = hi; a.vcp3[a.vcp3_plane + e] = mid; a.vcp3[2 * a.vcp3_plane + e] = lo;
            } else {
                a.vcp[(((((size_t)mt * 3 + c) * kCB + cb) * 4 + g) * 64 + hh * 32 + sl) * 4 + j] = val;
            }
        }
    }
    head_report(a, b, bad, poisoned);
}

__global__ __launch_bounds__(256) void k_mdr_head_finish(const HeadArgs a, const double* __restrict__ hpart) {
    __shared__ float bc[20][3];
    const int b = blockIdx.x;
    bool poisoned = false;
    if (a.persist_ctr) {      // the sample's launch must not have tripped its hang guard and must have counted all 14 last-stage tiles
        int ch, b0, n;
        a.plan.locate(b, ch, b0, n);
        const unsigned* blk = a.persist_ctr + a.plan.block(ch);
        poisoned = blk[kCtrError] != 0u || blk[kCtrDone + (size_t)3 * n + (b - b0)] != (unsigned)kVT;
    }
    head_finish<256>(a, hpart + (size_t)b * kVT * 64, b, poisoned, bc);
}

}  // namespace

// pc [B,J,133] (reference layout) -> ws.jkv, the joint tokens' K/V tiles of the three layers; zeroes the persistent launches' counters when p says so
int launch_mdr_joint(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pc, int B, void* stream) {
    const Weights& w = c->w;
    JointArgs ja;
    ja.pc = pc; ja.jw_p = f->jfeat_p; ja.jb = w.jfeat_b; ja.posj_T = f->posj_T; ja.jkv = ws.jkv; ja.J = c->J;
    for (int i = 0; i < 3; ++i) { ja.n1w[i] = w.lay[i].n1w; ja.n1b[i] = w.lay[i].n1b; ja.wk_p[i] = f->lay[i].wk; ja.wv_p[i] = f->lay[i].wv; }
    ja.mdr_ctr = p.ctr_zero == CtrZero::MDR_JOINT ? ws.mdr_ctr : nullptr;
    ja.x2 = f->opt.mdr_x3 == 2;
    StageTimer tm(c, "mdr_joint", stream);
    k_mdr_joint<<<B, 128, 0, (hipStream_t)stream>>>(ja);
    return GATOR_OK;
}

// ws.hf (and, for MdrHead::FINISH, ws.hpart) -> ws.vc [B,431,3] and the packed operand of the ctx's vertex GEMM; the head kernel is p.head
int launch_mdr_head(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, int B, void* stream, const float* pose2d) {
    hipStream_t st = (hipStream_t)stream;
    const Weights& w = c->w;
    HeadArgs ha;
    ha.hf = ws.hf; ha.bn_w = w.bn_w; ha.bn_b = w.bn_b; ha.bn_mean = w.bn_mean; ha.bn_var = w.bn_var;
    ha.bconv_w = w.bconv_w; ha.bconv_b = w.bconv_b; ha.vc = ws.vc; ha.vcp = ws.vcp;
    ha.persist_ctr = p.persist ? ws.mdr_ctr : nullptr;
    ha.plan = p.chunks;
    ha.status = c->status_dev;
    ha.pose2d = pose2d; ha.J = c->J;      // nullptr from the MDR-only entry point: its input is the pose features, not the poses
    ha.vcp2 = f->opt.up_x3 == 2 ? (_Float16*)ws.vcp3 : nullptr;
    ha.vcp3 = f->opt.up_x3 == 1 ? (__bf16*)ws.vcp3 : nullptr; ha.vcp3_plane = upsample_x3_vcp_elems(ws.cap) / 3;     // plane stride fixed by the workspace capacity
    ha.alpha = c->alpha;
    StageTimer tm(c, "mdr_head", stream);
    switch (p.head) {
    case MdrHead::FINISH: k_mdr_head_finish<<<B, 256, 0, st>>>(ha, reinterpret_cast<const double*>(ws.hpart)); break;      // the conv came out of the tiles as partial sums: what is left is light
    case MdrHead::WHOLE_HOIST: k_mdr_head<512, true><<<B, 512, 0, st>>>(ha); break;
    case MdrHead::WHOLE: k_mdr_head<512, false><<<B, 512, 0, st>>>(ha); break;
    }
    return GATOR_OK;
}

}  // namespace gator
