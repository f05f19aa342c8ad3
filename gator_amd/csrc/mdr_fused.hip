// MDR head (lib/models/MDR.py:124-170) as register-resident MFMA kernels (fp32 values; products on split 16-bit operands, see TokOp<XA> in mdr_ops.h).
//
// One wave owns one 32-token tile of one sample's 431 coarse-vertex tokens (14 tiles/sample) and keeps its 64-channel
// token state in registers in the MFMA accumulator layout (fused_common.h).  Everything that is row-wise in the
// reference -- LayerNorms, the cross-attention over the J joint tokens (MDR.py:34-46), the Mlp 64->256->64 (timm Mlp,
// MDR.py:61,68), the Annotated-Transformer LayerNorm (vanilla_transformer_encoder.py:31-34), the q/k/v in-projections and
// the out-projection + residual of the 431x431 self-attention (vanilla_transformer_encoder.py:82-94) -- chains through
// MFMAs without touching LDS.  The only cross-token dependency is the self-attention's K/V of the whole sample, so the
// three LBF layers become four stages - four launches (k_mdr_layer<MODE>) or, where the batch leaves a fractional generation of
// workgroups, ONE persistent launch that hands the same stages out as tickets (k_mdr_persist, further down):
//     L0: tokenise -> tokenwise(0)              (writes vf, Q, K, V of layer 0, all in operand-packed tiles)
//     L1: attention(0)+out-proj+res -> tokenwise(1)
//     L2: attention(1)+out-proj+res -> tokenwise(2)
//     L3: attention(2)+out-proj+res -> head features (motion_linear | bias_linear | scale_linear, MDR.py:156-162)
// Attention is flash-style: S^T = K Q^T per 32-key tile with the key on the accumulator row, online softmax in registers
// (one lane<->lane^32 max exchange per tile), and the probability registers are fed straight back as the B operand of
// O^T += V^T P^T.  K and V tiles are stored by the producer in exactly the operand order the consumer loads (1 KiB
// coalesced float4 wave loads from L2), so no LDS staging or barrier is needed.
// Here: the tile body, k_mdr_layer, k_mdr_persist, the diagnostic probes and launch_mdr.  mdr_ops.h: the row-wise helpers, the attention loops and the
// operand policy TokOp<XA> of the four arithmetic forms.  mdr_head.hip: the joint-token kernel and the head kernels.
#include "fused_common.h"
#include "fused_state.h"
#include "x3_common.h"

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <type_traits>

// Diagnostic library only (GATOR_MDR_CUT, time-only experiments: results are meaningless): bit 0 = every weight load of a matrix reads its
// tile 0, bit 1 = every K / V load of the 431-key attention reads key tile 0 -- the loads stay, their L2 -> L1 traffic goes (L1 hits).
#ifdef GATOR_DIAG
namespace gator { namespace {
__device__ int g_mdr_wmask = -1, g_mdr_kvmask = -1;
__device__ unsigned long long* g_persist_ends = nullptr;      // GATOR_MDR_ENDS=1: [workgroup][start, last ticket taken, end] wall-clock stamps (100 MHz) of k_mdr_persist
} }
#define MDR_WIDX(i) ((i) & g_mdr_wmask)
#define MDR_KVIDX(i) ((i) & g_mdr_kvmask)
#endif
#include "mdr_ops.h"

namespace gator {
namespace {

struct LayerW {   // packed tiles (MdrLayerP) + reference-layout vectors of one LBF layer
    const float *wq, *proj, *fc1, *fc2, *sa0, *sa1, *sa2, *sa3;
    const float *n1w, *n1b, *proj_b, *n2w, *n2b, *fc1_b, *fc2_b, *a2, *b2, *sa0_b, *sa1_b, *sa2_b, *sa3_b;
};

struct MdrArgs {
    int B, J, layer;
    const float *vf_in, *q_in, *k_in, *v_in;
    float *vf_out, *q_out, *k_out, *v_out;
    const float* jkv;        // [B][3][2][2][kTile]
    const float* pc;         // [B][J][133]  (stand-alone MDR entry) or nullptr when x_out is given
    const float* xout;       // [B][3J] pose3d in mm (full forward: pose_combine is never materialised)
    const int32_t* vj;       // [431]
    const float *tok_base, *tok_w3;
    const float *head_w, *head_b;
    float *hf, *lbf;
    LayerW prev, cur;        // prev: layer whose attention/out-proj runs first; cur: layer whose tokenwise part runs
    float lin_s, lin_inv;    // GATOR_MDR_X3=2: every token-wise linear returns lin_s x its value (x3_common.h: 4-product linears); lin_inv = 1 / lin_s
    // the head's Conv1d(431 -> 20, k3, p1) (MDR.py:121,163) as per-tile partial sums made by the tile that has the tokens' bias features in registers (round 6)
    double* hpart;           // [B][14][64] (60 used: row m, position l at m * 3 + l); nullptr: not computed (the A/B form with k_mdr_head)
    const float *bconv_w, *hbn_w, *hbn_b, *hbn_mean, *hbn_var;
    int halpha;
#ifdef GATOR_DIAG
    unsigned long long* stamps;   // diagnostic build only (libgator_hip_diag.so, GATOR_MDR_STAMPS=1)
#endif
};

// ---- GELU by table (XA == 3 only).  The exact GELU is a quarter of the one-plane tile's vector work (one degree-8 polynomial + exp2 per
// value, in packed fp32 that the SIMD issues at half rate); its result is rounded to ONE fp16 plane right afterwards, so Phi(x) is read
// from an LDS table instead: 3 072 (value, forward difference) pairs on [-6, 6) in steps of 1 / 256, linear interpolation -- error of Phi
// below 4.6e-7 (h^2 / 8 max|Phi''|), against 2.4e-4 |x| for the fp16 rounding that follows; |x| >= 6 clamps to Phi = 0 / 1 (exact to 1e-9).
// Seven vector instructions and one ds_read_b64 per value instead of ~14 issue slots.  The fp32 configuration keeps the polynomial.
constexpr int kGeluTab = 3072;
__device__ __forceinline__ void gelu_table_fill(float* GT) {      // cooperative (256 threads); the caller puts a barrier behind it
    for (int e = threadIdx.x; e < kGeluTab; e += 256) {
        const float x0 = (float)(e - kGeluTab / 2) * (1.0f / 256.0f), x1 = x0 + (1.0f / 256.0f);
        const float p0 = 0.5f * (1.0f + erf_fast(x0 * 0.70710678118654752440f)), p1 = 0.5f * (1.0f + erf_fast(x1 * 0.70710678118654752440f));
        GT[2 * e] = p0;
        GT[2 * e + 1] = e + 1 < kGeluTab ? p1 - p0 : 0.f;
    }
}
// v holds S x value (k = 1 / S): returns S x GELU(value)
__device__ __forceinline__ void gelu_tile_table(f32x16& v, float k, const float* GT) {
    const float ks = k * 256.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float t = __builtin_fmaf(v[r], ks, (float)(kGeluTab / 2));
        t = __builtin_amdgcn_fmed3f(t, 0.0f, (float)kGeluTab - 0.0005f);
        const float fl = __builtin_floorf(t);
        const f32x2 e = *reinterpret_cast<const f32x2*>(GT + 2 * (int)fl);
        v[r] = v[r] * __builtin_fmaf(t - fl, e[1], e[0]);
    }
}

// MODE 0: tokenise + tokenwise(0) ; 1: attention + tokenwise ; 2: attention + head features
// XA   the arithmetic form (mdr_ops.h: TokOp<XA>)
// per-channel vectors of a stage (biases, norm weights) staged once per workgroup in LDS
enum { VO_SA3B = 0, VO_N1W = 64, VO_N1B = 128, VO_PROJB = 192, VO_N2W = 256, VO_N2B = 320, VO_FC2B = 384, VO_A2 = 448, VO_B2 = 512,
       VO_SA0B = 576, VO_SA1B = 640, VO_HEADB = 704, VO_FC1B = 768, VO_TOKW3 = 1024, VO_TOTAL = 1216 };
// ---- the head's Conv1d(431 -> 20, kernel 3, padding 1 over the xyz axis; MDR.py:121,163) as per-tile partial sums ------------------------------
// Until round 6 k_mdr_head did the whole conv per sample: a 15 us launch of its own whose conv loop and cross-lane sums were most of its chain.  The tile
// that computes a token's head features has the conv's input -- the token's three bias features -- in registers, so it leaves the tile's 60 partial sums
// (20 rows x 3 positions over its 32 tokens) behind; the finish (head_finish: sum of the 14 partials in tile order, softmax-mix per token) is light.
// Everything in double: each product exact, fixed association -- the result does not depend on who computes it.
// The finish stays a launch of its own (11 us against k_mdr_head's 15): inside the persistent launch -- as a fifth ticket stage, or run by the workgroup that
// publishes a sample's last tile -- it measured +8 .. +51 us, because the last ~18 samples of an XCD finish together at the launch's end and their heads then
// stand behind the last tile instead of beside each other (DESIGN 4c'', profiles/r06_fused_head_stage.txt, docs/history/r06_inlaunch_head.patch).
// Sum of 32 values per lane over the 32 lanes of its half (lanes 0..31 | 32..63) as a reduce-scatter: at step s a lane hands the half of its list that its partner
// keeps (row mirror, half-row mirror, quad reverse, quad swap, v_permlane16_swap) and adds what it receives to the half it keeps -- 16 + 8 + 4 + 2 + 1 exchanges
// instead of 32 x 5, and lane p ends with the total of entry slot32(p).  A fixed tree: the result does not depend on who runs it.
// the partner's value at step s.  The partner must hold the SAME entries as the lane, i.e. differ from it only in bits that have not been decided yet: the row
// mirror (15 - i: flips bits 0..3, decided: bit 3), the half-row mirror (7 - i: bits 0..2, decided: bit 2), the quad reverse (3 - i: bits 0, 1, decided: bit 1), the
// quad swap (bit 0), v_permlane16_swap (bit 4)
__device__ __forceinline__ double lane_xchg_f64(double v, int step) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    int lo = (int)(unsigned)u, hi = (int)(unsigned)(u >> 32);
    if (step == 0) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xf, 0xf, false); }           // row_mirror
    else if (step == 1) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xf, 0xf, false); }      // row_half_mirror
    else if (step == 2) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x1B, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x1B, 0xf, 0xf, false); }        // quad_perm [3,2,1,0]
    else if (step == 3) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xf, 0xf, false); }        // quad_perm [1,0,3,2]
    else {
        const auto rl = __builtin_amdgcn_permlane16_swap((unsigned)lo, (unsigned)lo, false, false), rh = __builtin_amdgcn_permlane16_swap((unsigned)hi, (unsigned)hi, false, false);
        const bool up = (threadIdx.x & 16) != 0;      // [0]: the value of the lane with bit 4 clear, [1]: with bit 4 set
        lo = (int)(up ? rl[0] : rl[1]); hi = (int)(up ? rh[0] : rh[1]);
    }
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// the lane keeps the upper half of its list iff the step's deciding bit of its own index is set; its partner (the other value of that bit) keeps the other half
template <int N, int STEP, int BIT>
__device__ __forceinline__ void rs_step(double (&v)[32], int lane) {
    const bool up = ((lane >> BIT) & 1) != 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double send = up ? v[i] : v[N + i], keep = up ? v[N + i] : v[i];
        v[i] = keep + lane_xchg_f64(send, STEP);
    }
}
// -> the lane's total and (slot) which of the 32 entries it is the total of
__device__ __forceinline__ double half_reduce_scatter32(double (&v)[32], int lane, int& slot) {
    rs_step<16, 0, 3>(v, lane);
    rs_step<8, 1, 2>(v, lane);
    rs_step<4, 2, 1>(v, lane);
    rs_step<2, 3, 0>(v, lane);
    rs_step<1, 4, 4>(v, lane);
    slot = 16 * ((lane >> 3) & 1) + 8 * ((lane >> 2) & 1) + 4 * ((lane >> 1) & 1) + 2 * (lane & 1) + ((lane >> 4) & 1);
    return v[0];
}
// lane (token, h) of a T-layout tile: `x` = the token's bias features after bias_norm + GELU (MDR.py:159-160; zeros for a token that does not exist).  Half h makes
// rows m = 10 h .. 10 h + 9: position l of row m collects tap k of the input at l + k - 1.  `dst`: the tile's 64 doubles, entry (m, l) at m * 3 + l.
__device__ __forceinline__ void head_conv_partial(const float* __restrict__ bconv_w, int token, const float (&x)[3], int lane, double* __restrict__ dst) {
    const int h = lane >> 5;
    const float* wp = bconv_w + (size_t)(10 * h) * (kV * 3) + 3 * (token < kV ? token : 0);
    double v[32];
#pragma unroll
    for (int mm = 0; mm < 10; ++mm) {      // per token in fp32 (three products each: the shipped head's lanes ran 21-term fp32 chains), across tokens and tiles in double
        const float w0 = wp[mm * (kV * 3)], w1 = wp[mm * (kV * 3) + 1], w2 = wp[mm * (kV * 3) + 2];
        v[mm * 3 + 0] = (double)fmaf(w2, x[1], w1 * x[0]);
        v[mm * 3 + 1] = (double)fmaf(w2, x[2], fmaf(w1, x[1], w0 * x[0]));
        v[mm * 3 + 2] = (double)fmaf(w1, x[2], w0 * x[1]);
    }
    v[30] = 0.0; v[31] = 0.0;
    int slot;
    const double tot = half_reduce_scatter32(v, lane, slot);
    if (slot < 30) dst[30 * h + slot] = tot;
}
constexpr int kParkF4 = 8 * 256;       // f32x4 slots of the residual-stream parking area (split-precision forms only)

// cooperative (256 threads); the caller puts a barrier behind it
template <int MODE, int XA>
__device__ __forceinline__ void mdr_stage_vectors(const MdrArgs& a, float* VT) {
    for (int e = threadIdx.x; e < VO_TOTAL / 4; e += 256) {
        const int off = 4 * e;
        const float* src = nullptr;
        if (off < VO_N1W) { if (MODE > 0) src = a.prev.sa3_b + off; }
        else if (off >= VO_HEADB && off < VO_HEADB + 32) { if (MODE == 2) src = a.head_b + (off - VO_HEADB); }
        else if (off >= VO_TOKW3) { if (MODE == 0) src = a.tok_w3 + (off - VO_TOKW3); }
        else if (MODE < 2 && off < VO_HEADB) {
            const float* tab[10] = {a.cur.n1w, a.cur.n1b, a.cur.proj_b, a.cur.n2w, a.cur.n2b, a.cur.fc2_b, a.cur.a2, a.cur.b2, a.cur.sa0_b, a.cur.sa1_b};
            src = tab[(off - VO_N1W) >> 6] + (off & 63);
        } else if (MODE < 2 && off >= VO_FC1B && off < VO_TOKW3) src = a.cur.fc1_b + (off - VO_FC1B);
        if (src) {
            f32x4 v = *reinterpret_cast<const f32x4*>(src);
            // 4-product linears return lin_s x their value: the biases that start or join their accumulators carry the factor too
            if (XA >= 2 && (off < VO_N1W || (off >= VO_PROJB && off < VO_N2W) || (off >= VO_FC2B && off < VO_A2) || (off >= VO_SA0B && off < VO_TOKW3)))
                v = v * a.lin_s;
            // norm1 / norm2 only feed 4-product linears: their affine part carries the operand scale, so LayerNorm's FMA delivers 16 x value
            if (XA >= 2 && ((off >= VO_N1W && off < VO_PROJB) || (off >= VO_N2W && off < VO_FC2B))) v = v * kActScale;
            reinterpret_cast<f32x4*>(VT)[e] = v;
        }
    }
}

// one wave, one 32-token tile `id` = sample * 14 + tile of the sample
template <int MODE, int XA>
__device__ __forceinline__ void mdr_tile(const MdrArgs& a, const int id, const float* VT, f32x4* park, const float* GT = nullptr, const MdrArgs* a_mem = nullptr) {      // a_mem: the same arguments IN MEMORY (kernel-argument segment)
    typedef TokOp<XA> Op;
    constexpr bool X = XA != 0;
    constexpr int TQ = Op::kTileQ;
    auto park_vf = [&](const f32x16 (&v)[2]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x4 t4;
#pragma unroll
            for (int j = 0; j < 4; ++j) t4[j] = v[i >> 2][4 * (i & 3) + j];
            park[i * 256 + threadIdx.x] = t4;
        }
    };
    auto unpark_vf = [&](f32x16 (&v)[2]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 t4 = park[i * 256 + threadIdx.x];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i >> 2][4 * (i & 3) + j] = t4[j];
        }
    };
    // `lane` is opaque to the optimiser: inside k_mdr_persist's ticket loops every address that depends only on the lane (the
    // weight tiles) would otherwise be loop-invariant, hoisted in front of the loop and kept alive across it (470 B of scratch)
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    const int h = lane >> 5;
    if (id >= a.B * kVT) return;
#ifdef GATOR_DIAG
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_last = a.stamps ? clock64() : 0;
    const unsigned long long rt0 = a.stamps ? wall_clock64() : 0, ck0 = st_last;
#define MDR_STAMP(i)                                      \
    __builtin_amdgcn_sched_barrier(0);                    \
    if (a.stamps) {                                       \
        const unsigned long long now_ = clock64();        \
        st_acc[i] += now_ - st_last;                      \
        st_last = now_;                                   \
    }
#else
#define MDR_STAMP(i)
#endif
    constexpr bool H = XA >= 2;                 // 4-product (XA 2) / 2-product (XA 3) linears: their raw outputs carry the factor a.lin_s
    const float inv = H ? a.lin_inv : 1.0f;
    const int b = id / kVT, t = id % kVT;
    const size_t tile = ((size_t)b * kVT + t) * 2;          // index of this wave's first block in vf/q/k/v
    const int token = 32 * t + (lane & 31);
    const LayerW& w = a.cur;
    f32x16 vf[2];
    typename Op::W A, B;
    typedef typename Op::A Act;
    if (MODE == 0) {
        A = Op::ldw(w.wq, 0, 1, lane);
        B = Op::ldw(w.wq, 2, 3, lane);
        // verts tokens = Linear(6->64)([v431, pose3d[vj]/1000]) + pos_v   (MDR.py:126-137); the v431/bias/pos part is folded
        const int tk = token < kV ? token : kV - 1;
        float x0, x1, x2;
        if (a.xout) {             // pose3d / 1000 (GATOR.py:19), same fp32 division as the reference
            const float* p3 = a.xout + ((size_t)b * a.J + a.vj[tk]) * 3;
            x0 = p3[0] / 1000.f; x1 = p3[1] / 1000.f; x2 = p3[2] / 1000.f;
        } else {
            const float* p3 = a.pc + ((size_t)b * a.J + a.vj[tk]) * 133 + 2;
            x0 = p3[0]; x1 = p3[1]; x2 = p3[2];
        }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x16 v = load_block(a.tok_base + ((size_t)t * 2 + nb) * kTile, lane);
            v += chanvec_lds(VT, VO_TOKW3 + 32 * nb, h) * x0;
            v += chanvec_lds(VT, VO_TOKW3 + 64 + 32 * nb, h) * x1;
            v += chanvec_lds(VT, VO_TOKW3 + 128 + 32 * nb, h) * x2;
            vf[nb] = v;
        }
    } else {
        f32x16 att[2];
        // (two written-out calls: as a two-trip loop, or through a lambda, the heads' inlined key loops are unrolled late and k_mdr_layer / k_mdr_persist come out with other instructions)
        att[0] = Op::attend(a.q_in + (tile + 0) * TQ, a.k_in + ((size_t)b * kVT * 2 + 0) * TQ, a.v_in + ((size_t)b * kVT * 2 + 0) * TQ, lane);
        att[1] = Op::attend(a.q_in + (tile + 1) * TQ, a.k_in + ((size_t)b * kVT * 2 + 1) * TQ, a.v_in + ((size_t)b * kVT * 2 + 1) * TQ, lane);
        A = Op::ldw(a.prev.sa3, 0, 1, lane);
        B = Op::ldw(a.prev.sa3, 2, 3, lane);
        vf[0] = load_block(a.vf_in + (tile + 0) * kTile, lane);
        vf[1] = load_block(a.vf_in + (tile + 1) * kTile, lane);
        MDR_PIN();
        MDR_STAMP(0)
        // linears[-1] + residual (vanilla_transformer_encoder.py:94, MDR.py:143)
        const Act attx[2] = {Op::from_scaled(att[0]), Op::from_scaled(att[1])};      // the heads come out at the operand scale already
        const f32x16 y0 = lin2_T(A, attx, chanvec_lds(VT, VO_SA3B, h));
        if (MODE == 1) A = Op::ldw(w.wq, 0, 1, lane); else if (XA != 3) A = Op::ldw(a.head_w, 0, 1, lane);
        MDR_PIN();
        const f32x16 y1 = lin2_T(B, attx, chanvec_lds(VT, VO_SA3B + 32, h));
        if (MODE == 1) B = Op::ldw(w.wq, 2, 3, lane);
        MDR_PIN();
        if constexpr (H) { vf[0] = fma16(y0, inv, vf[0]); vf[1] = fma16(y1, inv, vf[1]); }
        else { vf[0] += y0; vf[1] += y1; }
    }
    if (MODE == 2) {
        if (a.lbf != nullptr && token < kV) {      // the "mdr_lbf2" tap (110 KB per sample): only when taps are recorded
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v4[j] = vf[nb][4 * g + j];
                    *reinterpret_cast<f32x4*>(a.lbf + ((size_t)b * kV + token) * kE + 32 * nb + 8 * g + 4 * h) = v4;
                }
        }
        // the head features (mat_A | bias_linear | scale_linear | mat_C, MDR.py:156-162) keep the fp32 configuration's operands even in
        // 16-bit mode: mat_C goes straight into the coarse vertices, and this is 8 MFMAs of a tile's ~350 (profiles/r05_emulate_16bit.txt, C3d)
        typedef TokOp<XA == 3 ? 2 : XA> HeadOp;
        const typename HeadOp::A vfx[2] = {HeadOp::from(vf[0]), HeadOp::from(vf[1])};
        f32x16 acc;
        if constexpr (XA == 3) acc = lin2_T(HeadOp::ldw(a.head_w, 0, 1, lane), vfx, chanvec_lds(VT, VO_HEADB, h));
        else acc = lin2_T(A, vfx, chanvec_lds(VT, VO_HEADB, h));
        if constexpr (H) acc = acc * inv;
        if (token < kV) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v4;
#pragma unroll
                for (int j = 0; j < 4; ++j) v4[j] = acc[4 * g + j];
                *reinterpret_cast<f32x4*>(a.hf + ((size_t)b * kV + token) * 32 + 8 * g + 4 * h) = v4;
            }
        }
        {   // the head conv's partial sums over this tile's tokens (their bias features are channels 24..26 = registers 12..14 of the lower half's lanes)
            const MdrArgs* ah = a_mem;        // (taking the address of a by-value kernel argument would copy all of it to scratch)
            asm volatile("" : "+s"(ah));      // its fields are fetched here, behind the tile body: nothing of them lives across it
            if (ah != nullptr && ah->hpart) {
                float x[3] = {acc[12], acc[13], acc[14]};
                if (h == 0 && token < kV) head_bias_act(ah->halpha != 0, ah->hbn_w, ah->hbn_b, ah->hbn_mean, ah->hbn_var, token, x);
                else { x[0] = x[1] = x[2] = 0.f; }
#pragma unroll
                for (int c = 0; c < 3; ++c) {      // the upper half works on the same tokens: rows 10..19
                    const float other = xhalf(x[c]);
                    x[c] = h ? other : x[c];
                }
                head_conv_partial(ah->bconv_w, token, x, lane, ah->hpart + ((size_t)b * kVT + t) * 64);
            }
        }
        return;
    }
    MDR_STAMP(1)
    // ---- CrossAttentionBlock (MDR.py:64-69) ----
    {
        f32x16 q[2], o[2];
        Act fz[2];
        {
            f32x16 fzf[2];
            layernorm64_L(vf, VT + VO_N1W, VT + VO_N1B, h, fzf);
            fz[0] = Op::from_scaled(fzf[0]); fz[1] = Op::from_scaled(fzf[1]);      // XA >= 2: already 16 x value (staged 16 w, 16 b)
        }
        const float* jb = a.jkv + (((size_t)b * 3 + a.layer) * 4) * kTile;       // [k/v][head] tiles
        q[0] = lin2_T(A, fz, zero16());
        A = Op::ldw(w.proj, 0, 1, lane);
        MDR_PIN();
        q[1] = lin2_T(B, fz, zero16());
        B = Op::ldw(w.proj, 2, 3, lane);
        MDR_PIN();
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            o[hd] = cross_attention_head<XA>(jb + hd * kTile, jb + (2 + hd) * kTile, q[hd], Op::JOp::kScale * inv, a.J, lane);      // q carries lin_s
        }
        const Act ox[2] = {Op::from_scaled(o[0]), Op::from_scaled(o[1])};      // cross_attention_head returns the operand scale x value
        const f32x16 y0 = lin2_T(A, ox, chanvec_lds(VT, VO_PROJB, h));
        A = Op::ldw(w.fc1, 0, 1, lane);                                            // MLP chunk 0: fc1 rows 0..31
        MDR_PIN();
        const f32x16 y1 = lin2_T(B, ox, chanvec_lds(VT, VO_PROJB + 32, h));
        B = Op::ldw(w.fc2, 0, 8, lane);                                            //              fc2 columns 0..31, both row blocks
        MDR_PIN();
        if constexpr (H) { vf[0] = fma16(y0, inv, vf[0]); vf[1] = fma16(y1, inv, vf[1]); }
        else { vf[0] += y0; vf[1] += y1; }
    }
    MDR_STAMP(2)
    {
        f32x16 acc2[2][2];
        Act y2[2];
        {
            f32x16 y2f[2];
            layernorm64_L(vf, VT + VO_N2W, VT + VO_N2B, h, y2f);
            y2[0] = Op::from_scaled(y2f[0]); y2[1] = Op::from_scaled(y2f[1]);
        }
        if constexpr (X) {      // the residual stream waits in LDS while the MLP needs the registers
            park_vf(vf);
        }
        acc2[0][0] = chanvec_lds(VT, VO_FC2B, h);
        acc2[1][0] = chanvec_lds(VT, VO_FC2B + 32, h);
        acc2[0][1] = zero16();
        acc2[1][1] = zero16();
        // XA 3 is a latency-bound kernel (waves parked or issue-stalled 64 % of their time, profiles/r05_pmc_config3_B256.txt): its loop is
        // software-pipelined by one chunk inside the wave -- fc1 of chunk c + 1 is issued BEFORE the bias + GELU + conversion of chunk c, so
        // the eight dependent MFMAs run under that vector work instead of in front of it, and fc2's two chains are interleaved.
        if constexpr (XA == 3) {
            f32x16 hn = lin2_T(A, y2, zero16());                                        // fc1, chunk 0
            A = Op::ldw(w.fc1, 2, 3, lane);
            MDR_PIN();
#pragma unroll 1
            for (int c = 0; c < 8; ++c) {
                f32x16 hdn = hn;
                if (c < 7) hn = lin2_T(A, y2, zero16());                               // fc1, chunk c + 1: independent of everything below
                hdn += chanvec_lds(VT, VO_FC1B + 32 * c, h);
                gelu_tile_table(hdn, inv, GT);
                const X1 hx = Op::from(hdn, inv);
                __builtin_amdgcn_sched_barrier(0);
                if (c < 6) A = Op::ldw(w.fc1, 2 * (c + 2), 2 * (c + 2) + 1, lane); else if (c == 6) A = Op::ldw(w.sa0, 0, 1, lane);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 2; ++s) {                                          // fc2: two independent chains, small planes first
                    acc2[0][0] = GATOR_MFMA_F16(B.t[0].mid[s], hx.p[s], acc2[0][0]);
                    acc2[1][0] = GATOR_MFMA_F16(B.t[1].mid[s], hx.p[s], acc2[1][0]);
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    acc2[0][0] = GATOR_MFMA_F16(B.t[0].hi[s], hx.p[s], acc2[0][0]);
                    acc2[1][0] = GATOR_MFMA_F16(B.t[1].hi[s], hx.p[s], acc2[1][0]);
                }
                if (c < 7) B = Op::ldw(w.fc2, c + 1, 8 + c + 1, lane); else B = Op::ldw(w.sa0, 2, 3, lane);
                MDR_PIN();
            }
        } else
#pragma unroll 1
        for (int c = 0; c < 8; ++c) {           // 256 hidden units in 8 chunks of 32: fc1 -> GELU -> fc2 partial
            f32x16 hdn;
            if constexpr (X) {      // bias after the products: its scalar loads fly during the MFMAs instead of in front of them
                hdn = lin2_T(A, y2, zero16());
                if (c < 7) A = Op::ldw(w.fc1, 2 * (c + 1), 2 * (c + 1) + 1, lane); else A = Op::ldw(w.sa0, 0, 1, lane);
                MDR_PIN();
                hdn += chanvec_lds(VT, VO_FC1B + 32 * c, h);
            } else {
                hdn = lin2_T(A, y2, chanvec_lds(VT, VO_FC1B + 32 * c, h));
                if (c < 7) A = Op::ldw(w.fc1, 2 * (c + 1), 2 * (c + 1) + 1, lane); else A = Op::ldw(w.sa0, 0, 1, lane);
                MDR_PIN();
            }
            if constexpr (H) gelu_tile_scaled(hdn, inv); else gelu_tile(hdn);
            if constexpr (H) {
                const X2 hx = Op::from(hdn, inv);
                acc2[0][0] = h3_mma_wa(B.t[0], hx, acc2[0][0]);
                acc2[1][0] = h3_mma_wa(B.t[1], hx, acc2[1][0]);
            } else if constexpr (X) {
                const X3 hx = x3_split(hdn);
                acc2[0][0] = x3_mma(B.t[0], hx, acc2[0][0]);
                acc2[1][0] = x3_mma(B.t[1], hx, acc2[1][0]);
            } else {
                mma2_T(B.t[0], hdn, acc2[0][c & 1], B.t[1], hdn, acc2[1][c & 1]);   // even / odd chunks: 2 chains of 128 products each
            }
            if (c < 7) B = Op::ldw(w.fc2, c + 1, 8 + c + 1, lane); else B = Op::ldw(w.sa0, 2, 3, lane);
            MDR_PIN();
        }
        if constexpr (H) {
            unpark_vf(vf);
            vf[0] = fma16(acc2[0][0], inv, vf[0]);
            vf[1] = fma16(acc2[1][0], inv, vf[1]);
        } else if constexpr (X) {
            unpark_vf(vf);
            vf[0] += acc2[0][0];
            vf[1] += acc2[1][0];
        } else {
            vf[0] += acc2[0][0] + acc2[0][1];
            vf[1] += acc2[1][0] + acc2[1][1];
        }
    }
    MDR_STAMP(3)
    custom_ln64_L(vf, VT + VO_A2, VT + VO_B2, h);                                           // MDR.py:142 self.norm
    store_block(a.vf_out + (tile + 0) * kTile, lane, vf[0]);
    store_block(a.vf_out + (tile + 1) * kTile, lane, vf[1]);
    // ---- in-projections of the self-attention (vanilla_transformer_encoder.py:87-89) in the consumer's operand order ----
    {
        const Act vfx[2] = {Op::from(vf[0]), Op::from(vf[1])};
        f32x16 y0 = lin2_T(A, vfx, chanvec_lds(VT, VO_SA0B, h));
        A = Op::ldw(w.sa1, 0, 1, lane);
        MDR_PIN();
        f32x16 y1 = lin2_T(B, vfx, chanvec_lds(VT, VO_SA0B + 32, h));
        B = Op::ldw(w.sa1, 2, 3, lane);
        MDR_PIN();
        if constexpr (X) {      // the consumer's softmax works in the exp2 domain: fold log2(e) / sqrt(d_k) into Q once, here
            const float qs = kLog2e * 0.17677669529663688110f * (XA == 2 ? kX2QK : 1.0f) * inv;      // (XA 3: Q . K is the exp2-domain score itself)
            y0 = y0 * qs;
            y1 = y1 * qs;
        }
        Op::store(a.q_out + (tile + 0) * TQ, lane, y0);
        Op::store(a.q_out + (tile + 1) * TQ, lane, y1);
        y0 = lin2_T(A, vfx, chanvec_lds(VT, VO_SA1B, h));
        A = Op::ldw(w.sa2, 0, 1, lane);
        MDR_PIN();
        y1 = lin2_T(B, vfx, chanvec_lds(VT, VO_SA1B + 32, h));
        B = Op::ldw(w.sa2, 2, 3, lane);
        const float bv0 = w.sa2_b[lane & 31], bv1 = w.sa2_b[32 + (lane & 31)];
        MDR_PIN();
        if (token >= kV) { y0 = zero16(); y1 = zero16(); }                   // pad keys: finite (they are masked anyway)
        if constexpr (XA == 2) { y0 = y0 * (kX2QK * inv); y1 = y1 * (kX2QK * inv); }
        if constexpr (XA == 3) { y0 = y0 * inv; y1 = y1 * inv; }
        Op::store(a.k_out + (tile + 0) * TQ, lane, y0);
        Op::store(a.k_out + (tile + 1) * TQ, lane, y1);
        y0 = lin2_C(A, vfx);                                                  // V in C-layout: channel on the lane
        y1 = lin2_C(B, vfx);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool ok = 32 * t + kap(r) + 4 * h < kV;
            y0[r] = ok ? (H ? __builtin_fmaf(y0[r], inv, bv0) : y0[r] + bv0) : 0.f;
            y1[r] = ok ? (H ? __builtin_fmaf(y1[r], inv, bv1) : y1[r] + bv1) : 0.f;
        }
        if constexpr (XA >= 2) { y0 = y0 * kX2V; y1 = y1 * kX2V; }
        Op::store(a.v_out + (tile + 0) * TQ, lane, y0);
        Op::store(a.v_out + (tile + 1) * TQ, lane, y1);
    }
    MDR_STAMP(4)
#ifdef GATOR_DIAG
    if (a.stamps && id == 0 && lane == 0)
        for (int i = 0; i < 8; ++i) a.stamps[i] = st_acc[i];
    if (a.stamps && (id % 64) == 0 && lane == 0) {      // timeline sample: [start, end] in 100 MHz ticks, cycles, XCC id
        unsigned long long* q = a.stamps + 8 + 4 * (id / 64);
        q[0] = rt0;
        q[1] = wall_clock64();
        q[2] = clock64() - ck0;
        unsigned xcc, hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        q[3] = ((unsigned long long)(xcc & 0xf) << 32) | hwid;
    }
#endif
}

template <int MODE, int XA>
__global__ __launch_bounds__(256, 2) void k_mdr_layer(const MdrArgs a, int nwg) {
    __shared__ f32x4 park[XA != 0 ? kParkF4 : 1];
    __shared__ __attribute__((aligned(16))) float VT[VO_TOTAL];
    __shared__ __attribute__((aligned(16))) float GT[XA == 3 && MODE < 2 ? 2 * kGeluTab : 2];
    if constexpr (XA == 3 && MODE < 2) gelu_table_fill(GT);
    mdr_stage_vectors<MODE, XA>(a, VT);
    __syncthreads();
    mdr_tile<MODE, XA>(a, xcd_remap(blockIdx.x, nwg) * 4 + (threadIdx.x >> 6), VT, park, GT,
                       (const MdrArgs*)(const __attribute__((address_space(4))) MdrArgs*)__builtin_amdgcn_kernarg_segment_ptr());      // `a` is the first kernel argument
}

// ---- all four stages in ONE persistent launch -------------------------------------------------------------------------------
// Why: a tile costs one SIMD ~85k cycles whether or not a second wave shares the SIMD, so a launch takes
// ceil(tiles / 1024 SIMDs) tile times -- at B = 256 that is 3 584 tiles = 3.5 per SIMD, billed as 4, in each of the four launches
// (measured: B = 219 / 256 / 292 -> 127 / 160 / 164 us for the middle launch).  Over all four stages there are exactly 14 tiles per
// SIMD, so one launch that hands out (stage, tile) units from a queue and lets a unit wait only for ITS OWN sample's previous
// stage -- the path's only cross-tile dependency is the self-attention's K/V of the sample -- has no fractional generation left.
//   * one queue per XCD: sample b lives on XCD b % 8 for all four stages, so the Q/K/V/residual tile sets of a sample are written
//     and read through the same L2 (workgroups are dealt round-robin to the XCDs; if they were not, only locality would suffer);
//   * a workgroup takes a ticket (4 consecutive tiles of its XCD's list, stage-major), stages the stage's channel vectors, each
//     wave waits until `done[stage - 1][sample]` says all 14 tiles of its sample are finished (agent-scope acquire), runs the
//     unchanged tile body and bumps `done[stage][sample]` behind an agent-scope release;
//   * tickets are handed out in dependency order and a workgroup holds a ticket only while it runs, so every wait is for a unit
//     that some running workgroup already owns: no deadlock whatever the residency.  A poll budget (~6 s) turns a would-be hang (a bug)
//     into a flag in ctr[kCtrError] and garbage output instead of a dead GPU.
// What if an XCD gets no workgroup (a CU mask, reserved CUs, a partitioned device)?  Its queue is never served and nobody waits for it.
// That must not be silent: EVERY stage counts its finished tiles per sample (the last one too), k_mdr_head refuses a sample whose 14
// head-feature tiles were not all written -- NaN vertices plus the ctx's sticky status word -- and the host side answers the report
// (GATOR_EDEVICE at the next call, api.hip) by switching that ctx to the four-launch form for good.  (Serving foreign queues instead
// was built and measured in round 4: a workgroup claimed a queue by compare-and-swap, its own first, then any unowned one, so that an
// orphan queue was adopted as a whole by ONE other XCD.  Correct in every placement tried -- grids of 1, 3, 5, 13 workgroups -- but with
// the queue loop around the three ticket loops hipcc lays the tile bodies out differently and the launch takes 423 us instead of 385
// even when the loop runs once; a second, cold copy of the body spills 2 KB per lane.  Not worth 10 % of the dominant kernel.)
// Counter block of ONE persistent launch: [0..7] tickets per XCD, [8] error flag, [kCtrDone + stage * B + b] finished tiles of (stage,
// sample), stage 0..3, with B and b the launch's own batch (a large forward runs as several launches over chunks of its samples,
// forward_plan.h: their blocks follow each other in FusedWs::mdr_ctr, see MdrChunkPlan::block).  The kernel's argument block stays exactly
// {stage arguments, ctr}: the tile body needs every scalar register there is, and each further scalar that must survive it
// (measured with a base pointer, an offset and a stride more) is spilled into VGPR lanes and reloaded in its loops: +30 - 40 us.
struct MdrPersistArgs {
    MdrArgs st[4];            // their B and every per-sample pointer are this launch's CHUNK of the batch
    unsigned* ctr;            // this launch's counter block
};
// (Round 5, measured and dropped: the one-plane form XA = 3 built for 168 registers and launched with THREE workgroups per CU -- a SIMD
// issues the vector instructions of three waves faster than of two, tools/microbench/valu_rate.hip -- spills 164 B per lane even with
// one weight pair alive at a time, and runs in the same time: 3.25 ms per forward of 2 048 samples either way.)
template <int XA>
__global__ __launch_bounds__(256, 2) void k_mdr_persist(const MdrPersistArgs p) {
    __shared__ f32x4 park[XA != 0 ? kParkF4 : 1];
    __shared__ __attribute__((aligned(16))) float VT[VO_TOTAL];
    __shared__ __attribute__((aligned(16))) float GT[XA == 3 ? 2 * kGeluTab : 2];
    __shared__ int s_unit;
    if constexpr (XA == 3) gelu_table_fill(GT);      // published by the first ticket's barriers
    const int B = p.st[0].B, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned xcc;                                                // the XCD this workgroup REALLY runs on picks its queue
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const int xcd = (int)(xcc & 7u);
    const int nb = xcd < B ? (B - xcd + 7) >> 3 : 0;            // samples of this XCD: xcd, xcd + 8, ...
    const int ntile = nb * kVT, units = (ntile + 3) >> 2;       // per stage
    if (units == 0) return;
    auto ticket = [&]() {
        __syncthreads();                                        // everyone is done with s_unit (and, at a stage change, with VT)
        if (threadIdx.x == 0) s_unit = (int)atomicAdd(p.ctr + xcd, 1u);
        __syncthreads();
        return __builtin_amdgcn_readfirstlane(s_unit);          // a scalar: stage, tile and sample ids stay out of the VGPRs
    };
    int staged = -1;                                            // the stage whose channel vectors are in VT
    // one ticket: (stage the channel vectors,) wait for the sample's previous stage, run the tile, publish it
    auto run = [&](auto mode, int stage, int unit) {
        constexpr int MODE = decltype(mode)::value;
        // the stage's arguments (p.st[stage]) through a pointer into the kernel-argument segment that the optimiser cannot see
        // through: otherwise every argument load of the body is loop-invariant, hoisted in front of the ticket loop and held in
        // SGPRs across it (106 SGPRs, spills into VGPRs, scratch)
        typedef const __attribute__((address_space(4))) MdrArgs* KArgPtr;
        typedef const __attribute__((address_space(4))) char* KBytePtr;
        unsigned aoff = (unsigned)offsetof(MdrPersistArgs, st) + (unsigned)__builtin_amdgcn_readfirstlane(stage) * (unsigned)sizeof(MdrArgs);
        asm volatile("" : "+s"(aoff));
        KArgPtr ap = (KArgPtr)((KBytePtr)__builtin_amdgcn_kernarg_segment_ptr() + aoff);
        const MdrArgs& a = *(const MdrArgs*)ap;
        const int lt = 4 * (unit - stage * units) + wave;
        const bool live = lt < ntile;                           // (wave-uniform) a ticket's last waves may have nothing left
        const int smp = xcd + 8 * (lt / kVT), id = smp * kVT + lt % kVT;
        // the completion count of the sample's previous stage is requested FIRST: its L2 round trip (1 - 2 us under load, once per
        // tile) hides behind the staging below instead of standing in front of the tile
        const unsigned* d = p.ctr + kCtrDone + (size_t)(MODE > 0 ? stage - 1 : 0) * B + smp;
        unsigned seen = kVT;
        if (MODE > 0 && live && lane == 0) seen = __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (staged != stage) {                                  // tickets come in stage order: at most four times per workgroup
            mdr_stage_vectors<MODE, XA>(a, VT);
            staged = stage;
            __syncthreads();
        }
        if (!live) return;
        if (MODE > 0) {
            if (lane == 0) {
                int budget = 1 << 24;                           // ~6 s of polling
                while (seen < (unsigned)kVT && --budget > 0) {
                    __builtin_amdgcn_s_sleep(8);
                    seen = __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (budget <= 0) atomicExch(p.ctr + kCtrError, 1u + stage);
            }
            // Acquire among CUs that share an L2, with NO cache invalidate: every tile of the three tile sets is written exactly once
            // per launch (launch_mdr) and read only behind its completion count, and the L1 starts a launch empty, so neither
            // the L1 nor the L2 can hold an older copy of what is read from here on.  (The agent-scope fence pair instead --
            // `buffer_wbl2 sc1` / `buffer_inv sc1` at each of ~10k tile starts -- measured +240 us per forward; `buffer_inv sc1`
            // alone +30 us.)  The compiler barrier keeps the tile's loads behind the poll.
            asm volatile("" ::: "memory");
        }
        mdr_tile<MODE, XA>(a, id, VT, park, GT, &a);
        // Release to the same L2: the L1 is write-through, so once the stores are acknowledged (vmcnt 0) every CU of the XCD
        // sees them; then the count goes up (an atomic executed in that L2).  The last stage counts too (for k_mdr_head, see above).
        wait_vm<0>();
        if (lane == 0) __hip_atomic_fetch_add(p.ctr + kCtrDone + (size_t)stage * B + smp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // Tickets come in stage order, so a workgroup's stages only ever go up: three plain loops, one tile body each (one loop with a
    // switch keeps all three bodies' state alive at once: 256 VGPRs + 760 B of scratch).
#ifdef GATOR_DIAG
    const unsigned long long pe_t0 = wall_clock64();
    unsigned long long pe_last = pe_t0;
#define PERSIST_END_MARK() pe_last = wall_clock64()
#else
#define PERSIST_END_MARK()
#endif
    int unit = ticket();
    for (; unit < units; unit = ticket()) run(std::integral_constant<int, 0>(), 0, unit);
    for (; unit < 3 * units; unit = ticket()) {
        const int stage = unit >= 2 * units ? 2 : 1;
        run(std::integral_constant<int, 1>(), stage, unit);
    }
    for (; unit < 4 * units; unit = ticket()) { PERSIST_END_MARK(); run(std::integral_constant<int, 2>(), 3, unit); }
#ifdef GATOR_DIAG
    if (g_persist_ends && threadIdx.x == 0) {
        g_persist_ends[3 * blockIdx.x] = pe_t0;
        g_persist_ends[3 * blockIdx.x + 1] = pe_last;
        g_persist_ends[3 * blockIdx.x + 2] = wall_clock64();
    }
#endif
}

LayerW make_layer(const FusedState* f, const gator_ctx* c, int li) {
    const MdrLayerP& p = f->lay[li];
    const MdrLayerW& r = c->w.lay[li];
    LayerW w;
    // X3 images mirror the fp32 tile grids tile for tile (fused_create)
    auto sel = [&](const float* t) { return f->opt.mdr_x3 ? f->wxbuf + (size_t)(t - f->lay[0].wq) / kTile * kTileX3 : t; };
    w.wq = sel(p.wq); w.proj = sel(p.proj); w.fc1 = sel(p.fc1); w.fc2 = sel(p.fc2);
    w.sa0 = sel(p.sa[0]); w.sa1 = sel(p.sa[1]); w.sa2 = sel(p.sa[2]); w.sa3 = sel(p.sa[3]);
    w.n1w = r.n1w; w.n1b = r.n1b; w.proj_b = r.proj_b; w.n2w = r.n2w; w.n2b = r.n2b; w.fc1_b = r.fc1_b; w.fc2_b = r.fc2_b;
    w.a2 = r.a2; w.b2 = r.b2; w.sa0_b = r.sa_b[0]; w.sa1_b = r.sa_b[1]; w.sa2_b = r.sa_b[2]; w.sa3_b = r.sa_b[3];
    return w;
}

// Each kernel family names its instantiations once, from XA = 3 down (the order the kernels are emitted in): [3 - xa][stage form]
using MdrLayerKernel = void (*)(const MdrArgs, int);
using MdrPersistKernel = void (*)(const MdrPersistArgs);
constexpr MdrLayerKernel kMdrLayer[4][3] = {{k_mdr_layer<0, 3>, k_mdr_layer<1, 3>, k_mdr_layer<2, 3>}, {k_mdr_layer<0, 2>, k_mdr_layer<1, 2>, k_mdr_layer<2, 2>},
                                            {k_mdr_layer<0, 1>, k_mdr_layer<1, 1>, k_mdr_layer<2, 1>}, {k_mdr_layer<0, 0>, k_mdr_layer<1, 0>, k_mdr_layer<2, 0>}};
constexpr MdrPersistKernel kMdrPersist[4] = {k_mdr_persist<3>, k_mdr_persist<2>, k_mdr_persist<1>, k_mdr_persist<0>};

#ifdef GATOR_DIAG
// The diagnostic library's probes around the MDR launches (set-up before them, synchronous read-back and printing behind them): GATOR_MDR_STAMPS' and
// GATOR_MDR_ENDS' buffers, GATOR_MDR_SOLO's dynamic LDS that leaves one workgroup per CU (1 wave/SIMD)
struct MdrDiag { DevBuf<unsigned long long> st, ends; size_t solo = 0; };

int mdr_diag_setup(const FusedState* f, bool persist, hipStream_t st, MdrDiag& d) {
    static const int keep = -1, cut = 0;      // (sources of the asynchronous copies: they outlive the call)
    GATOR_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_mdr_wmask), (f->opt.mdr_cut & 1) ? &cut : &keep, sizeof(int), 0, hipMemcpyHostToDevice, st));
    GATOR_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_mdr_kvmask), (f->opt.mdr_cut & 2) ? &cut : &keep, sizeof(int), 0, hipMemcpyHostToDevice, st));
    d.solo = f->opt.mdr_solo ? 60 * 1024 : 0;
    if (f->opt.mdr_stamps) { GATOR_TRY(d.st.alloc(512 * sizeof(unsigned long long))); GATOR_HIP_CHECK(hipMemset(d.st, 0, 512 * sizeof(unsigned long long))); }
    if (f->opt.mdr_ends && persist) {
        GATOR_TRY(d.ends.alloc(3 * 1024 * sizeof(unsigned long long)));
        unsigned long long* d_ends = d.ends.get();
        GATOR_HIP_CHECK(hipMemset(d_ends, 0, 3 * 1024 * sizeof(unsigned long long)));
        GATOR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_persist_ends), &d_ends, sizeof(d_ends)));
    }
    return GATOR_OK;
}

int mdr_diag_report(MdrDiag& d, int B) {
    if (d.ends) {      // synchronous read-back (diagnostic build only): when did each workgroup of the LAST persistent launch start / take its last ticket / end?
        std::vector<unsigned long long> he(3 * 1024);
        GATOR_HIP_CHECK(hipMemcpy(he.data(), d.ends, he.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long* none = nullptr;
        GATOR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_persist_ends), &none, sizeof(none)));
        d.ends.reset();
        unsigned long long t0 = ~0ull, t1 = 0;
        int n = 0;
        for (int i = 0; i < 1024; ++i) if (he[3 * i + 2]) { t0 = std::min(t0, he[3 * i]); t1 = std::max(t1, he[3 * i + 2]); ++n; }
        if (n) {
            double idle = 0, lastlen = 0, first_end = 1e30, start_spread = 0;
            std::vector<double> ends;
            for (int i = 0; i < 1024; ++i) if (he[3 * i + 2]) {
                idle += (double)(t1 - he[3 * i + 2]) / 100.0;
                lastlen += (double)(he[3 * i + 2] - he[3 * i + 1]) / 100.0;
                first_end = std::min(first_end, (double)(he[3 * i + 2] - t0) / 100.0);
                start_spread = std::max(start_spread, (double)(he[3 * i] - t0) / 100.0);
                ends.push_back((double)(he[3 * i + 2] - t0) / 100.0);
            }
            std::sort(ends.begin(), ends.end());
            fprintf(stderr, "[k_mdr_persist ends, B=%d, %d workgroups] span %.1f us; workgroup starts spread over %.1f us; ends: first %.1f, p10 %.1f, median %.1f, p90 %.1f, last %.1f us; "
                            "mean idle before the last workgroup ends %.1f us; mean length of a workgroup's last stage-3 ticket %.1f us\n",
                    B, n, (double)(t1 - t0) / 100.0, start_spread, first_end, ends[n / 10], ends[n / 2], ends[n * 9 / 10], ends[n - 1], idle / n, lastlen / n);
        }
    }
    if (d.st) {
        unsigned long long hst[512];
        GATOR_HIP_CHECK(hipMemcpy(hst, d.st, sizeof(hst), hipMemcpyDeviceToHost));
        const int ns = (B * kVT + 63) / 64;
        unsigned long long t0 = ~0ull;
        for (int i = 0; i < ns && i < 120; ++i) if (hst[8 + 4 * i] && hst[8 + 4 * i] < t0) t0 = hst[8 + 4 * i];
        fprintf(stderr, "[k_mdr_layer<1> timeline, every 64th tile: tile:(start_us end_us kcycles xcc cu)]");
        for (int i = 0; i < ns && i < 120; ++i)
            fprintf(stderr, " %d:(%.0f,%.0f,%llu,x%llu,cu%llu.se%llu)", i * 64, (hst[8 + 4 * i] - t0) / 100.0, (hst[9 + 4 * i] - t0) / 100.0,
                    hst[10 + 4 * i] / 1000, hst[11 + 4 * i] >> 32, (hst[11 + 4 * i] >> 8) & 0xf, (hst[11 + 4 * i] >> 13) & 0x7);
        fprintf(stderr, "\n");
        d.st.reset();
        fprintf(stderr, "[k_mdr_layer<1> stamps, tile 0] attention(2 heads)=%llu outproj+res=%llu cross-attn block=%llu mlp=%llu customLN+qkv=%llu\n",
                hst[0], hst[1], hst[2], hst[3], hst[4]);
    }
    return GATOR_OK;
}
#endif

}  // namespace

// pc [B,J,133] (reference layout) -> ws.vc [B,431,3] (vert431) ; taps: ws.lbf.  Layer form, persistent launches and chunks, head, who zeroes the counters: p
int launch_mdr(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pc, int B, void* stream, const float* x_out, const float* pose2d) {
    const int xa = p.xa, persist = p.persist;
    hipStream_t st = (hipStream_t)stream;
    const Weights& w = c->w;
    if (pc) GATOR_TRY(launch_mdr_joint(c, f, ws, p, pc, B, stream));      // else: done by k_gat8's epilogue / k_gat_joint
    const size_t per = (size_t)ws.cap * kVT * 2 * kTile;      // one [B][14][2] tile set
    const size_t perq = (size_t)ws.cap * kVT * 2 * kTileQ[f->opt.mdr_x3];      // q/k/v tile sets, sized for the ctx's own form (TokOp<XA>::kTileQ; X1 tiles are 2 KiB: config 3 uses half of a set)
    float* set[3][4] = {{ws.vf, ws.q, ws.k, ws.v}, {ws.vf + per, ws.q + perq, ws.k + perq, ws.v + perq},
                        {ws.vf + 2 * per, ws.q + 2 * perq, ws.k + 2 * perq, ws.v + 2 * perq}};
    MdrArgs a{};
    a.B = B; a.J = c->J; a.jkv = ws.jkv; a.pc = pc; a.xout = pc ? nullptr : x_out; a.vj = w.vj; a.tok_base = f->tok_base; a.tok_w3 = f->tok_w3;
    a.head_w = f->opt.mdr_x3 ? f->wxbuf + (size_t)(f->head_w - f->lay[0].wq) / kTile * kTileX3 : f->head_w; a.head_b = f->head_b; a.hf = ws.hf; a.lbf = c->block_taps ? ws.lbf : nullptr;      // the "mdr_lbf2" tap costs 110 KB of stores per sample: recorded with the block taps only
    a.hpart = p.head == MdrHead::FINISH ? reinterpret_cast<double*>(ws.hpart) : nullptr;      // the tiles leave the head conv's partial sums; else the whole head runs in k_mdr_head (A/B)
    a.bconv_w = w.bconv_w; a.hbn_w = w.bn_w; a.hbn_b = w.bn_b; a.hbn_mean = w.bn_mean; a.hbn_var = w.bn_var; a.halpha = c->alpha;
    a.lin_s = f->opt.mdr_x3 == 2 ? std::ldexp(kActScale, f->mdr_wshift) : 1.0f;      // 4-product linears: 16 x activations, 2^wshift x weights
    a.lin_inv = 1.0f / a.lin_s;
    const int nwg = (B * kVT + 3) / 4;
#ifdef GATOR_DIAG
    MdrDiag diag;
    GATOR_TRY(mdr_diag_setup(f, persist, st, diag));
    const size_t solo = xa != 0 ? diag.solo : 0;
#else
    constexpr size_t solo = 0;
#endif
    MdrPersistArgs pa{};
    for (int li = 0; li <= 3; ++li) {
#ifdef GATOR_DIAG
        a.stamps = (li == 1) ? diag.st.get() : nullptr;
#endif
        // four launches: two sets in turn.  One persistent launch: stage li writes set li and nothing else ever does, so no CU can
        // hold a stale L1 copy of a tile it reads (a line is only read after its one and only write) -- no cache invalidate in the
        // kernel at all (`buffer_inv sc1` per tile start cost 30 us per forward, and `sc0` does not touch the L1 in this mode)
        float** in = persist ? set[(li + 2) % 3] : set[(li + 1) & 1];
        float** out = persist ? set[li % 3] : set[li & 1];
        a.layer = li;
        a.vf_in = in[0]; a.q_in = in[1]; a.k_in = in[2]; a.v_in = in[3];
        a.vf_out = out[0]; a.q_out = out[1]; a.k_out = out[2]; a.v_out = out[3];
        if (li > 0) a.prev = make_layer(f, c, li - 1);
        if (li < 3) a.cur = make_layer(f, c, li);
        if (persist) { pa.st[li] = a; continue; }
        StageTimer tm(c, li == 0 ? "mdr_layer0" : (li < 3 ? "mdr_layer" : "mdr_attn_head"), stream);
        const MdrLayerKernel layer = kMdrLayer[3 - xa][li == 0 ? 0 : li < 3 ? 1 : 2];
        layer<<<nwg, 256, li < 3 ? solo : 0, st>>>(a, nwg);
    }
    if (persist) {      // the four stages as persistent launches (k_mdr_persist): tickets and per-sample completion counts start from zero (p.ctr_zero's launch)
        StageTimer tm(c, "mdr_layers", stream);
        const size_t tq = kTileQ[xa];
        for (int ch = 0, b0 = 0; ch < p.chunks.nch; ++ch) {
            const int n = p.chunks.base + (ch < p.chunks.rem ? 1 : 0);
            MdrPersistArgs pc_ = pa;
            for (int li = 0; li <= 3; ++li) {
                MdrArgs& s = pc_.st[li];
                const size_t ov = (size_t)b0 * kVT * 2 * kTile, oq = (size_t)b0 * kVT * 2 * tq;
                s.B = n;
                s.vf_in += ov; s.q_in += oq; s.k_in += oq; s.v_in += oq;
                s.vf_out += ov; s.q_out += oq; s.k_out += oq; s.v_out += oq;
                s.jkv += (size_t)b0 * 12 * kTile;
                if (s.pc) s.pc += (size_t)b0 * c->J * 133;
                if (s.xout) s.xout += (size_t)b0 * c->J * 3;
                s.hf += (size_t)b0 * kV * 32;
                if (s.hpart) s.hpart += (size_t)b0 * kVT * 64;
                if (s.lbf) s.lbf += (size_t)b0 * kV * kE;
            }
            pc_.ctr = ws.mdr_ctr + p.chunks.block(ch);
            const MdrPersistKernel layers = kMdrPersist[3 - xa];
            layers<<<p.grid, 256, 0, st>>>(pc_);
            b0 += n;
        }
    }
#ifdef GATOR_DIAG
    GATOR_TRY(mdr_diag_report(diag, B));
#endif
    GATOR_TRY(launch_mdr_head(c, f, ws, p, B, stream, pose2d));
    GATOR_HIP_CHECK(hipGetLastError());
    c->set_tap(TAP_MDR_LBF2, c->block_taps ? ws.lbf : nullptr, c->block_taps ? (int64_t)B * kV * kE : 0);
    c->set_tap(TAP_VERT431, ws.vc, (int64_t)B * kV * 3);
    return GATOR_OK;
}

}  // namespace gator

