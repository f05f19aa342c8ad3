// What one call of the fused path launches, as a value, and the switches (FusedOptions) it follows from.  plan_forward() is a pure function; the
// launchers (fused_state.h) execute their part of its plan.  Plain C++17, no HIP header (tests/host_forward_plan.cpp).  Rules: DESIGN.md 4f.
#pragma once
#include <cstddef>

#ifdef __HIP__
#define GATOR_PLAN_HD __host__ __device__
#else
#define GATOR_PLAN_HD
#endif

namespace gator {

constexpr int kVT = 14;                 // 32-token tiles per sample (431 -> 448)
constexpr int kMdrCtrChunks = 64;       // persistent MDR launches one forward may be cut into (plan_forward: chunks of 256 .. 511 samples)
constexpr int kTiledTokens = 128;       // token slots per workgroup of the sample-tiled encoder (gat_tiled.hip: four 32-token tiles)

// The fused path's environment switches: read once per ctx, at gator_create (fused_api.hip: read_fused_options), which also applies
// the rules that combine them and gator_config.arithmetic.  What only the weights or the device can tell (the config-3 guard, the
// byte-lo round trip, the tile-ratio check of the fp16 x 3 weight sets: fused_state.h h3_demote) narrows them later by clearing a flag.  plan_forward turns them into launches.
struct FusedOptions {
    // encoder
    bool gat_x3 = true;                 // GATOR_GAT_X3 (default 1): GAT linears on split-precision bf16 MFMA; =0: fp32-input MFMA (k_gat only)
    bool gat8 = true;                   // GATOR_GAT8 (default 1): the one-sample-per-workgroup encoder is the two-role kernel k_gat8; =0: k_gat.  Needs gat_x3
    bool gat8_h4 = true;                // GATOR_GAT8_H4 (default 1): k_gat8's token-wise products on four partial products (x3_common.h); =0: the exact six.  Off under exact arithmetic
    bool gat8_lobyte = true;            // GATOR_GAT8_LOBYTE (default 1): k_gat8 streams the byte-lo image of its weights (H3B, gat8_forms.h); =0: the three fp16 planes.
                                        // Needs gat8 and gat8_h4; cleared unless every lo value survives the byte round trip (always, for finite weights)
    bool gat8_tail = true;              // GATOR_GAT8_TAIL (default 1): k_gat8 runs its samples' lifter and MDR joint tokens as its epilogue (round 6); =0: the two
                                        // launches of gat_tail.hip.  Needs gat8, gat8_h4 and mdr_x3 = 2; cleared if one scale cannot hold the joint-feature weights (or a set it needs was demoted);
                                        // outside config 3 it also needs gat8_lobyte (forward_plan.h: plan_forward)
    bool gat_tiled_h4 = true;           // GATOR_GAT_TILED_H4 (default 1): the sample-tiled encoder's token-wise products on four partial products; =0: the exact six.  Off under exact arithmetic
    int gat_tiled = -1;                 // GATOR_GAT_TILED: -1 (default) by batch size (forward_plan.h: plan_tiled_samples), 0 never the sample-tiled encoder, 1 always; what GATOR_ENCODER_AUTO restores
    int gat_tiled_min_batch = 1024;     // GATOR_GAT_TILED_MIN_BATCH (default 1024; values <= 0 ignored): smallest batch the by-batch-size policy gives the sample-tiled encoder
    // MDR layers and vertex regressor
    int mdr_x3 = 2;                     // GATOR_MDR_X3: 0 fp32-input MFMA; 1 exact bf16 x 3 split everywhere; 2 (default) that + the 431x431 attention on two fp16 planes.  1 under exact arithmetic
    int up_x3 = 2;                      // GATOR_UPSAMPLE_X3: 0 the fp32-input MFMA vertex regressor; 1 the exact three bf16 planes; 2 (default) two scaled fp16 planes.  1 under exact arithmetic
    int mdr_persist = -1;               // GATOR_MDR_PERSIST: the four MDR stages as persistent launches (k_mdr_persist): -1 (default) by batch size (forward_plan.h: plan_mdr_persist), 0 never, 1 always.
                                        // A persistent launch that did not complete sets it to 0 (fused_disable_persist)
    int mdr_persist_chunk = 0;          // GATOR_MDR_PERSIST_CHUNK: most samples per persistent launch (0, default: floor(B / 256) launches, ceil(B / 384) in config 3)
    int mdr_persist_grid = 0;           // GATOR_MDR_PERSIST_GRID: workgroups of the persistent launch (0, default: two per CU; tests: a grid that leaves XCDs without one)
    bool mdr_head_partials = true;      // GATOR_MDR_HEAD_PARTIALS (default 1): the tiles' head-conv partial sums + k_mdr_head_finish; =0: the whole head in k_mdr_head (A/B)
    // gator_forward_bf16 (BASELINE config 3): which stages run on ONE 16-bit operand plane
    bool c3_mdr = true;                 // GATOR_C3_MDR (default 1): the MDR layers on one fp16 activation plane; =0: the fp32 configuration's form.  Needs mdr_x3 = 2; cleared by the guard
    bool c3_encoder = true;             // GATOR_C3_ENCODER (default 1): the encoder's token-wise products on one fp16 activation plane as well; =0: the fp32 configuration's.
                                        // Needs gat8 and both encoders' four-product forms; cleared by the guard
    bool c3_up_w1 = true;               // GATOR_C3_UPSAMPLE_W1 (default 1): the vertex regressor's weights on ONE fp16 plane, coarse vertices on two; =0: weights on two
    bool c3_up_bf16 = false;            // GATOR_C3_UPSAMPLE_BF16 (default 0): the vertex regressor on one bf16 plane instead of its two fp16 planes.  Set unless up_x3 = 2
    bool c3_guard = true;               // GATOR_C3_GUARD (default 1): clear c3_mdr and c3_encoder if the weights bound the logits of any of the three attentions above 2^10 (fused_create); =0: never
    // forward
    bool graph = false;                 // GATOR_GRAPH (default 0): =1 starts the ctx with hipGraph replay of repeated forwards on (gator_set_graph_replay)
    int subbatch_streams = 0;           // GATOR_SUBBATCH_STREAMS: 2 runs batches >= 128 as two half-batches on two streams, if gator_config.subbatch_streams is 0 (fused_forward)
    // diagnostic library only (-DGATOR_DIAG; not read otherwise)
    int gat8_dbg = 0;                   // GATOR_GAT8_DBG: k_gat8's debug mode (1: the helper waves reduced to their barriers)
    bool gat_stamps = false;            // GATOR_GAT_STAMPS (set): k_gat / k_gat8 record and print in-kernel cycle stamps
    int mdr_cut = 0;                    // GATOR_MDR_CUT: bit 0 makes every MDR weight load read its tile 0, bit 1 every K / V load (L2 -> CU traffic probe)
    bool mdr_stamps = false;            // GATOR_MDR_STAMPS (set): k_mdr_layer<1> records and prints stamps (four launches only)
    bool mdr_solo = false;              // GATOR_MDR_SOLO (set): the MDR layer launches hold one workgroup per CU (one wave per SIMD)
    bool mdr_ends = false;              // GATOR_MDR_ENDS (set): the last persistent launch prints when its workgroups started and ended
};

constexpr int kCtrError = 8, kCtrDone = 32;      // words of a persistent MDR launch's counter block (mdr_fused.hip: k_mdr_persist; read back by the head kernels, mdr_head.hip)
// chunk plan of a forward of B samples in nch launches: the first B % nch chunks have one sample more.  -> (chunk, first sample, size)
// of sample b, and the word offset of a chunk's counter block
struct MdrChunkPlan {
    int nch, base, rem;
    GATOR_PLAN_HD void locate(int b, int& ch, int& b0, int& n) const {
        const int split = rem * (base + 1);
        if (b < split) { ch = b / (base + 1); n = base + 1; b0 = ch * n; }
        else { ch = rem + (b - split) / base; n = base; b0 = split + (ch - rem) * base; }
    }
    GATOR_PLAN_HD size_t block(int ch) const {
        const int big = ch < rem ? ch : rem;
        return (size_t)ch * kCtrDone + 4 * ((size_t)big * (base + 1) + (size_t)(ch - big) * base);
    }
};
inline bool operator==(const MdrChunkPlan& a, const MdrChunkPlan& b) { return a.nch == b.nch && a.base == b.base && a.rem == b.rem; }

struct Gat8Form { bool h4; int lr; bool h2, lb, tail; };       // k_gat8<H4, LR, H2, LB, TAIL>
struct GatForm { bool x3k, tail; };                            // k_gat<X3K, TAIL>
struct TiledForm { int J; bool h4, h2; };                      // k_gat_tiled<J, H4, H2>
inline bool operator==(const Gat8Form& a, const Gat8Form& b) { return a.h4 == b.h4 && a.lr == b.lr && a.h2 == b.h2 && a.lb == b.lb && a.tail == b.tail; }
inline bool operator==(const GatForm& a, const GatForm& b) { return a.x3k == b.x3k && a.tail == b.tail; }
inline bool operator==(const TiledForm& a, const TiledForm& b) { return a.J == b.J && a.h4 == b.h4 && a.h2 == b.h2; }
enum class PlanEntry { FORWARD, GAT, MDR };                    // gator_forward_* / gator_forward_joints_f32 | gator_gat_forward_f32 | gator_mdr_forward_f32
enum class SampleEncoder { NONE, GAT, GAT8 };                  // the one-sample-per-workgroup kernel of the samples the tiled encoder does not take
enum class CtrZero { NOBODY, MDR_JOINT, GAT_JOINT, GAT8_TAIL };      // which launch zeroes FusedWs::mdr_ctr for this forward
enum class MdrHead { FINISH, WHOLE_HOIST, WHOLE };             // k_mdr_head_finish | k_mdr_head<512, true> | k_mdr_head<512, false>
enum class Regressor { NONE, FP32, X3, X2, BF16 };             // k_upsample | k_upsample_x3 | k_upsample_x2 | k_upsample_bf16
struct RegressorPlan { Regressor form; bool with_joints, w1; };

struct ForwardPlan {
    // encoder: samples [0, n_tiled) on k_gat_tiled, the rest on `sample`; the two batched tail launches (gat_tail.hip) cover [0, n_tail)
    int n_tiled = 0, n_tail = 0;
    SampleEncoder sample = SampleEncoder::NONE;
    TiledForm tiled{0, false, false};
    Gat8Form gat8{false, 0, false, false, false};
    GatForm gat{false, false};
    bool enc16 = false, fused_tail = false;      // config 3's one-plane encoders; k_gat8 runs its samples' lifter and joint tokens as its epilogue
    CtrZero ctr_zero = CtrZero::NOBODY;
    // MDR layers: k_mdr_layer<stage, xa> x 4, or k_mdr_persist<xa> over `chunks` with `grid` workgroups each; xa < 0: no MDR in this call
    int xa = -1, grid = 0; bool persist = false;
    MdrChunkPlan chunks{1, 0, 0};
    MdrHead head = MdrHead::FINISH; RegressorPlan up{Regressor::NONE, false, false};
};
inline bool operator==(const ForwardPlan& a, const ForwardPlan& b) {
    return a.n_tiled == b.n_tiled && a.n_tail == b.n_tail && a.sample == b.sample && a.tiled == b.tiled && a.gat8 == b.gat8 && a.gat == b.gat && a.enc16 == b.enc16 &&
           a.fused_tail == b.fused_tail && a.ctr_zero == b.ctr_zero && a.xa == b.xa && a.grid == b.grid && a.persist == b.persist && a.chunks == b.chunks &&
           a.head == b.head && a.up.form == b.up.form && a.up.with_joints == b.up.with_joints && a.up.w1 == b.up.w1;
}

// Samples the sample-tiled encoder takes: from gat_tiled_min_batch on every FULL round (n_cu workgroups of 7 / 6 samples), and the remainder unless k_gat8 is cheaper for it (<= 4 n_cu).  pin: 0 never, 1 all
inline int plan_tiled_samples(const FusedOptions& o, int J, int n_cu, int B, int pin) {
    if (!o.gat_x3 || pin == 0) return 0;
    if (pin == 1) return B;
    if (B < o.gat_tiled_min_batch) return 0;
    const int round = n_cu * (kTiledTokens / J), n_tiled = (B / round) * round;
    return B - n_tiled > 4 * n_cu ? B : n_tiled;
}

// The vertex regressor the ctx was created with; config 3 (bf16) moves it to one weight plane or to the bf16 kernel
inline RegressorPlan plan_regressor(const FusedOptions& o, bool bf16, bool with_joints) {
    const Regressor form = bf16 && o.c3_up_bf16 ? Regressor::BF16 : o.up_x3 == 0 ? Regressor::FP32 : o.up_x3 == 2 ? Regressor::X2 : Regressor::X3;
    return RegressorPlan{form, with_joints, form == Regressor::X2 && bf16 && o.c3_up_w1};
}

// Persistent launch(es) or four per-stage launches?  By itself from 3 workgroups per CU (B >= 220), and only on the whole 8-XCD part: the persistent kernel's queues are per XCD
inline bool plan_mdr_persist(const FusedOptions& o, int n_cu, int B) {
    if (o.mdr_stamps) return false;              // (set by the diagnostic library's read_fused_options only: its stamps describe the per-stage launches)
    if (o.mdr_persist >= 0) return o.mdr_persist > 0;
    return n_cu == 256 && (B * kVT + 3) / 4 >= 3 * n_cu;
}

// Persistent launches over chunks of 256 .. 511 samples (a sample's tiles stay cache-resident between stages): floor(B / 256), ceil(B / 384) for the one-plane form, at most kMdrCtrChunks
inline MdrChunkPlan plan_mdr_chunks(const FusedOptions& o, int xa, int B) {
    int nch = o.mdr_persist_chunk > 0 ? (B + o.mdr_persist_chunk - 1) / o.mdr_persist_chunk : (xa == 3 ? (B + 383) / 384 : B / 256);
    nch = nch < 1 ? 1 : nch > kMdrCtrChunks ? kMdrCtrChunks : nch;
    return MdrChunkPlan{nch, B / nch, B % nch};
}

// -> nullptr and *out, or why the ctx cannot run this call (GATOR_EUNSUPPORTED): known before anything is queued.  pin: FusedState::gat_tiled
inline const char* plan_forward(const FusedOptions& o, int J, int n_cu, int B, PlanEntry entry, bool bf16, bool with_joints, int pin, ForwardPlan* out) {
    ForwardPlan p;
    if (with_joints && (o.up_x3 == 0 || bf16)) return "gator_forward_joints_f32 needs the split-precision vertex regressor";
    if (entry == PlanEntry::GAT) {               // k_gat runs the lifter itself; nothing else is launched
        p.sample = SampleEncoder::GAT; p.gat = GatForm{o.gat_x3, true};
        *out = p;
        return nullptr;
    }
    if (entry == PlanEntry::FORWARD) {
        p.n_tiled = plan_tiled_samples(o, J, n_cu, B, pin);
        p.enc16 = bf16 && o.c3_encoder;
        if (p.n_tiled > 0 && p.enc16 && !o.gat_tiled_h4) return "the 16-bit encoder needs the four-product weight image (GATOR_GAT_TILED_H4=1, the default)";
        if (p.n_tiled > 0) p.tiled = TiledForm{J == 17 ? 17 : 19, o.gat_tiled_h4, p.enc16};
        if (p.n_tiled < B && !o.gat8) {
            p.sample = SampleEncoder::GAT; p.gat = GatForm{o.gat_x3, false};
        } else if (p.n_tiled < B) {
            p.sample = SampleEncoder::GAT8;
            if (p.enc16 && !o.gat8_h4) return "the 16-bit encoder needs the four-product weight stream (GATOR_GAT8_H4=1, the default)";
            if (J > 20) return "k_gat8: more than 20 joints (gator_create admits 17 and 19)";
            const bool lb = o.gat8_lobyte && !p.enc16;       // the byte-lo stream (the one-plane form reads hi and mid of the H3 stream)
            // (the three-plane stream's kernel has no registers left for the epilogue: outside config 3, GATOR_GAT8_LOBYTE=0 keeps the two launches)
            p.fused_tail = o.gat8_tail && (p.enc16 || o.gat8_lobyte);
            if (p.fused_tail && !(o.gat8_h4 && (p.enc16 || lb))) return "k_gat8: no fused tail on the three-plane weight stream";
            // token rows that exist sit in registers r < LR of a row-over-token tile: token t <-> r = (t & 3) + 4 (t >> 3), so J <= 18 / 20 -> 10 / 12
            p.gat8 = o.gat8_h4 ? Gat8Form{true, J <= 18 ? 10 : 12, p.enc16, lb, p.fused_tail} : Gat8Form{false, 16, false, false, false};
        }
        p.n_tail = p.fused_tail ? p.n_tiled : B;
    }
    // the joint-token launch in front of the MDR layers zeroes the counters (with a fused tail k_gat8: it runs ahead of k_gat_joint), unless the ctx never runs persistent launches
    if (o.mdr_persist != 0) p.ctr_zero = entry == PlanEntry::MDR ? CtrZero::MDR_JOINT : p.fused_tail ? CtrZero::GAT8_TAIL : CtrZero::GAT_JOINT;
    const bool half16 = bf16 && o.c3_mdr;        // config 3: the layers on ONE fp16 activation plane
    if (half16 && o.mdr_x3 != 2) return "16-bit MDR layers need GATOR_MDR_X3=2 (the default)";
    p.xa = half16 ? 3 : o.mdr_x3;
    p.persist = plan_mdr_persist(o, n_cu, B);
    p.grid = !p.persist ? 0 : o.mdr_persist_grid > 0 ? o.mdr_persist_grid : 2 * n_cu;      // two workgroups per CU is what the registers allow; any grid drains the queues
    p.chunks = p.persist ? plan_mdr_chunks(o, p.xa, B) : MdrChunkPlan{1, B, 0};
    p.head = o.mdr_head_partials ? MdrHead::FINISH : B <= 2 * n_cu ? MdrHead::WHOLE_HOIST : MdrHead::WHOLE;
    p.up = plan_regressor(o, bf16, with_joints);
    *out = p;
    return nullptr;
}

}  // namespace gator
