// State of the fused path: packed (MFMA-operand-order) weights and the per-batch workspace.
#pragma once
#include "internal.h"
#include "forward_plan.h"
#include "regressor_slots.h"            // kOB, kCB, kS16, the vertex regressor's operand layouts and their sizes
#include <vector>

namespace gator {

constexpr int kTile = 32 * 32;          // floats in one packed 32x32 tile ([4 g][64 lanes][4])
// words of k_mdr_persist's counters for a forward of B samples: per launch a 32-word header (tickets, error flag) + 4 counts per sample
__host__ __device__ inline size_t mdr_ctr_words(int B) { return (size_t)32 * kMdrCtrChunks + (size_t)4 * B; }

struct MdrLayerP {                      // packed weights of one LBF layer (device pointers into FusedState::wbuf)
    const float *wq, *wk, *wv, *proj, *fc1, *fc2, *sa[4];
};

// A GATBlock's small vectors (LayerNorm weights, biases) as one table of V_TOTAL floats, FusedState::g_vecs + block * V_TOTAL: the
// offsets the encoder kernels read at and fused_create_gat packs at
enum { V_N1W = 0, V_N1B = 128, V_QKVB = 256, V_PROJB = 640, V_GCNB = 768, V_LIN0B = 896, V_BACKB = 1024, V_N2W = 1152,
       V_N2B = 1280, V_FC1B = 1408, V_FC2B = 1920, V_TOTAL = 2048 };

struct GatBlockPk {                     // packed tiles of one GATBlock
    const float *qkv, *proj, *w0, *w1, *lin0, *lin1, *back, *fc1, *fc2;
    const float *mc, *mdT, *aoffT, *f1b; // M (channel on lane), diag(A).M (TOKEN on lane), offdiag(A)^T B-operand tile, hop-2 bias term
};

// Per-sub-batch workspace: one block carved into regions (fused_api.hip: fused_ensure_ws).  FusedState holds two sets; every launcher is
// handed the one it works on: fused_forward gives half-batch i sets[i] when it runs two halves on two streams, everything else sets[0].
struct FusedWs {
    DevBuf<float> base;                 // the block (per cap batch); everything below but vcp16 points into it
    int cap = 0;
    float *vcp = nullptr;               // [MT][3][kCB][4][64][4]  packed vert431 (A operand of the fp32-MFMA upsample GEMM)
    void* vcp3 = nullptr;               // split-precision A operand of the vertex GEMM: bf16 [plane 3][MT][3][28][64][8] (hi/mid/lo, upsample_x3.hip)
                                        // or fp16 [MT/4][28][4][3][plane 2][64][8] (hi/lo, upsample_x2.hip); sized for the larger
    float *vc = nullptr;                // [B][431][3]
    float *vf = nullptr, *q = nullptr, *k = nullptr, *v = nullptr;   // [B][14][2][kTile] each
    float *jkv = nullptr;               // [B][3 layers][2 (k,v)][2 heads][kTile]
    float *hf = nullptr;                // [B][431][32] head features
    float *lbf = nullptr;               // [B][431][64] tap: verts tokens after LBF3 (reference layout)
    float *feat = nullptr;              // [B][J][128] encoder output
    float* hpart = nullptr;             // [cap][14][64] DOUBLES: the head conv's per-tile partial sums (mdr_fused.hip: head_conv_partial)
    float *lpart = nullptr;             // [MT][J][2][kTile] lifter partial tiles (gat_tail.hip)
    unsigned* mdr_ctr = nullptr;        // k_mdr_persist: the counter blocks of a forward's launches, mdr_ctr_words(cap) words (forward_plan.h: MdrChunkPlan; ForwardPlan::ctr_zero names the launch that zeroes them)
    DevBuf<void> vcp16;                 // bf16 packed vert431 for the bf16 vertex GEMM (cap-sized)
    int vcp16_cap = 0;
};

struct FusedState {
    ~FusedState();                      // fused_api.hip: graphs, streams and events; the buffers free themselves
    FusedOptions opt;                   // the switches this ctx was created with, narrowed by the weights and the device
    DevBuf<float> wbuf;                 // all packed weights
    DevBuf<float> gbuf;                 // packed GAT weights + tables
    GatBlockPk gblk[kDepth];
    const float *g_biasT = nullptr, *g_m1T = nullptr, *g_m2T = nullptr, *g_gl3 = nullptr, *g_posT = nullptr, *g_vecs = nullptr;
    // upsample: Wp[tap][ob][cb][4][64][4]
    const float* up_w = nullptr;
    DevBuf<void> up_w3;                 // bf16 [plane 3][tap][ob][28][64][8]  hi/mid/lo split of upsample_conv.weight
    int gat_tiled = -1;                 // encoder policy in force (opt.gat_tiled until gator_set_encoder changes it)
    int n_cu = 256;                     // compute units of the ctx's device
    DevBuf<float> gxbuf;                // X3 tiles of the GAT block weights, tile-for-tile image of gbuf from gblk[0].qkv on
    DevBuf<float> gxbuf_h3;             // the same grids as three fp16 planes of 2^gat_tiled_wshift * w (k_gat_tiled's four-product form)
    int gat_tiled_wshift = 0;
    DevBuf<float> g8stream;             // the same tiles as four per-wave streams in consumption order (gat8_forms.h, gat8_stream.hip)
    DevBuf<float> g8stream_b;           // ... and its byte-lo image (H3B tiles, 5 KiB: gat8_forms.h), what k_gat8<true, LR, false, true> streams
    int gat8_wshift = 0;                // its weight stream holds three fp16 planes of 2^gat8_wshift * w
    DevBuf<float> wxbuf;                // X3 tiles of the MDR layer + head weights, tile-for-tile image of wbuf from lay[0].wq on
    DevBuf<float> jf128_h3;             // get_joint_feature columns 5..132 as H3 tiles [2][4] of 2^jf128_wshift * w (k_gat8's fused tail)
    int jf128_wshift = 0;
    int mdr_wshift = 0;                 // mdr_x3 = 2: wxbuf holds three fp16 planes of 2^mdr_wshift * w
    // What the weights decided about the three-plane weight sets (x3_common.h: kH3MinTileRatio; gator_operand_state): the smallest
    // tile ratio of each set that was looked at (0: not looked at), and which default forms this ctx gave up for the exact ones
    float h3_tile_ratio[4] = {0.f, 0.f, 0.f, 0.f};      // [GATOR_H3SET_*]
    int h3_demoted = 0;                 // bit GATOR_H3SET_*: that set's four-product form was demoted (gat8_h4 / gat_tiled_h4 off, mdr_x3 2 -> 1, fused tail off)
    float c3_logit_bound = 0.f;         // bound on the logits of the mode's one-plane attentions (MDR self- and cross-attention, encoder) in the exp2 domain, from the weights (fused_create)
    DevBuf<void> up_w2;                 // fp16 [ob/2][28][2][tap 3][plane 2][64][8]  scaled hi/lo split of upsample_conv.weight
    float up_w2_unscale = 1.f;          // 2^-(weight shift + activation shift), applied to the finished sums
    DevBuf<void> up_w16;                // bf16 [tap][ob][28][64][8] (packed on the first bf16 call, which waits for the pack)
    // joint regressor fused into the vertex GEMM's epilogue (gator_set_joint_regressor / gator_forward_joints_f32)
    DevBuf<void> jr_blk, jr_ent;                  // int2 [kOB] (first, count) ; int2 [nnz] (vertex, slot)
    DevBuf<float> jr_w;                           // [nnz] weights in entry order
    DevBuf<int> jr_rowptr;                        // [nj + 1] CSR row pointers over the slots (sorted by joint, then vertex)
    DevBuf<float> jr_P;                           // [cap][nnz][3] partial products
    int jr_nnz = 0, jr_nj = 0, jr_cap = 0;
    DevBuf<float> blk_tap;              // debug: residual stream after every GATBlock [depth][B][J][128] (gator_enable_block_taps)
    int blk_tap_cap = 0;
    // MDR
    MdrLayerP lay[3];
    const float* head_w = nullptr;      // [1 nb][2 kb] combined motion/bias/scale linear
    const float* head_b = nullptr;      // [32]
    const float* tok_base = nullptr;    // [14][2][4][64][4]  v431 part of get_verts_feature + bias + pos_v  (T-layout tiles)
    const float* tok_w3 = nullptr;      // [3][64]            pose3d part of get_verts_feature (columns 3..5), row-major [i][ch]
    // hipGraph replay of the full forward (gator_set_graph_replay / GATOR_GRAPH=1).  A forward is identified by (batch, the three
    // caller pointers, its ForwardPlan -- everything that decides the launch sequence --, workspace): the first time a key is seen the forward runs
    // directly (lazy allocations happen there), the second time it is captured on a private stream, from then on one hipGraphLaunch
    // on the caller's stream replaces the six launches.  Keys are kept LRU (kGraphSlots); anything unexpected switches the feature off.
    struct GraphSlot {
        int B = 0; const void *in = nullptr, *verts = nullptr, *pose3d = nullptr;
        ForwardPlan plan; const void* ws = nullptr;
        void *graph = nullptr, *exec = nullptr;
        unsigned long long used = 0;
    };
    static constexpr int kGraphSlots = 8;
    bool graph_replay = false;
    void* cap_stream = nullptr;
    std::vector<GraphSlot> graphs;
    unsigned long long graph_clock = 0, graph_launches = 0;
    // sub-batch pipelining (two half-batches on two streams: one half's kernel tails are filled by the other's work)
    FusedWs sets[2];                    // set 0 is the normal workspace, set 1 the second half-batch's
    void* aux_stream = nullptr;
    void *ev_fork = nullptr, *ev_join = nullptr;
    const float* jfeat_p = nullptr;     // get_joint_feature.weight packed [2 nb][5 kb]
    const float* jfeat5 = nullptr;      // its columns 0..4 (pose2d, pose3d/1000) as [5][64]
    const float* jfeat128_p = nullptr;  // its columns 5..132 (feat) packed [2 nb][4 kb]
    const float* posj_T = nullptr;      // [2] T-layout tiles of pos_j_id_embed[1..J]
};

// A three-plane weight set whose tiles differ too much in magnitude for one scale (x3_common.h: h3_set_holds) is not packed: the ctx gives up the
// form that reads it for the one the environment switch of that set selects -- slower, never less accurate -- and with it the options that need it
// (the rules of read_fused_options, applied again).  Recorded for gator_operand_state.
inline void h3_demote(FusedState* f, int set) {
    FusedOptions& o = f->opt;
    f->h3_demoted |= 1 << set;
    if (set == GATOR_H3SET_GAT8) o.gat8_h4 = false;
    if (set == GATOR_H3SET_GAT_TILED) o.gat_tiled_h4 = false;
    if (set == GATOR_H3SET_MDR) o.mdr_x3 = 1;
    if (set == GATOR_H3SET_JFEAT) o.gat8_tail = false;
    o.gat8_lobyte = o.gat8_lobyte && o.gat8_h4;
    o.gat8_tail = o.gat8_tail && o.gat8_h4 && o.mdr_x3 == 2;
    o.c3_mdr = o.c3_mdr && o.mdr_x3 == 2;
    o.c3_encoder = o.c3_encoder && o.gat8_h4 && o.gat_tiled_h4;
}

// fused_pack.hip
int fused_pack_linear(const float* W, int64_t wsn, int64_t wsk, int N, int K, float* dst, void* stream);   // -> [NB][KB] tiles
inline int nblk32(int n) { return (n + 31) / 32; }
// The launchers execute their part of a ForwardPlan (forward_plan.h) on the workspace set they are handed; none reads a switch to choose a kernel.
// gat_fused.hip
int gat_prepare_device();
int gat_ensure_blk_tap(gator_ctx* c, FusedState* f, int B);
int launch_gat(gator_ctx* c, FusedState* f, const GatForm& form, const float* pose2d, int B, float* x_out, float* feat, void* stream, int B_total, int tap_row0);      // B samples: rows tap_row0 .. of a batch of B_total
// gat8_stream.hip
int gat8_build_stream(FusedState* f, void* stream);
// gat_roles.hip
int gat8_prepare_device();
int launch_gat8(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pose2d, int B, float* pose3d, void* stream);      // k_gat8<p.gat8> on samples p.n_tiled .. B of the whole batch's pose2d / pose3d
// gat_tiled.hip
int gat_tiled_prepare_device();
int launch_gat_tiled(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pose2d, int B, void* stream);      // k_gat_tiled<p.tiled> on samples 0 .. p.n_tiled
// gat_tail.hip
size_t gat_tail_part_floats(int B, int J);
int launch_gat_tail(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pose2d, float* x_out, void* stream);  // lifter + MDR joint tokens of samples 0 .. p.n_tail
// The vertex regressor (upsample_common.h states the row; the entries are in upsample_fused.hip): every form through one pack and one launch entry
int pack_upsample_any(Regressor form, const float* up_w, void* dst, float* unscale, void* stream);      // the packed weights of X3 | X2 | BF16 (FP32: fused_pack_linear)
int upsample_x2_prepare_device();
int launch_pack_vc_any(const RegressorPlan& r, const float* vc, int B, const FusedWs& ws, void* stream);      // vc -> ws.vcp | ws.vcp3 | ws.vcp16
int launch_upsample_any(const FusedState* f, const gator_ctx* c, const FusedWs& ws, const RegressorPlan& r, int B, float* verts, void* stream);
int launch_jreg_reduce(const FusedState* f, int B, float* joints, void* stream);
// mdr_fused.hip: the joint tokens (pc, the MDR entry point; else x_out and pose2d of the whole forward), the layers and the head, as p says; the first
// and the last through mdr_head.hip's launchers below
int launch_mdr(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pc, int B, void* stream, const float* x_out, const float* pose2d);
// mdr_head.hip: what launch_mdr runs in front of the layers (the MDR entry point's joint tokens) and behind them (the head kernel p.head)
int launch_mdr_joint(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, const float* pc, int B, void* stream);
int launch_mdr_head(gator_ctx* c, FusedState* f, FusedWs& ws, const ForwardPlan& p, int B, void* stream, const float* pose2d);

}  // namespace gator
