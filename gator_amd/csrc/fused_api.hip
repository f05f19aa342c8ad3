// Fused path: create-time packing, workspace, and stage dispatch.  No fallback to anything but HIP kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "fused_state.h"
#include "x3_common.h"

namespace gator {
namespace {

static void graph_slot_free(FusedState::GraphSlot& g) {
    if (g.exec) (void)hipGraphExecDestroy((hipGraphExec_t)g.exec);
    if (g.graph) (void)hipGraphDestroy((hipGraph_t)g.graph);
    g.exec = g.graph = nullptr;
}
static void graphs_clear(FusedState* f) {
    for (auto& g : f->graphs) graph_slot_free(g);
    f->graphs.clear();
}
// (Re-)allocates workspace set w for a batch of B: one block, zeroed once, carved into its regions.
int fused_ensure_ws(gator_ctx* c, FusedWs& w, int B) {
    FusedState* f = c->fused;
    if (w.base && B <= w.cap) return GATOR_OK;
    if (w.base) {
        GATOR_HIP_CHECK(hipDeviceSynchronize());
        graphs_clear(f);                                 // captured forwards hold pointers into the old workspace
    }
    const int cap = B, MT = (cap + 31) / 32, J = c->J;
    const size_t tiles = (size_t)cap * kVT * 2 * kTile;
    // The layout, every region once and in block order: without a block it only adds the sizes up, with one it also points the members into it.
    size_t n = 0;
    auto layout = [&](float* block) {
        n = 0;
        auto region = [&](auto*& member, size_t floats) {      // (64-float aligned offsets: 8-byte alignment of hpart's doubles holds)
            if (block) member = reinterpret_cast<std::remove_reference_t<decltype(member)>>(block + n);
            n += (floats + 63) & ~(size_t)63;
        };
        region(w.vcp, (size_t)MT * 3 * kCB * kTile); region(w.vc, (size_t)cap * kV * 3);
        // THREE tile sets each (k_mdr_persist writes every set once per forward); q/k/v sized for X3 tiles (1.5x)
        region(w.vf, 3 * tiles); region(w.q, 9 * tiles / 2); region(w.k, 9 * tiles / 2); region(w.v, 9 * tiles / 2);
        region(w.jkv, (size_t)cap * 12 * kTile); region(w.hf, (size_t)cap * kV * 32); region(w.lbf, (size_t)cap * kV * kE);
        region(w.feat, (size_t)cap * J * kC); region(w.vcp3, std::max(upsample_x3_vcp_elems(cap), upsample_x2_vcp_elems(cap)) / 2);
        region(w.lpart, gat_tail_part_floats(cap, J)); region(w.mdr_ctr, mdr_ctr_words(cap)); region(w.hpart, (size_t)cap * kVT * 128);
    };
    layout(nullptr);
    GATOR_TRY(w.base.alloc(n * sizeof(float)));
    GATOR_HIP_CHECK(hipMemset(w.base, 0, n * sizeof(float)));
    GATOR_HIP_CHECK(hipDeviceSynchronize());      // the memset runs on the null stream; a non-blocking stream would not wait for it
    w.cap = cap;
    layout(w.base);
    return GATOR_OK;
}

std::vector<float> d2h(const float* p, size_t n) {
    std::vector<float> v(n);
    (void)hipMemcpy(v.data(), p, n * sizeof(float), hipMemcpyDeviceToHost);
    return v;
}

// B-operand / T-layout tile of a [32][32] table: tile[g][lane][j] = tab(row = lane&31, col = 8g + 4(lane>>5) + j)
template <class F>
void fill_tile(float* dst, F tab) {
    for (int g = 0; g < 4; ++g)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j) dst[(g * 64 + lane) * 4 + j] = tab(lane & 31, 8 * g + 4 * (lane >> 5) + j);
}

// Every environment switch of the fused path (forward_plan.h: FusedOptions), read once per ctx, with the rules that depend only on
// the switches and on gator_config.arithmetic.  Exact arithmetic (GATOR_ARITH_EXACT_SPLIT: no two-plane operand anywhere) wins over
// the environment.
int read_fused_options(const gator_ctx* c, FusedOptions* o) {
    auto flag = [](const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; };      // =0 means off
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    const bool exact = c->arithmetic == GATOR_ARITH_EXACT_SPLIT;
    o->gat_x3 = flag("GATOR_GAT_X3", true);
    o->gat8 = o->gat_x3 && flag("GATOR_GAT8", true);
    o->gat8_h4 = !exact && flag("GATOR_GAT8_H4", true);
    o->gat8_lobyte = o->gat8 && o->gat8_h4 && flag("GATOR_GAT8_LOBYTE", true);
    o->gat_tiled_h4 = !exact && flag("GATOR_GAT_TILED_H4", true);
    o->gat_tiled = num("GATOR_GAT_TILED", -1);
    if (const int m = num("GATOR_GAT_TILED_MIN_BATCH", 0); m > 0) o->gat_tiled_min_batch = m;
    o->mdr_x3 = exact ? 1 : num("GATOR_MDR_X3", 2);
    o->up_x3 = exact ? 1 : num("GATOR_UPSAMPLE_X3", 2);
    if (c->parts & GATOR_PART_MDR) {      // (a ctx without the MDR weights has no use for them)
        if (o->up_x3 < 0 || o->up_x3 > 2) return fail(GATOR_EINVAL, "GATOR_UPSAMPLE_X3 must be 0, 1 or 2");
        if (o->mdr_x3 < 0 || o->mdr_x3 > 2) return fail(GATOR_EINVAL, "GATOR_MDR_X3 must be 0, 1 or 2");
    }
    o->gat8_tail = o->gat8 && o->gat8_h4 && o->mdr_x3 == 2 && flag("GATOR_GAT8_TAIL", true);
    o->mdr_persist = set("GATOR_MDR_PERSIST") ? flag("GATOR_MDR_PERSIST", false) : -1;
    o->mdr_persist_chunk = num("GATOR_MDR_PERSIST_CHUNK", 0);
    o->mdr_persist_grid = num("GATOR_MDR_PERSIST_GRID", 0);
    o->mdr_head_partials = flag("GATOR_MDR_HEAD_PARTIALS", true);
    // Config 3's default: the MDR layers on one fp16 activation plane (mdr_fused.hip XA = 3), the vertex regressor on its two fp16
    // planes (a single bf16 / fp16 plane there costs 4 / 0.5 mm: profiles/r05_emulate_16bit.txt).  GATOR_C3_MDR=0 /
    // GATOR_C3_UPSAMPLE_BF16=1 restore round 4's form (bf16 regressor only).
    o->c3_mdr = o->mdr_x3 == 2 && flag("GATOR_C3_MDR", true);
    o->c3_encoder = o->gat8 && o->gat8_h4 && o->gat_tiled_h4 && flag("GATOR_C3_ENCODER", true);
    o->c3_up_w1 = flag("GATOR_C3_UPSAMPLE_W1", true);
    o->c3_up_bf16 = o->up_x3 != 2 || flag("GATOR_C3_UPSAMPLE_BF16", false);
    o->c3_guard = flag("GATOR_C3_GUARD", true);
    o->graph = flag("GATOR_GRAPH", false);
    o->subbatch_streams = num("GATOR_SUBBATCH_STREAMS", 0);
#ifdef GATOR_DIAG
    o->gat8_dbg = num("GATOR_GAT8_DBG", 0);
    o->gat_stamps = set("GATOR_GAT_STAMPS");
    o->mdr_cut = num("GATOR_MDR_CUT", 0);
    o->mdr_stamps = set("GATOR_MDR_STAMPS");
    o->mdr_solo = set("GATOR_MDR_SOLO");
    o->mdr_ends = set("GATOR_MDR_ENDS");
#endif
    return GATOR_OK;
}

// Largest eigenvalue of a symmetric n x n matrix (row-major; destroyed): cyclic Jacobi rotations until the off-diagonal part is gone to
// double rounding.  Unlike a power iteration it needs no start vector, so no weight can hide its top direction from it.
static double sym_eig_max(std::vector<double>& A, int n) {
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0, all = 0;
        for (int p = 0; p < n; ++p)
            for (int q = 0; q < n; ++q) { all += A[p * n + q] * A[p * n + q]; if (q > p) off += A[p * n + q] * A[p * n + q]; }
        if (!(off > 1e-30 * all)) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0) continue;
                const double th = (A[q * n + q] - A[p * n + p]) / (2 * apq);
                const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1));
                const double cs = 1 / std::sqrt(t * t + 1), sn = t * cs;
                for (int k = 0; k < n; ++k) {       // A <- A J, then A <- J^T A: zeroes A[p][q]
                    const double kp = A[k * n + p], kq = A[k * n + q];
                    A[k * n + p] = cs * kp - sn * kq; A[k * n + q] = sn * kp + cs * kq;
                }
                for (int k = 0; k < n; ++k) {
                    const double pk = A[p * n + k], qk = A[q * n + k];
                    A[p * n + k] = cs * pk - sn * qk; A[q * n + k] = sn * pk + cs * qk;
                }
            }
    }
    double m = 0;
    for (int i = 0; i < n; ++i) m = std::max(m, A[i * n + i]);
    return m;
}

// sigma_max of rows [r0, r0 + n) of a row-major [.][K] matrix: the root of the largest eigenvalue of the n x n Gram matrix, in double (exact,
// no start vector).  n <= 32
static double sigma_max_rows(const std::vector<float>& W, int r0, int n, int K) {
    std::vector<double> G((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double acc = 0;
            for (int k = 0; k < K; ++k) acc += (double)W[(size_t)(r0 + i) * K + k] * (double)W[(size_t)(r0 + j) * K + k];
            G[i * n + j] = acc;
        }
    return std::sqrt(std::max(sym_eig_max(G, n), 0.0));
}
static double norm_rows(const std::vector<float>& v, int r0, int n) {
    double s = 0;
    for (int i = 0; i < n; ++i) s += (double)v[r0 + i] * v[r0 + i];
    return std::sqrt(s);
}
static double max_abs(const std::vector<float>& v) {
    double m = 0;
    for (float x : v) m = std::max(m, (double)std::fabs(x));
    return m;
}

// Guard of config 3's 16-bit mode (round 6): its 431 x 431 attention carries q and k on ONE fp16 plane each, which moves a
// score by up to 2^-11 |q| |k|.  |q| |k| is bounded from the weights alone: the custom LayerNorm in front of the in-projections gives
// every token unit unbiased standard deviation, |x| <= max|a_2| sqrt(63) + |b_2| (vanilla_transformer_encoder.py:31-34), and per head
// |q_h| <= sigma_max(Wq_h) |x| + |bq_h|, |k_h| likewise, so |q_h . k_h| / sqrt(d_k) <= (sigma_max(Wq_h) |x| + |bq_h|) (sigma_max(Wk_h) |x| +
// |bk_h|) / sqrt(d_k).  sigma_max is exact: the largest eigenvalue of the 32 x 32 Gram matrix W_h W_h^T, in double.
// The other two attentions of the mode carry one-plane operands as well and get the same construction (tests/test_gpu_softmax_edges.py:
// sharp cross-attention cost 2.2 mm in the mode, sharp encoder attention 1.3 mm, with the self-attention's bound at 75):
//   cross-attention (JointX1): q and k come from nn.LayerNorm(64) without biases (MDR.py:27-28), |x| <= max|norm1.weight| sqrt(64) + |norm1.bias|,
//     bound sigma_max(Wq_h) sigma_max(Wk_h) |x|^2 / sqrt(32);
//   encoder (its token-wise products on one activation plane): nn.LayerNorm(128) in front of qkv, |x| <= max|norm1.weight| sqrt(128) + |norm1.bias|,
//     heads of 16 rows, bound (sigma_max(Wq_h) |x| + |bq_h|) (sigma_max(Wk_h) |x| + |bk_h|) / sqrt(16) + max|hop / path bias|.
// Returns the largest bound over the three sites, layers / blocks and heads, in the exp2 domain; gator_c3_state() reports it.  hop_bias: the
// ctx's folded [8][J][J] tile, or nullptr for a ctx without the encoder.
float c3_logit_bound(const Weights& w, const float* hop_bias, int J) {
    double worst = 0;
    for (int li = 0; li < 3; ++li) {
        const MdrLayerW& r = w.lay[li];
        const std::vector<float> wq = d2h(r.sa_w[0], 64 * 64), wk = d2h(r.sa_w[1], 64 * 64), bq = d2h(r.sa_b[0], 64), bk = d2h(r.sa_b[1], 64),
                                 a2 = d2h(r.a2, 64), b2 = d2h(r.b2, 64);
        const double xn = max_abs(a2) * std::sqrt(63.0) + norm_rows(b2, 0, 64);
        // |W_h x + b_h| <= sigma_max(W_h) |x| + |b_h| for head hd's 32 rows of an in-projection
        for (int hd = 0; hd < 2; ++hd)
            worst = std::max(worst, (sigma_max_rows(wq, 32 * hd, 32, 64) * xn + norm_rows(bq, 32 * hd, 32)) *
                                        (sigma_max_rows(wk, 32 * hd, 32, 64) * xn + norm_rows(bk, 32 * hd, 32)) / std::sqrt(32.0));
        const std::vector<float> cq = d2h(r.wq, 64 * 64), ck = d2h(r.wk, 64 * 64), n1w = d2h(r.n1w, 64), n1b = d2h(r.n1b, 64);
        const double cn = max_abs(n1w) * std::sqrt(64.0) + norm_rows(n1b, 0, 64);
        for (int hd = 0; hd < 2; ++hd)
            worst = std::max(worst, sigma_max_rows(cq, 32 * hd, 32, 64) * cn * sigma_max_rows(ck, 32 * hd, 32, 64) * cn / std::sqrt(32.0));
    }
    if (hop_bias != nullptr) {
        const double hop = max_abs(d2h(hop_bias, (size_t)kH * J * J));
        for (int i = 0; i < kDepth; ++i) {
            const GatBlockW& r = w.blk[i];
            const std::vector<float> qkv = d2h(r.qkv_w, 384 * 128), qb = d2h(r.qkv_b, 384), n1w = d2h(r.n1w, 128), n1b = d2h(r.n1b, 128);
            const double xn = max_abs(n1w) * std::sqrt(128.0) + norm_rows(n1b, 0, 128);
            for (int hd = 0; hd < kH; ++hd)
                worst = std::max(worst, (sigma_max_rows(qkv, 16 * hd, 16, 128) * xn + norm_rows(qb, 16 * hd, 16)) *
                                            (sigma_max_rows(qkv, 128 + 16 * hd, 16, 128) * xn + norm_rows(qb, 128 + 16 * hd, 16)) / std::sqrt(16.0) + hop);
        }
    }
    return (float)(worst * 1.4426950408889634);
}

// Packs each linear into the tiles at p, one after the other, and stores where it went.
struct PackItem { const float* src; int64_t wsn, wsk; int N, K; const float** dst; };
template <size_t n>
int pack_linears(const PackItem (&items)[n], float*& p, void* stream) {
    for (const PackItem& it : items) {
        GATOR_TRY(fused_pack_linear(it.src, it.wsn, it.wsk, it.N, it.K, p, stream));
        *it.dst = p;
        p += (size_t)nblk32(it.N) * nblk32(it.K) * kTile;
    }
    return GATOR_OK;
}

int fused_create_gat(gator_ctx* c, FusedState* f, void* stream) {
    const Weights& w = c->w;
    const int J = c->J;
    const size_t blk_tiles = 48 + 16 + 16 + 16 + 16 + 4 + 20 + 64 + 64 + 4 + 4 + 1 + 1;     // 274
    const size_t total = (kDepth * blk_tiles + 8 + 2 + 8 + 4 + 12) * kTile;
    GATOR_TRY(f->gbuf.alloc(total * sizeof(float)));
    float* p = f->gbuf;
    auto take = [&](size_t tiles) { float* r = p; p += tiles * kTile; return r; };
    std::vector<float> host;
    auto upload = [&](const std::vector<float>& v) -> const float* {
        float* d = take(v.size() / kTile);
        (void)hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice);
        return d;
    };
    const std::vector<float> adiag = d2h(c->adj_diag, (size_t)kDepth * J), aoff = d2h(c->adj_off, (size_t)kDepth * J * J),
                             m1 = d2h(c->mask1, (size_t)J * J), m2 = d2h(c->mask2, (size_t)J * J), hb = d2h(c->hop_bias, (size_t)kH * J * J);
    for (int i = 0; i < kDepth; ++i) {
        const GatBlockW& r = w.blk[i];
        GatBlockPk& q = f->gblk[i];
        const PackItem items[] = {
            {r.qkv_w, 128, 1, 384, 128, &q.qkv}, {r.proj_w, 128, 1, 128, 128, &q.proj},
            {r.gcn_W, 1, 128, 128, 128, &q.w0}, {r.gcn_W + 128 * 128, 1, 128, 128, 128, &q.w1},     // applied as x @ W (modules.py:244-245)
            {r.xl0_w, 128, 1, 128, 128, &q.lin0}, {r.xl1_w, 128, 1, 16, 128, &q.lin1}, {r.xlb_w, 144, 1, 128, 144, &q.back},
            {r.fc1_w, 128, 1, 512, 128, &q.fc1}, {r.fc2_w, 512, 1, 128, 512, &q.fc2}};
        GATOR_TRY(pack_linears(items, p, stream));
        const std::vector<float> M = d2h(r.gcn_M, (size_t)J * kC), b1 = d2h(r.xl1_b, 16);
        // C-layout tiles (channel on the lane, token in the register): tile[nb][g][lane][j] <-> token 8g+4h+j, channel 32nb+(lane&31)
        std::vector<float> mc(4 * kTile), md(4 * kTile);
        for (int nb = 0; nb < 4; ++nb) {
            for (int g = 0; g < 4; ++g)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int tok = 8 * g + 4 * (lane >> 5) + j, n = 32 * nb + (lane & 31);
                        mc[((nb * 4 + g) * 64 + lane) * 4 + j] = tok < J ? M[(size_t)tok * kC + n] : 0.f;
                    }
            // T-layout (token on the lane, channel in the register): diag(A)[t] * M[t][n], for the token-wise h0 term
            fill_tile(md.data() + (size_t)nb * kTile, [&](int t, int ch) { return t < J ? adiag[i * J + t] * M[(size_t)t * kC + 32 * nb + ch] : 0.f; });
        }
        q.mc = upload(mc);
        q.mdT = upload(md);
        std::vector<float> t1(kTile), t2(kTile);
        fill_tile(t1.data(), [&](int t, int j) { return (t < J && j < J) ? aoff[((size_t)i * J + t) * J + j] : 0.f; });
        q.aoffT = upload(t1);
        fill_tile(t2.data(), [&](int t, int ch) {      // m2 @ (u1 + b1) = m2 @ u1 + rowsum(m2)[t] * b1[ch]
            if (t >= J || ch >= 16) return 0.f;
            float deg = 0.f;
            for (int j = 0; j < J; ++j) deg += m2[(size_t)t * J + j];
            return deg * b1[ch];
        });
        q.f1b = upload(t2);
    }
    if (f->opt.gat_x3) {   // split-precision image of every block's weight grids (the tables mc/md/aoffT/f1b in between are converted too, unused)
        const int64_t ntiles = (p - f->gblk[0].qkv) / kTile;
        GATOR_TRY(f->gxbuf.alloc((size_t)ntiles * kTileX3 * sizeof(float)));
        int rc = fused_repack_x3(f->gblk[0].qkv, f->gxbuf, ntiles, stream);
        if (rc) return rc;
        if (f->opt.gat_tiled_h4) {
            float& ratio = f->h3_tile_ratio[GATOR_H3SET_GAT_TILED];
            GATOR_TRY(f->gxbuf_h3.alloc((size_t)ntiles * kTileX3 * sizeof(float)));
            // the scale comes from the nine weight grids of each block (264 tiles), not from the mc / mdT / aoffT / f1b tables behind them
            rc = fused_repack_h3(f->gblk[0].qkv, f->gxbuf_h3, ntiles, &f->gat_tiled_wshift, &ratio, stream, (int64_t)blk_tiles, 264);
            if (rc) return rc;
            if (!h3_set_holds(ratio)) { f->gxbuf_h3.reset(); h3_demote(f, GATOR_H3SET_GAT_TILED); }      // the exact six products on gxbuf, as under GATOR_GAT_TILED_H4=0
        }
        if (f->opt.gat8) {
            rc = gat8_build_stream(f, stream);
            if (rc) return rc;
        }
    }
    std::vector<float> bt(8 * kTile), mt(kTile);
    for (int hd = 0; hd < kH; ++hd)
        fill_tile(bt.data() + (size_t)hd * kTile, [&](int t, int j) { return (t < J && j < J) ? hb[((size_t)hd * J + t) * J + j] : 0.f; });
    f->g_biasT = upload(bt);
    fill_tile(mt.data(), [&](int t, int j) { return (t < J && j < J) ? m1[(size_t)t * J + j] : 0.f; });
    f->g_m1T = upload(mt);
    fill_tile(mt.data(), [&](int t, int j) { return (t < J && j < J) ? m2[(size_t)t * J + j] : 0.f; });
    f->g_m2T = upload(mt);
    {   // per-block small vectors, each at its offset of the block's table (fused_state.h: V_*)
        std::vector<float> vv((size_t)kDepth * V_TOTAL);
        for (int i = 0; i < kDepth; ++i) {
            const GatBlockW& r = w.blk[i];
            const struct { const float* p; int at, n; } parts[] = {
                {r.n1w, V_N1W, 128}, {r.n1b, V_N1B, 128}, {r.qkv_b, V_QKVB, 384}, {r.proj_b, V_PROJB, 128}, {r.gcn_bias, V_GCNB, 128}, {r.xl0_b, V_LIN0B, 128},
                {r.xlb_b, V_BACKB, 128}, {r.n2w, V_N2W, 128}, {r.n2b, V_N2B, 128}, {r.fc1_b, V_FC1B, 512}, {r.fc2_b, V_FC2B, 128}};
            for (auto& pt : parts) {
                const std::vector<float> h = d2h(pt.p, pt.n);
                std::copy(h.begin(), h.end(), vv.begin() + (size_t)i * V_TOTAL + pt.at);
            }
            // K's bias adds q_i . b_k to every logit of query row i: constant over the keys, so the softmax - the only reader of K - does not
            // see it and no loss keeps it small; as the start value of the K projection's accumulator a large one rounds every partial product
            // at ITS magnitude (at |b_k| ~ 170: 2.5 x the fp32 reference's error in k_gat / k_gat_tiled, tests/test_gpu_softmax_edges.py).  Each
            // channel loses the multiple of 8 nearest to it: 0 for |b_k| < 4, so an ordinary checkpoint is packed as it is; exact in fp32.
            for (int ch = 0; ch < 128; ++ch) {
                float& bk = vv[(size_t)i * V_TOTAL + V_QKVB + 128 + ch];
                const float shift = 8.0f * std::nearbyint(bk / 8.0f);
                if (std::isfinite(shift)) bk -= shift;
            }
        }
        f->g_vecs = upload(vv);
    }
    {   // embed: GLinear.3 packed, pos_id_embed[1..J] + pos_num_embed[deg] as T-layout tiles (GAT.py:141-144)
        float* dst = take(8);
        int rc = fused_pack_linear(w.gl3_W, 64, 1, 128, 64, dst, stream);
        if (rc) return rc;
        f->g_gl3 = dst;
        const std::vector<float> pe = d2h(c->pos_embed, (size_t)J * kC);
        std::vector<float> pt(4 * kTile);
        for (int kb = 0; kb < 4; ++kb)
            fill_tile(pt.data() + (size_t)kb * kTile, [&](int t, int ch) { return t < J ? pe[(size_t)t * kC + 32 * kb + ch] : 0.f; });
        f->g_posT = upload(pt);
    }
    // (the lifter reads the reference weight [3J][128J] as it is, gat_fused.hip)
    {
        int rc = gat_prepare_device();
        if (rc == GATOR_OK) rc = gat_tiled_prepare_device();
        if (rc == GATOR_OK) rc = gat8_prepare_device();
        if (rc) return rc;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) f->n_cu = prop.multiProcessorCount;
    }
    GATOR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

}  // namespace

int fused_create(gator_ctx* c, void* stream) {
    if (c->impl == GATOR_IMPL_BASIC) return GATOR_OK;
    FusedState* f = new FusedState();
    c->fused = f;
    int rc = read_fused_options(c, &f->opt);
    if (rc) return rc;
    f->gat_tiled = f->opt.gat_tiled;
    f->graph_replay = f->opt.graph;
    const Weights& w = c->w;
    if (c->parts & GATOR_PART_GAT) {
        rc = fused_create_gat(c, f, stream);
        if (rc) return rc;
    }
    if (!(c->parts & GATOR_PART_MDR)) return GATOR_OK;
    if (f->opt.c3_mdr) {
        // Above 2^10 in the exp2 domain - a worst-case shift of half a unit, 41 % of a probability - the MDR layers of gator_forward_bf16
        // keep the fp32 configuration's two planes for this ctx (measured: bound 470 -> 0.63 mm max, 3 340 -> 7.6 mm; tests/test_gpu_bf16.py).
        // (the encoder leaves the mode with them: under such weights the MDR layers amplify the 11-bit rounding of its activations too -
        // measured at bound 3 449: 5.1 mm max in the mode, 1.9 with the MDR layers on two planes, and the figure of the test with both out)
        f->c3_logit_bound = c3_logit_bound(w, (c->parts & GATOR_PART_GAT) ? c->hop_bias : nullptr, c->J);
        if (f->opt.c3_guard && !(f->c3_logit_bound <= 1024.0f)) f->opt.c3_mdr = f->opt.c3_encoder = false;
    }
    const size_t n_up = f->opt.up_x3 == 0 ? (size_t)3 * kOB * kCB * kTile : 0, n_layer = (size_t)64 * kTile;
    const size_t total = n_up + 3 * n_layer + 24 * kTile + 64 + (size_t)kVT * 2 * kTile + 3 * 64 + 1024;
    GATOR_TRY(f->wbuf.alloc(total * sizeof(float)));
    float* p = f->wbuf;
    auto take = [&](size_t k) { float* r = p; p += k; return r; };
    // upsample_conv.weight [6890][431][3] -> one packed [216][14] tile grid per tap
    float* up = take(n_up);
    if (f->opt.up_x3 == 2) {
        GATOR_TRY(f->up_w2.alloc(upsample_x2_weight_elems() * 2));
        int rc = pack_upsample_any(Regressor::X2, w.up_w, f->up_w2, &f->up_w2_unscale, stream);
        if (rc == GATOR_OK) rc = upsample_x2_prepare_device();
        if (rc) return rc;
    } else if (f->opt.up_x3 == 1) {
        GATOR_TRY(f->up_w3.alloc(upsample_x3_weight_elems() * 2));
        int rc = pack_upsample_any(Regressor::X3, w.up_w, f->up_w3, nullptr, stream);
        if (rc) return rc;
    } else {
        for (int tap = 0; tap < 3; ++tap) {
            int rc = fused_pack_linear(w.up_w + tap, (int64_t)kV * 3, 3, kNV, kV, up + (size_t)tap * kOB * kCB * kTile, stream);
            if (rc) return rc;
        }
        f->up_w = up;
    }
    for (int li = 0; li < 3; ++li) {
        const MdrLayerW& r = w.lay[li];
        MdrLayerP& q = f->lay[li];
        const PackItem items[] = {      // (row-major [N][K] weights)
            {r.wq, 64, 1, 64, 64, &q.wq}, {r.wk, 64, 1, 64, 64, &q.wk}, {r.wv, 64, 1, 64, 64, &q.wv}, {r.proj_w, 64, 1, 64, 64, &q.proj},
            {r.fc1_w, 64, 1, 256, 64, &q.fc1}, {r.fc2_w, 256, 1, 64, 256, &q.fc2},
            {r.sa_w[0], 64, 1, 64, 64, &q.sa[0]}, {r.sa_w[1], 64, 1, 64, 64, &q.sa[1]}, {r.sa_w[2], 64, 1, 64, 64, &q.sa[2]}, {r.sa_w[3], 64, 1, 64, 64, &q.sa[3]}};
        GATOR_TRY(pack_linears(items, p, stream));
    }
    // head: one 32-row linear. rows 0..19 motion_linear[0..19] (mat_A), 24..26 bias_linear, 27 scale_linear (alpha head),
    // 28..30 motion_linear[20..22] (mat_C)   -- MDR.py:156-162
    {
        std::vector<float> hw(32 * 64, 0.f), hb(32, 0.f);
        const std::vector<float> mw = d2h(w.motion_w, 23 * 64), mb = d2h(w.motion_b, 23), bw = d2h(w.biasl_w, 3 * 64), bb = d2h(w.biasl_b, 3);
        for (int r = 0; r < 20; ++r) { std::copy(mw.begin() + r * 64, mw.begin() + (r + 1) * 64, hw.begin() + r * 64); hb[r] = mb[r]; }
        for (int r = 0; r < 3; ++r) {
            std::copy(bw.begin() + r * 64, bw.begin() + (r + 1) * 64, hw.begin() + (24 + r) * 64); hb[24 + r] = bb[r];
            std::copy(mw.begin() + (20 + r) * 64, mw.begin() + (21 + r) * 64, hw.begin() + (28 + r) * 64); hb[28 + r] = mb[20 + r];
        }
        {   // mat_A feeds nothing but the softmax over its 20 columns (MDR.py:161-166), which a shift common to all 20 biases does not change - so
            // no loss keeps that shift small, and as the start value of the head linear's accumulator it would round every partial product at
            // ITS magnitude (at +-100: 2.7 x the fp32 reference's error, tests/test_gpu_softmax_edges.py).  The multiple of 8 nearest to the
            // biases' mean is taken out here: 0 for |mean| < 4, so an ordinary checkpoint is packed as it is; the subtraction is exact in fp32
            // (both sides are multiples of the larger one's ulp and the result is small) unless the 20 biases themselves span more than 2^20 ulps.
            double mean = 0;
            for (int r = 0; r < 20; ++r) mean += mb[r];
            const float shift = 8.0f * std::nearbyint((float)(mean / 20.0) / 8.0f);
            if (std::isfinite(shift))
                for (int r = 0; r < 20; ++r) hb[r] = mb[r] - shift;
        }
        if (c->alpha) {
            const std::vector<float> sw = d2h(w.scale_w, 64), sb = d2h(w.scale_b, 1);
            std::copy(sw.begin(), sw.end(), hw.begin() + 27 * 64);
            hb[27] = sb[0];
        }
        DevBuf<float> tmp;
        GATOR_TRY(tmp.alloc(hw.size() * sizeof(float)));
        GATOR_HIP_CHECK(hipMemcpy(tmp, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice));
        float* dst = take(2 * kTile);
        int rc = fused_pack_linear(tmp, 64, 1, 32, 64, dst, stream);
        GATOR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        tmp.reset();
        if (rc) return rc;
        f->head_w = dst;
        if (f->opt.mdr_x3) {     // split-precision image of the three layers' tile grids and the head tiles (contiguous in wbuf)
            const int64_t ntiles = (dst + 2 * kTile - f->lay[0].wq) / kTile;
            GATOR_TRY(f->wxbuf.alloc((size_t)ntiles * kTileX3 * sizeof(float)));
            if (f->opt.mdr_x3 == 2) {     // three fp16 planes under one power-of-two scale (x3_common.h: the 4-product linears)
                float& ratio = f->h3_tile_ratio[GATOR_H3SET_MDR];
                rc = fused_repack_h3(f->lay[0].wq, f->wxbuf, ntiles, &f->mdr_wshift, &ratio, stream);
                if (rc) return rc;
                if (!h3_set_holds(ratio)) h3_demote(f, GATOR_H3SET_MDR);      // the exact six products, as under GATOR_MDR_X3=1
            }
            if (f->opt.mdr_x3 != 2) rc = fused_repack_x3(f->lay[0].wq, f->wxbuf, ntiles, stream);
            if (rc) return rc;
        }
        float* hbd = take(64);
        GATOR_HIP_CHECK(hipMemcpy(hbd, hb.data(), 32 * sizeof(float), hipMemcpyHostToDevice));
        f->head_b = hbd;
    }
    {   // joint tokens: get_joint_feature packed, pos_j_id_embed[1..J] as T-layout tiles (MDR.py:130-134)
        float* dst = take(10 * kTile);
        int rc = fused_pack_linear(w.jfeat_w, 133, 1, 64, 133, dst, stream);
        if (rc) return rc;
        f->jfeat_p = dst;
        float* d128 = take(8 * kTile);                                  // feat columns 5..132 for the GAT-kernel epilogue
        rc = fused_pack_linear(w.jfeat_w + 5, 133, 1, 64, 128, d128, stream);
        if (rc) return rc;
        f->jfeat128_p = d128;
        if (f->opt.mdr_x3 == 2) {      // the same eight tiles as three fp16 planes under their own power-of-two scale (k_gat8's fused tail, gat8_tail.h)
            float& ratio = f->h3_tile_ratio[GATOR_H3SET_JFEAT];
            GATOR_TRY(f->jf128_h3.alloc((size_t)8 * kTileX3 * sizeof(float)));
            rc = fused_repack_h3(d128, f->jf128_h3, 8, &f->jf128_wshift, &ratio, stream);
            if (rc) return rc;
            if (!h3_set_holds(ratio)) { f->jf128_h3.reset(); h3_demote(f, GATOR_H3SET_JFEAT); }      // (the two tail launches stay)
        }
        const std::vector<float> jw = d2h(w.jfeat_w, 64 * 133);
        std::vector<float> j5(5 * 64);
        for (int i = 0; i < 5; ++i)
            for (int n = 0; n < 64; ++n) j5[i * 64 + n] = jw[n * 133 + i];
        float* j5d = take(kTile);
        GATOR_HIP_CHECK(hipMemcpy(j5d, j5.data(), j5.size() * sizeof(float), hipMemcpyHostToDevice));
        f->jfeat5 = j5d;
        const std::vector<float> pj = d2h(w.pos_j, (size_t)(c->J + 1) * 64);
        std::vector<float> pt(2 * kTile);
        for (int nb = 0; nb < 2; ++nb)
            fill_tile(pt.data() + (size_t)nb * kTile, [&](int t, int ch) { return t < c->J ? pj[(size_t)(t + 1) * 64 + 32 * nb + ch] : 0.f; });
        float* pd = take(2 * kTile);
        GATOR_HIP_CHECK(hipMemcpy(pd, pt.data(), pt.size() * sizeof(float), hipMemcpyHostToDevice));
        f->posj_T = pd;
    }
    // tokenise constants: get_verts_feature on [v431 | pose3d_nn] + pos_v (MDR.py:126-137); v431/bias/pos part folded per token
    {
        const std::vector<float> vw = d2h(w.vfeat_w, 64 * 6), vb = d2h(w.vfeat_b, 64), pv = d2h(w.pos_v, (size_t)(kV + 1) * 64), v4 = d2h(w.v431, kV * 3);
        std::vector<float> base((size_t)kVT * 2 * kTile, 0.f), w3(3 * 64);
        for (int t = 0; t < kVT; ++t)
            for (int nb = 0; nb < 2; ++nb)
                for (int g = 0; g < 4; ++g)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j) {
                            const int token = 32 * t + (lane & 31), ch = 32 * nb + 8 * g + 4 * (lane >> 5) + j;
                            if (token >= kV) continue;
                            double s = (double)vb[ch];
                            for (int i = 0; i < 3; ++i) s += (double)vw[ch * 6 + i] * (double)v4[token * 3 + i];
                            base[(((size_t)(t * 2 + nb) * 4 + g) * 64 + lane) * 4 + j] = (float)(s + (double)pv[(size_t)(token + 1) * 64 + ch]);
                        }
        for (int i = 0; i < 3; ++i)
            for (int ch = 0; ch < 64; ++ch) w3[i * 64 + ch] = vw[ch * 6 + 3 + i];
        float* bd = take(base.size());
        GATOR_HIP_CHECK(hipMemcpy(bd, base.data(), base.size() * sizeof(float), hipMemcpyHostToDevice));
        f->tok_base = bd;
        float* wd = take(3 * 64);
        GATOR_HIP_CHECK(hipMemcpy(wd, w3.data(), w3.size() * sizeof(float), hipMemcpyHostToDevice));
        f->tok_w3 = wd;
    }
    GATOR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return GATOR_OK;
}

FusedState::~FusedState() {
    for (FusedWs& w : sets) { w.base.reset(); w.vcp16.reset(); }
    graphs_clear(this);
    if (cap_stream) (void)hipStreamDestroy((hipStream_t)cap_stream);
    if (aux_stream) (void)hipStreamDestroy((hipStream_t)aux_stream);
    if (ev_fork) (void)hipEventDestroy((hipEvent_t)ev_fork);
    if (ev_join) (void)hipEventDestroy((hipEvent_t)ev_join);
}

void fused_destroy(gator_ctx* c) {
    delete c->fused;
    c->fused = nullptr;
}

// The plan of one call on this ctx (forward_plan.h), or GATOR_EUNSUPPORTED with the planner's reason: before anything is queued
static int fused_plan(const gator_ctx* c, int B, PlanEntry entry, bool bf16, bool with_joints, ForwardPlan* p) {
    const FusedState* f = c->fused;
    const char* why = plan_forward(f->opt, c->J, f->n_cu, B, entry, bf16, with_joints, f->gat_tiled, p);
    return why ? fail(GATOR_EUNSUPPORTED, "%s", why) : GATOR_OK;
}

int fused_gat_forward(gator_ctx* c, const float* pose2d, int B, float* x_out, float* feat, void* stream) {
    ForwardPlan p;
    GATOR_TRY(fused_plan(c, B, PlanEntry::GAT, false, false, &p));
    StageTimer tm(c, "gat", stream);
    return launch_gat(c, c->fused, p.gat, pose2d, B, x_out, feat, stream, B, 0);
}

int fused_upsample(gator_ctx* c, const float* vert431, int B, float* verts, void* stream) {
    FusedState* f = c->fused;
    FusedWs& ws = f->sets[0];
    GATOR_TRY(fused_ensure_ws(c, ws, B));
    const RegressorPlan r = plan_regressor(f->opt, false, false);
    GATOR_TRY(launch_pack_vc_any(r, vert431, B, ws, stream));
    StageTimer tm(c, "upsample", stream);
    return launch_upsample_any(f, c, ws, r, B, verts, stream);
}

static int fused_upsample_bf16_in(gator_ctx* c, FusedWs& ws, const float* vert431, int B, float* verts, void* stream) {
    GATOR_TRY(fused_ensure_ws(c, ws, B));
    FusedState* f = c->fused;
    if (!f->up_w16) {      // first bf16 call: pack the regressor weights once
        GATOR_TRY(f->up_w16.alloc(upsample_bf16_weight_elems() * 2));
        GATOR_TRY(pack_upsample_any(Regressor::BF16, c->w.up_w, f->up_w16, nullptr, stream));
        // One-time: the pack must be COMPLETE before any other stream may read up_w16.  In sub-batch mode the second half
        // runs on a different (non-blocking) stream whose fork event was recorded before this pack was queued.
        GATOR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    }
    if (B > ws.vcp16_cap) {
        if (ws.vcp16) GATOR_HIP_CHECK(hipDeviceSynchronize());
        GATOR_TRY(ws.vcp16.alloc(upsample_bf16_vcp_elems(B) * 2));
        ws.vcp16_cap = B;
    }
    StageTimer tm(c, "upsample_bf16", stream);
    const RegressorPlan r{Regressor::BF16, false, false};
    GATOR_TRY(launch_pack_vc_any(r, vert431, B, ws, stream));
    return launch_upsample_any(f, c, ws, r, B, verts, stream);
}

int fused_upsample_bf16(gator_ctx* c, const float* vert431, int B, float* verts, void* stream) {
    return fused_upsample_bf16_in(c, c->fused->sets[0], vert431, B, verts, stream);
}

// The vertex regressor of a forward, in the form its plan names, on the coarse vertices launch_mdr left in ws
static int fused_regress(gator_ctx* c, FusedWs& ws, const RegressorPlan& r, int B, float* verts, void* stream) {
    if (r.form == Regressor::BF16) return fused_upsample_bf16_in(c, ws, ws.vc, B, verts, stream);
    StageTimer tm(c, "upsample", stream);
    return launch_upsample_any(c->fused, c, ws, r, B, verts, stream);
}

int fused_mdr_forward(gator_ctx* c, const float* pc, int B, float* verts, void* stream) {
    FusedWs& ws = c->fused->sets[0];
    ForwardPlan p;
    GATOR_TRY(fused_plan(c, B, PlanEntry::MDR, false, false, &p));
    GATOR_TRY(fused_ensure_ws(c, ws, B));
    GATOR_TRY(launch_mdr(c, c->fused, ws, p, pc, B, stream, nullptr, nullptr));        // also writes the packed vertex-GEMM operand ws.vcp / ws.vcp3
    return fused_regress(c, ws, p.up, B, verts, stream);
}

static int fused_forward_one(gator_ctx* c, FusedWs& ws, const ForwardPlan& p, const float* pose2d, int B, float* verts, float* pose3d, void* stream, float* joints);

int fused_set_graph_replay(gator_ctx* c, int on) {
    FusedState* f = c->fused;
    if (!f) return fail(GATOR_EUNSUPPORTED, "gator_set_graph_replay: fused ctx only");
    if (on >= 0) {
        if (!on && f->graph_replay) { GATOR_HIP_CHECK(hipDeviceSynchronize()); graphs_clear(f); }
        f->graph_replay = on != 0;
    }
    return (int)std::min<unsigned long long>(f->graph_launches, 0x7fffffffull);
}

// The forward of fused_forward_one replayed from a hipGraph (see FusedState::GraphSlot)
static int fused_forward_graph(gator_ctx* c, FusedWs& ws, const ForwardPlan& p, const float* pose2d, int B, float* verts, float* pose3d, void* stream) {
    FusedState* f = c->fused;
    int rc = fused_ensure_ws(c, ws, B);                  // may reallocate: before the key is formed, never inside a capture
    if (rc) return rc;
    FusedState::GraphSlot* slot = nullptr;
    for (auto& g : f->graphs)
        if (g.B == B && g.in == pose2d && g.verts == verts && g.pose3d == pose3d && g.ws == ws.base.get() && g.plan == p) { slot = &g; break; }
    if (!slot) {                                         // first sight: remember the key, run directly
        if ((int)f->graphs.size() >= FusedState::kGraphSlots) {
            // evict a key that was never captured if there is one (no replay can be in flight: no device-wide wait), else the least recently used
            auto lru = std::min_element(f->graphs.begin(), f->graphs.end(), [](const FusedState::GraphSlot& a, const FusedState::GraphSlot& b) {
                return (a.exec != nullptr) != (b.exec != nullptr) ? a.exec == nullptr : a.used < b.used; });
            if (lru->exec) GATOR_HIP_CHECK(hipDeviceSynchronize());      // a replay of it may still be running
            graph_slot_free(*lru);
            f->graphs.erase(lru);
        }
        FusedState::GraphSlot g;
        g.B = B; g.in = pose2d; g.verts = verts; g.pose3d = pose3d; g.plan = p; g.ws = ws.base.get();
        g.used = ++f->graph_clock;
        f->graphs.push_back(g);
        return fused_forward_one(c, ws, p, pose2d, B, verts, pose3d, stream, nullptr);
    }
    slot->used = ++f->graph_clock;
    if (!slot->exec) {                                   // second sight: capture on the private stream
        if (!f->cap_stream) {
            hipStream_t s2;
            GATOR_HIP_CHECK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
            f->cap_stream = s2;
        }
        hipStream_t cs = (hipStream_t)f->cap_stream;
        hipGraph_t g = nullptr;
        hipGraphExec_t ex = nullptr;
        bool ok = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            rc = fused_forward_one(c, ws, p, pose2d, B, verts, pose3d, cs, nullptr);
            ok = hipStreamEndCapture(cs, &g) == hipSuccess && rc == GATOR_OK && g != nullptr;
            if (ok) ok = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess;
        }
        if (!ok) {                                       // not capturable here: fall back to direct launches for good
            (void)hipGetLastError();
            if (ex) (void)hipGraphExecDestroy(ex);
            if (g) (void)hipGraphDestroy(g);
            f->graph_replay = false;
            if (rc) return rc;
            return fused_forward_one(c, ws, p, pose2d, B, verts, pose3d, stream, nullptr);
        }
        slot->graph = g; slot->exec = ex;
    }
    GATOR_HIP_CHECK(hipGraphLaunch((hipGraphExec_t)slot->exec, (hipStream_t)stream));
    ++f->graph_launches;
    c->set_tap(TAP_FEAT, ws.feat, (int64_t)B * c->J * kC);      // the same taps a direct forward leaves (launch_mdr sets vert431 only while it runs)
    c->set_tap(TAP_VERT431, ws.vc, (int64_t)B * kV * 3);
    return GATOR_OK;
}

// Sub-batch pipelining: with >= 2 x 64 samples the batch runs as two halves on two streams (fork/join by events, so the
// caller's stream semantics are unchanged and the pattern is graph-capturable).  Samples are independent and every kernel
// is batch-size invariant bit for bit, so the result is identical; the gain (+8 % at B=256) comes from one half's kernels
// filling the idle SIMDs in the tail of the other half's kernels.  Enabled by gator_config.flags / GATOR_SUBBATCH_STREAMS=2.
int fused_forward(gator_ctx* c, const float* pose2d, int B, float* verts, float* pose3d, void* stream, bool bf16) {
    FusedState* f = c->fused;
    const int want = c->subbatch_streams > 0 ? c->subbatch_streams : f->opt.subbatch_streams;
    ForwardPlan p;
    if (want < 2 || B < 128) {
        GATOR_TRY(fused_plan(c, B, PlanEntry::FORWARD, bf16, false, &p));
        if (f->graph_replay && !c->profiling && !c->block_taps) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;      // a caller that is capturing the forward itself gets the plain launches
            if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
            if (cs == hipStreamCaptureStatusNone) return fused_forward_graph(c, f->sets[0], p, pose2d, B, verts, pose3d, stream);
        }
        return fused_forward_one(c, f->sets[0], p, pose2d, B, verts, pose3d, stream, nullptr);
    }
    if (!f->aux_stream) {
        hipStream_t s2; hipEvent_t e1, e2;
        GATOR_HIP_CHECK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        GATOR_HIP_CHECK(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
        GATOR_HIP_CHECK(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
        f->aux_stream = s2; f->ev_fork = e1; f->ev_join = e2;
    }
    const int B0 = ((B / 2 + 31) / 32) * 32, B1 = B - B0;       // halves on 32-sample tile boundaries
    const int J = c->J;
    GATOR_HIP_CHECK(hipEventRecord((hipEvent_t)f->ev_fork, (hipStream_t)stream));
    GATOR_HIP_CHECK(hipStreamWaitEvent((hipStream_t)f->aux_stream, (hipEvent_t)f->ev_fork, 0));
    int rc = GATOR_OK;
    for (int i = 0; i < 2 && rc == GATOR_OK; ++i) {
        const int off = i ? B0 : 0, n = i ? B1 : B0;
        rc = fused_plan(c, n, PlanEntry::FORWARD, bf16, false, &p);      // each half is a forward of its own
        if (rc == GATOR_OK) rc = fused_forward_one(c, f->sets[i], p, pose2d + (size_t)off * J * 2, n, verts + (size_t)off * kNV * 3, pose3d + (size_t)off * J * 3,
                               i ? f->aux_stream : stream, nullptr);
    }
    GATOR_HIP_CHECK(hipEventRecord((hipEvent_t)f->ev_join, (hipStream_t)f->aux_stream));
    GATOR_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)f->ev_join, 0));
    c->clear_taps();          // taps describe a whole batch; not available in sub-batch mode
    return rc;
}

// gator_encoder_for_batch: under the ctx's own policy (pin = AUTO, whatever gator_set_encoder has pinned); a split batch counts as tiled
int fused_encoder_for_batch(const gator_ctx* c, int B) {
    const FusedState* f = c->fused;
    return f && plan_tiled_samples(f->opt, c->J, f->n_cu, B, f->opt.gat_tiled) > 0 ? GATOR_ENCODER_TILED : GATOR_ENCODER_SAMPLE;
}

// One forward as its plan says.  p is the plan of THIS call: of a batch of B, with_joints iff joints is given
static int fused_forward_one(gator_ctx* c, FusedWs& ws, const ForwardPlan& p, const float* pose2d, int B, float* verts, float* pose3d, void* stream, float* joints) {
    GATOR_TRY(fused_ensure_ws(c, ws, B));
    FusedState* f = c->fused;
    int rc = GATOR_OK;
    {   // x_out [B,3J] IS pose3d [B,J,3]: the tail writes the caller's buffer and produces the MDR joint K/V
        StageTimer tm(c, "gat", stream);
        if (p.n_tiled > 0) rc = launch_gat_tiled(c, f, ws, p, pose2d, B, stream);
        if (rc == GATOR_OK && p.sample == SampleEncoder::GAT8) rc = launch_gat8(c, f, ws, p, pose2d, B, pose3d, stream);
        if (rc == GATOR_OK && p.sample == SampleEncoder::GAT) {
            const size_t o = (size_t)p.n_tiled * c->J;
            rc = launch_gat(c, f, p.gat, pose2d + o * 2, B - p.n_tiled, pose3d + o * 3, ws.feat + o * kC, stream, B, p.n_tiled);
        }
    }
    if (rc) return rc;
    if (p.n_tail > 0) {   // lifter + MDR joint tokens as two batched launches (gat_tail.hip)
        StageTimer tm(c, "gat_tail", stream);
        GATOR_TRY(launch_gat_tail(c, f, ws, p, pose2d, pose3d, stream));
    }
    c->set_tap(TAP_FEAT, ws.feat, (int64_t)B * c->J * kC);
    GATOR_TRY(launch_mdr(c, f, ws, p, nullptr, B, stream, pose3d, pose2d));      // pose_combine is never materialised on this path
    if (!joints) return fused_regress(c, ws, p.up, B, verts, stream);
    // vertex GEMM with the joint-regression epilogue (verts may be null: nothing of 82 kB/mesh is stored)
    if (B > f->jr_cap) {
        if (f->jr_P) GATOR_HIP_CHECK(hipDeviceSynchronize());
        GATOR_TRY(f->jr_P.alloc((size_t)B * f->jr_nnz * 3 * sizeof(float)));
        f->jr_cap = B;
    }
    GATOR_TRY(fused_regress(c, ws, p.up, B, verts, stream));
    StageTimer tm(c, "jreg_reduce", stream);
    return launch_jreg_reduce(f, B, joints, stream);
}

// Register a sparse [nj, 6890] joint regressor (COO, host or device pointers are both read through hipMemcpy) for the fused epilogue
int fused_set_joint_regressor(gator_ctx* c, const int32_t* row, const int32_t* col, const float* val, int nnz, int nj) {
    FusedState* f = c->fused;
    if (!f) return fail(GATOR_EUNSUPPORTED, "gator_set_joint_regressor: fused ctx only");
    std::vector<int32_t> r(nnz), cc(nnz);
    std::vector<float> v(nnz);
    GATOR_HIP_CHECK(hipMemcpy(r.data(), row, nnz * sizeof(int32_t), hipMemcpyDefault));
    GATOR_HIP_CHECK(hipMemcpy(cc.data(), col, nnz * sizeof(int32_t), hipMemcpyDefault));
    GATOR_HIP_CHECK(hipMemcpy(v.data(), val, nnz * sizeof(float), hipMemcpyDefault));
    for (int e = 0; e < nnz; ++e)
        if (r[e] < 0 || r[e] >= nj || cc[e] < 0 || cc[e] >= kNV) return fail(GATOR_EINVAL, "gator_set_joint_regressor: entry %d out of range", e);
    // slots: sorted by (joint, vertex) -> CSR; epilogue entries: sorted by vertex, grouped by 32-vertex block
    std::vector<int> order(nnz);
    for (int e = 0; e < nnz; ++e) order[e] = e;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return r[a] != r[b] ? r[a] < r[b] : cc[a] < cc[b]; });
    std::vector<int> slot_of(nnz), rowptr(nj + 1, 0);
    for (int s = 0; s < nnz; ++s) { slot_of[order[s]] = s; rowptr[r[order[s]] + 1]++; }
    for (int j = 0; j < nj; ++j) rowptr[j + 1] += rowptr[j];
    std::vector<int> byv(nnz);
    for (int e = 0; e < nnz; ++e) byv[e] = e;
    std::stable_sort(byv.begin(), byv.end(), [&](int a, int b) { return cc[a] < cc[b]; });
    std::vector<int32_t> ent(2 * nnz), blk(2 * kOB, 0);
    std::vector<float> w(nnz);
    for (int i = 0; i < nnz; ++i) {
        const int e = byv[i], ob = cc[e] / 32;
        ent[2 * i] = cc[e]; ent[2 * i + 1] = slot_of[e]; w[i] = v[e];
        if (blk[2 * ob + 1] == 0) blk[2 * ob] = i;
        blk[2 * ob + 1]++;
    }
    if (f->jr_nnz) GATOR_HIP_CHECK(hipDeviceSynchronize());      // a forward that reads the old regressor may still run
    f->jr_P.reset(); f->jr_cap = f->jr_nnz = f->jr_nj = 0;
    GATOR_TRY(f->jr_blk.alloc(blk.size() * 4));
    GATOR_TRY(f->jr_ent.alloc(ent.size() * 4));
    GATOR_TRY(f->jr_w.alloc(w.size() * 4));
    GATOR_TRY(f->jr_rowptr.alloc(rowptr.size() * 4));
    GATOR_HIP_CHECK(hipMemcpy(f->jr_blk, blk.data(), blk.size() * 4, hipMemcpyHostToDevice));
    GATOR_HIP_CHECK(hipMemcpy(f->jr_ent, ent.data(), ent.size() * 4, hipMemcpyHostToDevice));
    GATOR_HIP_CHECK(hipMemcpy(f->jr_w, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    GATOR_HIP_CHECK(hipMemcpy(f->jr_rowptr, rowptr.data(), rowptr.size() * 4, hipMemcpyHostToDevice));
    f->jr_nnz = nnz; f->jr_nj = nj;
    return GATOR_OK;
}

void fused_disable_persist(gator_ctx* c) {
    if (c->fused) c->fused->opt.mdr_persist = 0;
}

int fused_c3_state(const gator_ctx* c, float* bound) {
    const FusedState* f = c->fused;
    if (!f) return fail(GATOR_EUNSUPPORTED, "gator_c3_state: fused ctx only");
    if (bound) *bound = f->c3_logit_bound;
    return f->opt.c3_mdr ? 1 : 0;
}

int fused_operand_state(const gator_ctx* c, float* tile_ratio) {
    const FusedState* f = c->fused;
    for (int i = 0; i < 4; ++i)
        if (tile_ratio) tile_ratio[i] = f ? f->h3_tile_ratio[i] : 0.f;
    return f ? f->h3_demoted : 0;
}

int fused_set_encoder(gator_ctx* c, int mode) {
    if (mode == 1 && !c->fused->opt.gat_x3) return fail(GATOR_EUNSUPPORTED, "gator_set_encoder: the sample-tiled encoder needs the split-precision path (GATOR_GAT_X3)");
    c->fused->gat_tiled = mode == GATOR_ENCODER_AUTO ? c->fused->opt.gat_tiled : mode;      // AUTO = the ctx's own policy, incl. a GATOR_GAT_TILED pin of the environment
    return GATOR_OK;
}

int fused_forward_joints(gator_ctx* c, const float* pose2d, int B, float* joints, float* pose3d, float* verts, void* stream) {
    FusedState* f = c->fused;
    if (!f || f->jr_nnz == 0) return fail(GATOR_EINVAL, "gator_forward_joints_f32: call gator_set_joint_regressor first");
    ForwardPlan p;
    GATOR_TRY(fused_plan(c, B, PlanEntry::FORWARD, false, true, &p));      // (refuses the fp32-input regressor: before anything is queued)
    return fused_forward_one(c, f->sets[0], p, pose2d, B, verts, pose3d, stream, joints);
}

}  // namespace gator
