/*
 * gator_hip.h -- C ABI of libgator_hip.so: the MI355X (gfx950) implementation of the GATOR inference
 * forward pass (GAT graph-aware transformer encoder -> MDR regression head -> 6890 SMPL vertices).
 *
 * The reference (kasvii/GATOR) has no FFI of its own: its boundary for this path is the Python
 * nn.Module API of lib/models (GATOR.py:16-27, GAT.py:133-156, MDR.py:124-174).  These entry points are
 * what a binding for that boundary calls; the modules under gator_amd/models/ are such a binding (ctypes) and
 * INTEGRATION.md shows the stub a reference maintainer would add.  Plain pointers and sizes only.
 *
 * Conventions
 *   - every function returns 0 on success, a negative gator_status otherwise; gator_last_error() then
 *     returns a thread-local human-readable message (reference convention: Python exceptions,
 *     lib/funcs_utils.py:121-127 -> the Python wrapper raises RuntimeError).
 *   - "device pointer" = hipMalloc'd memory on the ctx's device (a torch tensor's data_ptr()).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is enqueued on it
 *     and nothing synchronises the host.  A ctx is not thread-safe: one ctx per device per thread.
 */
#ifndef GATOR_HIP_H
#define GATOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gator_ctx gator_ctx;

typedef enum { GATOR_OK = 0, GATOR_EINVAL = -1, GATOR_EMISSING = -2, GATOR_ESHAPE = -3, GATOR_EHIP = -4,
               GATOR_ENOMEM = -5, GATOR_EUNSUPPORTED = -6,
               GATOR_EDEVICE = -7,    /* a kernel of an EARLIER call flagged its result as invalid (gator_device_status) */
               GATOR_EDEVICE_DEFERRED = -8   /* the same report, riding on a forward that WAS queued normally: this call's outputs are being
                                                written and are valid unless the next call reports again (gator_status_reason says why) */
} gator_status;

/* ABI 2 (round 6): gator_config starts with struct_size; forwards return GATOR_EDEVICE_DEFERRED instead of GATOR_EDEVICE when they carry
 * an earlier call's report; gator_abi_version / gator_status_reason added.  A binding checks gator_abi_version() == GATOR_ABI_VERSION at load. */
#define GATOR_ABI_VERSION 2

typedef enum { GATOR_F32 = 0, GATOR_I64 = 1, GATOR_I32 = 2 } gator_dtype;

/* One named tensor.  Names are the reference checkpoint's state_dict keys (SURVEY.md Appendix B:
 * "pose_lifter.blocks.0.attn.qkv.weight", "pose2mesh.upsample_conv.weight", ...) -- the checkpoint layout IS
 * the weight contract (lib/core/base.py:70, demo/run.py:98) -- plus the derived constants the reference keeps as
 * plain module attributes:
 *     "const.shortest_path" i64 [J,J]   (data/base_data/shortest_path_*.npy, lib/models/GAT.py:89-93)
 *     "const.edge_input"    f32 [J,J,D] (gen_edg_input, lib/models/backbones/modules.py:13-29)
 *     "const.vj_relation"   i32 [431]   (build_verts_joints_relation, lib/graph_utils.py:71-89)
 * `data` may be a device or a host pointer (is_host says which); the ctx copies what it needs. */
typedef struct {
    const char* name;
    const void* data;
    int32_t dtype;      /* gator_dtype */
    int32_t ndim;       /* <= 4 */
    int64_t shape[4];
    int32_t is_host;
    int32_t reserved;
} gator_tensor;

/* GATOR_IMPL_FUSED computes every large product on the 16-bit MFMA from SPLIT fp32 operands (csrc/x3_common.h): weights always
 * exactly (three fp16 or bf16 planes), and by default activations, attention operands and the vertex regressor's operands as TWO
 * fp16 planes of 16 x value (22 significant bits; four resp. three partial products per fp32 product instead of six).
 * Operand range of that default: every value that feeds a token-wise linear and every coarse vertex must stay below 4 094 in
 * magnitude (16 x value must fit an fp16 plane); beyond it the plane overflows, the vertices of that forward come out NaN and the
 * NEXT call on the ctx (or gator_device_status) returns GATOR_EDEVICE -- loud, never silently wrong.  Trained checkpoints are
 * orders of magnitude inside (LayerNorm outputs, GELU hiddens, metres).
 * Weight dynamic range of that default: the three fp16 weight planes of the four-product linears share ONE power-of-two scale per weight
 * set (k_gat8's stream, the sample-tiled encoder's grids, the MDR layers + head, get_joint_feature), which holds every weight to 2^-38 of
 * the set's LARGEST one -- exact to fp32 only while the 32 x 32 tiles of a set stay within 2^12 of each other in max|w|.  gator_create
 * measures that; a set beyond it is not packed and its products run on the exact three-way bf16 split for this ctx (slower, never less
 * accurate; gator_operand_state reports it).  A function-preserving rescaling of a checkpoint (q against k, v against proj, fc1 against
 * fc2 by 2^k: what weight decay does) therefore never changes the result beyond fp32 noise (tests/test_gpu_rescaled_weights.py).
 * gator_config.arithmetic = GATOR_ARITH_EXACT_SPLIT (or the environment
 * variables it stands for, read by gator_create) selects the forms without a rounded operand and without that limit (GATOR_MDR_X3=1 GATOR_UPSAMPLE_X3=1 GATOR_GAT8_H4=0 GATOR_GAT_TILED_H4=0: exact
 * three-way bf16 split, six products) or the fp32-input MFMA form of a stage (GATOR_GAT_X3 / GATOR_MDR_X3 / GATOR_UPSAMPLE_X3 = 0);
 * all forms are the same accuracy class and under test (tests/test_gpu_x3.py; statistics: profiles/r04_error_budget.md). */
typedef enum { GATOR_IMPL_FUSED = 0,   /* MFMA / register-resident fused kernels (default) */
               GATOR_IMPL_BASIC = 1    /* bring-up kernels: one simple HIP kernel per reference op; used as an
                                          on-device cross-check of the fused path */
} gator_impl;

typedef enum { GATOR_ARITH_DEFAULT = 0, GATOR_ARITH_EXACT_SPLIT = 1 } gator_arith;

typedef enum { GATOR_PART_GAT = 1,    /* pose_lifter.*  (models.GAT.get_model used stand-alone, lib/core/base.py:59) */
               GATOR_PART_MDR = 2     /* pose2mesh.*    (models.MDR.get_model, lib/models/MDR.py:172-174) */
} gator_parts;

typedef struct {
    int32_t struct_size; /* = sizeof(gator_config) of the header the caller was built with.  Fields the caller's header does not have yet
                            read as 0 (their defaults); a value that is not a multiple of 4 in [8, 1024] is refused (GATOR_EINVAL) -- which is
                            what a caller built against the ABI-1 header (first field num_joint = 17 / 19) gets instead of a mis-read struct */
    int32_t num_joint;   /* 17 (Human3.6M) or 19 (COCO + pelvis + neck); lib/models/GAT.py:79-93 */
    int32_t alpha;       /* cfg.MODEL.alpha: LayerNorm(3)+scale head instead of BatchNorm1d(431); MDR.py:115-119,162 */
    int32_t impl;        /* gator_impl */
    int32_t max_batch;   /* workspace is sized for this many samples up front (0 = grow on demand) */
    int32_t parts;       /* gator_parts bitmask: which sub-modules' weights are present (0 = both) */
    int32_t subbatch_streams; /* 2: run batches >= 128 as two half-batches on two streams (identical results, better tails) */
    int32_t arithmetic;  /* gator_arith: 0 = default (two-plane activations, operand range |value| < 4 094, see above);
                            1 = GATOR_ARITH_EXACT_SPLIT: every product on the exact three-way bf16 split (six partial products), no
                            rounded operand and no operand-range limit -- what a ctx that reported GATOR_EDEVICE for an out-of-range
                            operand is re-created with.  Same accuracy class, ~1.5 x the time (tests/test_gpu_x3.py) */
} gator_config;

/* Replaces: models.GATOR.get_model(...) + load_state_dict + .cuda()  (lib/models/GATOR.py:24-27,
 * lib/core/base.py:57,70,197).  Copies/packs the weights, folds the input-independent constants
 * (hop/path attention bias modules.py:98-107, MGCN adjacency :247-249, hop masks :163-170, BatchNorm affine). */
int gator_create(const gator_tensor* tensors, int32_t n_tensors, const gator_config* cfg, gator_ctx** out);
int gator_destroy(gator_ctx* ctx);

/* Device-side validity of the forwards issued so far.  Kernels never synchronise the host, so a failure that only the device can
 * see -- non-finite / out-of-range coarse vertices (operand range above), or a persistent MDR launch that did not finish every
 * sample (an XCD without workgroups under a CU mask; the ctx then switches to the four-launch form for good) -- is recorded in a sticky,
 * host-visible status word and reported by the NEXT entry point called on the ctx, once, as GATOR_EDEVICE (the affected vertices are NaN).  gator_device_status reports it on demand; sync != 0 waits for the device first
 * (the reference raises at the point of use, lib/core/base.py:210-237; this is the asynchronous equivalent). */
int gator_device_status(gator_ctx* ctx, int32_t sync);
/* Why the last GATOR_EDEVICE / GATOR_EDEVICE_DEFERRED of this ctx was returned: 1 = a persistent MDR launch did not finish (the ctx has switched to
 * the four-launch form), 2 = non-finite / out-of-range coarse vertices in samples with finite input poses (the default arithmetic's operand range:
 * re-create the ctx with GATOR_ARITH_EXACT_SPLIT -- gator_amd/models/_base.py does exactly that by itself), 3 = samples whose input pose is not
 * finite (their vertices are NaN, as the reference's are; nothing to change), 0 = none yet.  When one forward has several reasons, 2 is
 * reported before 1 and 1 before 3; the MDR-only entry point (gator_mdr_forward_f32) does not see the poses and reports 2 for those. */
int gator_status_reason(gator_ctx* ctx);

/* Replaces: GATOR.forward (lib/models/GATOR.py:16-22).
 *   pose2d [B,J,2] f32 device, contiguous  ->  verts [B,6890,3] f32 (metres), pose3d [B,J,3] f32 (mm).
 * fp32 in, fp32 out, fp32 accumulation; within 1e-3 mm of the fp64 evaluation of the reference (tests/).  The products themselves run
 * on the 16-bit MFMA with split operands: weights are always carried exactly (three planes); by default activations, the attention
 * operands and the vertex regressor's operands are rounded to 22 bits (two fp16 planes), which costs less than the fp32 rounding noise
 * the reference forward has itself.  Environment switches read at gator_create select the forms without any rounded operand
 * (GATOR_MDR_X3=1 GATOR_UPSAMPLE_X3=1 GATOR_GAT8_H4=0 GATOR_GAT_TILED_H4=0) or the fp32-input MFMA (=0). */
int gator_forward_f32(gator_ctx* ctx, const float* pose2d, int32_t batch, float* verts, float* pose3d, void* stream);

/* BASELINE config 3 ("full GATOR forward bf16"): the same forward in 16-bit operand mode (round 5).  Activations travel as ONE fp16 plane
 * into every token-wise linear of the encoder (lib/models/GAT.py:33-43, backbones/modules.py:121-196) and of the three MDR layers
 * (lib/models/MDR.py:140-153, vanilla_transformer_encoder.py:82-94), whose attention cores take Q, K, V and the probabilities as one plane
 * too; weights stay on two planes (22 bits) - except upsample_conv's (MDR.py:122,167-168), which go on one while the coarse vertices stay on
 * two.  fp32 accumulate / softmax / norms / GELU / residual stream / output; the head features, the encoder's J x J operators, the lifter
 * and the tokenisers keep gator_forward_f32's operands.  Which operand may be one plane was decided with the fp64 oracle under operand
 * rounding (tools/emulate_16bit.py): a single 16-bit plane for the WEIGHTS of the linears, or bf16 anywhere, is what costs millimetres.
 * Against the fp64 evaluation of the reference over 2048 samples x every coordinate: 0.76 mm max, 0.10 mm rms, |delta MPJPE| < 1e-3 mm
 * (tests/test_gpu_bf16.py; bar 1 mm / 0.2 mm / 0.05 mm); 1.6 x the fp32 forward at B = 2048.  Not for weights that drive the attention
 * logits to hundreds (near one-hot softmaxes): there one plane moves a score by 2^-12 of its magnitude.  Needs the default operand forms
 * (GATOR_MDR_X3=2, GATOR_UPSAMPLE_X3=2, GATOR_GAT8_H4=1, GATOR_GAT_TILED_H4=1).  Read at gator_create: GATOR_C3_ENCODER=0 (encoder as in
 * gator_forward_f32), GATOR_C3_UPSAMPLE_W1=0 (regressor weights on two planes), GATOR_C3_MDR=0 (MDR layers as in gator_forward_f32),
 * GATOR_C3_UPSAMPLE_BF16=1 (round 4's form of the regressor: both operands one bf16 plane, 8 mm max / 1 mm rms).
 * gator_upsample_bf16: the stage entry point of that bf16 vertex regressor. */
int gator_forward_bf16(gator_ctx* ctx, const float* pose2d, int32_t batch, float* verts, float* pose3d, void* stream);
/* Guard of that mode (round 6).  One fp16 plane moves an attention score by up to 2^-11 |q| |k|; gator_create bounds |q . k| / sqrt(d_k) of the three
 * 431 x 431 self-attentions from the weights alone (per head (sigma_max(Wq_h) |x| + |bq_h|) (sigma_max(Wk_h) |x| + |bk_h|) / sqrt(d_k) with the custom
 * LayerNorm's bound on |x|, exp2 domain), and in the same way the logits of the other two attentions that carry one-plane operands in the mode: the MDR
 * cross-attention (nn.LayerNorm(64), no biases) and the encoder's J x J attention (nn.LayerNorm(128), qkv biases, plus max|hop / path bias|);
 * *logit_bound is the largest of the three.  Above 2^10 the MDR
 * layers and the encoder of gator_forward_bf16 keep gator_forward_f32's two planes for this ctx (the vertex regressor stays in the mode); GATOR_C3_GUARD=0
 * switches the guard off.  Returns 1 if the MDR layers run on one plane under gator_forward_bf16, 0 if not (guard, GATOR_C3_MDR=0 or a ctx without the
 * default operand forms), negative on error; *logit_bound (may be NULL) receives the bound. */
int gator_c3_state(gator_ctx* ctx, float* logit_bound);
/* What gator_create decided from the weights about the default arithmetic's three-plane weight sets (weight dynamic range, above).  The four
 * sets share one power-of-two scale each; a set whose smallest 32 x 32 tile is below 2^-12 of its largest is not packed, and the ctx runs the
 * products that would have read it on the exact three-way bf16 split instead (slower, never less accurate).  Returns a bitmask of the sets that
 * were demoted (bit GATOR_H3SET_*; 0 for a ctx that uses none of them: exact arithmetic, GATOR_IMPL_BASIC), negative on error; tile_ratio[4]
 * (may be NULL) receives each set's smallest ratio of a non-zero tile's max|w| to the set's max|w|, 0 for a set that was not looked at. */
typedef enum { GATOR_H3SET_GAT8 = 0,      /* k_gat8's weight stream; demoted: the exact six products (as GATOR_GAT8_H4=0), no fused tail */
               GATOR_H3SET_GAT_TILED = 1, /* the sample-tiled encoder's grids; demoted: as GATOR_GAT_TILED_H4=0 */
               GATOR_H3SET_MDR = 2,       /* the three MDR layers and the head; demoted: as GATOR_MDR_X3=1, no fused tail */
               GATOR_H3SET_JFEAT = 3      /* get_joint_feature for k_gat8's fused tail; demoted: the two tail launches (as GATOR_GAT8_TAIL=0) */
} gator_h3set;
int gator_operand_state(gator_ctx* ctx, float* tile_ratio);
int gator_upsample_bf16(gator_ctx* ctx, const float* vert431, int32_t batch, float* verts, void* stream);

/* Stage entry points (parity tests; same semantics as the reference sub-modules):
 *   GAT.forward   lib/models/GAT.py:133-152 : pose2d [B,J,2] -> x_out [B,3J] (mm), feat [B,J,128]
 *   MDR.forward   lib/models/MDR.py:124-170 : pose_combine [B,J,133] -> verts [B,6890,3]
 *   upsample_conv + template add  MDR.py:167-168 : vert431 [B,431,3] -> verts [B,6890,3]              */
int gator_gat_forward_f32(gator_ctx* ctx, const float* pose2d, int32_t batch, float* x_out, float* feat, void* stream);
int gator_mdr_forward_f32(gator_ctx* ctx, const float* pose_combine, int32_t batch, float* verts, void* stream);
int gator_upsample_f32(gator_ctx* ctx, const float* vert431, int32_t batch, float* verts, void* stream);

/* Debug taps of the LAST forward on this ctx, converted to the reference's layout:
 *   "hop_path_bias" [8,J,J]   "feat" [B,J,128]   "mdr_lbf2" [B,431,64]   "vert431" [B,431,3]
 * dst is a device pointer with room for `capacity` floats; *count receives the element count. */
int gator_get_tap(gator_ctx* ctx, const char* name, float* dst, int64_t capacity, int64_t* count, void* stream);
/* Additional taps "gat_block0" .. "gat_block5" [B,J,128]: the residual stream after each GATBlock (lib/models/GAT.py:33-43,
 * :145-147).  Off by default (the stores cost time); fused ctx only.  On a fused ctx the same switch also governs "mdr_lbf2" (110 KB of
 * stores per sample that nothing else reads): without it gator_get_tap("mdr_lbf2") returns GATOR_EMISSING.  Taps never outlive the next call on the ctx; the "feat" tap
 * of the stand-alone gator_gat_forward_f32 aliases the caller's `feat` buffer. */
int gator_enable_block_taps(gator_ctx* ctx, int32_t on);

/* Encoder policy of a fused ctx.  The six GAT blocks (lib/models/GAT.py:145-147) have two kernels: one workgroup per sample
 * (bit-identical results whatever the batch size or the position in the batch) and a sample-tiled one for large batches
 * (7 / 6 samples per workgroup; bit-identical within itself, equal to the first to fp32 rounding).  mode GATOR_ENCODER_AUTO (the
 * default) picks per call from the batch size, so above 1 024 samples a sample's last bits depend on how the batch was cut;
 * GATOR_ENCODER_SAMPLE / GATOR_ENCODER_TILED pin one kernel for every call on the ctx - what a sharded run uses so that the
 * all-gathered result is independent of the number of ranks (gathered == single-GPU, bit for bit). */
#define GATOR_ENCODER_AUTO (-1)
#define GATOR_ENCODER_SAMPLE 0
#define GATOR_ENCODER_TILED 1
int gator_set_encoder(gator_ctx* ctx, int32_t mode);
/* Which kernel GATOR_ENCODER_AUTO would use for a call of `batch` samples on this ctx (its environment switches, the device's CU
 * count): GATOR_ENCODER_SAMPLE or GATOR_ENCODER_TILED (a batch the policy splits between both counts as TILED); negative on error.
 * What a sharded run pins for every call so that the rule lives in one place (gator_amd/parallel.py). */
int gator_encoder_for_batch(gator_ctx* ctx, int32_t batch);

/* hipGraph replay of repeated forwards on a fused ctx (off by default; GATOR_GRAPH=1 switches it on at gator_create).  A forward is
 * identified by (batch, the three pointers, precision, encoder pin): the second time the same call is seen it is captured on a private
 * stream, from then on gator_forward_f32 / _bf16 is ONE hipGraphLaunch on the caller's stream (same kernels, same results bit for
 * bit; up to 8 calls are remembered, least recently used first out).  Needs stable pointers (pre-allocated outputs); a call that
 * is profiled, tapped or split into sub-batches runs directly.  on = 1 / 0 switches, on < 0 only queries; returns the number of
 * graph launches so far (>= 0) or a negative error. */
int gator_set_graph_replay(gator_ctx* ctx, int32_t on);

/* Measurement hook (bench.py `roofline`): gator_profile_enable(ctx, n) with n >= 1 brackets every stage launch of every
 * n-th forward by a hipEvent pair recorded on the launch stream (n = 0 switches it off).  gator_profile_read synchronises those events and returns, per stage name
 * ('\n'-separated in `names`), the summed duration in ms and the number of launches since the last enable/read. */
int gator_profile_enable(gator_ctx* ctx, int32_t on);
int gator_profile_read(gator_ctx* ctx, char* names, int64_t names_capacity, float* total_ms, int32_t* calls,
                       int32_t max_entries, int32_t* n_entries);

/* "Next" row 8(f)-1: J_regressor @ verts (lib/core/base.py:221, demo/run.py:142) as a sparse product.
 *   coo_{row,col,val}: nnz entries of a [n_joint,6890] regressor (device); joints [B,n_joint,3]. */
int gator_regress_joints_f32(const float* verts, int32_t batch, const int32_t* coo_row, const int32_t* coo_col,
                             const float* coo_val, int32_t nnz, int32_t n_joint, float* joints, void* stream);

/* The same regression FUSED into the forward: register a sparse regressor once (COO; host or device pointers), then
 * gator_forward_joints_f32 = GATOR.forward + J_regressor @ mesh in one go -- the vertex GEMM's epilogue forms the regressor's
 * partial products while the vertices are still in registers, a tiny kernel sums them in a fixed order (no atomics).
 *   joints [B,n_joint,3] f32 (metres, like the mesh; the reference scales by 1000 before regressing, lib/core/base.py:219-221),
 *   pose3d [B,J,3] (mm); verts [B,6890,3] or NULL: with NULL no vertex is ever written -- evaluation (lib/core/base.py:219-237,
 *   which copies every mesh to the host twice) then needs 12*n_joint bytes per sample instead of 82 680. */
int gator_set_joint_regressor(gator_ctx* ctx, const int32_t* coo_row, const int32_t* coo_col, const float* coo_val, int32_t nnz,
                              int32_t n_joint);
int gator_forward_joints_f32(gator_ctx* ctx, const float* pose2d, int32_t batch, float* joints, float* pose3d, float* verts, void* stream);

/* "Next" row 8(f)-3: the input contract in front of the path (demo/run.py:103-121,127-134, data/PW3D/dataset.py:168-183,241-250):
 *   joints [batch, num_joint_in, comps] raw 2D joints in pixels (comps >= 2: x, y[, score]); add_pelvis_neck != 0 appends
 *   pelvis = (joint 11 + joint 12)/2 and neck = (joint 5 + joint 6)/2 (COCO order); pose2d [batch, num_joint_out, 2] =
 *   per-sample per-axis (xy - mean) / std over the joints (population std) -- what the bbox/affine/normalise chain reduces
 *   to for rot = 0, flip = 0. */
int gator_preprocess_pose2d_f32(const float* joints, int32_t batch, int32_t num_joint_in, int32_t comps,
                                int32_t add_pelvis_neck, float* pose2d, void* stream);

/* The same contract WITHOUT the reduction: the reference's whole chain per sample (data/PW3D/dataset.py:236-250) -- tight bbox
 * (lib/coord_utils.py:21-39), process_bbox (:42-66), get_affine_transform with in-plane rotation rot_deg[b] (lib/aug_utils.py:140-173),
 * affine per joint, horizontal flip with left/right pairs when flip[b] != 0 (:31-38), /[res_w,res_h], standardisation.
 * valid[b] = 0 (and pose2d[b] = 0) where process_bbox returns None (a box under one pixel wide or high; the datasets drop such
 * samples).  rot_deg / flip / valid may be NULL (no rotation / no flip / not reported); res = (288, 384) in every reference config. */
int gator_preprocess_chain_f32(const float* joints, int32_t batch, int32_t num_joint_in, int32_t comps, int32_t add_pelvis_neck,
                               const float* rot_deg, const int32_t* flip, const int32_t* flip_pairs, int32_t n_pairs,
                               int32_t res_w, int32_t res_h, float* pose2d, int32_t* valid, void* stream);

/* "Next" row 8(f)-2: per-sample similarity (Procrustes) alignment of a onto b, [batch, n_points, 3] each
 * (rigid_transform_3D / rigid_align, lib/coord_utils.py:127-149: 3x3 SVD with the reflection fix, scale, translation);
 * the kernel under PA-MPJPE (data/PW3D/dataset.py:337-375). */
int gator_rigid_align_f32(const float* a, const float* b, int32_t batch, int32_t n_points, float* aligned, void* stream);

/* The demo's crop-space target (demo/run.py:124-127), batched, rot = 0 and no flip: get_bbox (lib/coord_utils.py:21-39),
 * process_bbox(bbox, box_aspect, box_scale) (:42-66), j2d_processing(joints, (crop_w, crop_h), bbox1, 0, 0, None) (lib/aug_utils.py:51-64).
 *   joints [batch, num_joint_in, comps] raw 2D joints in pixels; add_pelvis_neck as in gator_preprocess_pose2d_f32 (demo/run.py:103-121).
 *   joints_crop [batch, num_joint_out, 2] in crop pixels (not standardised); bbox [batch, 4] = bbox1 as (x, y, w, h);
 *   valid [batch] = 0 where process_bbox returns None, and joints_crop / bbox of that sample are 0.
 * The demo uses box_aspect 1.0, box_scale 1.25, crop 500 x 500. */
int gator_crop_joints_f32(const float* joints, int32_t batch, int32_t num_joint_in, int32_t comps, int32_t add_pelvis_neck,
                          float box_aspect, float box_scale, int32_t crop_w, int32_t crop_h, float* joints_crop, float* bbox,
                          int32_t* valid, void* stream);

/* The demo's camera fit (demo/run.py:123-164 with lib/models/project_net.py:6-17), one sample per lane, in one launch:
 * `steps` torch.optim.Adam steps (betas 0.9 / 0.999, eps 1e-8) of cam = (s, tx, ty) on nn.L1Loss between
 * (joints3d_xy + t) * s * r + r  (r = crop_size / 2)  and target, over the first n_fit joints of both.
 *   joints3d [batch, n_joint_in, 3] (metres, gator_forward_joints_f32's joints); target [batch, n_target_in, 2] (crop pixels,
 *   gator_crop_joints_f32's joints_crop); init [batch, 3]; all device pointers.
 *   Schedule (host arrays, 1..8 pairs): lrs[0] from the first step, then lrs[i] from 0-based step milestones[i] + 1 on, i.e. after the
 *   optimizer step at j == milestones[i] (the demo: {0, 500, 1000} / {0.1, 0.05, 0.001}; milestones[0] is ignored).  The per-step
 *   Adam factors are formed on the host in double, as torch does, and kept on the device for the process's life per schedule.
 *   cam [batch, 3]; loss [batch] or NULL: the mean L1 error in crop pixels at the final cam.
 *   bbox [batch, 4] (gator_crop_joints_f32's bbox) with orig_cam [batch, 4], or both NULL: orig_cam = (sx, sy, tx, ty) of
 *   convert_crop_cam_to_orig_img (demo/run.py:21-39) for an image img_w pixels wide and img_h high.  The demo's call site passes
 *   orig_img.shape[:2] (height, width) as (width, height) (demo/run.py:202,211,42-51); pass the true width and height here.
 * steps = 0 returns init.  A non-finite input gives NaN outputs for its own sample only (no device status). */
int gator_fit_camera_f32(const float* joints3d, int32_t batch, int32_t n_joint_in, const float* target, int32_t n_target_in,
                         int32_t n_fit, const float* init, int32_t crop_size, int32_t steps, const int32_t* milestones,
                         const double* lrs, int32_t n_schedule, const float* bbox, float img_w, float img_h, float* cam,
                         float* loss, float* orig_cam, void* stream);

/* The SMPL body-model layer (smplpytorch/pytorch/smpl_layer.py:65-158), batched, on the device: what every training dataset of the
 * reference calls at batch 1 on the CPU to build its target mesh (data/AMASS/dataset.py:182-213).  The model's arrays come from the
 * caller (the weights are licence-gated and are no part of this library); all six are HOST pointers, copied and packed at create:
 *     v_template [NV,3]   shapedirs [NV,3,NB] (may be NULL when NB = 0)   posedirs [NV,3,(NJ-1)*9]   weights [NV,NJ]
 *     j_regressor [NJ,NV] dense   parents int32 [NJ]: parents[j] < j for j >= 1, parents[0] is ignored (the model files hold 2^32-1)
 * Limits: NV >= 1, 2 <= NJ <= 32, 0 <= NB <= 16 (SMPL: 6890 / 24 / 10; MANO's 778 / 16 / 10 arrays are accepted as well).
 * struct_size = sizeof of the struct below.  Anything else is GATOR_EINVAL, decided on the host before any device work.  The ctx is
 * created on the current device; it owns the packed model and a workspace (the samples' coefficient rows and skinning transforms)
 * that grows only when a larger batch arrives. */
typedef struct gator_smpl gator_smpl;
typedef struct {
    int32_t struct_size, n_verts, n_joints, n_betas;
    const float* v_template;
    const float* shapedirs;
    const float* posedirs;
    const float* weights;
    const float* j_regressor;
    const int32_t* parents;
} gator_smpl_model;
int gator_smpl_create(const gator_smpl_model* model, gator_smpl** out);
int gator_smpl_destroy(gator_smpl* ctx);

/* pose [batch, NJ*3] axis-angle, betas [batch, NB] or NULL (the template shape), trans [batch, 3] or NULL -> verts [batch, NV, 3] and
 * joints [batch, NJ, 3], either may be NULL; device pointers.
 *     out = (layer output + trans - centre) * out_scale
 * trans in the layer's unit (metres), out_scale 1 or 1000 (the datasets' `*= 1000` after their translation); center_idx >= 0 subtracts
 * that joint from both outputs and goes with trans = NULL only (the layer centres when the whole batch's trans is numerically zero; here
 * the argument decides, not device data, so nothing synchronises); center_idx < 0: no centring.
 * Rodrigues as the layer has it: angle = |axisang + 1e-8|, normalised quaternion -- the all-zero pose is the identity, not NaN.
 * batch = 0 is a no-op.  A repeated call at a batch no larger than an earlier one allocates nothing, never synchronises the host and can
 * be captured into a graph.  A sample's result does not depend on the batch around it (bit for bit); a non-finite pose or beta makes
 * that sample's outputs non-finite and changes no other sample.  There is no device status. */
int gator_smpl_forward_f32(gator_smpl* ctx, const float* pose, const float* betas, const float* trans, int32_t batch,
                           int32_t center_idx, float out_scale, float* verts, float* joints, void* stream);

/* The backward of gator_smpl_forward_f32: the exact vector-Jacobian product at (pose, betas, trans), which are the forward's inputs with
 * the forward's center_idx / out_scale (and its argument checks).  grad_verts [batch, NV, 3] and grad_joints [batch, NJ, 3] are the
 * upstream gradients of the two outputs, either may be NULL (that output was not used: with grad_verts = NULL no per-vertex work is
 * done); grad_pose [batch, NJ*3], grad_betas [batch, NB] and grad_trans [batch, 3] are written, a NULL one is simply not computed.
 * Everything is recomputed from the inputs: the forward keeps nothing per vertex.  The mathematics and the kernels are stated once in
 * csrc/smpl_backward.hip.
 * GATOR_EINVAL with a reason, before any launch: what the forward refuses, and grad_verts = grad_joints = NULL.  batch = 0 is a no-op.
 * No host synchronisation and no float atomics; a repeated call at a batch no larger than an earlier one allocates nothing and can be
 * captured into a graph (the first call with grad_verts also builds the ctx's transposed basis and waits for the stream once).  Row b
 * of every output is the same bits whatever the batch around it and from run to run.  A non-finite
 * pose, beta, trans or upstream gradient of sample b makes sample b's three gradient rows NaN and changes no other row. */
int gator_smpl_backward_f32(gator_smpl* ctx, const float* pose, const float* betas, const float* trans, int32_t batch,
                            int32_t center_idx, float out_scale, const float* grad_verts, const float* grad_joints,
                            float* grad_pose, float* grad_betas, float* grad_trans, void* stream);

/* Test hook: the base of the ctx's workspace and the batch it holds (0 / NULL before the first forward). */
int gator_smpl_workspace(const gator_smpl* ctx, const void** base, int64_t* capacity);
/* Test hook, as the other handles' *_workspace: the bytes the ctx's grown blocks hold now (the forward's, the fit's and the backward's
 * workspaces, the backward's transposed basis) and the number of growths since create.  Either pointer may be NULL. */
int gator_smpl_workspace_bytes(const gator_smpl* ctx, int64_t* bytes, int64_t* allocations);

/* The inverse of the layer: a batched Levenberg-Marquardt fit of (pose [batch, NJ*3], betas [batch, NB], trans [batch, 3]) to target
 * vertices [batch, NV, 3] in the layer's unit, out_scale 1, no centring; device pointers.  The result is the UNCONSTRAINED least-squares
 * fit in vertex space: no pose or shape prior, no joint limits, no per-vertex weights, no 2D evidence.  Models with more than 4
 * influences per vertex are refused (GATOR_EUNSUPPORTED with a reason); the layer itself takes them.
 *   unknowns  P = 3 NJ + NB + 3: a world-frame rotation increment per joint, the betas, the translation;
 *   M         [J | r]^T [J | r] of width N = 32 ceil((P + 1) / 32) (96 for SMPL): H = M[:P,:P], g = M[:P,P], squared error M[P][P];
 *             the Jacobian, the damping schedule and the update are stated once in csrc/smpl_fit.hip.
 * gator_smpl_fit_f32: `iters` (1..256) steps from the given start (init_pose, init_betas, init_trans: NULL together or set together;
 *   the warm start of a video is the previous frame's result) or from zero pose, zero betas and trans = centroid(target) -
 *   centroid(v_template).  out_pose / out_betas / out_trans: the float32 state to feed back to gator_smpl_forward_f32; out_rms [batch]:
 *   the root mean square vertex distance of that state.  A fixed number of launches decided by the arguments: no host read, no early
 *   exit, capturable into a graph; a repeated call at a batch no larger than an earlier one allocates nothing.  A sample's result does
 *   not depend on the batch around it (bit for bit) and is the same from run to run; a non-finite target or start makes that sample's
 *   four outputs NaN and changes no other sample.
 * gator_smpl_fit_normal_f32: the stage entry, M at a given state: out_M [batch, N, N], of which the upper 32x32 tiles (every element
 *   [a][b] with a / 32 <= b / 32, so the whole upper triangle) are written and the rest is left alone.
 * gator_smpl_fit_width: P and N of the ctx's model (either pointer may be NULL).
 * GATOR_EINVAL with a reason, before any launch: a NULL ctx, target or output, iters outside 1..256, a partial init, batch < 0 or above
 * 65535.  batch = 0 is a no-op. */
int gator_smpl_fit_f32(gator_smpl* ctx, const float* target_verts, const float* init_pose, const float* init_betas, const float* init_trans,
                       int32_t batch, int32_t iters, float* out_pose, float* out_betas, float* out_trans, float* out_rms, void* stream);
int gator_smpl_fit_normal_f32(gator_smpl* ctx, const float* pose, const float* betas, const float* trans, const float* target_verts,
                              int32_t batch, float* out_M, void* stream);
int gator_smpl_fit_width(const gator_smpl* ctx, int32_t* P, int32_t* N);

/* Multi-GPU: samples are independent, the batch is sharded contiguously over one process per GPU, and the path's one
 * collective is the all-gather of the predicted vertices [B/N,6890,3] (+ pose3d [B/N,J,3]) over xGMI.  gator_amd/parallel.py issues
 * it through torch.distributed ("nccl" = RCCL); these entry points do the same on RCCL directly for hosts without torch:
 * rank 0 calls gator_comm_unique_id and hands the 128 bytes to every rank (any host-side channel), every rank calls
 * gator_comm_create on its device, then gator_allgather_verts per step (rank-major outputs: rank r's rows at r*batch_local).
 * librccl is resolved at run time (the copy already loaded in the process, e.g. PyTorch's, else the system one), never linked. */
#define GATOR_COMM_ID_BYTES 128
typedef struct gator_comm gator_comm;
int gator_comm_unique_id(uint8_t* id /* [GATOR_COMM_ID_BYTES] */);
int gator_comm_create(const uint8_t* id, int32_t rank, int32_t world_size, gator_comm** out);
int gator_comm_destroy(gator_comm* comm);
int gator_allgather_verts(gator_comm* comm, const float* verts_local, const float* pose3d_local /* or NULL */, int32_t batch_local,
                          int32_t num_joint, float* verts_all, float* pose3d_all /* or NULL */, void* stream);

/* Measurement helper (tools/contention_model.py): the memory traffic a rank's share of an all-gather causes on ITS device --
 * read `bytes` at src, write them `copies` times to dst (dst holds copies x bytes) -- from `n_workgroups` workgroups of 256 threads on `stream`,
 * i.e. a stand-in for RCCL's send / receive kernels at a given channel count, to be run beside the forward on a one-GPU box.  No reference counterpart. */
int gator_emulate_gather_traffic(const void* src, void* dst, int64_t bytes, int32_t copies, int32_t n_workgroups, void* stream);

/* Evaluation errors of a batch in ONE launch (data/PW3D/dataset.py:273-286 compute_both_err, :337-375 PA alignment):
 *   pred_joints [B,n_joint,3] (scaled by pred_scale, e.g. 1000 for metres -> mm, lib/core/base.py:219), target_joints [B,n_joint,3];
 *   eval_joints: n_eval joint indices (device) or NULL for all; root: the joint both sets are aligned to.
 *   errors [B,2]: per sample (MPJPE, PA-MPJPE) = mean joint distance after root alignment, resp. after the similarity alignment of
 *   the evaluation joints; the caller averages over samples (or all-reduces the sums: gator_amd.parallel, mode='eval'). */
int gator_joint_errors_f32(const float* pred_joints, const float* target_joints, int32_t batch, int32_t n_joint,
                           const int32_t* eval_joints, int32_t n_eval, int32_t root, float pred_scale, float* errors, void* stream);

/* Whole-mesh evaluation of a batch in ONE launch: what the datasets' `evaluate` (data/PW3D/dataset.py:322-375,
 * data/Human36M/dataset.py:515-600) and compute_both_err (data/PW3D/dataset.py:273-286, lib/core/base.py:219-223) take from the two
 * meshes on the host.  A regressor is a sparse [n_joint, n_verts] matrix as COO in DEVICE arrays; the struct itself is read on the
 * host at the call.  Entries may come in any order and duplicates add; a col is used as a raw vertex offset, so every col in
 * [0, n_verts) is the caller's contract (gator_amd.eval checks it), as for gator_regress_joints_f32.
 *   pred, target [batch, n_verts, 3], n_verts >= 3; each coordinate is multiplied by pred_scale / target_scale in float32 (1000 for
 *   metres -> mm, lib/core/base.py:219), everything after that is fp64.
 *   root_regressor with 1..64 joints, root in [0, n_joint): both meshes are aligned on their own regressed root joint (the 24-joint
 *   SMPL regressor with root 0 for `evaluate`, the H36M regressor with root 0 for compute_both_err).
 *   eval_regressor (1..64 joints) with eval_root, and eval_joints: n_eval = 3..32 joint indices (device), each in [0, n_joint), or NULL
 *   for all joints.  No evaluation regressor: eval_regressor = NULL, or nnz = 0 with three NULL arrays.
 *   errors [batch, 5], per sample:
 *     0  MPJPE of the evaluation joints, each set aligned on its own eval_root           (PW3D/dataset.py:364-373)
 *     1  PA-MPJPE of the same joints                                                     (:374-375)
 *     2  mean error of ALL root-regressor joints after root alignment, mpjpe_smpl        (:351-353)
 *     3  MPVPE, the mean over vertices of |(p - root_p) - (t - root_t)|                  (:356-358; compute_both_err :275,283)
 *     4  PA-MPVPE, the mean over vertices of |c R p + tr - t| with the similarity fit of all n_verts vertices
 *        (:360-361, which the reference leaves commented out; lib/coord_utils.py:127-149)
 *   Columns 0 and 1 are NaN without an evaluation regressor.  A non-finite coordinate makes the columns that depend on it NaN in its
 *   own sample; a prediction of zero variance has column 4 = NaN (c = 0 / 0, as numpy gives).  A sample's row does not depend on the
 *   batch around it, bit for bit.
 * Enqueues one kernel on `stream`: no allocation, no synchronisation, capturable into a graph.  GATOR_EINVAL, before any launch and
 * with `errors` untouched: a NULL mesh / errors / root_regressor, batch <= 0, n_verts < 3, n_joint outside 1..64, a root outside its
 * joints, nnz < 0, nnz > 0 with a NULL array, an evaluation count outside 3..32. */
typedef struct {
    const int32_t* row;
    const int32_t* col;
    const float* val;
    int32_t nnz, n_joint;
} gator_coo;
int gator_mesh_errors_f32(const float* pred, const float* target, int32_t batch, int32_t n_verts, float pred_scale, float target_scale,
                          const gator_coo* root_regressor, int32_t root, const gator_coo* eval_regressor, int32_t eval_root,
                          const int32_t* eval_joints, int32_t n_eval, float* errors, void* stream);

/* The per-video, temporal part of the evaluation (data/PW3D/dataset.py:383-415, commented out there but complete; gator_amd/csrc/temporal.hip).
 * The frames of n_videos videos lie one video after another; seg_start [n_videos + 1] (int64, DEVICE) holds each video's first frame and,
 * last, n_frames.  It must start at 0 and increase strictly (every video has a frame): the kernels use it as raw offsets, unchecked --
 * gator_amd.temporal builds it from checked lengths.
 *
 * gator_one_euro_f32: lib/smooth_utils.smooth_pose (a one-euro filter) along every channel of every video in ONE launch.
 *   x [n_frames, n_channels] float32; out the same shape, float64 (out_f64 != 0) or float32 (the float32 rounding of the float64 value;
 *   the state is always carried in fp64).  The recursion is lib/smooth_utils.py:27-46 step for step in fp64, t_e = dt at every step,
 *   no contracted multiply-add: for finite inputs the float64 output equals numpy's bit for bit.  smooth_pose itself has d_cutoff = 1, dt = 1.
 *   A non-finite input makes its own channel of its own video NaN from that frame on, as numpy does, and nothing else.
 *
 * gator_sequence_errors: two launches.
 *   pred [n_frames, n_eval, 3] float64 (pred_f64 != 0, e.g. gator_one_euro_f32's output) or float32; gt the same shape, float32;
 *   valid [n_frames] uint8 or NULL; 3 <= n_eval <= 32.  No root is subtracted: the caller passes root-aligned joints, as the reference does.
 *   rows [n_frames, 3] float64, per frame i of a video that ends before frame e:
 *     0  the acceleration error of the triple (i, i+1, i+2), mean over joints of |(p_i - 2 p_i+1 + p_i+2) - (g_i - 2 g_i+1 + g_i+2)|
 *        (lib/coord_utils.py:194-222); NaN when i + 2 >= e or one of the three frames is not valid
 *     1  mean over joints of |p_i - g_i|                                                   (:398)
 *     2  the same after the similarity fit of p_i onto g_i                                 (:400-403, lib/coord_utils.py:127-149)
 *   video_sums [n_videos, 6] float64: the sums of the three columns over the video's frames (column 0 over its non-NaN rows), the number
 *   of those rows, the number of frames, 0 -- summed in a fixed order.
 * Both enqueue on `stream` without allocation or synchronisation and use no atomics: the same input gives the same bits.
 * GATOR_EINVAL before any launch: a NULL array, a count < 1, more videos than frames, dt <= 0, n_eval outside 3..32. */
int gator_one_euro_f32(const float* x, const int64_t* seg_start, int64_t n_frames, int32_t n_videos, int32_t n_channels, double min_cutoff,
                       double beta, double d_cutoff, double dt, int32_t out_f64, void* out, void* stream);
int gator_sequence_errors(const void* pred, int32_t pred_f64, const float* gt, const uint8_t* valid, const int64_t* seg_start,
                          int64_t n_frames, int32_t n_videos, int32_t n_eval, double* rows, double* video_sums, void* stream);

/* Camera-frame training targets: the deterministic part of the datasets' __getitem__ around the SMPL layer, for a whole batch
 * (data/Human36M/dataset.py:254-309,339-407, data/AMASS/dataset.py:182-304; gator_amd/csrc/train_batch.hip, gator_amd.batch).  The
 * detector noise (lib/noise_utils.py) is not part of it.  All pointers are device pointers unless said otherwise; both calls enqueue one
 * kernel on `stream`, never allocate or synchronise, and can be captured into a graph; batch == 0 is GATOR_OK and launches nothing.
 *
 * gator_batch_prepare_f32, before the layer.  pose [batch, n_pose] (n_pose = 3 per joint), R [batch,3,3] row major or NULL, betas
 * [batch, n_betas] or NULL.  pose_out = pose with joint root_idx replaced by the rotation vector of R exp(root) (Human36M:267-274,
 * AMASS:188-196), computed in fp64 through the product's quaternion: angle in [0, pi], accurate near 0 and near pi.  A ZERO root vector
 * is the identity (the reference divides 0 / 0 there and yields NaN); a non-finite root or R makes that sample's root NaN and nothing
 * else.  With R == NULL the pose is copied bit for bit.  betas_out: a row with any |beta| > 3 becomes zeros (Human36M:265), any other
 * row is copied bit for bit.  pose_out == pose and betas_out == betas are allowed.  GATOR_EINVAL: a NULL pose / pose_out, betas without
 * betas_out, n_pose < 3 or no multiple of 3, root_idx outside the joints, batch < 0.
 *
 * gator_camera_targets_f32, after the layer, one workgroup per sample; fp64 throughout with one rounding per output; no atomics, a
 * sample's outputs are the same bits whatever the batch.  In the struct below:
 *   verts [batch, n_verts, 3], joints [batch, n_smpl_joints, 3]: the layer's outputs in metres, not translated (joints is read only with
 *     compensate_root); trans, cam_t [batch,3] in metres, each may be NULL (= 0); R [batch,3,3] or NULL.
 *   T = R trans + cam_t - root + R root with root = joints[root_idx] when compensate_root (Human36M:288-292), else trans + cam_t
 *     (AMASS:205-207); mesh_cam = (verts + T) * 1000.
 *   reg_h36m (1..64 joints), reg_coco (13..62 joints, or n_joint = 0 for none): COO over n_verts columns -- reg_*_n_verts states the
 *     width each was built for; a column inside it is the caller's contract, as for gator_mesh_errors_f32.  The coco set gets its
 *     pelvis (mean of joints 11, 12) and neck (mean of 5, 6) appended.  Jh = reg_h36m.n_joint; Jl = Jh (GATOR_LIFT_HUMAN36) or
 *     reg_coco.n_joint + 2 (GATOR_LIFT_COCO).
 *   focal, princpt [batch,2]: cam2pixel, x = X / Z * fx + cx (lib/coord_utils.py:104-109); Z = 0 gives the IEEE result.
 *   joint_cam [batch,Jh,3] in mm and joint_img [batch,Jh,2] or NULL: the dataset's own joints (Human3.6M has them).
 *   rot_deg [batch] float, flip [batch] int32, each may be NULL; flip_pairs [n_pairs,2] int32 (a pair outside the lift set is skipped).
 *   Outputs: mesh [batch,n_verts,3] = (mesh_cam - root_h) / 1000 with root_h = joint_cam[0] when given, else the regressed h36m[0];
 *     mesh == verts is allowed.  reg_pose3d [batch,Jh,3] = joint_cam - joint_cam[0] when given, else h36m - h36m[0].  lift_pose3d
 *     [batch,Jl,3]: the lift set relative to its root (coco: its pelvis) after j3d_processing (lib/aug_utils.py:67-83: about z by
 *     -rot_deg, then the pairs swapped and x negated).  joint_img_out [batch,Jl,2]: the lift set's pixels -- the dataset's joint_img
 *     passed through when given and the lift set is human36.  fit_error [batch]: get_fitting_error in mm (Human36M:302-309), NaN
 *     without joint_cam.  valid [batch,3] = (mesh, lift, reg): ones; fit_error > fitting_thr clears mesh, and lift too for coco.
 * GATOR_EINVAL with a text, before any launch: NULL args or a required pointer, struct_size not this header's, n_verts < 1, a
 * regressor's n_verts != n_verts, GATOR_LIFT_COCO without reg_coco, a coco regressor outside 13..62 joints, joint_cam without joint_img
 * for GATOR_LIFT_HUMAN36, compensate_root without R, root_idx outside [0, n_smpl_joints). */
#define GATOR_LIFT_HUMAN36 0
#define GATOR_LIFT_COCO 1
typedef struct {
    int32_t struct_size; /* = sizeof of this struct in the caller's header */
    int32_t batch, n_verts, n_smpl_joints, root_idx;
    int32_t compensate_root, lift_set, n_pairs;
    int32_t reg_h36m_n_verts, reg_coco_n_verts;
    float fitting_thr;
    int32_t reserved;
    const float *verts, *joints, *trans, *cam_t, *R, *focal, *princpt;
    gator_coo reg_h36m, reg_coco;
    const float *joint_cam, *joint_img;
    const float* rot_deg;
    const int32_t* flip;
    const int32_t* flip_pairs;
    float *mesh, *reg_pose3d, *lift_pose3d, *joint_img_out, *fit_error, *valid;
} gator_camera_targets_args;
int gator_batch_prepare_f32(const float* pose, const float* R, const float* betas, int32_t batch, int32_t n_pose, int32_t n_betas,
                            int32_t root_idx, float* pose_out, float* betas_out, void* stream);
int gator_camera_targets_f32(const gator_camera_targets_args* args, void* stream);

/* The training input with the detector's errors on it (use_gt_input: False, every *_train_*.yml of the reference): the input chain of
 * gator_preprocess_chain_f32 with the datasets' replace_joint_img step in its place (data/Human36M/dataset.py:369-389, 421-453) --
 * tight box -> process_bbox -> crop affine with rotation -> float32 crop joints -> NOISE in crop pixels -> flip_2d_joint on the
 * float32 joints -> /[W,H] -> standardise.  gator_amd/csrc/detector_noise.hip; gator_amd.noise; DESIGN.md "Detector noise".
 *
 * mode GATOR_NOISE_COCO: lib/noise_utils.synthesize_pose on joints 0..16 (n_joints >= 17; later rows, the pelvis and neck of a 19-joint
 *   input, keep their clean values), with `area` = the product of the side lengths of the tight box's corners after the affine
 *   (dataset.py:425-431).  It is the reference's algorithm candidate for candidate -- per joint 500 jitter, 2000 miss around each
 *   centre, 500 inversion and 125 good candidates (the model's n_* fields), accepted under the reference's distance masks, the k-th
 *   accepted one taken, one of the five cases chosen with the tier's probabilities renormalised over the cases that found a point --
 *   with numpy's generators replaced by the stream below.  near_joints is empty and num_overlap 0 as at every call site: no swap case.
 *   A joint's centres are its own current position and, when it has a partner whose joint_valid > 0, the partner's current position:
 *   the lower joint of a pair is perturbed first and the higher one sees the perturbed (possibly zeroed) lower one.  Invalid joints are
 *   perturbed too; the number of valid joints among 0..16 picks the tier.  A joint whose cases all come up empty becomes (0, 0).
 *   fp64 throughout, no contracted multiply-add; the chosen point is rounded to float32 once, when it is stored.
 * mode GATOR_NOISE_STATS: generate_syn_error (dataset.py:143-155, 440-446) from stats [n_joints,5] float64 = (mean x, mean y, std x,
 *   std y, weight) per joint: noise = float32(mean + std z), z by Box-Muller (z_x = sqrt(-2 ln u1) cos(2 pi u2), z_y = .. sin ..),
 *   applied where float32(weight) > u3, as float32: crop + noise / 256 * [W, H].
 * mode GATOR_NOISE_DETECTIONS: the test split's branch: `detections` [batch, n_joints, comps] (a detector's joints in image pixels)
 *   go through the affine of the box of `joints` in their place.  Nothing is drawn.
 *
 * The stream.  Key = seed.  The word of draw site (set, joint j, index i) of sample b is output word k of the Philox4x32 block
 * (GATOR_PHILOX_ROUNDS = 7 rounds, the dropout masks' generator) with the counter
 *     c0 = i,   c1 = j | set << 8,   c2 = low 32 bits of (sample_offset + b),   c3 = low 32 bits of step
 * and a uniform is (word + 0.5) * 2^-32 in fp64, an index into n items (word * n) >> 32 in 64-bit integers.  Sets:
 *     0 jitter, 1 miss around the joint, 2 miss around the partner, 3 inversion, 4 good:  candidate i, word 0 -> angle = 2 pi u,
 *                                                                                         word 1 -> r = lo + (hi - lo) u
 *     5 picks:  i = 0: words 0..3 -> the index among the accepted jitter / miss (n_miss0 + n_miss1 / 4 entries) / inversion / good
 *               points;  i = 1: word 0 -> the case (numpy's choice: the normalised cumulative sum searched from the right)
 *     6 the reference's resampled quarter of the partner's miss points:  entry i of that list, word 0 -> an index into the n_miss1 points
 *     7 stats:  i = 0: words 0, 1 -> u1, u2 of Box-Muller, word 2 -> u3
 * A sample's row depends on (seed, step, sample_offset + b) and its own inputs only: the same bits whatever the batch or its sharding.
 * step_dev (DEVICE int64, or NULL) replaces `step` when given: a captured graph draws fresh noise per replay when the caller advances it.
 *
 * All array pointers are device pointers; `coco` is a HOST pointer, copied at the call.  joints [batch, n_joints, comps] float32, image
 * pixels (x and y first); joint_valid [batch, n_joints] float32 or NULL (all valid); rot_deg [batch], flip [batch] int32, each may be
 * NULL; flip_pairs [n_pairs,2] int32 (a pair beyond n_joints is skipped).  Outputs: pose2d [batch, n_joints, 2]; valid [batch] int32 (0
 * where process_bbox rejects the box: that sample's pose2d and noisy_crop are zeros); noisy_crop [batch, n_joints, 2] float32, the
 * perturbed joints in crop pixels before the flip; area [batch] float64 (required for GATOR_NOISE_COCO, else may be NULL); decisions
 * [batch,17,8] int32 or NULL (GATOR_NOISE_COCO): the accepted counts of sets 0..4, the case (0 jitter, 1 miss, 2 inversion, 4 good, -1
 * zeroed), the picked index, and for a miss taken from the partner's points the index into them (else -1).
 * Two launches (three for GATOR_NOISE_COCO) on `stream`; no allocation, no synchronisation, no atomics; capturable.  batch == 0 is
 * GATOR_OK.  GATOR_EINVAL with a text, before any launch: NULL args or a required pointer, struct_size not this header's, n_joints
 * outside 1..32, comps < 2, a resolution < 1, an unknown mode, GATOR_NOISE_COCO with fewer than 17 joints, without model or area, or with
 * a model whose partner table is no involution inside 0..16 or whose counts lie outside 1..2^20, GATOR_NOISE_STATS without stats,
 * GATOR_NOISE_DETECTIONS without detections, sample_offset < 0 or sample_offset + batch > 2^32. */
#define GATOR_NOISE_COCO 0
#define GATOR_NOISE_STATS 1
#define GATOR_NOISE_DETECTIONS 2
#define GATOR_NOISE_COCO_JOINTS 17
typedef struct {                     /* the rule table of synthesize_pose, as data (gator_amd.noise.CocoDetectorNoise fills it) */
    double var[GATOR_NOISE_COCO_JOINTS];            /* (2 sigma_j)^2 */
    double log_ks[3];                               /* log(0.10), log(0.50), log(0.85): dist = sqrt(-2 area var log_ks) */
    double jitter_prob[2][GATOR_NOISE_COCO_JOINTS]; /* n_valid <= tier_valid[1], else */
    double miss_prob[3][GATOR_NOISE_COCO_JOINTS];   /* n_valid <= tier_valid[0], <= tier_valid[1], else */
    double inv_prob[GATOR_NOISE_COCO_JOINTS];
    int32_t partner[GATOR_NOISE_COCO_JOINTS];       /* the symmetric joint, -1 for none */
    int32_t n_jitter, n_miss, n_inv, n_good;        /* candidates per set */
    int32_t tier_valid[2];                          /* 5, 10 */
    int32_t reserved;
} gator_coco_noise_model;
typedef struct {
    int32_t struct_size; /* = sizeof of this struct in the caller's header */
    int32_t batch, n_joints, comps, mode, n_pairs, res_w, res_h;
    uint64_t seed;
    int64_t step, sample_offset;
    const int64_t* step_dev;
    const float *joints, *joint_valid, *detections, *rot_deg;
    const int32_t *flip, *flip_pairs;
    const gator_coco_noise_model* coco; /* HOST */
    const double* stats;
    float* pose2d;
    int32_t* valid;
    float* noisy_crop;
    double* area;
    int32_t* decisions;
} gator_preprocess_noise_args;
int gator_preprocess_noise_f32(const gator_preprocess_noise_args* args, void* stream);

/* The demo's mesh overlay (demo/renderer.py) on the device: a batched software rasteriser for the weak-perspective camera
 * (gator_amd/csrc/render.hip derives the geometry; DESIGN.md "Renderer").  For a vertex (x, y, z) of the model's output and
 * cam = (sx, sy, tx, ty):  column = (1 + sx (x + tx)) / 2 * W,  row = (1 + sy (y + ty)) / 2 * H,  depth = z (smaller is nearer, fragments
 * outside [-1, 1] are clipped), sampled at pixel centres; rot3x3 (HOST, row major, or NULL = identity) is the reference's `rotate` /
 * `angle, axis` matrix, applied to the mesh after its Rx(180 deg) flip as the reference applies it.
 *
 * gator_renderer_create: faces [n_faces,3] on the HOST.  GATOR_EINVAL with a reason for a vertex index outside [0, n_verts),
 * n_faces < 1, n_verts < 3.  Builds the vertex-to-face lists, uploads both, and owns every allocation until gator_renderer_destroy.
 *
 * gator_render_f32: n_meshes meshes verts [n_meshes,n_verts,3] with cams [n_meshes,4] and colors [n_meshes,3] (linear base colour; NULL:
 * (1, 1, 0.9)), all on the device, drawn into n_images images of H x W.  image_index [n_meshes] on the HOST names the image of each
 * mesh: several meshes of one image share its depth buffer; NULL: mesh m alone in image m (needs n_meshes <= n_images).
 * background [n_images,H,W,3] uint8 on the device or NULL (black).  lights: n_lights <= 4 HOST rows (lx, ly, lz, intensity), the unit
 * direction TOWARDS the light in the model's output coordinates; shading is lin = base (ambient + (1/pi) sum_k I_k max(0, n . l_k)),
 * out = round(255 clamp(lin^(1/2.2))) -- a documented diffuse model, not pyrender's shader.  flags: GATOR_RENDER_CULL_BACKFACES.
 * Outputs (device, each may be NULL, not all): out_rgb [n_images,H,W,3] uint8; out_face_id [n_images,H,W] int32 = slot * n_faces + face
 * with slot the rank of the winning mesh among the meshes of its image, -1 where empty; out_depth [n_images,H,W] f32, +Inf where empty.
 * An image is the same bits from run to run and whatever else is in the batch (integer atomic min on (depth, id) keys).
 * A vertex that is not finite or projects beyond +-2^20 px drops every face that touches it.  Workspace grows inside the handle (the
 * device is synchronised when a block is replaced); a call no larger than an earlier one allocates nothing; a growth that fails leaves the handle
 * usable for smaller calls.  image_index is read before the call returns (into a pinned block of the handle, copied on `stream`).  The
 * calls on one handle are ordered by the caller: one stream, or events between streams.
 * GATOR_EINVAL, before any launch: a NULL handle / verts / cams, no output, H or W outside 1..8192, n_meshes or n_images < 1,
 * n_meshes > 65535, an image_index[m] outside [0, n_images), (most meshes in one image) * n_faces >= 2^32 (2^31 with out_face_id),
 * more than 4 lights, a non-finite light, ambient or rot3x3 entry.
 *
 * The three launches alone, for callers that keep the intermediates (and for the tests):
 *   gator_render_vertices_f32 -> xy_fixed [n_meshes,n_verts,2] int32 (24.8 fixed point, round to nearest even; INT32_MIN for a dropped
 *                                vertex), z [n_meshes,n_verts] (without a rotation the input's z bit for bit, except that -0 becomes +0 and that z
 *                                is NaN where x or y is not finite -- a dropped vertex), normals [n_meshes,n_verts,3] (area-weighted, unit length)
 *   gator_render_raster       -> keys [n_images,H,W] uint64: ordered_bits(depth) << 32 | face id, all ones where empty
 *   gator_render_resolve      -> the outputs of gator_render_f32 from those */
#define GATOR_RENDER_CULL_BACKFACES 1
typedef struct gator_renderer gator_renderer;
int gator_renderer_create(const int32_t* faces, int32_t n_faces, int32_t n_verts, gator_renderer** out);
int gator_renderer_destroy(gator_renderer* r);
int gator_render_f32(gator_renderer* r, const float* verts, const float* cams, const float* colors, const int32_t* image_index,
                     int32_t n_meshes, const uint8_t* background, int32_t n_images, int32_t H, int32_t W, const float* rot3x3,
                     const float* lights, int32_t n_lights, float ambient, int32_t flags, uint8_t* out_rgb, int32_t* out_face_id,
                     float* out_depth, void* stream);
int gator_render_vertices_f32(gator_renderer* r, const float* verts, const float* cams, int32_t n_meshes, int32_t H, int32_t W,
                              const float* rot3x3, int32_t* xy_fixed, float* z, float* normals, void* stream);
int gator_render_raster(gator_renderer* r, const int32_t* xy_fixed, const float* z, const int32_t* image_index, int32_t n_meshes,
                        int32_t n_images, int32_t H, int32_t W, int32_t flags, uint64_t* keys, void* stream);
int gator_render_resolve(gator_renderer* r, const uint64_t* keys, const int32_t* xy_fixed, const float* normals, const float* colors,
                         const int32_t* image_index, int32_t n_meshes, const uint8_t* background, int32_t n_images, int32_t H, int32_t W,
                         const float* lights, int32_t n_lights, float ambient, uint8_t* out_rgb, int32_t* out_face_id, float* out_depth,
                         void* stream);
/* Test hook: bytes of workspace the handle holds and how many allocations it has made since create. */
int gator_renderer_workspace(const gator_renderer* r, int64_t* bytes, int64_t* allocations);
/* Measurement hook (tools/render_bench.py): bounding-box area in pixels up to which one lane walks a triangle alone; 0 = built-in. */
int gator_renderer_set_small_box(gator_renderer* r, int32_t pixels);

/* The demo's 2D pose overlay (lib/vis.py: vis_2d_keypoints, vis_coco_skeleton) on the device: an ordered, anti-aliased composite of
 * capsules (cv2.line), discs and rings (cv2.circle) into uint8 frames (gator_amd/csrc/draw2d.hip states the primitive model, the blend
 * and the final mix; tests/draw_refs.py is the same rule in numpy and the device agrees with it byte for byte).
 * Byte parity with OpenCV's LINE_AA is not claimed: the documented rule is the contract.
 *
 * gator_draw2d_create: skeleton [n_limbs,2] joint index pairs on the HOST.  GATOR_EINVAL with a reason for a NULL argument, n_limbs
 * outside 1..4096, n_joints < 1, a joint index outside 0..n_joints-1.
 *
 * gator_draw2d_u8 draws n_people skeletons into n_images frames of H x W.  Device pointers: joints [n_people,n_joints,joint_dim]
 * float32 pixels, joint_dim = 2 (x, y) or 3 (x, y, confidence); colors [n_limbs,3] float32 in the image's channel order on the 0..255
 * scale; bbox [n_people,4,2] float32 corners or NULL; images and out [n_images,H,W,3] uint8, out == images draws in place (no other
 * overlap).  image_index [n_people] on the HOST names the frame of each person, people of one frame are drawn in person order; NULL:
 * person p alone in frame p (needs n_people <= n_images; later frames are copied).  kp_thre: with joint_dim == 3 a limb's line needs
 * both joints' confidence > kp_thre and a joint's mark its own; ignored when joint_dim == 2.  A primitive with a non-finite coordinate
 * is skipped; coordinates are truncated towards zero and clamped to +-2^20.  alpha in [0, 1]: out = img (1 - alpha) + canvas alpha,
 * rounded half to even in float32; 1 returns the canvas.  style GATOR_DRAW_KEYPOINTS: lines of thickness 2, filled discs of radius 3,
 * colors[l] per limb (vis_2d_keypoints); GATOR_DRAW_COCO: lines of thickness 2, rings of radius 2 and thickness 3 (vis_coco_skeleton,
 * which passes one colour for every limb and joints without confidence).
 * Two launches on `stream`, no atomics, no host synchronisation; the same bytes from run to run and whatever else is in the batch.  The
 * primitive records live in the handle and grow when a larger call arrives (the device is synchronised when a block is replaced); a call no larger
 * than an earlier one allocates nothing and, with image_index NULL, is capturable into a graph.  image_index is read before the call
 * returns.  The calls on one handle are ordered by the caller.
 * GATOR_EINVAL naming the field, before any launch: a NULL handle, args, joints, colors, images or out; struct_size smaller than this
 * struct; H or W outside 1..8192; n_people < 1; n_images outside 1..65535; joint_dim not 2 or 3; an unknown style; alpha outside [0, 1]
 * or NaN; an image_index[p] outside 0..n_images-1; image_index NULL with n_people > n_images. */
#define GATOR_DRAW_KEYPOINTS 0
#define GATOR_DRAW_COCO 1
typedef struct gator_draw2d gator_draw2d;
typedef struct {
    int32_t struct_size; /* = sizeof of this struct in the caller's header */
    int32_t n_people, n_images, H, W, joint_dim, style;
    float kp_thre, alpha;
    int32_t reserved;
    const float *joints, *colors, *bbox;
    const uint8_t* images;
    uint8_t* out;
    const int32_t* image_index; /* HOST */
} gator_draw2d_args;
int gator_draw2d_create(const int32_t* skeleton, int32_t n_limbs, int32_t n_joints, gator_draw2d** out);
int gator_draw2d_destroy(gator_draw2d* d);
int gator_draw2d_u8(gator_draw2d* d, const gator_draw2d_args* args, void* stream);
/* Test hook: bytes of workspace the handle holds and how many allocations it has made since create. */
int gator_draw2d_workspace(const gator_draw2d* d, int64_t* bytes, int64_t* allocations);
/* Measurement and test hook (tools/draw_bench.py): the tile kernel has two forms that write the same bytes, 64 x 4 pixel tiles with one
 * pixel a thread (rows = 1) and 64 x 16 tiles with four (rows = 4); 0 = the built-in choice by the size of the grid. */
int gator_draw2d_set_tile_rows(gator_draw2d* d, int32_t rows);

/* Host-side graph constants (no GPU needed).  Replace the absent Cython algos.pyx
 * (lib/models/backbones/setup.py:1-6) and lib/models/backbones/modules.py:6-29, lib/graph_utils.py:71-89. */
int gator_floyd_warshall(const float* adj, int32_t n, int64_t* dist, int64_t* path);
int gator_gen_edge_input(const int64_t* path, const float* edge_len, int32_t n, int32_t max_dist, float* out);
int gator_verts_joints_relation(const float* joints, int32_t n_joint, const float* verts, int32_t n_vert, int32_t* rel);

const char* gator_last_error(void);
const char* gator_version(void);
int gator_abi_version(void);      /* GATOR_ABI_VERSION of the library that is loaded */

#ifdef __cplusplus
}
#endif
#endif /* GATOR_HIP_H */
