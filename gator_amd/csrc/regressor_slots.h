// Where an operand element of the vertex regressor lives: the contract between whoever writes a packed operand (the pack kernel of
// upsample_common.h; the MDR head in mdr_head.hip, which restates the three activation layouts by hand because its kernels' listings
// move on any other wording -- tests/host_regressor_slots.cpp and test_forward_packer hold it to this file) and the four kernels that
// read it (upsample_*.hip).  Plain C++, nothing of HIP, so
// that tests/host_regressor_slots.cpp builds it alone.  A slot is the element index of plane 0; further planes follow at the layout's
// plane stride.  Coordinates: b sample, v coarse vertex (0..447, 431 real), lp input position (xyz of the input), o output vertex
// (0..6911, 6890 real), tap of the 3-tap convolution.  Every layout is built from 64-lane MFMA operand fragments: lane = 32 h + row.
#pragma once
#include <cstddef>

#ifndef GATOR_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GATOR_HD __host__ __device__
#else
#define GATOR_HD
#endif
#endif

namespace gator {

constexpr int kOB = 216;                // 32-vertex output blocks of the upsample GEMM (6890 -> 6912)
constexpr int kCB = 14;                 // 32-wide k blocks over the 431 coarse vertices
constexpr int kS16 = 28;                // 16-deep k-steps over the 431 (-> 448) coarse vertices
constexpr int kRegK = 16 * kS16;        // the padded k extent, 448 (= 32 kCB)

// element of a 16-deep fragment [lane 64][8]: k index k = 8 h + j on lane 32 h + row
GATOR_HD inline size_t frag16(int row, int k) { return (size_t)(((k >> 3) & 1) * 32 + row) * 8 + (k & 7); }

// two fp16 planes (upsample_x2.hip): activations [mt / 4][s][mt % 4][lp 3][plane 2][64][8], weights [ob / 2][s][ob % 2][tap 3][plane 2][64][8]
constexpr size_t kX2Plane = 512;
GATOR_HD inline size_t act_slot_x2(int b, int v, int lp) {
    const int mt = b >> 5;
    return ((((size_t)(mt >> 2) * kS16 + (v >> 4)) * 4 + (mt & 3)) * 3 + lp) * 2 * kX2Plane + frag16(b & 31, v);
}
GATOR_HD inline size_t w_slot_x2(int o, int c, int tap) {
    const int ob = o >> 5;
    return ((((size_t)(ob >> 1) * kS16 + (c >> 4)) * 2 + (ob & 1)) * 3 + tap) * 2 * kX2Plane + frag16(o & 31, c);
}
// bf16 planes (upsample_x3.hip: three, upsample_bf16.hip: one): activations [plane][mt][lp 3][s][64][8], weights [plane][tap 3][ob][s][64][8].
// The activation planes of the three-plane form are strided by the workspace CAPACITY (upsample_x3_vcp_elems(cap) / 3), not by the batch.
GATOR_HD inline size_t act_slot_b16(int b, int v, int lp) { return (((size_t)(b >> 5) * 3 + lp) * kS16 + (v >> 4)) * 512 + frag16(b & 31, v); }
GATOR_HD inline size_t w_slot_b16(int o, int c, int tap) { return (((size_t)tap * kOB + (o >> 5)) * kS16 + (c >> 4)) * 512 + frag16(o & 31, c); }
// fp32 tiles (upsample_fused.hip): activations [mt][lp 3][cb][g 4][64][4], k index 8 g + 4 h + j on lane 32 h + row; the weights are fused_pack_linear's [tap][ob][cb] tile grids
GATOR_HD inline size_t act_slot_f32(int b, int v, int lp) {
    return ((((size_t)(b >> 5) * 3 + lp) * kCB + (v >> 5)) * 4 + ((v & 31) >> 3)) * 256 + (size_t)(((v & 7) >> 2) * 32 + (b & 31)) * 4 + (v & 3);
}

// sizes in elements, all planes
GATOR_HD inline size_t upsample_x2_weight_elems() { return (size_t)(kOB / 2) * kS16 * 2 * 3 * 2 * kX2Plane; }
GATOR_HD inline size_t upsample_x2_vcp_elems(int B) { return (size_t)((B + 127) / 128) * kS16 * 4 * 3 * 2 * kX2Plane; }
GATOR_HD inline size_t upsample_bf16_weight_elems() { return (size_t)3 * kOB * kS16 * 512; }
GATOR_HD inline size_t upsample_bf16_vcp_elems(int B) { return (size_t)((B + 31) / 32) * 3 * kS16 * 512; }
GATOR_HD inline size_t upsample_x3_weight_elems() { return 3 * upsample_bf16_weight_elems(); }
GATOR_HD inline size_t upsample_x3_vcp_elems(int B) { return 3 * upsample_bf16_vcp_elems(B); }
GATOR_HD inline size_t upsample_f32_vcp_elems(int B) { return (size_t)((B + 31) / 32) * 3 * kCB * 1024; }

// The taps of the convolution (MDR.py:167, padding 1): input position lp meets tap k for output l = lp + 1 - k; the two padding taps
// of the outer positions are never multiplied.  Grouped by input position, taps descending, so every output sees tap order 0, 1, 2.
struct RegTap { int lp, k, l; };
constexpr RegTap kRegTaps[7] = {{0, 1, 0}, {0, 0, 1}, {1, 2, 0}, {1, 1, 1}, {1, 0, 2}, {2, 2, 1}, {2, 1, 2}};

}  // namespace gator
