// The demo's 2D pose overlay (lib/vis.py: vis_2d_keypoints, vis_coco_skeleton) on the device: a batched, ordered, anti-aliased
// line / disc / ring rasteriser over uint8 frames, two launches.  tests/draw_refs.py restates this comment in numpy; every byte is to
// agree with it.
//
// Primitive model.  Pixel centres sit on integer coordinates.  A joint's float32 coordinate is truncated towards zero (the reference's
// astype(np.int32)) and clamped to +-2^20, so a difference is below 2^22, a product below 2^44 and every sum of two below 2^53: all
// integers here are exact in int64 AND in float64.  Three kinds, d = distance from the pixel centre p, in float64:
//     capsule (a, b, thickness t)   cv2.line        h = t / 2,  cov = clamp((h + 0.5) - d, 0, 1), d to the segment:
//                                                   dot = (b - a).(p - a);  dot <= 0: d = sqrt(|p - a|^2);  dot >= |b - a|^2: d = sqrt(|p - b|^2);
//                                                   else d = |(b - a) x (p - a)| / sqrt(|b - a|^2).  a == b is the disc of radius h (dot = 0).
//     disc (c, radius r)            cv2.circle -1   cov = clamp((r + 0.5) - d, 0, 1),  d = sqrt(|p - c|^2)
//     ring (c, radius r, t)         cv2.circle t    cov = clamp((t / 2 + 0.5) - |d - r|, 0, 1)
// The squares, the dot and the cross product are int64; sqrt, the division, the subtractions and 255 cov + 0.5 are single correctly
// rounded float64 operations (the library is built with -ffp-contract=off and without fast-math).  q = floor(255 cov + 0.5), 0..255.
// Blend, per channel in int32, as soon as a primitive is drawn:  dst = (dst (255 - q) + c8 q + 127) / 255, c8 = the colour rounded
// half-to-even and clamped to 0..255 (NaN: 0).  q = 0 leaves dst as it was, so a primitive's footprint box is only a shortcut.
// Order: per person, the box (4 capsules, thickness 1, colour (255, 255, 0)), then per limb: line, mark at p1, mark at p2; people of one
// image in person order; later primitives lie on top.  A primitive with a non-finite coordinate is skipped; with joint_dim == 3 the
// line needs both joints' confidence > kp_thre and a mark its own joint's (vis_2d_keypoints' three ifs).
// Final mix (cv2.addWeighted(img, 1 - alpha, canvas, alpha, 0)), float32: out = clamp(rne(img * (1 - alpha) + canvas * alpha)), two
// products and one sum, 1 - alpha formed in float32 on the host.  alpha lies in [0, 1]: then a pixel whose canvas equals its source
// keeps its value (the error of the sum is below 255 * 2^-22), so untouched tiles are copied, and alpha == 1 is the canvas.
//
//   k_draw_build : one thread per (person, limb), one more per person for the box.  Writes the primitive records: kind, end points,
//                  radius / thickness, c8, and the inclusive box of the footprint (cov > 0 needs d < extent + 0.5, and d >= the
//                  distance from the end points' box along either axis: the box grows by t / 2 (integer), r, or r + t / 2).
//   k_draw_tiles : one workgroup of 256 threads per tile, grid (tiles, images).  A frame is [H,W,3] uint8, a row 3 W bytes, 4-byte
//                  aligned only when W is a multiple of 4, which rules out dword access; so a wave's access is 64 pixels of ONE row, 192
//                  contiguous bytes: its three byte loads and stores per lane fall into two or three cache lines whatever W is, and
//                  the footprint test of a primitive's rows is uniform in a wave.  A narrower tile would cut that span into several
//                  shorter ones.  Two forms of the one kernel, the same bytes: ROWS = 1, a tile of 64 x 4 and one pixel a thread, and
//                  ROWS = kTallRows, a tile of 64 x 16 where a thread owns its column's pixels in rows wave, wave + 4, wave + 8, wave + 12.
//                  The tall form has a quarter of the workgroups and record scans but four times the dependent work in a tile that is
//                  drawn on: it wins once the one-row form's grid is large (kTallTileFrom workgroups; profiles/draw2d.txt has both
//                  forms at every shape).  The workgroup takes the image's records 256 at a time, 64 per wave, tests
//                  footprint against tile and appends the survivors' indices IN ORDER to an LDS list: ballot, the count of the lanes
//                  below, the counts of the waves below.  When the list is full (kListCap) every pixel walks it in order, its three
//                  channels in registers, and the list starts again with the rest of the chunk: no cap on the primitives of an image.
//                  A pixel reads only its own source pixel, so out may alias images; a tile nothing touches is copied (not at all when
//                  they alias).  Lanes outside the frame take part in the ballots and barriers and touch no memory.
// No atomics, no host synchronisation; an image's bytes do not depend on what else is in the batch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "handle.h"

namespace gator {
namespace {

constexpr int kTileW = 64, kTileH = 4;          // the one-row form: a wave per row of the tile (header comment)
constexpr int kTallRows = 4;                    // the tall form: kTallRows rows a thread, a tile of kTileW x (kTileH * kTallRows)
constexpr int kTallTileFrom = 24576;            // workgroups of the one-row form from which the tall form is launched (profiles/draw2d.txt)
constexpr int kListCap = 1024;                  // entries of the LDS list (4 KiB); at least 256, so that one chunk of records refills it at most once
constexpr int kMaxSide = 8192;
constexpr int kMaxLimbs = 4096;
constexpr double kGuard = 1048576.0;            // 2^20
enum Kind { kSkip = 0, kCapsule = 1, kDisc = 2, kRing = 3 };

struct Prim {          // 48 bytes: three 16-byte loads
    int32_t kind, ax, ay, bx;
    int32_t by, r, t, c8;      // c8 = channel 0 | channel 1 << 8 | channel 2 << 16
    int32_t x0, y0, x1, y1;    // inclusive footprint; empty (x0 > x1) for a skip record
};
static_assert(sizeof(Prim) == 48, "Prim is three int4");

struct Tables { const int32_t *img_off, *person_of; };      // both NULL: person p alone in image p

}  // namespace
}  // namespace gator

struct gator_draw2d : gator::Handle {
    int L = 0, J = 0;
    int rows = 0;                                 // gator_draw2d_set_tile_rows: 0 = the built-in choice
    gator::DevBuf<int32_t> skeleton;              // [L][2]
    // workspace, grown when a larger call arrives (gator::Handle::grow)
    gator::WorkBuf<gator::Prim> recs;             // [P][records per person]
    gator::StagedTable<int32_t> tab;              // img_off [N+1] | person_of [P]
};

namespace gator {
namespace {

__device__ __forceinline__ bool to_pixel(float v, int32_t& o) {      // astype(np.int32) of a finite value, clamped to +-2^20
    if (!isfinite(v)) { o = 0; return false; }
    o = (int32_t)fmin(fmax((double)v, -kGuard), kGuard);             // the cast truncates towards zero
    return true;
}

__device__ __forceinline__ int32_t to_c8(float c) {                  // half-to-even, clamped; fmaxf(NaN, 0) = 0
    return (int32_t)fminf(fmaxf(rintf(c), 0.f), 255.f);
}

__device__ __forceinline__ Prim make_prim(bool ok, int kind, int ax, int ay, int bx, int by, int r, int t, int32_t c8, int grow) {
    Prim p;
    p.kind = ok ? kind : kSkip;
    p.ax = ax; p.ay = ay; p.bx = bx; p.by = by; p.r = r; p.t = t; p.c8 = c8;
    p.x0 = ok ? min(ax, bx) - grow : 1; p.x1 = ok ? max(ax, bx) + grow : 0;
    p.y0 = ok ? min(ay, by) - grow : 1; p.y1 = ok ? max(ay, by) + grow : 0;
    return p;
}

__global__ __launch_bounds__(256) void k_draw_build(const float* __restrict__ joints, int J, int D, const int32_t* __restrict__ skel, int L,
                                                    const float* __restrict__ colors, const float* __restrict__ bbox, int P, float kp_thre,
                                                    int style, Prim* __restrict__ recs) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P * (L + 1)) return;
    const int p = t / (L + 1), l = t - p * (L + 1);
    const int box_recs = bbox ? 4 : 0;
    Prim* rec = recs + (size_t)p * (box_recs + 3 * L);
    if (l == L) {
        if (!bbox) return;
        int32_t x[4], y[4];
        bool ok[4];
        for (int k = 0; k < 4; ++k) {
            const bool okx = to_pixel(bbox[((size_t)p * 4 + k) * 2], x[k]), oky = to_pixel(bbox[((size_t)p * 4 + k) * 2 + 1], y[k]);
            ok[k] = okx && oky;
        }
        for (int k = 0; k < 4; ++k) {
            const int n = (k + 1) & 3;
            rec[k] = make_prim(ok[k] && ok[n], kCapsule, x[k], y[k], x[n], y[n], 0, 1, 255 | 255 << 8, 0);
        }
        return;
    }
    rec += box_recs + 3 * l;
    const int i1 = skel[l * 2], i2 = skel[l * 2 + 1];
    const float *j1 = joints + ((size_t)p * J + i1) * D, *j2 = joints + ((size_t)p * J + i2) * D;
    int32_t x1, y1, x2, y2;
    const bool f1x = to_pixel(j1[0], x1), f1y = to_pixel(j1[1], y1), f2x = to_pixel(j2[0], x2), f2y = to_pixel(j2[1], y2);
    const bool ok1 = f1x && f1y && (D < 3 || j1[2] > kp_thre), ok2 = f2x && f2y && (D < 3 || j2[2] > kp_thre);
    const int32_t c8 = to_c8(colors[l * 3]) | to_c8(colors[l * 3 + 1]) << 8 | to_c8(colors[l * 3 + 2]) << 16;
    rec[0] = make_prim(ok1 && ok2, kCapsule, x1, y1, x2, y2, 0, 2, c8, 1);
    if (style == GATOR_DRAW_COCO) {
        rec[1] = make_prim(ok1, kRing, x1, y1, x1, y1, 2, 3, c8, 3);
        rec[2] = make_prim(ok2, kRing, x2, y2, x2, y2, 2, 3, c8, 3);
    } else {
        rec[1] = make_prim(ok1, kDisc, x1, y1, x1, y1, 3, 0, c8, 3);
        rec[2] = make_prim(ok2, kDisc, x2, y2, x2, y2, 3, 0, c8, 3);
    }
}

// q of one primitive at pixel (px, py): the header comment's rule, operation for operation
__device__ __forceinline__ int coverage_q(const Prim& pr, int px, int py) {
    const int64_t apx = px - pr.ax, apy = py - pr.ay;
    double cov;
    if (pr.kind == kCapsule) {
        const int64_t abx = pr.bx - pr.ax, aby = pr.by - pr.ay;
        const int64_t dot = abx * apx + aby * apy, len2 = abx * abx + aby * aby;
        double d;
        if (dot <= 0) d = sqrt((double)(apx * apx + apy * apy));
        else if (dot >= len2) {
            const int64_t bpx = px - pr.bx, bpy = py - pr.by;
            d = sqrt((double)(bpx * bpx + bpy * bpy));
        } else {
            const int64_t cross = abx * apy - aby * apx;
            d = (double)(cross < 0 ? -cross : cross) / sqrt((double)len2);
        }
        cov = ((double)pr.t * 0.5 + 0.5) - d;
    } else {
        const double d = sqrt((double)(apx * apx + apy * apy));
        cov = pr.kind == kDisc ? ((double)pr.r + 0.5) - d : ((double)pr.t * 0.5 + 0.5) - fabs(d - (double)pr.r);
    }
    cov = fmin(fmax(cov, 0.0), 1.0);
    return (int)floor(255.0 * cov + 0.5);
}

// every pixel walks the first n entries of the list in order; row r of a thread is pixel (px, py + 4 r), drawn on iff inside[r]
template <int ROWS>
__device__ __forceinline__ void walk(const int* list, int n, const Prim* __restrict__ recs, const bool (&inside)[ROWS], int px, int py,
                                     int (&c)[ROWS][3]) {
    for (int i = 0; i < n; ++i) {
        const int idx = __builtin_amdgcn_readfirstlane(list[i]);      // uniform: the record comes through the scalar cache
        const Prim pr = recs[idx];      // (no early-out on the box's columns: it would split the record's fetch into two dependent ones)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int y = py + 4 * r;
            if (inside[r] && px >= pr.x0 && px <= pr.x1 && y >= pr.y0 && y <= pr.y1) {
                const int q = coverage_q(pr, px, y);
#pragma unroll
                for (int k = 0; k < 3; ++k) c[r][k] = (c[r][k] * (255 - q) + ((pr.c8 >> (8 * k)) & 255) * q + 127) / 255;
            }
        }
    }
}

template <int ROWS>
__global__ __launch_bounds__(256) void k_draw_tiles(const Prim* __restrict__ recs, int R, Tables tb, int P, const uint8_t* images,
                                                    uint8_t* out, int H, int W, int tiles_x, float alpha, float one_minus_alpha) {
    __shared__ int list[kListCap];
    __shared__ int wcount[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int tx0 = tx * kTileW, ty0 = ty * (kTileH * ROWS), tx1 = tx0 + kTileW - 1, ty1 = ty0 + kTileH * ROWS - 1;
    const int px = tx0 + lane, py = ty0 + wave;
    bool inside[ROWS];
    int src[ROWS][3], c[ROWS][3];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        inside[r] = px < W && py + 4 * r < H;
        const size_t at = (((size_t)n * H + py + 4 * r) * W + px) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) src[r][k] = 0;
        if (inside[r])
            for (int k = 0; k < 3; ++k) src[r][k] = images[at + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[r][k] = src[r][k];
    }
    const int first = tb.img_off ? tb.img_off[n] : 0;
    const int people = tb.img_off ? tb.img_off[n + 1] - first : (n < P ? 1 : 0);
    const int total = people * R;
    int count = 0;
    bool touched = false;
    for (int base = 0; base < total; base += 256) {
        const int k = base + tid;
        bool survive = false;
        int idx = 0;
        if (k < total) {
            const int slot = k / R;
            const int person = tb.person_of ? tb.person_of[first + slot] : n;
            idx = person * R + (k - slot * R);
            const int4 box = *reinterpret_cast<const int4*>(&recs[idx].x0);
            survive = box.x <= tx1 && box.z >= tx0 && box.y <= ty1 && box.w >= ty0;      // a skip record's box is empty
        }
        const unsigned long long mask = __ballot(survive);
        const int below = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[wave] = __popcll(mask);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 4; ++w) { const int v = wcount[w]; woff += w < wave ? v : 0; tot += v; }
        const int pos = count + woff + below;
        if (survive && pos < kListCap) list[pos] = idx;
        __syncthreads();
        if (count + tot >= kListCap) {      // full: draw it, then the rest of this chunk starts the next list
            walk<ROWS>(list, kListCap, recs, inside, px, py, c);
            touched = true;
            __syncthreads();
            if (survive && pos >= kListCap) list[pos - kListCap] = idx;
            count += tot - kListCap;
        } else {
            count += tot;
        }
    }
    __syncthreads();
    if (count > 0) {
        walk<ROWS>(list, count, recs, inside, px, py, c);
        touched = true;
    }
    if (!touched && out == images) return;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if (!inside[r]) continue;
        const size_t at = (((size_t)n * H + py + 4 * r) * W + px) * 3;
        if (touched && alpha != 1.f)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float a = (float)src[r][k] * one_minus_alpha, b = (float)c[r][k] * alpha;
                c[r][k] = (int)fminf(fmaxf(rintf(a + b), 0.f), 255.f);
            }
        for (int k = 0; k < 3; ++k) out[at + k] = (uint8_t)c[r][k];
    }
}

// image_index (host) or NULL for "person p alone in image p"; people of an image keep person order (image_groups.h)
int make_tables(gator_draw2d* h, const char* who, const int32_t* image_index, int P, int N, hipStream_t st, Tables* tb) {
    *tb = Tables{nullptr, nullptr};
    const size_t count = (size_t)N + 1 + P;
    int32_t* t = nullptr;
    ImageGroups g = image_groups(nullptr, P, N, nullptr, nullptr, nullptr);
    if (image_index) {
        GATOR_TRY(h->tab.stage(h, count, &t));
        g = image_groups(image_index, P, N, t, t + N + 1, nullptr);
    }
    if (g.error == ImageGroups::kNullTooMany)
        return fail(GATOR_EINVAL, "%s: image_index is NULL, so person p goes into image p, but n_people %d > n_images %d", who, P, N);
    if (g.error) return fail(GATOR_EINVAL, "%s: image_index[%d] = %d outside 0..%d", who, g.at, g.value, N - 1);
    if (!image_index) return GATOR_OK;
    const int32_t* d = nullptr;
    GATOR_TRY(h->tab.upload(h, count, st, &d));
    *tb = Tables{d, d + N + 1};
    return GATOR_OK;
}

}  // namespace
}  // namespace gator

extern "C" int gator_draw2d_create(const int32_t* skeleton, int32_t n_limbs, int32_t n_joints, gator_draw2d** out) {
    using namespace gator;
    const char* who = "gator_draw2d_create";
    if (!skeleton || !out) return fail(GATOR_EINVAL, "%s: null argument", who);
    *out = nullptr;
    if (n_limbs < 1 || n_limbs > kMaxLimbs) return fail(GATOR_EINVAL, "%s: n_limbs %d outside 1..%d", who, n_limbs, kMaxLimbs);
    if (n_joints < 1) return fail(GATOR_EINVAL, "%s: n_joints %d, a skeleton has at least one joint", who, n_joints);
    for (int k = 0; k < n_limbs * 2; ++k)
        if (skeleton[k] < 0 || skeleton[k] >= n_joints)
            return fail(GATOR_EINVAL, "%s: skeleton limb %d has joint index %d outside 0..%d", who, k / 2, skeleton[k], n_joints - 1);
    return create_handle(out, [&](gator_draw2d* h) -> int {
        h->L = n_limbs; h->J = n_joints;
        GATOR_TRY(h->skeleton.alloc((size_t)n_limbs * 2 * sizeof(int32_t)));
        GATOR_HIP_CHECK(hipMemcpy(h->skeleton.get(), skeleton, (size_t)n_limbs * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
        return GATOR_OK;
    });
}

extern "C" int gator_draw2d_destroy(gator_draw2d* h) { return gator::destroy_handle(h); }

extern "C" int gator_draw2d_workspace(const gator_draw2d* h, int64_t* bytes, int64_t* allocations) {
    return gator::handle_workspace(h, "gator_draw2d_workspace", bytes, allocations);
}

extern "C" int gator_draw2d_set_tile_rows(gator_draw2d* h, int32_t rows) {
    using namespace gator;
    if (!h) return fail(GATOR_EINVAL, "gator_draw2d_set_tile_rows: null handle");
    if (rows != 0 && rows != 1 && rows != kTallRows) return fail(GATOR_EINVAL, "gator_draw2d_set_tile_rows: rows is 0 (the built-in choice), 1 or %d", kTallRows);
    h->rows = rows;
    return GATOR_OK;
}

extern "C" int gator_draw2d_u8(gator_draw2d* h, const gator_draw2d_args* a, void* stream) {
    using namespace gator;
    const char* who = "gator_draw2d_u8";
    GATOR_TRY(check_handle(h, who));
    if (!a) return fail(GATOR_EINVAL, "%s: null args", who);
    GATOR_TRY(check_struct_size(who, "gator_draw2d_args", a->struct_size, sizeof(gator_draw2d_args), true));
    if (!a->joints) return fail(GATOR_EINVAL, "%s: joints is NULL", who);
    if (!a->colors) return fail(GATOR_EINVAL, "%s: colors is NULL", who);
    if (!a->images) return fail(GATOR_EINVAL, "%s: images is NULL", who);
    if (!a->out) return fail(GATOR_EINVAL, "%s: out is NULL", who);
    if (a->H < 1 || a->H > kMaxSide) return fail(GATOR_EINVAL, "%s: H = %d outside 1..%d", who, a->H, kMaxSide);
    if (a->W < 1 || a->W > kMaxSide) return fail(GATOR_EINVAL, "%s: W = %d outside 1..%d", who, a->W, kMaxSide);
    if (a->n_people < 1) return fail(GATOR_EINVAL, "%s: n_people = %d, must be >= 1", who, a->n_people);
    if (a->n_images < 1 || a->n_images > 65535) return fail(GATOR_EINVAL, "%s: n_images = %d outside 1..65535", who, a->n_images);
    if (a->joint_dim != 2 && a->joint_dim != 3) return fail(GATOR_EINVAL, "%s: joint_dim = %d, must be 2 or 3", who, a->joint_dim);
    if (a->style != GATOR_DRAW_KEYPOINTS && a->style != GATOR_DRAW_COCO) return fail(GATOR_EINVAL, "%s: unknown style %d", who, a->style);
    if (!(a->alpha >= 0.f && a->alpha <= 1.f)) return fail(GATOR_EINVAL, "%s: alpha must lie in [0, 1]", who);
    const int R = (a->bbox ? 4 : 0) + 3 * h->L;
    if ((int64_t)a->n_people * R >= ((int64_t)1 << 31)) return fail(GATOR_EINVAL, "%s: n_people * records per person must be below 2^31", who);
    hipStream_t st = (hipStream_t)stream;
    Tables tb;
    GATOR_TRY(make_tables(h, who, a->image_index, a->n_people, a->n_images, st, &tb));
    GATOR_TRY(h->grow(h->recs, (size_t)a->n_people * R));
    const int threads = a->n_people * (h->L + 1);
    k_draw_build<<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(a->joints, h->J, a->joint_dim, h->skeleton, h->L, a->colors, a->bbox,
                                                                    a->n_people, a->kp_thre, a->style, h->recs);
    GATOR_HIP_CHECK(hipGetLastError());
    const int tiles_x = (a->W + kTileW - 1) / kTileW, tiles_y = (a->H + kTileH - 1) / kTileH;
    const bool tall = h->rows ? h->rows != 1 : (int64_t)tiles_x * tiles_y * a->n_images >= kTallTileFrom;
    if (tall) {
        const int tall_y = (a->H + kTileH * kTallRows - 1) / (kTileH * kTallRows);
        k_draw_tiles<kTallRows><<<dim3((unsigned)(tiles_x * tall_y), (unsigned)a->n_images), 256, 0, st>>>(h->recs, R, tb, a->n_people, a->images,
                                                                                                         a->out, a->H, a->W, tiles_x, a->alpha, 1.f - a->alpha);
    } else {
        k_draw_tiles<1><<<dim3((unsigned)(tiles_x * tiles_y), (unsigned)a->n_images), 256, 0, st>>>(h->recs, R, tb, a->n_people, a->images, a->out,
                                                                                                  a->H, a->W, tiles_x, a->alpha, 1.f - a->alpha);
    }
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
