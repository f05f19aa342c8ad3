// The demo's mesh overlay (demo/renderer.py) on the device: a batched software rasteriser, three launches.
//
// Geometry, derived from demo/renderer.py:28-35,62-110.  render() flips the mesh with Rx(180 deg), f = (x, -y, -z), applies the optional
// rotations R (rotate: 60 deg about y; angle/axis) to f, and draws v' = R f with the camera at the origin looking down -z and the
// projection P = [[sx, 0, 0, tx sx], [0, sy, 0, -ty sy], [0, 0, -1, 0], [0, 0, 0, 1]] (orthographic: w = 1, no divide):
//     clip = (sx (v'x + tx), sy (v'y - ty), -v'z).
// OpenGL's window has y up, an image has row 0 at the top, so with u = F R F v, F = diag(1, -1, -1), i.e. u = (v'x, -v'y, -v'z):
//     pixel column = (1 + sx (ux + tx)) / 2 * W        pixel row = (1 + sy (uy + ty)) / 2 * H        NDC depth = uz
// and for R = I, u = v: the model's own x, y and z.  A smaller depth is nearer; a fragment with depth outside [-1, 1] is clipped.
// The host folds F R F into one matrix A (the flip conjugates R, it is applied "to the flipped mesh" exactly as the reference does),
// the kernels see A only.  Pixel (row i, column j) is sampled at its centre (j + 0.5, i + 0.5).  The material is single sided, so
// pyrender culls back faces: a face is front facing when (b - a) x (c - a) of its pixel positions (x right, y down) is negative, which
// for sx sy > 0 is its outward normal pointing at the camera, n_z < 0.
//
//   k_render_vertices : one thread per (mesh, vertex), fp64 (a thousandth of the work).  Projects, snaps the pixel position to 24.8
//                       fixed point (round to nearest even of px * 256), writes depth and the vertex normal: the sum of (b - a) x (c - a)
//                       over the vertex's faces of the drawn (rotated) mesh, gathered through a vertex-to-face CSR in face order -- no
//                       atomics -- and normalised n / max(|n|, tiny).  Guard band: a vertex that is not finite or lies beyond +-2^20 px gets
//                       xy = INT32_MIN, and every face that touches it is skipped.  So |coordinate| <= 2^28, a difference <= 2^29
//                       (int32) and an edge function, the sum of two products, <= 2^59 (int64): coverage is exact in integers.
//   k_render_raster   : the hot path, one wave per 64 faces of one mesh.  The triangle is oriented so that its three edge functions are
//                       positive inside; edge a->b with d = b - a owns the points on it iff d.y < 0 or (d.y == 0 and d.x > 0) (top-left
//                       rule), so a pixel centre on a shared edge belongs to exactly one face.  Depth at the centre is fp32,
//                       za + wb (zb - za) + wc (zc - za) (exact on a face of constant depth).  Visibility is one 64-bit word per pixel,
//                       ordered_bits(depth) << 32 | (mesh slot * F + face), resolved with an INTEGER atomic min: order independent, the id
//                       breaks depth ties, so an image is the same bits from run to run and whatever else is in the batch.
//                       Each lane first walks its own clamped bounding box when that is small; then the wave walks the box of every
//                       lane whose box is large together, 64 pixels of a row at a time (ballot loop).
//   k_render_resolve  : one thread per pixel.  An empty pixel copies the background; a covered one decodes (mesh, face), recomputes the
//                       exact edge values, interpolates and renormalises the vertex normals, shades
//                       lin = base (ambient + (1/pi) sum_k I_k max(0, n . l_k)), applies pow(., 1/2.2), clamps, writes round(255 c).
// The lighting is this documented diffuse model with the reference's scene parameters, not pyrender's GLSL (no specular lobe).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"

struct gator_renderer : gator::Handle {
    int F = 0, V = 0;
    int small_box = 0;                 // box area (pixels) up to which a lane walks its own triangle
    gator::DevBuf<int32_t> faces;      // [F][3]
    gator::DevBuf<int32_t> vf_off;     // [V+1]  vertex-to-face CSR ...
    gator::DevBuf<int32_t> vf;         // [3F][3] ... the faces of a vertex, ascending, each as its three vertex indices (one load less in the chain)
    // workspace of gator_render_f32, grown when a larger call arrives (gator::Handle::grow)
    gator::WorkBuf<int32_t> xy;        // [M][V][2]
    gator::WorkBuf<float> z;           // [M][V]
    gator::WorkBuf<float> nrm;         // [M][V][3]
    gator::WorkBuf<uint64_t> keys;     // [N][H][W]
    gator::StagedTable<int32_t> tab;   // the image tables of every entry point: mesh_img [M] | mesh_slot [M] | img_off [N+1] | mesh_of [M]
};

namespace gator {
namespace {

constexpr int kMaxLights = 4;
constexpr int kMaxSide = 8192;
constexpr double kGuardPx = 1048576.0;          // 2^20 px: the guard band of the fixed-point coordinates (header comment)
// Box area in pixels up to which a lane walks its own triangle; larger boxes are walked by the whole wave, a row strip of 64 pixels at
// a time, which wastes most of the wave on a box narrower than 64.  Measured (tools/render_bench.py, profiles/render.txt, SMPL-sized
// sphere over a tenth of a 1080p frame, ~30 px per face): raster 0.227 / 0.233 / 0.052 / 0.052 / 0.052 ms at 16 / 64 / 256 / 1024 / 4096;
// no difference at 224 x 224, where every box is small.  256 is the smallest of the best.  gator_renderer_set_small_box overrides it
// per handle for that measurement.
constexpr int kSmallBoxPixels = 256;
constexpr uint64_t kEmptyKey = ~0ull;

struct Mat3 { double a[9]; };
struct Lights { float4 l[kMaxLights]; int n; float ambient; };
struct Tables { const int32_t *mesh_img, *mesh_slot, *img_off, *mesh_of; };     // all NULL: mesh m is slot 0 of image m

__global__ __launch_bounds__(256) void k_render_vertices(const float* __restrict__ verts, const float* __restrict__ cams, Mat3 A,
                                                         const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf, int V,
                                                         size_t total, double W, double H,
                                                         int32_t* __restrict__ xy, float* __restrict__ zo, float* __restrict__ nrm) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t m = t / (size_t)V;
    const int v = (int)(t - m * (size_t)V);
    const float* mv = verts + m * (size_t)V * 3;
    const double x = mv[v * 3], y = mv[v * 3 + 1], z = mv[v * 3 + 2];
    const double ux = A.a[0] * x + A.a[1] * y + A.a[2] * z, uy = A.a[3] * x + A.a[4] * y + A.a[5] * z, uz = A.a[6] * x + A.a[7] * y + A.a[8] * z;
    const double sx = cams[m * 4], sy = cams[m * 4 + 1], tx = cams[m * 4 + 2], ty = cams[m * 4 + 3];
    const double px = (1.0 + sx * (ux + tx)) * 0.5 * W, py = (1.0 + sy * (uy + ty)) * 0.5 * H;
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && fabs(px) <= kGuardPx && fabs(py) <= kGuardPx;      // NaN px, py fail
    xy[t * 2] = ok ? (int32_t)rint(px * 256.0) : INT32_MIN;
    xy[t * 2 + 1] = ok ? (int32_t)rint(py * 256.0) : INT32_MIN;
    zo[t] = (float)uz;
    // the normal of the DRAWN mesh: the edges are rotated, not the sum (A is the caller's float32 matrix, orthogonal only to its rounding)
    double rx = 0.0, ry = 0.0, rz = 0.0;
    const int k0 = vf_off[v], k1 = vf_off[v + 1];
#pragma unroll 4      // the iterations' loads are independent, the sum keeps its order
    for (int k = k0; k < k1; ++k) {
        const int32_t* f = vf + (size_t)k * 3;
        const float *a = mv + (size_t)f[0] * 3, *b = mv + (size_t)f[1] * 3, *c = mv + (size_t)f[2] * 3;
        const double ax_ = a[0], ay_ = a[1], az_ = a[2];
        const double p0 = b[0] - ax_, p1 = b[1] - ay_, p2 = b[2] - az_, q0 = c[0] - ax_, q1 = c[1] - ay_, q2 = c[2] - az_;
        const double e1x = A.a[0] * p0 + A.a[1] * p1 + A.a[2] * p2, e1y = A.a[3] * p0 + A.a[4] * p1 + A.a[5] * p2, e1z = A.a[6] * p0 + A.a[7] * p1 + A.a[8] * p2;
        const double e2x = A.a[0] * q0 + A.a[1] * q1 + A.a[2] * q2, e2y = A.a[3] * q0 + A.a[4] * q1 + A.a[5] * q2, e2z = A.a[6] * q0 + A.a[7] * q1 + A.a[8] * q2;
        rx += e1y * e2z - e1z * e2y;
        ry += e1z * e2x - e1x * e2z;
        rz += e1x * e2y - e1y * e2x;
    }
    const double len = fmax(sqrt(rx * rx + ry * ry + rz * rz), DBL_MIN);
    nrm[t * 3] = (float)(rx / len);
    nrm[t * 3 + 1] = (float)(ry / len);
    nrm[t * 3 + 2] = (float)(rz / len);
}

// float -> uint32 with the same order (-0 is made +0 first, so that equal depths have equal bits), and back
__device__ __forceinline__ uint32_t ordered_bits(float z) {
    const uint32_t b = __float_as_uint(z + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// edge a->b with d = b - a of a triangle whose edge functions are positive inside: 0 if it owns the points on it, 1 if not
__device__ __forceinline__ int edge_bias(int dx, int dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

// One triangle, oriented and clipped to the image.  valid == false: nothing to draw (a sentinel vertex, zero area, culled, off screen).
struct Tri {
    int ax, ay, bx, by, cx, cy;        // 24.8 pixel positions, (b - a) x (c - a) > 0
    float za, dzb, dzc, area;
    int bias_ab, bias_bc, bias_ca;
    int x0, x1, y0, y1;                // pixels whose centre lies in the bounding box, clamped to the image
    bool valid;
};

__device__ __forceinline__ Tri tri_setup(int ax, int ay, int bx, int by, int cx, int cy, float za, float zb, float zc, int cull, int H, int W) {
    Tri t;
    t.valid = ax != INT32_MIN && bx != INT32_MIN && cx != INT32_MIN;
    if (!t.valid) { ax = ay = bx = by = cx = cy = 0; }
    int64_t area = (int64_t)(bx - ax) * (cy - ay) - (int64_t)(by - ay) * (cx - ax);
    if (area == 0 || (area > 0 && cull)) t.valid = false;      // x right, y down: a negative cross product faces the camera
    if (area < 0) {
        int s = bx; bx = cx; cx = s;
        s = by; by = cy; cy = s;
        const float f = zb; zb = zc; zc = f;
        area = -area;
    }
    t.ax = ax; t.ay = ay; t.bx = bx; t.by = by; t.cx = cx; t.cy = cy;
    t.za = za; t.dzb = zb - za; t.dzc = zc - za;
    t.area = (float)area;
    t.bias_ab = edge_bias(bx - ax, by - ay);
    t.bias_bc = edge_bias(cx - bx, cy - by);
    t.bias_ca = edge_bias(ax - cx, ay - cy);
    const int xmin = min(ax, min(bx, cx)), xmax = max(ax, max(bx, cx)), ymin = min(ay, min(by, cy)), ymax = max(ay, max(by, cy));
    t.x0 = max(0, (xmin - 128 + 255) >> 8);      // the first centre j * 256 + 128 >= xmin
    t.x1 = min(W - 1, (xmax - 128) >> 8);        // the last centre <= xmax
    t.y0 = max(0, (ymin - 128 + 255) >> 8);
    t.y1 = min(H - 1, (ymax - 128) >> 8);
    if (t.x0 > t.x1 || t.y0 > t.y1) t.valid = false;
    return t;
}

// pixel (row i, column j), inside the image: coverage in int64, depth in fp32, one integer atomic min
__device__ __forceinline__ void tri_pixel(const Tri& t, int i, int j, uint32_t id, uint64_t* __restrict__ img, int W) {
    const int X = j * 256 + 128, Y = i * 256 + 128;
    const int64_t e_ab = (int64_t)(t.bx - t.ax) * (Y - t.ay) - (int64_t)(t.by - t.ay) * (X - t.ax);
    const int64_t e_bc = (int64_t)(t.cx - t.bx) * (Y - t.by) - (int64_t)(t.cy - t.by) * (X - t.bx);
    const int64_t e_ca = (int64_t)(t.ax - t.cx) * (Y - t.cy) - (int64_t)(t.ay - t.cy) * (X - t.cx);
    if (e_ab < t.bias_ab || e_bc < t.bias_bc || e_ca < t.bias_ca) return;
    const float wb = (float)e_ca / t.area, wc = (float)e_ab / t.area;
    const float z = t.za + wb * t.dzb + wc * t.dzc;
    if (!(z >= -1.f && z <= 1.f)) return;
    atomicMin((unsigned long long*)(img + (size_t)i * W + j), ((unsigned long long)ordered_bits(z) << 32) | id);
}

__global__ __launch_bounds__(64) void k_render_raster(const int32_t* __restrict__ xy, const float* __restrict__ z,
                                                      const int32_t* __restrict__ faces, int F, int V, Tables tb, int H, int W, int cull,
                                                      int small_box, uint64_t* __restrict__ keys) {
    const int m = blockIdx.y, lane = threadIdx.x;
    const int f = blockIdx.x * 64 + lane;
    const int image = tb.mesh_img ? tb.mesh_img[m] : m;
    const uint32_t slot = tb.mesh_slot ? (uint32_t)tb.mesh_slot[m] : 0u;
    uint64_t* img = keys + (size_t)image * H * W;
    const int32_t* mxy = xy + (size_t)m * V * 2;
    const float* mz = z + (size_t)m * V;
    int ax = INT32_MIN, ay = 0, bx = 0, by = 0, cx = 0, cy = 0;
    float za = 0.f, zb = 0.f, zc = 0.f;
    if (f < F) {
        const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
        ax = mxy[i0 * 2]; ay = mxy[i0 * 2 + 1]; bx = mxy[i1 * 2]; by = mxy[i1 * 2 + 1]; cx = mxy[i2 * 2]; cy = mxy[i2 * 2 + 1];
        za = mz[i0]; zb = mz[i1]; zc = mz[i2];
    }
    const uint32_t id = slot * (uint32_t)F + (uint32_t)f;
    const Tri t = tri_setup(ax, ay, bx, by, cx, cy, za, zb, zc, cull, H, W);
    const bool small = t.valid && (t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) <= small_box;
    if (small)
        for (int i = t.y0; i <= t.y1; ++i)
            for (int j = t.x0; j <= t.x1; ++j) tri_pixel(t, i, j, id, img, W);
    unsigned long long big = __ballot(t.valid && !small);
    while (big) {
        const int l = __ffsll(big) - 1;
        big &= big - 1;
        const Tri s = tri_setup(__shfl(ax, l), __shfl(ay, l), __shfl(bx, l), __shfl(by, l), __shfl(cx, l), __shfl(cy, l), __shfl(za, l),
                                __shfl(zb, l), __shfl(zc, l), cull, H, W);
        const uint32_t sid = __shfl(id, l);
        for (int i = s.y0; i <= s.y1; ++i)
            for (int j = s.x0 + lane; j <= s.x1; j += 64) tri_pixel(s, i, j, sid, img, W);
    }
}

__global__ __launch_bounds__(256) void k_render_resolve(const uint64_t* __restrict__ keys, const int32_t* __restrict__ xy,
                                                        const float* __restrict__ nrm, const int32_t* __restrict__ faces, int F, int V,
                                                        const float* __restrict__ colors, Tables tb, const uint8_t* __restrict__ bg, int H,
                                                        int W, size_t total, Lights L, uint8_t* __restrict__ rgb, int32_t* __restrict__ fid,
                                                        float* __restrict__ depth) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const uint64_t key = keys[p];
    if (key == kEmptyKey) {
        if (rgb)
            for (int c = 0; c < 3; ++c) rgb[p * 3 + c] = bg ? bg[p * 3 + c] : (uint8_t)0;
        if (fid) fid[p] = -1;
        if (depth) depth[p] = INFINITY;
        return;
    }
    const uint32_t id = (uint32_t)key;
    if (fid) fid[p] = (int32_t)id;
    if (depth) depth[p] = from_ordered_bits((uint32_t)(key >> 32));
    if (!rgb) return;
    const size_t hw = (size_t)H * W;
    const size_t n = p / hw;
    const size_t r = p - n * hw;
    const int i = (int)(r / (size_t)W), j = (int)(r - (size_t)i * W);
    const uint32_t slot = id / (uint32_t)F, f = id - slot * (uint32_t)F;
    const size_t m = tb.mesh_of ? (size_t)tb.mesh_of[tb.img_off[n] + (int)slot] : n;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    const int32_t* mxy = xy + m * (size_t)V * 2;
    const int ax = mxy[i0 * 2], ay = mxy[i0 * 2 + 1], bx = mxy[i1 * 2], by = mxy[i1 * 2 + 1], cx = mxy[i2 * 2], cy = mxy[i2 * 2 + 1];
    const int X = j * 256 + 128, Y = i * 256 + 128;
    // the face's own winding: the three edge values and the area change sign together, the weights do not
    const int64_t e_ab = (int64_t)(bx - ax) * (Y - ay) - (int64_t)(by - ay) * (X - ax);
    const int64_t e_bc = (int64_t)(cx - bx) * (Y - by) - (int64_t)(cy - by) * (X - bx);
    const int64_t e_ca = (int64_t)(ax - cx) * (Y - cy) - (int64_t)(ay - cy) * (X - cx);
    const float area = (float)(e_ab + e_bc + e_ca);
    const float wa = (float)e_bc / area, wb = (float)e_ca / area, wc = (float)e_ab / area;
    const float *na = nrm + (m * (size_t)V + i0) * 3, *nb = nrm + (m * (size_t)V + i1) * 3, *nc = nrm + (m * (size_t)V + i2) * 3;
    float nx = wa * na[0] + wb * nb[0] + wc * nc[0], ny = wa * na[1] + wb * nb[1] + wc * nc[1], nz = wa * na[2] + wb * nb[2] + wc * nc[2];
    const float len = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), FLT_MIN);
    nx /= len; ny /= len; nz /= len;
    float acc = 0.f;
    for (int k = 0; k < kMaxLights; ++k)
        if (k < L.n) acc += L.l[k].w * fmaxf(0.f, nx * L.l[k].x + ny * L.l[k].y + nz * L.l[k].z);
    const float s = L.ambient + 0.318309886183790672f * acc;
    for (int c = 0; c < 3; ++c) {
        const float base = colors ? colors[m * 3 + c] : (c == 2 ? 0.9f : 1.f);       // demo/renderer.py:62 default colour
        const float g = powf(fmaxf(base * s, 0.f), 1.f / 2.2f);
        rgb[p * 3 + c] = (uint8_t)rintf(255.f * fminf(fmaxf(g, 0.f), 1.f));
    }
}

int check_shape(const gator_renderer* h, const char* who, int n_meshes, int n_images, int H, int W) {
    if (n_meshes < 1 || n_images < 1) return fail(GATOR_EINVAL, "%s: n_meshes and n_images must be >= 1", who);
    if (H < 1 || H > kMaxSide || W < 1 || W > kMaxSide) return fail(GATOR_EINVAL, "%s: H and W must be 1..%d", who, kMaxSide);
    if (n_meshes > 65535) return fail(GATOR_EINVAL, "%s: at most 65535 meshes per call", who);
    if ((size_t)n_meshes * h->V > ((size_t)1 << 36)) return fail(GATOR_EINVAL, "%s: more than 2^36 vertices in one call", who);
    if ((size_t)n_images * H * W > ((size_t)1 << 38)) return fail(GATOR_EINVAL, "%s: more than 2^38 pixels in one call", who);
    return GATOR_OK;
}

// image_index (host, or NULL: mesh m is drawn alone into image m) through image_groups.h (slot = rank of the mesh among those of its
// image, in mesh order), the id limit, the upload.  ids_out: face ids go out as int32, so an id has 31 bits and not the visibility key's 32.
int make_tables(gator_renderer* h, const char* who, const int32_t* image_index, int M, int N, bool ids_out, hipStream_t st, Tables* tb) {
    *tb = Tables{nullptr, nullptr, nullptr, nullptr};
    const size_t count = (size_t)3 * M + N + 1;
    int32_t* t = nullptr;
    ImageGroups g = image_groups(nullptr, M, N, nullptr, nullptr, nullptr);
    if (image_index) {
        GATOR_TRY(h->tab.stage(h, count, &t));
        g = image_groups(image_index, M, N, t + 2 * (size_t)M, t + 2 * (size_t)M + N + 1, t + M);
    }
    if (g.error == ImageGroups::kNullTooMany)
        return fail(GATOR_EINVAL, "%s: image_index is NULL, so mesh m goes into image m, but n_meshes %d > n_images %d", who, M, N);
    if (g.error) return fail(GATOR_EINVAL, "%s: image_index[%d] = %d outside 0..%d", who, g.at, g.value, N - 1);
    if ((uint64_t)g.most * (uint64_t)h->F >= (ids_out ? 1ull << 31 : 1ull << 32))
        return fail(GATOR_EINVAL, "%s: max_meshes_per_image * n_faces = %d * %d must be below 2^%d", who, g.most, h->F, ids_out ? 31 : 32);
    if (!image_index) return GATOR_OK;
    std::memcpy(t, image_index, (size_t)M * sizeof(int32_t));      // mesh_img
    const int32_t* d = nullptr;
    GATOR_TRY(h->tab.upload(h, count, st, &d));
    *tb = Tables{d, d + M, d + 2 * (size_t)M, d + 2 * (size_t)M + N + 1};
    return GATOR_OK;
}

// A = F R F (header comment); rot NULL = identity.  GATOR_EINVAL for a non-finite entry.
int fold_rotation(const char* who, const float* rot, Mat3* A) {
    static const double sgn[3] = {1.0, -1.0, -1.0};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double v = rot ? (double)rot[r * 3 + c] : (r == c ? 1.0 : 0.0);
            if (!std::isfinite(v)) return fail(GATOR_EINVAL, "%s: rot3x3 must be finite", who);
            A->a[r * 3 + c] = sgn[r] * v * sgn[c] + 0.0;
        }
    return GATOR_OK;
}

int launch_vertices(gator_renderer* h, const float* verts, const float* cams, int M, int H, int W, const Mat3& A, int32_t* xy, float* z,
                    float* nrm, hipStream_t st) {
    const size_t total = (size_t)M * h->V;
    k_render_vertices<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(verts, cams, A, h->vf_off, h->vf, h->V, total, (double)W,
                                                                      (double)H, xy, z, nrm);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

int launch_raster(gator_renderer* h, const int32_t* xy, const float* z, const Tables& tb, int M, int N, int H, int W, int flags,
                  uint64_t* keys, hipStream_t st) {
    GATOR_HIP_CHECK(hipMemsetAsync(keys, 0xff, (size_t)N * H * W * sizeof(uint64_t), st));
    k_render_raster<<<dim3((h->F + 63) / 64, M), 64, 0, st>>>(xy, z, h->faces, h->F, h->V, tb, H, W, (flags & GATOR_RENDER_CULL_BACKFACES) ? 1 : 0,
                                                             h->small_box, keys);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

int launch_resolve(gator_renderer* h, const uint64_t* keys, const int32_t* xy, const float* nrm, const float* colors, const Tables& tb,
                   const uint8_t* bg, int N, int H, int W, const Lights& L, uint8_t* rgb, int32_t* fid, float* depth, hipStream_t st) {
    const size_t total = (size_t)N * H * W;
    k_render_resolve<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(keys, xy, nrm, h->faces, h->F, h->V, colors, tb, bg, H, W, total, L, rgb,
                                                                     fid, depth);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

int make_lights(const char* who, const float* lights, int n_lights, float ambient, Lights* L) {
    if (n_lights < 0 || n_lights > kMaxLights || (n_lights > 0 && !lights)) return fail(GATOR_EINVAL, "%s: 0..%d lights, each (direction, intensity)", who, kMaxLights);
    if (!std::isfinite(ambient)) return fail(GATOR_EINVAL, "%s: ambient must be finite", who);
    std::memset(L, 0, sizeof(*L));
    L->n = n_lights;
    L->ambient = ambient;
    for (int k = 0; k < n_lights; ++k) {
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(lights[k * 4 + c])) return fail(GATOR_EINVAL, "%s: light %d is not finite", who, k);
        L->l[k] = make_float4(lights[k * 4], lights[k * 4 + 1], lights[k * 4 + 2], lights[k * 4 + 3]);
    }
    return GATOR_OK;
}
}  // namespace
}  // namespace gator

extern "C" int gator_renderer_create(const int32_t* faces, int32_t n_faces, int32_t n_verts, gator_renderer** out) {
    using namespace gator;
    if (!faces || !out) return fail(GATOR_EINVAL, "gator_renderer_create: null argument");
    *out = nullptr;
    if (n_faces < 1) return fail(GATOR_EINVAL, "gator_renderer_create: n_faces %d, a mesh has at least one face", n_faces);
    if (n_verts < 3) return fail(GATOR_EINVAL, "gator_renderer_create: n_verts %d, a mesh has at least three vertices", n_verts);
    if (n_faces > (1 << 28) || n_verts > (1 << 28)) return fail(GATOR_EINVAL, "gator_renderer_create: at most 2^28 faces and vertices");
    std::vector<int32_t> off((size_t)n_verts + 1, 0), vf((size_t)n_faces * 9);
    for (int64_t k = 0; k < (int64_t)n_faces * 3; ++k) {
        if (faces[k] < 0 || faces[k] >= n_verts)
            return fail(GATOR_EINVAL, "gator_renderer_create: face %d has vertex index %d outside 0..%d", (int)(k / 3), faces[k], n_verts - 1);
        off[faces[k] + 1]++;
    }
    for (int v = 0; v < n_verts; ++v) off[v + 1] += off[v];
    {
        std::vector<int32_t> fill(off.begin(), off.end() - 1);
        for (int f = 0; f < n_faces; ++f)
            for (int c = 0; c < 3; ++c) {      // ascending face order: the normal's sum has one order
                int32_t* slot = &vf[(size_t)fill[faces[(size_t)f * 3 + c]]++ * 3];
                for (int q = 0; q < 3; ++q) slot[q] = faces[(size_t)f * 3 + q];
            }
    }
    return create_handle(out, [&](gator_renderer* h) -> int {
        h->F = n_faces; h->V = n_verts; h->small_box = kSmallBoxPixels;
        GATOR_TRY(h->faces.alloc((size_t)n_faces * 3 * sizeof(int32_t)));
        GATOR_TRY(h->vf_off.alloc(off.size() * sizeof(int32_t)));
        GATOR_TRY(h->vf.alloc(vf.size() * sizeof(int32_t)));
        GATOR_HIP_CHECK(hipMemcpy(h->faces.get(), faces, (size_t)n_faces * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
        GATOR_HIP_CHECK(hipMemcpy(h->vf_off.get(), off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        GATOR_HIP_CHECK(hipMemcpy(h->vf.get(), vf.data(), vf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        return GATOR_OK;
    });
}

extern "C" int gator_renderer_destroy(gator_renderer* h) { return gator::destroy_handle(h); }

extern "C" int gator_renderer_workspace(const gator_renderer* h, int64_t* bytes, int64_t* allocations) {
    return gator::handle_workspace(h, "gator_renderer_workspace", bytes, allocations);
}

extern "C" int gator_renderer_set_small_box(gator_renderer* h, int32_t pixels) {
    using namespace gator;
    if (!h) return fail(GATOR_EINVAL, "gator_renderer_set_small_box: null handle");
    if (pixels < 0) return fail(GATOR_EINVAL, "gator_renderer_set_small_box: pixels must be >= 0 (0: the built-in threshold)");
    h->small_box = pixels ? pixels : kSmallBoxPixels;
    return GATOR_OK;
}

extern "C" int gator_render_vertices_f32(gator_renderer* h, const float* verts, const float* cams, int32_t n_meshes, int32_t H, int32_t W,
                                         const float* rot3x3, int32_t* xy_fixed, float* z, float* normals, void* stream) {
    using namespace gator;
    const char* who = "gator_render_vertices_f32";
    GATOR_TRY(check_handle(h, who));
    if (!verts || !cams || !xy_fixed || !z || !normals) return fail(GATOR_EINVAL, "%s: null argument", who);
    GATOR_TRY(check_shape(h, who, n_meshes, 1, H, W));
    Mat3 A;
    GATOR_TRY(fold_rotation(who, rot3x3, &A));
    return launch_vertices(h, verts, cams, n_meshes, H, W, A, xy_fixed, z, normals, (hipStream_t)stream);
}

extern "C" int gator_render_raster(gator_renderer* h, const int32_t* xy_fixed, const float* z, const int32_t* image_index, int32_t n_meshes,
                                   int32_t n_images, int32_t H, int32_t W, int32_t flags, uint64_t* keys, void* stream) {
    using namespace gator;
    const char* who = "gator_render_raster";
    GATOR_TRY(check_handle(h, who));
    if (!xy_fixed || !z || !keys) return fail(GATOR_EINVAL, "%s: null argument", who);
    GATOR_TRY(check_shape(h, who, n_meshes, n_images, H, W));
    Tables tb;
    GATOR_TRY(make_tables(h, who, image_index, n_meshes, n_images, false, (hipStream_t)stream, &tb));
    return launch_raster(h, xy_fixed, z, tb, n_meshes, n_images, H, W, flags, keys, (hipStream_t)stream);
}

extern "C" int gator_render_resolve(gator_renderer* h, const uint64_t* keys, const int32_t* xy_fixed, const float* normals, const float* colors,
                                    const int32_t* image_index, int32_t n_meshes, const uint8_t* background, int32_t n_images, int32_t H,
                                    int32_t W, const float* lights, int32_t n_lights, float ambient, uint8_t* out_rgb, int32_t* out_face_id,
                                    float* out_depth, void* stream) {
    using namespace gator;
    const char* who = "gator_render_resolve";
    GATOR_TRY(check_handle(h, who));
    if (!keys || !xy_fixed || !normals) return fail(GATOR_EINVAL, "%s: null argument", who);
    if (!out_rgb && !out_face_id && !out_depth) return fail(GATOR_EINVAL, "%s: no output", who);
    GATOR_TRY(check_shape(h, who, n_meshes, n_images, H, W));
    Lights L;
    GATOR_TRY(make_lights(who, lights, n_lights, ambient, &L));
    Tables tb;
    GATOR_TRY(make_tables(h, who, image_index, n_meshes, n_images, out_face_id != nullptr, (hipStream_t)stream, &tb));
    return launch_resolve(h, keys, xy_fixed, normals, colors, tb, background, n_images, H, W, L, out_rgb, out_face_id, out_depth, (hipStream_t)stream);
}

extern "C" int gator_render_f32(gator_renderer* h, const float* verts, const float* cams, const float* colors, const int32_t* image_index,
                                int32_t n_meshes, const uint8_t* background, int32_t n_images, int32_t H, int32_t W, const float* rot3x3,
                                const float* lights, int32_t n_lights, float ambient, int32_t flags, uint8_t* out_rgb, int32_t* out_face_id,
                                float* out_depth, void* stream) {
    using namespace gator;
    const char* who = "gator_render_f32";
    GATOR_TRY(check_handle(h, who));
    if (!verts || !cams) return fail(GATOR_EINVAL, "%s: null verts / cams", who);
    if (!out_rgb && !out_face_id && !out_depth) return fail(GATOR_EINVAL, "%s: no output", who);
    GATOR_TRY(check_shape(h, who, n_meshes, n_images, H, W));
    Mat3 A;
    GATOR_TRY(fold_rotation(who, rot3x3, &A));
    Lights L;
    GATOR_TRY(make_lights(who, lights, n_lights, ambient, &L));
    hipStream_t st = (hipStream_t)stream;
    Tables tb;
    GATOR_TRY(make_tables(h, who, image_index, n_meshes, n_images, out_face_id != nullptr, st, &tb));
    const size_t mv = (size_t)n_meshes * h->V, px = (size_t)n_images * H * W;
    GATOR_TRY(h->grow(h->xy, mv * 2));
    GATOR_TRY(h->grow(h->z, mv));
    GATOR_TRY(h->grow(h->nrm, mv * 3));
    GATOR_TRY(h->grow(h->keys, px));
    GATOR_TRY(launch_vertices(h, verts, cams, n_meshes, H, W, A, h->xy, h->z, h->nrm, st));
    GATOR_TRY(launch_raster(h, h->xy, h->z, tb, n_meshes, n_images, H, W, flags, h->keys, st));
    return launch_resolve(h, h->keys, h->xy, h->nrm, colors, tb, background, n_images, H, W, L, out_rgb, out_face_id, out_depth, st);
}
