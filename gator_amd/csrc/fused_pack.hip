// Create-time packing of reference-layout weights into MFMA operand order (see fused_common.h).
#include "fused_common.h"
#include "fused_state.h"
#include "x3_common.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace gator {
namespace {
// dst[(nb*KB + kb)][g][lane][j] = W[n*wsn + k*wsk],  n = 32nb + (lane&31),  k = 32kb + 8g + 4(lane>>5) + j
__global__ void k_pack_linear(const float* __restrict__ W, int64_t wsn, int64_t wsk, int N, int K, int KB,
                              float* __restrict__ dst, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int j = e & 3, lane = (e >> 2) & 63, g = (e >> 8) & 3;
    const int64_t tile = e >> 10;
    const int kb = (int)(tile % KB), nb = (int)(tile / KB);
    const int n = 32 * nb + (lane & 31), k = 32 * kb + 8 * g + 4 * (lane >> 5) + j;
    dst[e] = (n < N && k < K) ? W[(int64_t)n * wsn + (int64_t)k * wsk] : 0.f;
}
// X3 tile [plane][s][lane][jj] <- split3( fp32 tile [g = 2s + (jj>>2)][lane][j = jj&3] )
__global__ void k_repack_x3(const float* __restrict__ src, __bf16* __restrict__ dst, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (tile, s, lane, jj)
    if (e >= total) return;
    const int jj = e & 7, lane = (e >> 3) & 63, s = (e >> 9) & 1;
    const int64_t tile = e >> 10;
    const Split3<__bf16> q = split3<__bf16>(src[tile * kTile + ((2 * s + (jj >> 2)) * 64 + lane) * 4 + (jj & 3)]);
    __bf16* d = dst + tile * (2 * kTileX3) + (s * 64 + lane) * 8 + jj;
    d[0] = q.h;
    d[1024] = q.m;
    d[2048] = q.l();
}
// H3 tile [plane][s][lane][jj] <- three fp16 planes of scale * (fp32 tile element)
__global__ void k_repack_h3(const float* __restrict__ src, _Float16* __restrict__ dst, int64_t total, float scale) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int jj = e & 7, lane = (e >> 3) & 63, s = (e >> 9) & 1;
    const int64_t tile = e >> 10;
    const Split3<_Float16> q = split3<_Float16>(src[tile * kTile + ((2 * s + (jj >> 2)) * 64 + lane) * 4 + (jj & 3)] * scale);
    _Float16* d = dst + tile * (2 * kTileX3) + (s * 64 + lane) * 8 + jj;
    d[0] = q.h;
    d[1024] = q.m;
    d[2048] = q.l();
}
// out[tile] = max |w| of that tile; one 256-thread block per tile
__global__ void k_absmax_per_tile(const float* __restrict__ w, float* __restrict__ out) {
    __shared__ float part[4];
    const float* t = w + (int64_t)blockIdx.x * kTile;
    float m = 0.f;
    for (int i = threadIdx.x; i < kTile; i += 256) m = fmaxf(m, fabsf(t[i]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}
}  // namespace

int fused_repack_h3(const float* src_tiles, float* dst_tiles, int64_t ntiles, int* shift, float* tile_ratio, void* stream, int64_t period, int64_t live) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = ntiles * kTile;
    DevBuf<float> tmp;      // freed on every return path
    GATOR_TRY(tmp.alloc((size_t)ntiles * sizeof(float)));
    k_absmax_per_tile<<<(unsigned)ntiles, 256, 0, st>>>(src_tiles, tmp.get());
    GATOR_HIP_CHECK(hipGetLastError());
    std::vector<float> tmax((size_t)ntiles);
    GATOR_HIP_CHECK(hipMemcpyAsync(tmax.data(), tmp.get(), (size_t)ntiles * sizeof(float), hipMemcpyDeviceToHost, st));
    GATOR_HIP_CHECK(hipStreamSynchronize(st));
    float wmax = 0.f, wmin = 0.f;      // the largest tile maximum, and the smallest one of a tile that holds a weight at all
    for (int64_t t = 0; t < ntiles; ++t) {
        if (period != 0 && t % period >= live) continue;
        const float m = tmax[(size_t)t];
        if (m > wmax) wmax = m;
        if (m > 0.f && (wmin == 0.f || m < wmin)) wmin = m;
    }
    const int sh = pow2_shift_below_2_14(wmax, -16, 24);
    *shift = sh;
    *tile_ratio = wmax > 0.f ? wmin / wmax : 1.f;
    if (!h3_set_holds(*tile_ratio)) return GATOR_OK;      // the caller takes the form without a shared scale
    k_repack_h3<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(src_tiles, (_Float16*)dst_tiles, total, std::ldexp(1.0f, sh));
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

int fused_repack_x3(const float* src_tiles, float* dst_tiles, int64_t ntiles, void* stream) {
    const int64_t total = ntiles * kTile;
    k_repack_x3<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(src_tiles, (__bf16*)dst_tiles, total);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}

int fused_pack_linear(const float* W, int64_t wsn, int64_t wsk, int N, int K, float* dst, void* stream) {
    const int NB = nblk32(N), KB = nblk32(K);
    const int64_t total = (int64_t)NB * KB * kTile;
    k_pack_linear<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(W, wsn, wsk, N, K, KB, dst, total);
    GATOR_HIP_CHECK(hipGetLastError());
    return GATOR_OK;
}
}  // namespace gator
