// The weight streams of k_gat8 (gat_roles.hip): the tile grids of fused_create_gat re-ordered, per product wave, into the order the
// wave consumes them (gat8_forms.h: kGat8Units), in the tile format of the form that will read them.
#include "fused_common.h"
#include "fused_state.h"
#include "x3_common.h"
#include "gat8_forms.h"

#include <vector>

namespace gator {
namespace {

// one workgroup per destination tile: dst tile i <- src tile idx[i]  (TILE floats: 6 KiB X3 tiles or 4 KiB fp32 tiles)
template <int TILE>
__global__ void k_gather_tiles(const float* __restrict__ src, const int* __restrict__ idx, float* __restrict__ dst) {
    const f32x4* s = reinterpret_cast<const f32x4*>(src + (size_t)idx[blockIdx.x] * TILE);
    f32x4* d = reinterpret_cast<f32x4*>(dst + (size_t)blockIdx.x * TILE);
    for (int e = threadIdx.x; e < TILE / 4; e += blockDim.x) d[e] = s[e];
}
// H3 stream -> byte-lo stream, one wave per tile: hi and mid planes copied, lo packed as the top byte of fp16(2^24 lo); *bad counts
// the weights whose lo does not come back bit for bit from the product wave's own expansion (lo_expand)
__global__ void k_h3_to_h3b(const float* __restrict__ src, float* __restrict__ dst, unsigned* __restrict__ bad) {
    const int lane = threadIdx.x;
    const f16x8* q = reinterpret_cast<const f16x8*>(src + (size_t)blockIdx.x * kTileX3) + lane;
    f16x8* d = reinterpret_cast<f16x8*>(dst + (size_t)blockIdx.x * kTileH3B) + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i * 64] = q[i * 64];
    unsigned pk[4] = {0, 0, 0, 0};
    unsigned nbad = 0;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const f16x8 lo = q[(4 + s2) * 64];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const _Float16 up = (_Float16)((float)lo[j] * 16777216.0f);
            pk[s2 * 2 + (j >> 2)] |= (unsigned)(__builtin_bit_cast(unsigned short, up) >> 8) << (8 * (j & 3));
        }
        const f16x8 back = lo_expand(pk[s2 * 2], pk[s2 * 2 + 1]);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            nbad += __builtin_bit_cast(unsigned short, (_Float16)back[j]) != __builtin_bit_cast(unsigned short, (_Float16)lo[j]);
    }
    reinterpret_cast<uint4*>(dst + (size_t)blockIdx.x * kTileH3B + 1024)[lane] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    if (nbad) atomicAdd(bad, nbad);
}

}  // namespace

// The per-wave weight streams: the X3 tile grids of fused_create_gat (gxbuf, tile-for-tile image of gbuf from gblk[0].qkv on)
// re-ordered into the order product wave w consumes them, block after block.
int gat8_build_stream(FusedState* f, void* stream) {
    if (!f->opt.gat_x3 || !f->gxbuf) return GATOR_OK;
    std::vector<int> idx((size_t)kStreamTiles, 0);
    auto tile_of = [&](const float* grid) { return (int)((grid - f->gblk[0].qkv) / kTile); };
    for (int w = 0; w < 4; ++w) {
        int* o = idx.data() + (size_t)w * kWaveTiles;
        for (int bi = 0; bi < kDepth; ++bi) {
            const GatBlockPk& p = f->gblk[bi];
            for (int u = 0; u < U_COUNT; ++u)
                for (int i = 0; i < kGat8Units[u].tiles; ++i) *o++ = tile_of(p.*kGat8Units[u].grid) + gat8_unit_tile(u, w, i);
            for (int i = 0; i < kPadTiles; ++i) *o++ = tile_of(p.qkv);                  // dummy: loaded into a slot, never multiplied
        }
    }
    DevBuf<int> d_idx;      // temporaries: freed on every return path
    DevBuf<float> h3;
    GATOR_TRY(d_idx.alloc(idx.size() * sizeof(int)));
    GATOR_HIP_CHECK(hipMemcpyAsync(d_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
    GATOR_TRY(f->g8stream.alloc((size_t)kStreamTiles * kTileX3 * sizeof(float)));
    if (f->opt.gat8_h4) {      // the four-product form streams three fp16 planes of 2^shift * w: the fp32 tiles are put in stream order
        float& ratio = f->h3_tile_ratio[GATOR_H3SET_GAT8];  // first, so that the shift comes from exactly the weights the kernel multiplies (not the tables in between)
        GATOR_TRY(h3.alloc(idx.size() * kTile * sizeof(float)));
        k_gather_tiles<kTile><<<(unsigned)idx.size(), 128, 0, (hipStream_t)stream>>>(f->gblk[0].qkv, d_idx.get(), h3.get());
        int rc = fused_repack_h3(h3, f->g8stream, (int64_t)idx.size(), &f->gat8_wshift, &ratio, stream);
        if (rc) return rc;
        if (!h3_set_holds(ratio)) h3_demote(f, GATOR_H3SET_GAT8);      // the exact six products on the X3 stream below, as under GATOR_GAT8_H4=0
    }
    if (f->opt.gat8_h4) {
        if (f->opt.gat8_lobyte) {      // the byte-lo image of the same stream (H3B): used only if every lo value survives the round trip
            DevBuf<unsigned> d_bad;
            GATOR_TRY(d_bad.alloc(sizeof(unsigned)));
            GATOR_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(unsigned), (hipStream_t)stream));
            GATOR_TRY(f->g8stream_b.alloc((size_t)kStreamTiles * kTileH3B * sizeof(float)));
            k_h3_to_h3b<<<(unsigned)idx.size(), 64, 0, (hipStream_t)stream>>>(f->g8stream.get(), f->g8stream_b.get(), d_bad.get());
            GATOR_HIP_CHECK(hipGetLastError());
            unsigned nbad = 0;
            GATOR_HIP_CHECK(hipMemcpyAsync(&nbad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream));
            GATOR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
            if (nbad) { f->opt.gat8_lobyte = false; f->g8stream_b.reset(); }
        }
    } else {
        k_gather_tiles<kTileX3><<<(unsigned)idx.size(), 128, 0, (hipStream_t)stream>>>(f->gxbuf.get(), d_idx.get(), f->g8stream.get());
    }
    GATOR_HIP_CHECK(hipGetLastError());
    GATOR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return GATOR_OK;
}

}  // namespace gator
