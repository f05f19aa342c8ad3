// The project's counter-based generator, stated once: Philox4x32 of Salmon et al. (SC'11, Random123) at GATOR_PHILOX_ROUNDS rounds.
// The dropout masks (train_ops.hip, train_attn.inc; include/gator_train.h) and the detector noise (detector_noise.hip;
// include/gator_hip.h) draw from it; tests/train_refs.py::philox4x32 is its numpy form.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#ifndef GATOR_PHILOX_ROUNDS
// Philox4x32 rounds of every stream.  7 is the smallest count that Salmon et al. (SC'11, Random123) report as passing BigCrush
// ("Crush-resistant"); 10 is their default with a safety margin.  Measured in the fused attention kernels: at 10 rounds the integer
// multiplies of the generator (quarter rate) make the forward launch 1.7x its dropout-free time at B=1024, at 4 rounds they hide
// completely behind the MFMAs; 7 keeps the statistical guarantee at 0.7x the arithmetic.
#define GATOR_PHILOX_ROUNDS 7
#endif

namespace gator {
namespace {

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t (&k)[2]) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1];
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
}

// one Philox4x32 block: the counter c becomes the block's four words under the key `seed`
__device__ __forceinline__ void philox_block(uint32_t (&c)[4], uint64_t seed) {
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int r = 0; r < GATOR_PHILOX_ROUNDS; ++r) philox_round(c, k);
}

}  // namespace
}  // namespace gator
