// ws_hash.h -- the keyed draws of the sampling kernels (wholescene.hip, s3dis_sample.hip, cloud_sample.hip): one 32-bit mixer and one keyed bijection.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// lowbias32 mixer
__host__ __device__ __forceinline__ uint32_t ws_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// keyed bijection of [0, n): a 4-round balanced Feistel network on the smallest even bit width >= max(2, ceil(log2 n)), cycle-walked back into
// [0, n) (the walk ends: a permutation of the wider domain returns to [0, n) within its cycle).
__device__ __forceinline__ uint32_t ws_feistel(uint32_t x, uint32_t n, uint32_t key) {
    if (n <= 1) return 0;
    int bits = 32 - __clz(n - 1);
    if (bits < 2) bits = 2;
    bits += bits & 1;
    const int h = bits >> 1;
    const uint32_t mask = (1u << h) - 1u;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t F = ws_mix32(R ^ ws_mix32(key + i * 0x9e3779b9u)) & mask;
            const uint32_t nl = R;
            R = L ^ F;
            L = nl;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}
