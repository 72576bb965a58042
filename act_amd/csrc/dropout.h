// dropout.h -- how every kernel of this library draws from Philox4x32-10 and turns a draw into a dropout keep mask, stated once.
// tests/philox_ref.py restates this file on the host under the same names; include/act_hip.h documents the keys per entry point.
// A draw is philox4x32_10(counter (c0, c1, DOMAIN, c3), key = seed) -> four words; the domain word keeps the users of one seed apart:
//   0  PHILOX_DOMAIN_GUMBEL   gumbel noise of the tokenizer (dgcnn.hip)                         (column / 4, row, 0, 0)
//   1  PHILOX_DOMAIN_ROWS     dropout on dense rows [T, D] (norm.hip, bert.hip, prompt_kv.hip)  (column / 4, row, 1, 0): word k = channel 4 c + k
//   2  PHILOX_DOMAIN_ATTN     dropout on attention probabilities (bert.hip)                     (key / 4, (b H + h) S + query, 2, 0): word k = key 4 c + k
//   3  PHILOX_DOMAIN_AUGMENT  draws of the augmentation chain (augment.hip)                     (slot, cloud, 3, position + 8 sub)
// A new user takes the next free value and adds its line here and in tests/philox_ref.py.
// Seed: the host seed with the device-resident step counter seed_dev (nullable; replayable from a hipGraph) folded in by philox_fold_seed.
// Mask: an entry is DROPPED when the top 24 bits of its word are below thr = (uint32_t)(p * 2^24); kept entries are scaled by 1 / (1 - p).
// The caller draws nothing at p = 0 and lets an injected mask (parity tests hand in the reference's draws) win over Philox.
#pragma once
#include "common.h"

constexpr uint32_t PHILOX_DOMAIN_GUMBEL = 0u, PHILOX_DOMAIN_ROWS = 1u, PHILOX_DOMAIN_ATTN = 2u, PHILOX_DOMAIN_AUGMENT = 3u;
constexpr float DROPOUT_THR_SCALE = 16777216.0f;                        // 2^24

__device__ __forceinline__ uint64_t philox_fold_seed(uint64_t seed, const uint64_t* __restrict__ seed_dev) {
    return seed_dev ? seed ^ seed_dev[0] * 0x9E3779B97F4A7C15ull : seed;
}
__device__ __forceinline__ void philox_draw(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t domain, uint32_t c3, uint32_t r[4]) {
    philox4x32_10(c0, c1, domain, c3, (uint32_t)seed, (uint32_t)(seed >> 32), r);
}
__host__ __device__ __forceinline__ uint32_t dropout_thr(float drop_p) { return (uint32_t)(drop_p * DROPOUT_THR_SCALE); }
__host__ __device__ __forceinline__ float dropout_inv_keep(float drop_p) { return 1.0f / (1.0f - drop_p); }
struct DropoutKey { uint64_t seed; uint32_t thr; float inv_keep; };      // seed: already folded
__device__ __forceinline__ bool dropout_dropped(const DropoutKey& k, uint32_t word) { return (word >> 8) < k.thr; }
__device__ __forceinline__ DropoutKey dropout_key(float drop_p, uint64_t seed, const uint64_t* __restrict__ seed_dev) {
    return DropoutKey{philox_fold_seed(seed, seed_dev), dropout_thr(drop_p), dropout_inv_keep(drop_p)};
}

// ---- domain 1: the four channels 4c .. 4c+3 (float4 c) of row `row`
struct Dropped4 { bool x, y, z, w; };
__device__ __forceinline__ Dropped4 dropout_dropped4(const DropoutKey& k, uint32_t row, uint32_t c) {
    uint32_t r[4];
    philox_draw(k.seed, c, row, PHILOX_DOMAIN_ROWS, 0u, r);
    return Dropped4{dropout_dropped(k, r[0]), dropout_dropped(k, r[1]), dropout_dropped(k, r[2]), dropout_dropped(k, r[3])};
}
// keep / (1-p)
__device__ __forceinline__ float4 dropout_keep4(const DropoutKey& k, uint32_t row, uint32_t c) {
    const Dropped4 d = dropout_dropped4(k, row, c);
    return make_float4(d.x ? 0.f : k.inv_keep, d.y ? 0.f : k.inv_keep, d.z ? 0.f : k.inv_keep, d.w ? 0.f : k.inv_keep);
}
// a o keep / (1-p)
__device__ __forceinline__ float4 dropout_apply4(const DropoutKey& k, uint32_t row, uint32_t c, float4 a) {
    const Dropped4 d = dropout_dropped4(k, row, c);
    a.x = d.x ? 0.f : a.x * k.inv_keep; a.y = d.y ? 0.f : a.y * k.inv_keep;
    a.z = d.z ? 0.f : a.z * k.inv_keep; a.w = d.w ? 0.f : a.w * k.inv_keep;
    return a;
}

// ---- domain 2: keep / (1-p) of keys key0 .. key0+3 (key0 % 4 == 0) of query row `rowid` = (b H + h) S + query; mask: injected [B H S, S] or null
__device__ __forceinline__ void dropout_attn_keep4(const uint8_t* __restrict__ mask, int S, const DropoutKey& k, uint32_t rowid, int key0, float kf[4]) {
    if (mask) {
        const uint8_t* __restrict__ m = mask + (size_t)rowid * S;
#pragma unroll
        for (int j = 0; j < 4; ++j) kf[j] = (key0 + j < S && m[key0 + j]) ? k.inv_keep : 0.f;
    } else {
        uint32_t r[4];
        philox_draw(k.seed, (uint32_t)(key0 >> 2), rowid, PHILOX_DOMAIN_ATTN, 0u, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) kf[j] = dropout_dropped(k, r[j]) ? 0.f : k.inv_keep;
    }
}
// the same for ONE key (a lane that owns a key column and walks queries)
__device__ __forceinline__ float dropout_attn_keep1(const uint8_t* __restrict__ mask, int S, const DropoutKey& k, uint32_t rowid, int key) {
    if (mask) return (key < S && mask[(size_t)rowid * S + key]) ? k.inv_keep : 0.f;
    uint32_t r[4];
    philox_draw(k.seed, (uint32_t)(key >> 2), rowid, PHILOX_DOMAIN_ATTN, 0u, r);
    const int j = key & 3;
    const uint32_t v = j == 0 ? r[0] : (j == 1 ? r[1] : (j == 2 ? r[2] : r[3]));
    return dropout_dropped(k, v) ? 0.f : k.inv_keep;
}
