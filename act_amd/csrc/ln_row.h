// ln_row.h -- the register-resident part of a wave-per-row LayerNorm: the row sits in float4 v[MAXV] of the 64 lanes (lane holds float4 columns
// lane + 64 i; entries past nv = D / 4 are masked here, whatever they hold), statistics come from two DPP wave reductions (mean, then the centred
// second moment).  Loads and stores stay with each kernel: how they are scheduled is measured per kernel and differs on purpose.
#pragma once
#include "common.h"

#define LN_ROW_MAXV 8          // float4 per lane: D <= 64*4*8 = 2048

template <int MAXV>
__device__ __forceinline__ float ln_row_mean(const float4* v, int lane, int nv, int D) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (lane + 64 * i < nv) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    return wave_sum_f32(s) / (float)D;
}
template <int MAXV>
__device__ __forceinline__ float ln_row_rstd(const float4* v, float mean, int lane, int nv, int D, float eps) {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        if (lane + 64 * i < nv) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
    return rsqrtf(wave_sum_f32(q) / (float)D + eps);
}
// (v - mean) * rstd * g + b of one float4
__device__ __forceinline__ float4 ln_row_norm4(const float4& v, float mean, float rstd, const float4& g, const float4& b) {
    float4 o;
    o.x = (v.x - mean) * rstd * g.x + b.x; o.y = (v.y - mean) * rstd * g.y + b.y;
    o.z = (v.z - mean) * rstd * g.z + b.z; o.w = (v.w - mean) * rstd * g.w + b.w;
    return o;
}
