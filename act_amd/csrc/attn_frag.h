// attn_frag.h -- register fragment forms of the v_mfma_f32_32x32x2_f32 attention kernels (attention.hip's single-pass backward, bert.hip's dropout
// attention).  A wave owns a 32-row block of one (cloud, head) and meets the other side in 32-row tiles.  Operands go into the form their MFMA wants --
//   "row form"  lane (row = lane&31, half = lane>>5) holds X[row][half*HD/2 .. +HD/2)   (A or B operand of a head-dimension reduction: the
//               reduction index of an MFMA is a free permutation as long as A and B agree, so the two halves split the head dimension)
//   "col form"  lane (c = lane&31, half) holds X[f(r, half)][(HD/32)*c + dt], f(r, half) = (r&3) + 8*(r>>2) + 4*half   (A operand of a reduction over
//               rows: row f(r, half) is exactly the row the C/D register r of that half-wave belongs to, so P / dS / dS^t are B operands
//               straight from their accumulator registers)
// Two sets of loaders.  att_load_* (attention.hip, beside its two-segment addressing): every tile is a FULL tile inside one row segment (the last
// tile is shifted back to end at the last row; needs S0 % 32 == 0 and >= 32 rows per side), so a row address is a wave-uniform base + a 32-bit lane
// offset.  bert_load_* (here): any S >= 1, the caller clamps rows past S - 1 on the way in (their partner in P / dS is zero).
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define ATT_LOG2E 1.4426950408889634f
#define ATT_LN2 0.6931471805599453f
#define ATT_F(r, half) (((r) & 3) + 8 * ((r) >> 2) + 4 * (half))        // row of C/D register r of a half-wave (32x32x2 MFMA)

// rowp = the lane's (clamped) row, scaled by mul on the way in
template <int HD>
__device__ __forceinline__ void bert_load_row_form(const float* __restrict__ rowp, int half, float mul, float* x) {
    const float* p = rowp + half * (HD / 2);
#pragma unroll
    for (int i = 0; i < HD / 8; ++i) {
        const float4 t = *reinterpret_cast<const float4*>(p + 4 * i);
        x[4 * i] = t.x * mul; x[4 * i + 1] = t.y * mul; x[4 * i + 2] = t.z * mul; x[4 * i + 3] = t.w * mul;
    }
}
template <int HD>
__device__ __forceinline__ void bert_load_col_form(const float* __restrict__ base, int ld, int t0, int S, int c, int half, float (*x)[HD / 32]) {
    constexpr int NDT = HD / 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = min(t0 + ATT_F(r, half), S - 1);
        const float* p = base + (size_t)row * ld + NDT * c;
        if constexpr (NDT == 2) { const float2 v = *reinterpret_cast<const float2*>(p); x[r][0] = v.x; x[r][1] = v.y; }
        else x[r][0] = p[0];
    }
}
// store an accumulator set in the o-layout (acc[dt][r] = X^t[d = (HD/32) * f(r, half) + dt][row = lane&31]) as row-major X[row][d], scaled
template <int HD>
__device__ __forceinline__ void att_store_o(float* __restrict__ rowp, int half, const f32x16* acc, float mul) {
    constexpr int NDT = HD / 32;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                                        // registers 4g .. 4g+3 = rows m = 8g + 4 half + (0..3) -> NDT * 4 consecutive d
        if constexpr (NDT == 2) {
            float4 t0, t1;
            t0.x = acc[0][g * 4 + 0] * mul; t0.y = acc[1][g * 4 + 0] * mul; t0.z = acc[0][g * 4 + 1] * mul; t0.w = acc[1][g * 4 + 1] * mul;
            t1.x = acc[0][g * 4 + 2] * mul; t1.y = acc[1][g * 4 + 2] * mul; t1.z = acc[0][g * 4 + 3] * mul; t1.w = acc[1][g * 4 + 3] * mul;
            *reinterpret_cast<float4*>(rowp + 16 * g + 8 * half) = t0;
            *reinterpret_cast<float4*>(rowp + 16 * g + 8 * half + 4) = t1;
        } else {
            float4 t;
            t.x = acc[0][g * 4 + 0] * mul; t.y = acc[0][g * 4 + 1] * mul; t.z = acc[0][g * 4 + 2] * mul; t.w = acc[0][g * 4 + 3] * mul;
            *reinterpret_cast<float4*>(rowp + 8 * g + 4 * half) = t;
        }
    }
}
