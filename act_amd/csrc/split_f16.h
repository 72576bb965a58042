// split_f16.h -- the (h1, h2) f16 plane split of the split-f16 GEMM (gemm_bf16x3.hip, F16 form):  x * s ~= h1 + 2^-11 * h2,  s a power of two.
//   h1 = f16_rne(x s),  h2 = f16_rne((x s - h1) * 2^11);  a plane element below 2^-14 in magnitude (an f16 subnormal) is written as +0 BEFORE the residual is
//   taken, so h2 picks the whole value up and the product does not depend on how the matrix cores treat f16 subnormals.  |h2| <= |x s|: the low plane cannot
//   overflow if the high one does not, and the caller's scale keeps |x s| <= 2^15.  One definition for the split pass, the GEMM's planes-out epilogue, the
//   LayerNorm and the attention forward: a producer that writes planes is bit-identical to producing fp32 and splitting it (tests/f16x3_ref.py restates it).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned f16_plane_bits(float v) {
    const unsigned short b = __builtin_bit_cast(unsigned short, (_Float16)v);           // v_cvt_f16_f32, round to nearest even
    return (b & 0x7C00u) ? (unsigned)b : 0u;                                            // exponent field 0: zero or subnormal -> +0
}
__device__ __forceinline__ void split_f16x2(float xs, unsigned& h1, unsigned& h2) {
    h1 = f16_plane_bits(xs);
    h2 = f16_plane_bits((xs - (float)__builtin_bit_cast(_Float16, (unsigned short)h1)) * 2048.0f);   // the residual and its scaling are exact in fp32
}
// four consecutive values -> 8 bytes of each plane (element index i4 * 4)
__device__ __forceinline__ void store_f16_planes4(unsigned short* __restrict__ p1, unsigned short* __restrict__ p2, size_t i4, const float4& o, float s) {
    const float e[4] = {o.x * s, o.y * s, o.z * s, o.w * s};
    unsigned h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split_f16x2(e[j], h[j], l[j]);
    reinterpret_cast<uint2*>(p1)[i4] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    reinterpret_cast<uint2*>(p2)[i4] = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
}
