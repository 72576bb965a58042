// split_planes.h -- how a float becomes two 16-bit plane elements: the operand format of the split-operand GEMM (gemm_bf16x3.hip).  The ONE definition for the
// split pass, the GEMM's planes-out epilogue, the LayerNorm and the attention forward: a producer that writes planes is bit-identical to producing fp32 and
// splitting it.  Two formats:
//   bf16 (opt-in):  x ~= hi + lo,  hi = bf16_rne(x),  lo = bf16_rne(x - hi).
//   f16 (default):  x * s ~= h1 + 2^-11 * h2,  s a power of two (tests/f16x3_ref.py restates it).
//     h1 = f16_rne(x s),  h2 = f16_rne((x s - h1) * 2^11);  a plane element below 2^-14 in magnitude (an f16 subnormal) is written as +0 BEFORE the residual is
//     taken, so h2 picks the whole value up and the product does not depend on how the matrix cores treat f16 subnormals.  |h2| <= |x s|: the low plane cannot
//     overflow if the high one does not, and the caller's scale keeps |x s| <= 2^15.
#pragma once
#include <hip/hip_runtime.h>

// The format of a pair of planes as it travels through launchers and kernel arguments.  The convention lives here and nowhere else: a scale of ZERO means bf16
// (hi, lo) planes, a POSITIVE scale means the f16 (h1, h2) planes of x * f16_scale.  (An f16 scale is a positive power of two; entry points reject any other.)
struct PlaneFmt {
    float f16_scale;
    static constexpr PlaneFmt bf16() { return PlaneFmt{0.f}; }
    static constexpr PlaneFmt f16(float scale) { return PlaneFmt{scale}; }
    __host__ __device__ bool is_f16() const { return f16_scale > 0.f; }
};

__device__ __forceinline__ unsigned bf16_rne(float x) {          // finite inputs (activations / weights): no NaN handling needed
    unsigned u = __float_as_uint(x);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ void split_bf16x2(float x, unsigned& hi, unsigned& lo) {
    hi = bf16_rne(x);
    lo = bf16_rne(x - __uint_as_float(hi << 16));
}

__device__ __forceinline__ unsigned f16_plane_bits(float v) {
    const unsigned short b = __builtin_bit_cast(unsigned short, (_Float16)v);           // v_cvt_f16_f32, round to nearest even
    return (b & 0x7C00u) ? (unsigned)b : 0u;                                            // exponent field 0: zero or subnormal -> +0
}
__device__ __forceinline__ void split_f16x2(float xs, unsigned& h1, unsigned& h2) {
    h1 = f16_plane_bits(xs);
    h2 = f16_plane_bits((xs - (float)__builtin_bit_cast(_Float16, (unsigned short)h1)) * 2048.0f);   // the residual and its scaling are exact in fp32
}

// four consecutive values -> 8 bytes of each plane (element index i4 * 4).  Compile-time format: f16 planes of o * s, or bf16 planes of o (s is not read)
template <bool F16>
__device__ __forceinline__ void store_planes4(unsigned short* __restrict__ p1, unsigned short* __restrict__ p2, size_t i4, const float4& o, float s) {
    const float e[4] = {o.x, o.y, o.z, o.w};
    unsigned h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (F16) split_f16x2(e[j] * s, h[j], l[j]);
        else split_bf16x2(e[j], h[j], l[j]);
    }
    reinterpret_cast<uint2*>(p1)[i4] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    reinterpret_cast<uint2*>(p2)[i4] = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
}
// ... run-time format: one wave-uniform branch (the format is a kernel argument)
__device__ __forceinline__ void store_planes4(PlaneFmt fmt, unsigned short* __restrict__ p1, unsigned short* __restrict__ p2, size_t i4, const float4& o) {
    if (fmt.is_f16()) store_planes4<true>(p1, p2, i4, o, fmt.f16_scale);
    else store_planes4<false>(p1, p2, i4, o, 0.f);
}
