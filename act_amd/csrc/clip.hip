// clip.hip -- the one piece of arithmetic of CLIP's visual tower that the rest of the library lacks: QuickGELU, x * sigmoid(1.702 x), forward and
// backward, as streaming kernels over the [rows, 4D] pre-activation of a residual block's MLP (reference models/dvae.py:394-403 through CLIP's
// ResidualAttentionBlock).  Everything else of the block is the existing LayerNorm / GEMM / attention entries (kernels.ClipBlockFn).
#include "common.h"

#define QG_ALPHA 1.702f

// sigmoid(z) and 1 - sigmoid(z) from t = exp(-|z|) in (0, 1]: no overflow, no inf / inf and no 0 * inf for any finite z, and the small one of the two
// keeps its relative accuracy (1 - s is not formed by cancellation)
__device__ __forceinline__ void sigmoid_pair(float z, float& s, float& c) {
    const float t = expf(-fabsf(z));
    const float r = 1.0f / (1.0f + t);
    const float big = r, small = t * r;
    s = z >= 0.f ? big : small;
    c = z >= 0.f ? small : big;
}

template <bool BWD>
__device__ __forceinline__ float quickgelu_one(float x, float dy) {
    float s, c;
    sigmoid_pair(QG_ALPHA * x, s, c);
    if (!BWD) return x * s;
    return dy * (s * (1.0f + QG_ALPHA * x * c));        // d/dx [x s(ax)] = s + a x s (1 - s);  |a x c| <= a |x|, and s == 0 wherever that is huge and negative
}

// head: the < 4 leading floats in front of the first 16-byte boundary (block 0, lanes 0..2); body4: float4 count from there; the < 4 trailing floats
// go to lanes 4..6 of block 0.  Every element is read and written by one lane, so out may be pre or dy.  `vec` == 0 (the pointers disagree modulo 16 bytes): head == n, everything through the scalar grid-stride loop.
template <bool BWD>
__global__ __launch_bounds__(256) void quickgelu_kernel(const float* pre, const float* dy, float* out, long long n, int head, long long body4, int vec) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    if (!vec) {
        for (long long i = tid; i < n; i += nth) out[i] = quickgelu_one<BWD>(pre[i], BWD ? dy[i] : 0.f);
        return;
    }
    const float4* p4 = reinterpret_cast<const float4*>(pre + head);
    const float4* d4 = reinterpret_cast<const float4*>(BWD ? dy + head : pre + head);
    float4* o4 = reinterpret_cast<float4*>(out + head);
    for (long long i = tid; i < body4; i += nth) {
        const float4 x = p4[i];
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (BWD) g = d4[i];
        o4[i] = make_float4(quickgelu_one<BWD>(x.x, g.x), quickgelu_one<BWD>(x.y, g.y), quickgelu_one<BWD>(x.z, g.z), quickgelu_one<BWD>(x.w, g.w));
    }
    if (blockIdx.x == 0) {
        const long long tail0 = head + 4 * body4;
        long long i = -1;
        if ((int)threadIdx.x < head) i = threadIdx.x;
        else if (threadIdx.x >= 4 && tail0 + (threadIdx.x - 4) < n && threadIdx.x < 8) i = tail0 + (threadIdx.x - 4);
        if (i >= 0) out[i] = quickgelu_one<BWD>(pre[i], BWD ? dy[i] : 0.f);
    }
}

template <bool BWD>
static int quickgelu_launch(const float* pre, const float* dy, float* out, int rows, int cols, act_stream_t stream) {
    if (!pre || !out || (BWD && !dy)) return ACT_E_NULLPTR;
    if (rows < 0 || cols < 0) return ACT_E_BADARG;
    const uintptr_t all = (uintptr_t)pre | (uintptr_t)out | (BWD ? (uintptr_t)dy : 0);
    if (all & 3) return ACT_E_BADARG;
    const long long n = (long long)rows * cols;
    if (n == 0) return 0;
    const unsigned mis = (unsigned)((uintptr_t)pre & 15);
    const int vec = ((uintptr_t)out & 15) == mis && (!BWD || ((uintptr_t)dy & 15) == mis);
    long long head = vec ? (long long)(((16 - mis) & 15) / 4) : n;
    if (head > n) head = n;
    const long long body4 = vec ? (n - head) / 4 : 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, (BWD ? 12.0 : 8.0) * (double)n, (BWD ? 12.0 : 8.0) * (double)n);
    const long long work = vec ? (body4 > 0 ? body4 : 1) : n;
    long long g = (work + 255) / 256; if (g > 2048) g = 2048;
    hipLaunchKernelGGL(quickgelu_kernel<BWD>, dim3((unsigned)g), dim3(256), 0, s, pre, dy, out, n, (int)head, body4, vec);
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_quickgelu_fwd_f32(const float* pre, float* out, int rows, int cols, act_stream_t stream) {
    return quickgelu_launch<false>(pre, nullptr, out, rows, cols, stream);
}
extern "C" int act_quickgelu_bwd_f32(const float* pre, const float* dy, float* dx, int rows, int cols, act_stream_t stream) {
    return quickgelu_launch<true>(pre, dy, dx, rows, cols, stream);
}
