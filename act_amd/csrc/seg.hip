// seg.hip -- dense per-point prediction (semantic segmentation head, semantic_segmentation/models/pt.py): row log-softmax, weighted-mean NLL,
// confusion matrix.  (The three-NN feature propagation of the head is in sa.hip.)
//
// Every reduction runs in a fixed order: per-block partials, then one ordered pass.  The only atomics are integer ones (confusion-matrix
// counts), which are exact.
#include "common.h"

static inline unsigned cdiv(long long a, int b) { return (unsigned)((a + b - 1) / b); }

// ---- row log-softmax (C <= 64): one lane per row -----------------------------------------------------------------------
#define SEG_MAX_CLS 64
__global__ __launch_bounds__(256) void log_softmax_fwd_kernel(const float* __restrict__ z, long long R, int C, float* __restrict__ out) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float* zr = z + r * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, zr[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(zr[c] - m);
    const float lse = m + logf(s);
    float* o = out + r * C;
    for (int c = 0; c < C; ++c) o[c] = zr[c] - lse;
}
// dz = dout - exp(logp) * sum_c dout
__global__ __launch_bounds__(256) void log_softmax_bwd_kernel(const float* __restrict__ logp, const float* __restrict__ dout, long long R, int C,
                                                              float* __restrict__ dz) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float* g = dout + r * C;
    const float* lp = logp + r * C;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += g[c];
    float* o = dz + r * C;
    for (int c = 0; c < C; ++c) o[c] = g[c] - expf(lp[c]) * s;
}

extern "C" int act_log_softmax_fwd_f32(const float* z, long long R, int C, float* out, act_stream_t stream) {
    if (!z || !out) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || C > SEG_MAX_CLS) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 4.0 * R * C, 8.0 * R * C);
    hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, z, R, C, out);
    ACT_LAUNCH_CHECK(); return 0;
}
extern "C" int act_log_softmax_bwd_f32(const float* logp, const float* dout, long long R, int C, float* dz, act_stream_t stream) {
    if (!logp || !dout || !dz) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || C > SEG_MAX_CLS) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 4.0 * R * C, 12.0 * R * C);
    hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, logp, dout, R, C, dz);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- weighted-mean NLL: loss = sum_r w[t_r] * (-logp[r, t_r]) / sum_r w[t_r]; correct = #rows with arg-max == target ------
// fixed row -> (block, lane) map; a block reduces its lanes in a fixed tree, the final pass sums the block partials in block order
#define SEG_NLL_BLOCKS 512
__device__ __forceinline__ int row_argmax(const float* lp, int C) {
    int best = 0; float bv = lp[0];
    for (int c = 1; c < C; ++c) if (lp[c] > bv) { bv = lp[c]; best = c; }     // ties: lowest index (torch.argmax)
    return best;
}
__global__ __launch_bounds__(256) void nll_partial_kernel(const float* __restrict__ logp, const int64_t* __restrict__ tgt, const float* __restrict__ w,
                                                          long long R, int C, float* __restrict__ part, long long* __restrict__ part_cnt) {
    __shared__ float sn[256], sd[256];
    __shared__ long long sc[256];
    float num = 0.f, den = 0.f; long long cnt = 0;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long long)gridDim.x * 256) {
        const int t = (int)tgt[r];
        if (t < 0 || t >= C) continue;                                        // out-of-range targets are ignored (never read out of the row)
        const float* lp = logp + r * C;
        const float wt = w ? w[t] : 1.0f;
        num = fmaf(-wt, lp[t], num);
        den += wt;
        cnt += (row_argmax(lp, C) == t);
    }
    sn[threadIdx.x] = num; sd[threadIdx.x] = den; sc[threadIdx.x] = cnt;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) { sn[threadIdx.x] += sn[threadIdx.x + h]; sd[threadIdx.x] += sd[threadIdx.x + h]; sc[threadIdx.x] += sc[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blockIdx.x * 2] = sn[0]; part[blockIdx.x * 2 + 1] = sd[0]; part_cnt[blockIdx.x] = sc[0]; }
}
__global__ void nll_final_kernel(const float* __restrict__ part, const long long* __restrict__ part_cnt, int nparts, float* __restrict__ loss,
                                 float* __restrict__ wsum, long long* __restrict__ correct) {
    if (threadIdx.x != 0) return;
    float num = 0.f, den = 0.f; long long cnt = 0;
    for (int p = 0; p < nparts; ++p) { num += part[2 * p]; den += part[2 * p + 1]; cnt += part_cnt[p]; }
    loss[0] = num / den;
    wsum[0] = den;
    if (correct) correct[0] = cnt;
}

extern "C" size_t act_nll_weighted_workspace(long long R) {
    const long long nb = min((long long)SEG_NLL_BLOCKS, (R + 255) / 256);
    return (size_t)nb * (2 * sizeof(float) + sizeof(long long));
}

extern "C" int act_nll_weighted_fwd_f32(const float* logp, const int64_t* target, const float* weight, long long R, int C, float* loss, float* wsum,
                                        int64_t* correct, float* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!logp || !target || !loss || !wsum || !workspace) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || C > SEG_MAX_CLS) return ACT_E_BADARG;
    if (workspace_bytes < act_nll_weighted_workspace(R)) return ACT_E_BADARG;
    const int nb = (int)min((long long)SEG_NLL_BLOCKS, (R + 255) / 256);
    float* part = workspace;
    long long* part_cnt = reinterpret_cast<long long*>(workspace + 2 * nb);
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 3.0 * R * C, 4.0 * R * C + 8.0 * R);
    hipLaunchKernelGGL(nll_partial_kernel, dim3(nb), dim3(256), 0, s, logp, target, weight, R, C, part, part_cnt);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(nll_final_kernel, dim3(1), dim3(64), 0, s, part, part_cnt, nb, loss, wsum, reinterpret_cast<long long*>(correct));
    ACT_LAUNCH_CHECK(); return 0;
}

// dlogp[r, c] = (c == t_r) ? -g * w[t_r] / wsum : 0
__global__ __launch_bounds__(256) void nll_bwd_kernel(const int64_t* __restrict__ tgt, const float* __restrict__ w, const float* __restrict__ wsum,
                                                      const float* __restrict__ gloss, long long R, int C, float* __restrict__ dlogp) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int t = (int)tgt[r];
    const float wt = (w && t >= 0 && t < C) ? w[t] : 1.0f;
    const float v = -(gloss[0] * wt) / wsum[0];
    float* o = dlogp + r * C;
    for (int c = 0; c < C; ++c) o[c] = (c == t) ? v : 0.f;
}

extern "C" int act_nll_weighted_bwd_f32(const int64_t* target, const float* weight, const float* wsum, const float* gloss, long long R, int C,
                                        float* dlogp, act_stream_t stream) {
    if (!target || !wsum || !gloss || !dlogp) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || C > SEG_MAX_CLS) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 2.0 * R, 4.0 * R * C + 8.0 * R);
    hipLaunchKernelGGL(nll_bwd_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, target, weight, wsum, gloss, R, C, dlogp);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- confusion matrix: cm[t, argmax_c pred[r, c]] += 1 (int64, accumulated; per-block LDS histogram, then integer atomics) ----
__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ pred, const int64_t* __restrict__ tgt, long long R, int C,
                                                        unsigned long long* __restrict__ cm) {
    __shared__ unsigned int h[SEG_MAX_CLS * SEG_MAX_CLS];
    const int CC = C * C;
    for (int i = threadIdx.x; i < CC; i += 256) h[i] = 0u;
    __syncthreads();
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long long)gridDim.x * 256) {
        const int t = (int)tgt[r];
        if (t < 0 || t >= C) continue;
        atomicAdd(&h[t * C + row_argmax(pred + r * C, C)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC; i += 256)
        if (h[i]) atomicAdd(&cm[i], (unsigned long long)h[i]);
}

extern "C" int act_confusion_i64(const float* pred, const int64_t* target, long long R, int C, int64_t* cm, act_stream_t stream) {
    if (!pred || !target || !cm) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || C > SEG_MAX_CLS) return ACT_E_BADARG;
    const int nb = (int)min(1024LL, (R + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, (double)R * C, 4.0 * R * C + 8.0 * R);
    hipLaunchKernelGGL(confusion_kernel, dim3(nb), dim3(256), 0, s, pred, target, R, C, reinterpret_cast<unsigned long long*>(cm));
    ACT_LAUNCH_CHECK(); return 0;
}
