// edge_bn.h -- what the EdgeConv tails of edgeconv.hip (one convolution) and edge_mlp2.hip (two) share: the float64 column-sum shape, the centred
// BatchNorm evaluation, and the statistics / finalize / apply kernels over v = P[idx] + Q.  The kernels are static: each file that includes this
// header launches its own copy.
#pragma once
#include "common.h"

static inline unsigned cdiv(long long a, int b) { return (unsigned)((a + b - 1) / b); }

// ==================================================================================================== column sums over rows, in float64
// The statistics kernels below share one shape: a 256-thread block is TX lanes along the channels (a power of two, 64 at C >= 64) by
// TY = 256 / TX rows in flight, and owns a contiguous range of rows.  A thread adds its rows of one channel in registers (float64), the TY
// threads of a channel are then added in ascending ty through LDS, and the block writes one float64 partial per channel and sum:
// part[(block * NS + s) * C + c].  A finalize kernel adds the blocks in ascending order.  Fixed order throughout, no atomics.
#define CS_MAX_BLOCKS 512

struct ColShape { int tx_log, nblk, rpb; };
static ColShape col_shape(long long R, int C) {
    ColShape g;
    g.tx_log = 0;
    while ((1 << g.tx_log) < C && g.tx_log < 6) ++g.tx_log;
    const int ty = 256 >> g.tx_log;
    long long nblk = (R + ty - 1) / ty;
    if (nblk > CS_MAX_BLOCKS) nblk = CS_MAX_BLOCKS;
    g.nblk = (int)nblk;
    g.rpb = (int)((R + nblk - 1) / nblk);
    g.nblk = (int)((R + g.rpb - 1) / g.rpb);
    return g;
}
static size_t part_bytes(int C, int ns) { return (size_t)CS_MAX_BLOCKS * ns * C * sizeof(double); }
static size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

template <int NS>
__device__ __forceinline__ void col_reduce_store(double (&v)[NS], double* sh, int tx, int ty, int TX, int TY, bool act, int c, int C,
                                                 double* __restrict__ part) {
    __syncthreads();                                                              // sh is free again
#pragma unroll
    for (int s = 0; s < NS; ++s) sh[(s * TY + ty) * TX + tx] = v[s];
    __syncthreads();
    if (ty == 0 && act) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double a = 0.0;
            for (int y = 0; y < TY; ++y) a += sh[(s * TY + y) * TX + tx];
            part[((size_t)blockIdx.x * NS + s) * C + c] = a;
        }
    }
}

__device__ __forceinline__ int clampi(int v, int n) { return min(max(v, 0), n - 1); }
// The EdgeConv kernels use the CENTRED form z = scale * ((v - mean) - mean_lo) + beta, mean + mean_lo being the float64 mean split into a
// float32 and its remainder: with v of the order of 1000 and a spread of order 1, scale * v + shift would cancel two products of order 1000 * scale
// and lose the sign of small z, which the backward reads.  (v - mean) is exact or nearly so, every step is monotone in v.
__device__ __forceinline__ float centred(float v, float mean, float mean_lo) { return __fsub_rn(__fsub_rn(v, mean), mean_lo); }
__device__ __forceinline__ float lrelu_centred(float v, float mean, float mean_lo, float scale, float beta, float slope, float& z) {
    z = __fadd_rn(__fmul_rn(scale, centred(v, mean, mean_lo)), beta);
    return z > 0.f ? z : __fmul_rn(slope, z);
}

// v[b,i,j,c] = P[b, idx[b,i,j], c] + Q[b,i,c] (one rounded add) is formed in registers only.  Pass 1, per point and channel over the k
// values in ascending j: the largest and the smallest v with their first j (both, because which one the output takes depends on the sign of
// scale_c, known only after the statistics), sum_j v in fp32, and in float64 the moments of v - pivot_c around the pivot
// v[0,0,0,c] -- a value of v, so the moments stay of the size of the spread and var = q/M - dm^2 in float64 does not cancel.
// LeakyReLU(scale * v + shift) is monotone in v (non-decreasing for scale >= 0, non-increasing otherwise) and so is every rounding, hence
// out = LeakyReLU(scale * v* + shift) with v* the largest v (scale >= 0) or the smallest: exact in fp32.
// EXT = false (edge_mlp2.hip): the moments alone, nothing but the partials is written.
template <bool STATS, bool EXT = true>
static __global__ __launch_bounds__(256) void edge_bn_pass1_kernel(const float* __restrict__ pq, int ld, int qoff, const int32_t* __restrict__ idx, int N,
                                                            int k, int C, long long R, int rpb, int tx_log, float* __restrict__ vmax,
                                                            float* __restrict__ vmin, int32_t* __restrict__ arg2, float* __restrict__ vsum,
                                                            double* __restrict__ part) {
    __shared__ double sh[2 * 256];
    const int TX = 1 << tx_log, TY = 256 >> tx_log, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(R, r0 + rpb);
    for (int c0 = 0; c0 < C; c0 += TX) {
        const int c = c0 + tx;
        const bool act = c < C;
        double s[2] = {0.0, 0.0};
        if (act) {
            const float piv = STATS ? __fadd_rn(pq[(size_t)clampi(idx[0], N) * ld + c], pq[qoff + c]) : 0.f;
            for (long long r = r0 + ty; r < r1; r += TY) {
                const long long base = (r / N) * N;
                const float q = pq[r * ld + qoff + c];
                const int32_t* ir = idx + r * k;
                float mx = 0.f, mn = 0.f, sum = 0.f;
                int jx = 0, jn = 0;
                for (int j = 0; j < k; ++j) {
                    const float v = __fadd_rn(pq[(base + clampi(ir[j], N)) * ld + c], q);
                    if (j == 0) { mx = mn = sum = v; }
                    else {
                        if (v > mx) { mx = v; jx = j; }
                        if (v < mn) { mn = v; jn = j; }
                        sum = __fadd_rn(sum, v);
                    }
                    if (STATS) { const double d = (double)v - (double)piv; s[0] += d; s[1] += d * d; }
                }
                const long long o = r * C + c;
                if (EXT) { vmax[o] = mx; vmin[o] = mn; arg2[o] = jx | (jn << 16); vsum[o] = sum; }
            }
        }
        if (STATS) col_reduce_store<2>(s, sh, tx, ty, TX, TY, act, c, C, part);
    }
}

// mean / rstd / scale / shift per channel.  training: from the block partials (ascending block order, float64), and the running statistics
// move by momentum with the unbiased variance (count M = B*N*k; M == 1 keeps the biased one).  eval: from the running statistics.
// pivot == null: the pivot is v[0,0,0,c] as in pass 1; otherwise pivot[c] (edge_mlp2.hip, whose second BatchNorm is over y, not v).
static __global__ __launch_bounds__(256) void edge_bn_finalize_kernel(const float* __restrict__ pq, int ld, int qoff, const int32_t* __restrict__ idx, int N,
                                                               const double* __restrict__ part, int nblk, int C, double M, int training,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                               float* __restrict__ mean, float* __restrict__ mean_lo, float* __restrict__ rstd,
                                                               float* __restrict__ scale, const float* __restrict__ pivot = nullptr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float mu, rs, lo = 0.f;
    if (training) {
        const float piv = pivot ? pivot[c] : __fadd_rn(pq[(size_t)clampi(idx[0], N) * ld + c], pq[qoff + c]);
        double s1 = 0.0, s2 = 0.0;
        for (int p = 0; p < nblk; ++p) { s1 += part[((size_t)p * 2 + 0) * C + c]; s2 += part[((size_t)p * 2 + 1) * C + c]; }
        const double dm = s1 / M, m = (double)piv + dm;
        double var = s2 / M - dm * dm;
        if (var < 0.0) var = 0.0;
        mu = (float)m;
        lo = (float)(m - (double)mu);
        rs = (float)(1.0 / sqrt(var + (double)eps));
        if (rmean) {
            const double unb = M > 1.0 ? var * (M / (M - 1.0)) : var;
            rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * m);
            rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * unb);
        }
    } else {
        mu = rmean[c];
        rs = (float)(1.0 / sqrt((double)rvar[c] + (double)eps));
    }
    mean[c] = mu; mean_lo[c] = lo; rstd[c] = rs; scale[c] = __fmul_rn(gamma[c], rs);
}

// sel != null: also the selected extreme itself (edge_mlp2.hip keeps it for its backward)
static __global__ __launch_bounds__(256) void edge_bn_apply_kernel(const float* __restrict__ vmax, const float* __restrict__ vmin, int C, long long total,
                                                            const float* __restrict__ scale, const float* __restrict__ beta,
                                                            const float* __restrict__ mean, const float* __restrict__ mean_lo, float slope,
                                                            float* __restrict__ out, int ldo, int ooff, int32_t* __restrict__ arg,
                                                            float* __restrict__ sel = nullptr) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long r = e / C;
    const int c = (int)(e - r * C);
    const float sc = scale[c];
    const bool up = sc >= 0.f;
    const int a2 = arg[e];
    float z;
    const float v = up ? vmax[e] : vmin[e];
    if (sel) sel[e] = v;
    out[r * ldo + ooff + c] = lrelu_centred(v, mean[c], mean_lo[c], sc, beta[c], slope, z);
    arg[e] = up ? (a2 & 0xffff) : ((a2 >> 16) & 0xffff);
}

static __global__ __launch_bounds__(256) void clamp_idx_kernel(const int32_t* __restrict__ idx, long long total, int N, int32_t* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < total) out[e] = clampi(idx[e], N);
}
