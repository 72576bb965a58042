// dgcnn.hip -- the non-GEMM part of the teacher's DGCNN token mixers and of the dVAE tokenizer (models/dvae.py:26-117,587-588)
//
// Edge-conv layer, restructured: conv1x1(cat(x_j - x_i, x_i)) = Wa x_j + (Wb - Wa) x_i, so the GEMM runs once over the
// B*G points and produces YZ = [Y | Z]; the edge tensor [B, C, G, k] is never materialised:
//   pre(b,g,j,c) = Y[b, idx[b,j,g], c] + Z[b,g,c]
//   GroupNorm(4) statistics over (C/4, G, k) per sample  -> edge_gn_stats   (one workgroup per (sample, group))
//   max_j LeakyReLU(GN(pre)) -> because GN's affine map and LeakyReLU are monotone per channel, this equals
//   LeakyReLU(GN(max_j pre)) when gamma*rstd >= 0 and LeakyReLU(GN(min_j pre)) otherwise -> edge_gn_apply_max
// The same two kernels with k = 1 and no gather implement the GroupNorm + LeakyReLU head (layer5).
// Tokenizer: hard gumbel-softmax + one-hot x codebook == argmax_n(logits + G) followed by a row gather, fused with the
// head's GroupNorm + LeakyReLU so the [B,G,8192] logits are read exactly once and never rewritten.
#include "dropout.h"
#include <atomic>
#include <stdlib.h>

// ------------------------------------------------------------------------------------------------------- GN statistics
// yz [B*G, ldy] with Y at column offset 0 and Z at column offset zoff (zoff < 0: no Z term); idx int64 [B,k,G] or null
#define GN_SPLIT 8
// stage 1: grid (B*groups, GN_SPLIT); partial sums of (v - pivot), (v - pivot)^2 -> part[(bg*GN_SPLIT + sp)*2 + {0,1}]
__global__ __launch_bounds__(256) void edge_gn_stats_kernel(const float* __restrict__ yz, int ldy, int zoff,
                                                            const int64_t* __restrict__ idx, int G, int k, int C, int groups,
                                                            float* __restrict__ part) {
    __shared__ float sh[2][4];
    const int b = blockIdx.x / groups, gi = blockIdx.x % groups;
    const int cpg = C / groups, c0 = gi * cpg;
    const long long total = (long long)G * k * cpg;
    // pivot = first element of the group
    const int r00 = idx ? (int)idx[(size_t)b * k * G] : 0;
    const float pv = yz[((size_t)b * G + r00) * ldy + c0] + (zoff >= 0 ? yz[((size_t)b * G) * ldy + zoff + c0] : 0.f);
    float s = 0.f, q = 0.f;
    for (long long i = (long long)blockIdx.y * 256 + threadIdx.x; i < total; i += 256 * GN_SPLIT) {
        const int c = (int)(i % cpg); const long long t = i / cpg; const int g = (int)(t % G); const int j = (int)(t / G);
        const int src = idx ? (int)idx[((size_t)b * k + j) * G + g] : g;
        float v = yz[((size_t)b * G + src) * ldy + c0 + c];
        if (zoff >= 0) v += yz[((size_t)b * G + g) * ldy + zoff + c0 + c];
        v -= pv;
        s += v; q += v * v;
    }
    s = wave_sum_f32(s); q = wave_sum_f32(q);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[((size_t)blockIdx.x * GN_SPLIT + blockIdx.y) * 2 + 0] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        part[((size_t)blockIdx.x * GN_SPLIT + blockIdx.y) * 2 + 1] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    }
}
// stage 2: one workgroup per (sample, group): thread 0 folds the partials (fixed order) -> mean, rstd.  var = Q / n - dm^2 cancels once the pivot lies
// far from the mean (a first element 30 - 1000 deviations out: rstd wrong by 5e-5 - 2.8e-3, notebook/dgcnn_edges.md), so where dm^2 > FAR_PIVOT * var the whole
// workgroup walks the group a second time around the mean it has just found -- nothing cancels, the order is fixed, and every other group keeps the
// arithmetic above bit for bit (the workgroup leaves at once).  Serves the slab path, the generic path, the head and the tokenizer.
__global__ __launch_bounds__(256) void edge_gn_finalize_kernel(const float* __restrict__ yz, int ldy, int zoff, const int64_t* __restrict__ idx,
                                                               int G, int k, int C, int groups, const float* __restrict__ part, float eps,
                                                               float* __restrict__ mean_out, float* __restrict__ rstd_out) {
    __shared__ float sh[2][4];
    __shared__ float smu; __shared__ int sfar;
    const int bg = blockIdx.x;
    const int b = bg / groups, gi = bg % groups, cpg = C / groups, c0 = gi * cpg;
    const float total = (float)G * (float)k * (float)cpg;
    if (threadIdx.x == 0) {
        const int r00 = idx ? (int)idx[(size_t)b * k * G] : 0;
        const float pv = yz[((size_t)b * G + r00) * ldy + c0] + (zoff >= 0 ? yz[((size_t)b * G) * ldy + zoff + c0] : 0.f);
        float S = 0.f, Q = 0.f;
        for (int sp = 0; sp < GN_SPLIT; ++sp) { S += part[((size_t)bg * GN_SPLIT + sp) * 2]; Q += part[((size_t)bg * GN_SPLIT + sp) * 2 + 1]; }
        const float dm = S / total;
        const float var = fmaxf(Q / total - dm * dm, 0.f);
        mean_out[bg] = pv + dm;
        rstd_out[bg] = rsqrtf(var + eps);
        smu = pv + dm; sfar = dm * dm > FAR_PIVOT * var;
    }
    __syncthreads();
    if (!sfar) return;
    const float mu0 = smu;
    const long long n = (long long)G * k * cpg;
    float s = 0.f, q = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const int c = (int)(i % cpg); const long long t = i / cpg; const int g = (int)(t % G); const int j = (int)(t / G);
        const int src = idx ? (int)idx[((size_t)b * k + j) * G + g] : g;
        float v = yz[((size_t)b * G + src) * ldy + c0 + c];
        if (zoff >= 0) v += yz[((size_t)b * G + g) * ldy + zoff + c0 + c];
        v -= mu0;
        s += v; q += v * v;
    }
    s = wave_sum_f32(s); q = wave_sum_f32(q);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float d2 = ((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) / total;
        const float var = fmaxf(((sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3])) / total - d2 * d2, 0.f);
        mean_out[bg] = mu0 + d2;
        rstd_out[bg] = rsqrtf(var + eps);
    }
}

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// out[b*G+g, c] = max_j lrelu(gn(pre))    (ldo = row stride of out, written at column offset ooff)
__global__ __launch_bounds__(256) void edge_gn_apply_max_kernel(const float* __restrict__ yz, int ldy, int zoff,
                                                                const int64_t* __restrict__ idx, int G, int k, int C, int groups,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float slope, float* __restrict__ out, int ldo, int ooff,
                                                                long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C); const long long row = i / C; const int b = (int)(row / G), g = (int)(row % G);
        const int gi = c / (C / groups);
        float vmax = -3.0e38f, vmin = 3.0e38f;
        for (int j = 0; j < k; ++j) {
            const int src = idx ? (int)idx[((size_t)b * k + j) * G + g] : g;
            const float v = yz[((size_t)b * G + src) * ldy + c];
            vmax = fmaxf(vmax, v); vmin = fminf(vmin, v);
        }
        const float a = rstd[b * groups + gi] * gamma[c];
        float v = a >= 0.f ? vmax : vmin;
        if (zoff >= 0) v += yz[(size_t)row * ldy + zoff + c];
        out[(size_t)row * ldo + ooff + c] = lrelu((v - mean[b * groups + gi]) * a + beta[c], slope);
    }
}

__device__ __forceinline__ float gumbel_from_bits(uint32_t bits) {
    // 23 random bits + 1/2 is exact in fp32, so u lies in [2^-24, 1 - 2^-24]: never 0 and never 1.  (24 bits + 1/2 rounds its largest
    // value up to u == 1, i.e. +inf noise once per 2^24 draws -- a NaN in the soft-max of every Stage-I step at B = 128 x 64 x 8192.)
    const float u = ((float)(bits >> 9) + 0.5f) * (1.0f / 8388608.0f);
    return -__logf(-__logf(u));                                              // -log(Exponential(1)), finite: |g| <= 16.7
}

// one workgroup per token row: index = argmax_c ( lrelu(gn(h[row,c])) + gumbel ), out[row,:] = codebook[index,:]
// noise != null: use the given gumbel noise (parity tests); else Philox keyed by (seed, row, c/4).
__global__ __launch_bounds__(256) void gumbel_argmax_gather_kernel(const float* __restrict__ h, int G, int C, int groups,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float slope, const float* __restrict__ noise, uint64_t seed,
                                                                   const uint64_t* __restrict__ seed_dev,
                                                                   float inv_tau, const float* __restrict__ codebook, int D,
                                                                   int64_t* __restrict__ index_out, float* __restrict__ out,
                                                                   float* __restrict__ logits_out) {
    __shared__ float sv[4]; __shared__ int si[4]; __shared__ int swin;
    seed = philox_fold_seed(seed, seed_dev);
    const int row = blockIdx.x, b = row / G;
    const int cpg = C / groups;
    float best = -3.0e38f; int bi = 0;
    // group by group (the statistics are wave-uniform scalars, no per-element division), float4 for h / gamma / beta / noise / logits
    // (cpg % 4 == 0: a float4 never straddles two groups); same arithmetic per element as before
    if (cpg & 3) {                                       // (channel groups that are not a multiple of 4 wide: element-wise group lookup)
        for (int c4 = threadIdx.x * 4; c4 < C; c4 += 1024) {
            const float4 x = *reinterpret_cast<const float4*>(h + (size_t)row * C + c4);
            const float xs[4] = {x.x, x.y, x.z, x.w};
            uint32_t rnd[4] = {0, 0, 0, 0};
            if (!noise) philox_draw(seed, (uint32_t)(c4 >> 2), (uint32_t)row, PHILOX_DOMAIN_GUMBEL, 0u, rnd);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c4 + u, gi = c / cpg;
                const float v = lrelu((xs[u] - mean[b * groups + gi]) * rstd[b * groups + gi] * gamma[c] + beta[c], slope);
                if (logits_out) logits_out[(size_t)row * C + c] = v;
                const float gnoise = noise ? noise[(size_t)row * C + c] : gumbel_from_bits(rnd[u]);
                const float y = (v + gnoise) * inv_tau;
                if (y > best) { best = y; bi = c; }
            }
        }
    } else
    for (int gi = 0; gi < groups; ++gi) {
        const float mu = mean[b * groups + gi], rs = rstd[b * groups + gi];
        for (int c4 = gi * cpg + threadIdx.x * 4; c4 < (gi + 1) * cpg; c4 += 1024) {
            const float4 x = *reinterpret_cast<const float4*>(h + (size_t)row * C + c4);
            const float4 ga = *reinterpret_cast<const float4*>(gamma + c4), be = *reinterpret_cast<const float4*>(beta + c4);
            const float xs[4] = {x.x, x.y, x.z, x.w}, gs[4] = {ga.x, ga.y, ga.z, ga.w}, bs[4] = {be.x, be.y, be.z, be.w};
            uint32_t rnd[4] = {0, 0, 0, 0};
            float ns[4] = {0.f, 0.f, 0.f, 0.f};
            if (!noise) philox_draw(seed, (uint32_t)(c4 >> 2), (uint32_t)row, PHILOX_DOMAIN_GUMBEL, 0u, rnd);
            else { const float4 nz = *reinterpret_cast<const float4*>(noise + (size_t)row * C + c4); ns[0] = nz.x; ns[1] = nz.y; ns[2] = nz.z; ns[3] = nz.w; }
            float vs[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                vs[u] = lrelu((xs[u] - mu) * rs * gs[u] + bs[u], slope);
                const float gnoise = noise ? ns[u] : gumbel_from_bits(rnd[u]);
                const float y = (vs[u] + gnoise) * inv_tau;
                if (y > best) { best = y; bi = c4 + u; }    // ascending c inside a thread: first maximum wins
            }
            if (logits_out) *reinterpret_cast<float4*>(logits_out + (size_t)row * C + c4) = make_float4(vs[0], vs[1], vs[2], vs[3]);
        }
    }
    // block arg-max with lowest-index tie-break (torch.argmax returns the first maximum)
    const float wmax = wave_max_f32(best, -3.4e38f);
    int cand = (best == wmax) ? bi : 0x7fffffff;
    // min over the wave of candidate indices
    for (int off = 32; off > 0; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = wmax; si[threadIdx.x >> 6] = cand; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float gv = sv[0]; int gi2 = si[0];
        for (int w = 1; w < 4; ++w) if (sv[w] > gv || (sv[w] == gv && si[w] < gi2)) { gv = sv[w]; gi2 = si[w]; }
        swin = gi2;
        if (index_out) index_out[row] = gi2;
    }
    __syncthreads();
    const int win = swin;
    for (int d = threadIdx.x; d < D; d += 256) out[(size_t)row * D + d] = codebook[(size_t)win * D + d];
}

static inline unsigned grid_for(long long total, int block) {
    long long g = (total + block - 1) / block; if (g > 8192) g = 8192; if (g < 1) g = 1; return (unsigned)g;
}

// Graph layers whose (sample, group) slice of [Y | Z] fits the LDS (G x C/groups x 2 floats <= 140 KB: every layer of the 64-token DGCNNs):
// ONE kernel, one workgroup per (sample, group).  The slice is read from HBM once (the three-kernel path reads Y k times and Z once for the
// statistics and again for the apply pass, through gathers), statistics and the max / LeakyReLU pass run out of LDS.
#define EGF_THREADS 1024
__global__ __launch_bounds__(EGF_THREADS) void edge_gn_fused_kernel(const float* __restrict__ yz, int ldy, int zoff, const int64_t* __restrict__ idx,
                                                            int G, int k, int C, int groups, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, float slope,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                            float* __restrict__ out, int ldo, int ooff) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float sh[2][EGF_THREADS / 64];
    __shared__ float stat[2];
    __shared__ int sfar;
    const int b = blockIdx.x / groups, gi = blockIdx.x % groups;
    const int cpg = C / groups, c0 = gi * cpg, cq = cpg >> 2;
    float* Ys = lds; float* Zs = lds + (size_t)G * cpg; int* Is = reinterpret_cast<int*>(lds + (size_t)2 * G * cpg);     // Is[j][g]
    for (int i = threadIdx.x; i < G * cq; i += EGF_THREADS) {
        const int g = i / cq, c4 = (i % cq) * 4;
        const float* row = yz + ((size_t)b * G + g) * ldy + c0 + c4;
        *reinterpret_cast<float4*>(&Ys[g * cpg + c4]) = *reinterpret_cast<const float4*>(row);
        *reinterpret_cast<float4*>(&Zs[g * cpg + c4]) = *reinterpret_cast<const float4*>(row + zoff);
    }
    for (int i = threadIdx.x; i < k * G; i += EGF_THREADS) Is[i] = (int)idx[(size_t)b * k * G + i];
    __syncthreads();
    // statistics of pre = Y[src] + Z over (G, k, cpg), pivot = first element; channel fastest across the threads (conflict-free LDS rows)
    const float pv = Ys[Is[0] * cpg] + Zs[0];
    const int total = G * cpg;
    float s = 0.f, q = 0.f;
    for (int i = threadIdx.x; i < total; i += EGF_THREADS) {
        const int g = i / cpg, c = i % cpg;
        const float z = Zs[i] - pv;
        for (int j = 0; j < k; ++j) { const float v = Ys[Is[j * G + g] * cpg + c] + z; s += v; q += v * v; }
    }
    s = wave_sum_f32(s); q = wave_sum_f32(q);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float S = 0.f, Q = 0.f;
        for (int w = 0; w < EGF_THREADS / 64; ++w) { S += sh[0][w]; Q += sh[1][w]; }
        const float n = (float)G * (float)k * (float)cpg;
        const float dm = S / n, var = fmaxf(Q / n - dm * dm, 0.f);
        stat[0] = pv + dm; stat[1] = rsqrtf(var + eps);
        mean_out[blockIdx.x] = stat[0]; rstd_out[blockIdx.x] = stat[1];
        sfar = dm * dm > FAR_PIVOT * var;
    }
    __syncthreads();
    if (sfar) {
        // far pivot (see edge_gn_finalize_kernel): the slice is in LDS, so the workgroup sums it once more around the mean it has just found
        const float mu0 = stat[0];
        s = 0.f; q = 0.f;
        for (int i = threadIdx.x; i < total; i += EGF_THREADS) {
            const int g = i / cpg, c = i % cpg;
            const float z = Zs[i] - mu0;
            for (int j = 0; j < k; ++j) { const float v = Ys[Is[j * G + g] * cpg + c] + z; s += v; q += v * v; }
        }
        s = wave_sum_f32(s); q = wave_sum_f32(q);
        if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = q; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float S = 0.f, Q = 0.f;
            for (int w = 0; w < EGF_THREADS / 64; ++w) { S += sh[0][w]; Q += sh[1][w]; }
            const float n = (float)G * (float)k * (float)cpg;
            const float d2 = S / n, var = fmaxf(Q / n - d2 * d2, 0.f);
            stat[0] = mu0 + d2; stat[1] = rsqrtf(var + eps);
            mean_out[blockIdx.x] = stat[0]; rstd_out[blockIdx.x] = stat[1];
        }
        __syncthreads();
    }
    const float mu = stat[0], rs = stat[1];
    for (int i = threadIdx.x; i < total; i += EGF_THREADS) {
        const int g = i / cpg, c = i % cpg;
        float vmax = -3.0e38f, vmin = 3.0e38f;
        for (int j = 0; j < k; ++j) { const float v = Ys[Is[j * G + g] * cpg + c]; vmax = fmaxf(vmax, v); vmin = fminf(vmin, v); }
        const float a = rs * gamma[c0 + c];
        const float v = (a >= 0.f ? vmax : vmin) + Zs[i];
        out[((size_t)b * G + g) * ldo + ooff + c0 + c] = lrelu((v - mu) * a + beta[c0 + c], slope);
    }
}

// ---- slab form of the three-kernel path for graph layers whose (sample, group) slice does not fit the LDS (round 6: the stress geometry, G = 512) ----------
// edge_gn_stats_kernel / edge_gn_apply_max_kernel walk k global gathers (and k int64 index loads) per output element: 0.57 TB/s of compulsory traffic at
// 16,384 rows x 512 / 1,024 channels.  Here a workgroup = (sample, SW-channel slab) copies its [G][SW] slab of Y into LDS with unconditional, independent loads
// (SW = 32 at G <= 512: 64 KB, two workgroups per CU), the k = 4 source rows of every g come from an int4 table in LDS, Z and the output are touched once,
// coalesced.  Statistics: one partial (sum, sum of squares around the group's pivot) per slab, written into the GN_SPLIT slots of edge_gn_finalize_kernel
// (a group has cpg / SW <= GN_SPLIT slabs; slab 0 zeroes the unused slots), so the finalize stage is shared with the generic path.
template <int SW, bool APPLY>
__global__ __launch_bounds__(256) void edge_gn_slab_kernel(const float* __restrict__ yz, int ldy, int zoff, const int64_t* __restrict__ idx, int G, int C,
                                                           int groups, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                           float* __restrict__ part, float* __restrict__ out, int ldo, int ooff) {
    constexpr int K = 4, GL = 256 / SW;                      // g-lanes per workgroup
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float sh[2][4];
    float* ys = lds; int* es = reinterpret_cast<int*>(lds + (size_t)G * SW);        // Y slab [G][SW] | edges [G][K]
    const int cl = threadIdx.x % SW, gl = threadIdx.x / SW;
    const int c = blockIdx.x * SW + cl, b = blockIdx.y;                              // (C % SW == 0: every lane is live)
    const int cpg = C / groups, gi = (blockIdx.x * SW) / cpg, c0 = gi * cpg;
    const float* yb = yz + (size_t)b * G * ldy;
#pragma unroll 8
    for (int g = gl; g < G; g += GL) ys[g * SW + cl] = yb[(size_t)g * ldy + c];
    for (int e = threadIdx.x; e < K * G; e += 256) { const int j = e / G, g = e - j * G; es[g * K + j] = (int)idx[(size_t)b * K * G + e]; }
    __syncthreads();
    const int4* e4 = reinterpret_cast<const int4*>(es);
    if (!APPLY) {
        // pivot = first element of the GROUP (what edge_gn_finalize_kernel adds back)
        const int r00 = (int)idx[(size_t)b * K * G];
        const float pv = yb[(size_t)r00 * ldy + c0] + yb[zoff + c0];
        float s1 = 0.f, q1 = 0.f;
#pragma unroll 4
        for (int g = gl; g < G; g += GL) {
            const int4 sv = e4[g];
            const float z = yb[(size_t)g * ldy + zoff + c] - pv;
            const float t[K] = {ys[sv.x * SW + cl] + z, ys[sv.y * SW + cl] + z, ys[sv.z * SW + cl] + z, ys[sv.w * SW + cl] + z};
#pragma unroll
            for (int j = 0; j < K; ++j) { s1 += t[j]; q1 += t[j] * t[j]; }
        }
        s1 = wave_sum_f32(s1); q1 = wave_sum_f32(q1);
        if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s1; sh[1][threadIdx.x >> 6] = q1; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int nsl = cpg / SW, sl = (blockIdx.x * SW - c0) / SW;              // slabs per group, this slab's index inside its group
            float* pp = part + ((size_t)(b * groups + gi) * GN_SPLIT) * 2;
            pp[sl * 2 + 0] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
            pp[sl * 2 + 1] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
            if (sl == 0) for (int u = nsl; u < GN_SPLIT; ++u) { pp[u * 2] = 0.f; pp[u * 2 + 1] = 0.f; }
        }
    } else {
        const float mu = mean[b * groups + gi], a = rstd[b * groups + gi] * gamma[c], bt = beta[c];
        float* ob = out + (size_t)b * G * ldo + ooff + c;
#pragma unroll 4
        for (int g = gl; g < G; g += GL) {
            const int4 sv = e4[g];
            const float t0 = ys[sv.x * SW + cl], t1 = ys[sv.y * SW + cl], t2 = ys[sv.z * SW + cl], t3 = ys[sv.w * SW + cl];
            const float vmax = fmaxf(fmaxf(t0, t1), fmaxf(t2, t3)), vmin = fminf(fminf(t0, t1), fminf(t2, t3));
            const float v = (a >= 0.f ? vmax : vmin) + yb[(size_t)g * ldy + zoff + c];
            ob[(size_t)g * ldo] = lrelu((v - mu) * a + bt, slope);
        }
    }
}

extern "C" int act_edge_gn_lrelu_max_f32(const float* yz, int ldy, int zoff, const int64_t* idx, int B, int G, int k, int C,
                                         int groups, const float* gamma, const float* beta, float eps, float slope,
                                         float* stats /* [18][B*groups] */, float* out, int ldo, int ooff, act_stream_t stream) {
    if (!yz || !gamma || !beta || !stats || !out) return ACT_E_NULLPTR;
    if (B <= 0 || G <= 0 || k <= 0 || C <= 0 || groups <= 0 || C % groups) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    // compulsory bytes (round 6): y (and z) [B G, C] read once, out written once, the k-neighbour index list read once -- the k gathers of both passes hit
    // rows that are already on the chip (the previous model counted them as 2k reads of HBM)
    ActProfScope ps(KID_GN_LRELU_MAX, s, 0.0, 4.0 * B * G * (double)C * ((zoff >= 0 ? 2 : 1) + 1) + 8.0 * B * G * (double)k);
    float* mean = stats; float* rstd = stats + (size_t)B * groups;
    float* part = stats + (size_t)2 * B * groups;
    {
        static const bool fuse = [] { const char* e = getenv("ACT_EDGE_GN_FUSE"); return !(e && e[0] == '0'); }();
        const int cpg = C / groups;
        const size_t smem = ((size_t)2 * G * cpg + (size_t)k * G) * sizeof(float);
        if (fuse && idx && zoff >= 0 && (cpg & 3) == 0 && (ldy & 3) == 0 && (zoff & 3) == 0 && smem <= 140 * 1024 &&
            (reinterpret_cast<uintptr_t>(yz) & 15) == 0) {
            if (smem > 48 * 1024) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(edge_gn_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
                if (e != hipSuccess) return (int)e;
            }
            hipLaunchKernelGGL(edge_gn_fused_kernel, dim3(B * groups), dim3(EGF_THREADS), smem, s, yz, ldy, zoff, idx, G, k, C, groups, gamma, beta, eps, slope,
                               mean, rstd, out, ldo, ooff);
            ACT_LAUNCH_CHECK(); return 0;
        }
    }
    {   // slab form (round 6): graph layers with k = 4 whose slice is too large for the single-kernel path -- Y slab of 32 channels in LDS, G <= 512
        static const bool slab = [] { const char* e = getenv("ACT_EDGE_GN_SLAB"); return !(e && e[0] == '0'); }();
        const int cpg = C / groups;
        constexpr int SW = 32;
        const size_t smem = ((size_t)G * SW + (size_t)4 * G) * sizeof(float);
        if (slab && idx && zoff >= 0 && k == 4 && (cpg % SW) == 0 && cpg / SW <= GN_SPLIT && smem <= 72 * 1024) {
            auto ks = edge_gn_slab_kernel<SW, false>; auto ka = edge_gn_slab_kernel<SW, true>;
            if (smem > 48 * 1024) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ks), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
                if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(ka), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
                if (e != hipSuccess) return (int)e;
            }
            hipLaunchKernelGGL(ks, dim3(C / SW, B), dim3(256), smem, s, yz, ldy, zoff, idx, G, C, groups, mean, rstd, gamma, beta, slope, part, out, ldo, ooff);
            hipLaunchKernelGGL(edge_gn_finalize_kernel, dim3(B * groups), dim3(256), 0, s, yz, ldy, zoff, idx, G, k, C, groups,
                               part, eps, mean, rstd);
            hipLaunchKernelGGL(ka, dim3(C / SW, B), dim3(256), smem, s, yz, ldy, zoff, idx, G, C, groups, mean, rstd, gamma, beta, slope, part, out, ldo, ooff);
            ACT_LAUNCH_CHECK(); return 0;
        }
    }
    hipLaunchKernelGGL(edge_gn_stats_kernel, dim3(B * groups, GN_SPLIT), dim3(256), 0, s, yz, ldy, zoff, idx, G, k, C, groups, part);
    hipLaunchKernelGGL(edge_gn_finalize_kernel, dim3(B * groups), dim3(256), 0, s, yz, ldy, zoff, idx, G, k, C, groups,
                       part, eps, mean, rstd);
    const long long total = (long long)B * G * C;
    hipLaunchKernelGGL(edge_gn_apply_max_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, yz, ldy, zoff, idx, G, k, C, groups, mean, rstd,
                       gamma, beta, slope, out, ldo, ooff, total);
    ACT_LAUNCH_CHECK(); return 0;
}

// ------------------------------------------------------------------------------------------------ edge-conv tail, backward
// Forward (above): out[b,g,c] = max_j lrelu(GN(pre[b,g,c,j])), pre = Y[b, idx[b,j,g], c] + Z[b,g,c].  With j* the selected
// neighbour, dact = dout * lrelu'(.) at j* and zero elsewhere, and GroupNorm's backward over the (C/groups, G, k) group is
//   dpre[g,c,j] = rstd * ( gamma[c] * dact * [j == j*]  -  m1  -  xhat[g,c,j] * m2 )
//   m1 = mean(gamma * dact) , m2 = mean(gamma * dact * xhat)   (means over the whole group, zeros included)
//   dZ[b,g,c] = sum_j dpre ;  dY[b,r,c] = sum over the edges (g,j) with idx[b,j,g] == r of dpre   (fixed order: deterministic)
//   dgamma[c] = sum_{b,g} dact * xhat* ; dbeta[c] = sum_{b,g} dact.
__device__ __forceinline__ void edge_select(const float* __restrict__ yz, int ldy, const int64_t* __restrict__ idx, int b, int g, int G,
                                            int k, int c, float a, float& vsel, int& jsel) {
    vsel = 0.f; jsel = 0;
    for (int j = 0; j < k; ++j) {
        const int src = idx ? (int)idx[((size_t)b * k + j) * G + g] : g;
        const float v = yz[((size_t)b * G + src) * ldy + c];
        if (j == 0 || (a >= 0.f ? v > vsel : v < vsel)) { vsel = v; jsel = j; }     // first extremum wins (torch.max)
    }
}
// pass 1: per (sample, channel) partial sums over g:  part[0][b][c] = sum_g dact*xhat*, part[1][b][c] = sum_g dact
// workgroup = 64 channels x 4 g-lanes (the g loop is a chain of dependent gathers: four lanes per channel + unrolling keep
// enough loads in flight); lanes are folded through LDS in a fixed order
__global__ __launch_bounds__(256) void edge_gn_bwd_partials_kernel(const float* __restrict__ yz, int ldy, int zoff,
                                                                   const int64_t* __restrict__ idx, int B, int G, int k, int C, int groups,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float slope, const float* __restrict__ dout, int ldd,
                                                                   float* __restrict__ part) {
    __shared__ float red[2][3][64];
    const int cl = threadIdx.x & 63, gl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    float sg = 0.f, sb = 0.f;
    if (c < C) {
        const int gi = c / (C / groups);
        const float mu = mean[b * groups + gi], rs = rstd[b * groups + gi], gm = gamma[c], bt = beta[c], a = rs * gm;
#pragma unroll 2
        for (int g = gl; g < G; g += 4) {
            float v; int js;
            edge_select(yz, ldy, idx, b, g, G, k, c, a, v, js);
            if (zoff >= 0) v += yz[((size_t)b * G + g) * ldy + zoff + c];
            const float xh = (v - mu) * rs;
            const float y = xh * gm + bt;
            const float da = dout[((size_t)b * G + g) * ldd + c] * (y > 0.f ? 1.f : slope);
            sg += da * xh; sb += da;
        }
    }
    if (gl > 0) { red[0][gl - 1][cl] = sg; red[1][gl - 1][cl] = sb; }
    __syncthreads();
    if (gl == 0 && c < C) {
        part[((size_t)0 * B + b) * C + c] = (sg + red[0][0][cl]) + (red[0][1][cl] + red[0][2][cl]);
        part[((size_t)1 * B + b) * C + c] = (sb + red[1][0][cl]) + (red[1][1][cl] + red[1][2][cl]);
    }
}
// pass 2: one workgroup per (sample, group): m1 = sum_c gamma*db_part / N, m2 = sum_c gamma*dg_part / N
__global__ __launch_bounds__(256) void edge_gn_bwd_means_kernel(const float* __restrict__ part, const float* __restrict__ gamma, int B,
                                                                int C, int groups, float inv_n, float* __restrict__ mstat) {
    __shared__ float sh[2][4];
    const int b = blockIdx.x / groups, gi = blockIdx.x % groups, cpg = C / groups;
    float s1 = 0.f, s2 = 0.f;
    for (int c = gi * cpg + threadIdx.x; c < (gi + 1) * cpg; c += 256) {
        s1 += gamma[c] * part[((size_t)1 * B + b) * C + c];
        s2 += gamma[c] * part[((size_t)0 * B + b) * C + c];
    }
    s1 = wave_sum_f32(s1); s2 = wave_sum_f32(s2);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s1; sh[1][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mstat[blockIdx.x] = ((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) * inv_n;
        mstat[(size_t)B * groups + blockIdx.x] = ((sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3])) * inv_n;
    }
}
// pass 3 (graph layers): workgroup = (sample, 64 channels) x GL g-lanes; every (g-lane, channel) thread owns one column of its
// lane's LDS accumulator [G][64] for the dY scatter (no cross-thread races, fixed order), the GL lane images are summed at the end
template <int GL>
__global__ __launch_bounds__(64 * GL) void edge_gn_bwd_apply_kernel(const float* __restrict__ yz, int ldy, int zoff,
                                                                     const int64_t* __restrict__ idx, int B, int G,
                                         int k, int C, int groups, const float* __restrict__ mean, const float* __restrict__ rstd,
                                         const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                         const float* __restrict__ dout, int ldd, const float* __restrict__ mstat,
                                         float* __restrict__ dyz) {
    extern __shared__ float acc[];                          // [GL][G][64]
    const int cl = threadIdx.x & 63, gl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    float* mine = acc + (size_t)gl * G * 64;
    for (int r = 0; r < G; ++r) mine[r * 64 + cl] = 0.f;
    if (c < C) {
        const int gi = c / (C / groups);
        const float mu = mean[b * groups + gi], rs = rstd[b * groups + gi], gm = gamma[c], bt = beta[c], a = rs * gm;
        const float m1 = mstat[b * groups + gi], m2 = mstat[(size_t)B * groups + b * groups + gi];
#pragma unroll 2
        for (int g = gl; g < G; g += GL) {
            float vs; int js;
            edge_select(yz, ldy, idx, b, g, G, k, c, a, vs, js);
            const float z = zoff >= 0 ? yz[((size_t)b * G + g) * ldy + zoff + c] : 0.f;
            const float xs = (vs + z - mu) * rs;
            const float da = dout[((size_t)b * G + g) * ldd + c] * (xs * gm + bt > 0.f ? 1.f : slope) * gm;
            float dz = 0.f;
            for (int j = 0; j < k; ++j) {
                const int src = idx ? (int)idx[((size_t)b * k + j) * G + g] : g;
                const float xh = (yz[((size_t)b * G + src) * ldy + c] + z - mu) * rs;
                const float dp = rs * ((j == js ? da : 0.f) - m1 - xh * m2);
                dz += dp;
                mine[src * 64 + cl] += dp;
            }
            if (zoff >= 0) dyz[((size_t)b * G + g) * ldy + zoff + c] = dz;
        }
    }
    __syncthreads();
    if (c < C)
        for (int r = gl; r < G; r += GL) {
            float v = acc[r * 64 + cl];
#pragma unroll
            for (int l = 1; l < GL; ++l) v += acc[((size_t)l * G + r) * 64 + cl];
            dyz[((size_t)b * G + r) * ldy + c] = v;
        }
}
// pass 3 (head, k = 1, no gather, no Z): plain elementwise
__global__ __launch_bounds__(256) void gn_lrelu_bwd_apply_kernel(const float* __restrict__ h, int G, int C, int groups,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                                 const float* __restrict__ dout, int ldd, const float* __restrict__ mstat,
                                                                 int B, float* __restrict__ dh, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C); const long long row = i / C; const int b = (int)(row / G);
        const int gi = c / (C / groups);
        const float rs = rstd[b * groups + gi], gm = gamma[c];
        const float xh = (h[i] - mean[b * groups + gi]) * rs;
        const float da = dout[(size_t)row * ldd + c] * (xh * gm + beta[c] > 0.f ? 1.f : slope) * gm;
        dh[i] = rs * (da - mstat[b * groups + gi] - xh * mstat[(size_t)B * groups + b * groups + gi]);
    }
}

// ---- LDS-resident forms of passes 1 and 3 (round 6; G <= 128) ------------------------------------------------------------------------------
// The kernels above walk a chain of dependent global gathers per (g, neighbour) with four loads in flight per thread: 0.8 TB/s on the Stage-I shapes
// (8,192 rows x 512 / 1,024 channels).  Here a workgroup = (sample, 64 channels) first copies its [G][64] slabs of Y (and Z) into LDS with coalesced,
// independent loads -- every operand is read from HBM exactly once -- and all gathers become conflict-free LDS reads (lane = channel).
// Pass 3 also replaces the four [G][64] scatter images by a GATHER over the incoming edges of each row: an inverse adjacency (CSR over the k G edges of
// the sample, built in LDS by one thread per row) lists a row's edges in ascending (g, j); deterministic, same terms as the kernels above in another
// fixed order (agreement to fp32 rounding: tests/test_gpu_dense.py).
template <bool HASZ>
__global__ __launch_bounds__(256) void edge_gn_bwd_partials_lds_kernel(const float* __restrict__ yz, int ldy, int zoff,
                                                                       const int64_t* __restrict__ idx, int B, int G, int k, int C, int groups,
                                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                       float slope, const float* __restrict__ dout, int ldd,
                                                                       float* __restrict__ part) {
    extern __shared__ float lds[];                          // Y slab [G][64] | idx [k][G] (int)
    __shared__ float red[2][3][64];
    float* ys = lds; int* es = reinterpret_cast<int*>(lds + (size_t)G * 64);
    const int cl = threadIdx.x & 63, gl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    const bool live = c < C;
    const int cc = live ? c : C - 1;                        // unconditional loads (see the apply kernel): dead lanes read a valid column
#pragma unroll 8
    for (int r = gl; r < G; r += 4) ys[r * 64 + cl] = yz[((size_t)b * G + r) * ldy + cc];
    for (int e = threadIdx.x; e < k * G; e += 256) es[e] = (int)idx[(size_t)b * k * G + e];
    __syncthreads();
    float sg = 0.f, sb = 0.f;
    if (live) {
        const int gi = c / (C / groups);
        const float mu = mean[b * groups + gi], rs = rstd[b * groups + gi], gm = gamma[c], bt = beta[c], a = rs * gm;
#pragma unroll 4
        for (int g = gl; g < G; g += 4) {
            float v = 0.f;
            for (int j = 0; j < k; ++j) {
                const float t = ys[es[j * G + g] * 64 + cl];
                if (j == 0 || (a >= 0.f ? t > v : t < v)) v = t;
            }
            if (HASZ) v += yz[((size_t)b * G + g) * ldy + zoff + c];
            const float xh = (v - mu) * rs;
            const float y = xh * gm + bt;
            const float da = dout[((size_t)b * G + g) * ldd + c] * (y > 0.f ? 1.f : slope);
            sg += da * xh; sb += da;
        }
    }
    if (gl > 0) { red[0][gl - 1][cl] = sg; red[1][gl - 1][cl] = sb; }
    __syncthreads();
    if (gl == 0 && live) {
        part[((size_t)0 * B + b) * C + c] = (sg + red[0][0][cl]) + (red[0][1][cl] + red[0][2][cl]);
        part[((size_t)1 * B + b) * C + c] = (sb + red[1][0][cl]) + (red[1][1][cl] + red[1][2][cl]);
    }
}
// K = 4 (the DGCNN graphs) as a compile-time constant: with a runtime neighbour count the inner loops stay rolled and every LDS round trip of the dependent
// chain index -> gather -> select is exposed (measured per phase on the Stage-I shapes: 19 + 37 + 29 us of a 104 us launch; 20 us is the HBM time).
// MAXI = rows per g-lane as a compile-time bound (16: G <= 64, 32: G <= 128): the unrolled bodies are code, and the first version's 70 KB of it did not fit the
// instruction cache two CUs share
template <bool HASZ, int K, int MAXI>
__global__ __launch_bounds__(256) void edge_gn_bwd_apply_lds_kernel(const float* __restrict__ yz, int ldy, int zoff,
                                                                    const int64_t* __restrict__ idx, int B, int G, int C, int groups,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                                    const float* __restrict__ dout, int ldd, const float* __restrict__ mstat,
                                                                    float* __restrict__ dyz) {
    static_assert(K == 4, "edge list entries are int4 rows");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // Y [G][64] | Z [G][64] | da [G][64] | js [G][64] (int) | edges [G][K] (int, row g = its K source rows) | CSR [K G + 1] (int: g << 8 | j; last = dump slot)
    float* ys = lds; float* zs = ys + (size_t)G * 64; float* das = zs + (size_t)G * 64;
    int* jss = reinterpret_cast<int*>(das + (size_t)G * 64);
    int* es = jss + (size_t)G * 64; int* csr = es + K * G;
    __shared__ int s_base[128], s_tot[128];
    const int cl = threadIdx.x & 63, gl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (wave-uniform: the row guards below are scalar branches)
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    const bool live = c < C;
    const int cc = live ? c : C - 1;                        // dead lanes of a ragged last slab read a valid column and store nothing
    const int ni = (G - gl + 3) >> 2;                       // rows g = gl + 4 i of this g-lane
    // every global operand of the slab is requested up front, UNCONDITIONALLY (a predicated load becomes an exec-masked branch with a full wait behind it:
    // the first version serialised its 48 loads that way): Y, Z -> registers -> LDS, dout stays in registers (one value per (g, channel) of this thread)
    float dreg[MAXI], yv[MAXI], zv[MAXI];
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
        const size_t row = (size_t)b * G + min(gl + 4 * i, G - 1);
        yv[i] = yz[row * ldy + cc];
        zv[i] = HASZ ? yz[row * ldy + zoff + cc] : 0.f;
        dreg[i] = dout[row * ldd + cc];
    }
#pragma unroll
    for (int i = 0; i < MAXI; ++i)
        if (i < ni) {
            const int r = gl + 4 * i;
            ys[r * 64 + cl] = yv[i];
            if (HASZ) zs[r * 64 + cl] = zv[i];
        }
    for (int e = threadIdx.x; e < K * G; e += 256) { const int j = e / G, g = e - j * G; es[g * K + j] = (int)idx[(size_t)b * K * G + e]; }
    __syncthreads();
    // inverse adjacency (CSR over the K G edges, edges of a row in ascending (g, j)): one thread per row, int4 reads of the edge table
    const int4* e4 = reinterpret_cast<const int4*>(es);
    if ((int)threadIdx.x < G) {
        const int r = threadIdx.x;
        int cnt = 0;
#pragma unroll 8
        for (int g = 0; g < G; ++g) { const int4 v = e4[g]; cnt += (v.x == r) + (v.y == r) + (v.z == r) + (v.w == r); }
        s_tot[r] = cnt;
    }
    __syncthreads();
    if ((int)threadIdx.x < G) {
        int acc = 0;
        for (int q = 0; q < (int)threadIdx.x; ++q) acc += s_tot[q];
        s_base[threadIdx.x] = acc;
        const int r = threadIdx.x;
        int p = acc;
        const int dump = K * G;                              // branch-free fill: a non-matching edge is written to the dump slot
#pragma unroll 4
        for (int g = 0; g < G; ++g) {
            const int4 v = e4[g];
            csr[v.x == r ? p : dump] = (g << 8) | 0; p += v.x == r;
            csr[v.y == r ? p : dump] = (g << 8) | 1; p += v.y == r;
            csr[v.z == r ? p : dump] = (g << 8) | 2; p += v.z == r;
            csr[v.w == r ? p : dump] = (g << 8) | 3; p += v.w == r;
        }
    }
    float mu = 0.f, rs = 0.f, gm = 0.f, bt = 0.f, a = 0.f, m1 = 0.f, m2 = 0.f;
    if (live) {
        const int gi = c / (C / groups);
        mu = mean[b * groups + gi]; rs = rstd[b * groups + gi]; gm = gamma[c]; bt = beta[c]; a = rs * gm;
        m1 = mstat[b * groups + gi]; m2 = mstat[(size_t)B * groups + b * groups + gi];
#pragma unroll
        for (int i = 0; i < MAXI; ++i) {
            if (i < ni) {
                const int g = gl + 4 * i;
                const int4 sv = e4[g];
                const float t[K] = {ys[sv.x * 64 + cl], ys[sv.y * 64 + cl], ys[sv.z * 64 + cl], ys[sv.w * 64 + cl]};
                float vs = t[0]; int js = 0;
#pragma unroll
                for (int j = 1; j < K; ++j) if (a >= 0.f ? t[j] > vs : t[j] < vs) { vs = t[j]; js = j; }      // first extremum wins (torch.max)
                const float z = HASZ ? zs[g * 64 + cl] : 0.f;
                const float xs = (vs + z - mu) * rs;
                const float da = dreg[i] * (xs * gm + bt > 0.f ? 1.f : slope) * gm;
                das[g * 64 + cl] = da; jss[g * 64 + cl] = js;
                if (HASZ) {
                    float dz = 0.f;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const float xh = (t[j] + z - mu) * rs;
                        dz += rs * ((j == js ? da : 0.f) - m1 - xh * m2);
                    }
                    dyz[((size_t)b * G + g) * ldy + zoff + c] = dz;
                }
            }
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll 2
        for (int i = 0; i < ni; ++i) {
            const int r = gl + 4 * i;
            const float yr = ys[r * 64 + cl];
            const int base = s_base[r], n = s_tot[r];
            float acc = 0.f;
            for (int p0 = 0; p0 < n; p0 += 4) {                      // four edges per trip, branch-free: their LDS reads are independent, the sum keeps the edge order
                int e[4]; float zz[4], dd[4]; int jj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) e[u] = csr[base + min(p0 + u, n - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int g = e[u] >> 8;
                    zz[u] = HASZ ? zs[g * 64 + cl] : 0.f; dd[u] = das[g * 64 + cl]; jj[u] = jss[g * 64 + cl];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float xh = (yr + zz[u] - mu) * rs;
                    const float term = rs * (((e[u] & 255) == jj[u] ? dd[u] : 0.f) - m1 - xh * m2);
                    acc += p0 + u < n ? term : 0.f;
                }
            }
            dyz[((size_t)b * G + r) * ldy + c] = acc;
        }
    }
}
static std::atomic<int> g_edge_bwd_lds{[] { const char* e = getenv("ACT_EDGE_BWD_LDS"); return e ? atoi(e) : 1; }()};
// runtime switch (A/B, bit-identity test): 1 (default) = the LDS-resident backward passes where G <= 128, 0 = the global-gather kernels; on < 0 only reads
extern "C" int act_edge_bwd_lds(int on) { return on < 0 ? g_edge_bwd_lds.load() : g_edge_bwd_lds.exchange(on ? 1 : 0); }

extern "C" int act_edge_gn_lrelu_max_bwd_f32(const float* yz, int ldy, int zoff, const int64_t* idx, int B, int G, int k, int C, int groups,
                                             const float* gamma, const float* beta, const float* stats, float slope,
                                             const float* dout, int ldd, float* dyz, float* part /* [2][B][C] */,
                                             float* mstat /* [2][B*groups] */, act_stream_t stream) {
    if (!yz || !gamma || !beta || !stats || !dout || !dyz || !part || !mstat) return ACT_E_NULLPTR;
    if (B <= 0 || G <= 0 || k <= 0 || C <= 0 || groups <= 0 || C % groups || (!idx && (k != 1 || zoff >= 0))) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    // compulsory bytes: y (and z) and dout read once, dy (and dz) written once, index list read once
    ActProfScope ps(KID_GN_LRELU_MAX, s, 0.0, 4.0 * B * G * (double)C * (2.0 * (zoff >= 0 ? 2 : 1) + 1.0) + 8.0 * B * G * (double)k);
    const float* mean = stats; const float* rstd = stats + (size_t)B * groups;
    const bool use_lds = idx && G <= 128 && k == 4 && g_edge_bwd_lds.load() != 0;      // (k = 4: the DGCNN graphs; other neighbour counts keep the generic kernels)
    if (use_lds) {
        const size_t sm1 = ((size_t)G * 64 + (size_t)k * G) * sizeof(float);
        if (zoff >= 0) hipLaunchKernelGGL(edge_gn_bwd_partials_lds_kernel<true>, dim3((C + 63) / 64, B), dim3(256), sm1, s, yz, ldy, zoff, idx, B, G, k, C, groups,
                                          mean, rstd, gamma, beta, slope, dout, ldd, part);
        else           hipLaunchKernelGGL(edge_gn_bwd_partials_lds_kernel<false>, dim3((C + 63) / 64, B), dim3(256), sm1, s, yz, ldy, zoff, idx, B, G, k, C, groups,
                                          mean, rstd, gamma, beta, slope, dout, ldd, part);
    } else
    hipLaunchKernelGGL(edge_gn_bwd_partials_kernel, dim3((C + 63) / 64, B), dim3(256), 0, s, yz, ldy, zoff, idx, B, G, k, C, groups, mean,
                       rstd, gamma, beta, slope, dout, ldd, part);
    const float inv_n = 1.0f / ((float)(C / groups) * (float)G * (float)k);
    hipLaunchKernelGGL(edge_gn_bwd_means_kernel, dim3(B * groups), dim3(256), 0, s, part, gamma, B, C, groups, inv_n, mstat);
    if (use_lds) {
        const size_t sm3 = ((size_t)4 * G * 64 + (size_t)2 * k * G + 4) * sizeof(float);
#define APPLY_LDS(Z, MI) { auto kfn = edge_gn_bwd_apply_lds_kernel<Z, 4, MI>; \
            if (sm3 > 48 * 1024) { hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm3); if (e != hipSuccess) return (int)e; } \
            hipLaunchKernelGGL(kfn, dim3((C + 63) / 64, B), dim3(256), sm3, s, yz, ldy, zoff, idx, B, G, C, groups, mean, rstd, gamma, beta, slope, dout, ldd, mstat, dyz); }
        if (zoff >= 0) { if (G <= 64) APPLY_LDS(true, 16) else APPLY_LDS(true, 32) }
        else           { if (G <= 64) APPLY_LDS(false, 16) else APPLY_LDS(false, 32) }
#undef APPLY_LDS
    } else if (!idx) {
        const long long total = (long long)B * G * C;
        hipLaunchKernelGGL(gn_lrelu_bwd_apply_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, yz, G, C, groups, mean, rstd, gamma, beta,
                           slope, dout, ldd, mstat, B, dyz, total);
    } else {
        if (G > 512) return ACT_E_BADARG;
        const int GL = G <= 128 ? 4 : (G <= 256 ? 2 : 1);                       // lane images of [G][64] floats each: <= 128 KB of LDS
        const size_t smem = (size_t)GL * G * 64 * sizeof(float);
#define APPLY(N) { auto kfn = edge_gn_bwd_apply_kernel<N>; \
            if (smem > 48 * 1024) { hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); if (e != hipSuccess) return (int)e; } \
            hipLaunchKernelGGL(kfn, dim3((C + 63) / 64, B), dim3(64 * N), smem, s, yz, ldy, zoff, idx, B, G, k, C, groups, mean, rstd, gamma, \
                               beta, slope, dout, ldd, mstat, dyz); }
        if (GL == 4) APPLY(4) else if (GL == 2) APPLY(2) else APPLY(1)
#undef APPLY
    }
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_gn_gumbel_argmax_gather_f32(const float* h, int B, int G, int C, int groups, const float* gamma, const float* beta,
                                               float eps, float slope, const float* noise, uint64_t seed, const uint64_t* seed_dev,
                                               float tau, const float* codebook, int D, float* stats, int64_t* index_out, float* out,
                                               float* logits_out, act_stream_t stream) {
    if (!h || !gamma || !beta || !codebook || !stats || !out) return ACT_E_NULLPTR;
    if (B <= 0 || G <= 0 || C <= 0 || (C & 3) || groups <= 0 || C % groups || D <= 0 || tau <= 0.f) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GUMBEL_ARGMAX, s, 0.0, 4.0 * B * G * ((double)C * (2 + (noise ? 1 : 0) + (logits_out ? 1 : 0)) + 2.0 * D));
    float* mean = stats; float* rstd = stats + (size_t)B * groups;
    float* part = stats + (size_t)2 * B * groups;
    hipLaunchKernelGGL(edge_gn_stats_kernel, dim3(B * groups, GN_SPLIT), dim3(256), 0, s, h, C, -1, nullptr, G, 1, C, groups, part);
    hipLaunchKernelGGL(edge_gn_finalize_kernel, dim3(B * groups), dim3(256), 0, s, h, C, -1, nullptr, G, 1, C, groups,
                       part, eps, mean, rstd);
    hipLaunchKernelGGL(gumbel_argmax_gather_kernel, dim3(B * G), dim3(256), 0, s, h, G, C, groups, mean, rstd, gamma, beta, slope, noise, seed,
                       seed_dev, 1.0f / tau, codebook, D, index_out, out, logits_out);
    ACT_LAUNCH_CHECK(); return 0;
}

// ------------------------------------------------------------------------------------- Stage-I tokenizer: soft gumbel-softmax + KL
// y[row,:] = softmax((logits[row,:] + gumbel) / tau)  (F.gumbel_softmax(hard=False), models/dvae.py:600); one workgroup per row,
// the row lives in LDS between the three passes so the Philox noise is generated exactly once.
__global__ __launch_bounds__(256) void gumbel_softmax_fwd_kernel(const float* __restrict__ logits, int C, const float* __restrict__ noise,
                                                                 uint64_t seed, float inv_tau, float* __restrict__ y) {
    extern __shared__ float row_s[];
    __shared__ float red[4];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = -3.0e38f;
    for (int c4 = threadIdx.x * 4; c4 < C; c4 += 1024) {
        const float4 x = *reinterpret_cast<const float4*>(logits + (size_t)row * C + c4);
        const float xs[4] = {x.x, x.y, x.z, x.w};
        uint32_t rnd[4] = {0, 0, 0, 0};
        if (!noise) philox_draw(seed, (uint32_t)(c4 >> 2), (uint32_t)row, PHILOX_DOMAIN_GUMBEL, 0u, rnd);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float g = noise ? noise[(size_t)row * C + c4 + u] : gumbel_from_bits(rnd[u]);
            const float t = (xs[u] + g) * inv_tau;
            row_s[c4 + u] = t; m = fmaxf(m, t);
        }
    }
    m = wave_max_f32(m, -3.4e38f);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float se = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) { const float e = __expf(row_s[c] - m); row_s[c] = e; se += e; }
    se = wave_sum_f32(se);
    if (lane == 0) red[wave] = se;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    for (int c = threadIdx.x; c < C; c += 256) y[(size_t)row * C + c] = row_s[c] * inv;
}
// dlogits = y * (dy - sum_c y*dy) / tau
__global__ __launch_bounds__(256) void gumbel_softmax_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, int C,
                                                                 float inv_tau, float* __restrict__ dl) {
    __shared__ float red[4];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* yr = y + (size_t)row * C; const float* dr = dy + (size_t)row * C;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) s += yr[c] * dr[c];
    s = wave_sum_f32(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    for (int c = threadIdx.x; c < C; c += 256) dl[(size_t)row * C + c] = yr[c] * (dr[c] - s) * inv_tau;
}
// KL(mean_g softmax(logits) || uniform), 'batchmean' (models/dvae.py:470-476):
//   lse[row] = logsumexp(logits[row,:]) ; qbar[b,c] = mean_g exp(logits[b,g,c] - lse[b,g]) ;
//   klv = (1/B) sum_{b,c} u (log u - log qbar[b,c]),  u = 1/C
__global__ __launch_bounds__(256) void row_lse_kernel(const float* __restrict__ logits, int C, float* __restrict__ lse) {
    __shared__ float red[4];
    const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* lr = logits + (size_t)row * C;
    float m = -3.0e38f;
    for (int c = threadIdx.x; c < C; c += 256) m = fmaxf(m, lr[c]);
    m = wave_max_f32(m, -3.4e38f);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float se = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) se += __expf(lr[c] - m);
    se = wave_sum_f32(se);
    if (lane == 0) red[wave] = se;
    __syncthreads();
    if (threadIdx.x == 0) lse[row] = m + __logf((red[0] + red[1]) + (red[2] + red[3]));
}
__global__ __launch_bounds__(256) void mean_softmax_kernel(const float* __restrict__ logits, const float* __restrict__ lse, int G, int C,
                                                           float* __restrict__ qbar) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    float acc = 0.f;
    for (int g = 0; g < G; ++g) acc += __expf(logits[((size_t)b * G + g) * C + c] - lse[b * G + g]);
    qbar[(size_t)b * C + c] = acc / (float)G;
}
__global__ __launch_bounds__(1024) void kl_uniform_kernel(const float* __restrict__ qbar, long long n, int B, int C, float* __restrict__ out) {
    __shared__ float sh[16];
    const float u = 1.0f / (float)C, lu = __logf(u);
    float acc = 0.f;
    // consecutive threads read consecutive elements (a contiguous chunk per thread put every lane on its own cache line: 478 us for 1 M values)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    long long i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        a0 += u * (lu - __logf(qbar[i])); a1 += u * (lu - __logf(qbar[i + 1024]));
        a2 += u * (lu - __logf(qbar[i + 2048])); a3 += u * (lu - __logf(qbar[i + 3072]));
    }
    for (; i < n; i += 1024) a0 += u * (lu - __logf(qbar[i]));
    acc = (a0 + a1) + (a2 + a3);
    acc = wave_sum_f32(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) { float t = 0.f; for (int w = 0; w < 16; ++w) t += sh[w]; out[0] = t / (float)B; }
}
// dlogits[b,g,c] = p (w_c - sum_c' p_c' w_c'),  p = exp(logits - lse),  w_c = dklv * (-u / (B * qbar[b,c])) / G
__global__ __launch_bounds__(256) void kl_uniform_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                             const float* __restrict__ qbar, const float* __restrict__ gout, int B, int G,
                                                             int C, float* __restrict__ dl) {
    __shared__ float red[4];
    const int row = blockIdx.x, b = row / G, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* lr = logits + (size_t)row * C; const float* qb = qbar + (size_t)b * C;
    const float l0 = lse[row], k = -gout[0] / ((float)C * (float)B * (float)G);
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) s += __expf(lr[c] - l0) * (k / qb[c]);
    s = wave_sum_f32(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    for (int c = threadIdx.x; c < C; c += 256) dl[(size_t)row * C + c] = __expf(lr[c] - l0) * (k / qb[c] - s);
}

extern "C" int act_gumbel_softmax_fwd_f32(const float* logits, int R, int C, const float* noise, uint64_t seed, float tau, float* y,
                                          act_stream_t stream) {
    if (!logits || !y) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || (C & 3) || C > 16384 || tau <= 0.f) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GUMBEL_ARGMAX, s, 0.0, 4.0 * R * (double)C * (2 + (noise ? 1 : 0)));
    const size_t smem = (size_t)C * sizeof(float);
    auto k = gumbel_softmax_fwd_kernel;
    if (smem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3(R), dim3(256), smem, s, logits, C, noise, seed, 1.0f / tau, y);
    ACT_LAUNCH_CHECK(); return 0;
}
extern "C" int act_gumbel_softmax_bwd_f32(const float* y, const float* dy, int R, int C, float tau, float* dlogits, act_stream_t stream) {
    if (!y || !dy || !dlogits) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || tau <= 0.f) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GUMBEL_ARGMAX, s, 0.0, 12.0 * R * (double)C);
    hipLaunchKernelGGL(gumbel_softmax_bwd_kernel, dim3(R), dim3(256), 0, s, y, dy, C, 1.0f / tau, dlogits);
    ACT_LAUNCH_CHECK(); return 0;
}
extern "C" int act_kl_uniform_fwd_f32(const float* logits, int B, int G, int C, float* lse /*[B*G]*/, float* qbar /*[B,C]*/,
                                      float* klv_out, act_stream_t stream) {
    if (!logits || !lse || !qbar || !klv_out) return ACT_E_NULLPTR;
    if (B <= 0 || G <= 0 || C <= 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GUMBEL_ARGMAX, s, 0.0, 8.0 * B * G * (double)C);
    hipLaunchKernelGGL(row_lse_kernel, dim3(B * G), dim3(256), 0, s, logits, C, lse);
    hipLaunchKernelGGL(mean_softmax_kernel, dim3((C + 255) / 256, B), dim3(256), 0, s, logits, lse, G, C, qbar);
    hipLaunchKernelGGL(kl_uniform_kernel, dim3(1), dim3(1024), 0, s, qbar, (long long)B * C, B, C, klv_out);
    ACT_LAUNCH_CHECK(); return 0;
}
extern "C" int act_kl_uniform_bwd_f32(const float* logits, const float* lse, const float* qbar, const float* grad_klv, int B, int G, int C,
                                      float* dlogits, act_stream_t stream) {
    if (!logits || !lse || !qbar || !grad_klv || !dlogits) return ACT_E_NULLPTR;
    if (B <= 0 || G <= 0 || C <= 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GUMBEL_ARGMAX, s, 0.0, 12.0 * B * G * (double)C);
    hipLaunchKernelGGL(kl_uniform_bwd_kernel, dim3(B * G), dim3(256), 0, s, logits, lse, qbar, grad_klv, B, G, C, dlogits);
    ACT_LAUNCH_CHECK(); return 0;
}
