// tsne.hip -- exact t-SNE of classifier features (tools/runner_tsne.py: openTSNE's TSNE(perplexity=25, metric="cosine") on the concat_f features),
// embedded on the device.  Stages, each a C entry of its own:
//     kNN graph      x^ = x / |x| once; 1 - x^_i . x^_j in slabs of TSNE_SLAB rows (64 x 64 tile per workgroup, the slab is the only N-wide buffer);
//                    per row a bitwise k-th-value search on the ordered keys, a k-th-index search among the ties, a compaction and a rank sort:
//                    ascending distance, ties to the lower index, the row itself excluded.  A row of zero norm has x^ = 0: distance 1 to every row.
//     conditional p  per row (one wave) the bisection on beta of sklearn / openTSNE in float64: entropy of exp(-beta (d - d_min)) = log(perplexity)
//     P as CSR       in-degree count and list fill with INTEGER atomics, every list then rank-sorted (a function of idx alone), rows merged from the
//                    sorted neighbours and the sorted in-list: count -> scan -> fill
//     step           tsne_repulse_kernel: the exact all-pairs sweep (Z and sum_j w^2 (y_i - y_j)), j range split across workgroups, fp32 inside a
//                    64-pair chunk, float64 across chunks, partials per split;  tsne_update_kernel: partials in split order, attractive term along
//                    the CSR row, gains / momentum / Y + update;  tsne_centre_kernel: Y -= mean(Y).   act_tsne_steps_f32 repeats the three launches.
//     KL             sum P (log P - log w + log Z) in float64 into one device double
//     PCA init       column means, centred copy, D x D covariance by the TN GEMM, two leading eigenvectors by orthogonal iteration (float64, one
//                    workgroup) and a Rayleigh-Ritz rotation, projection, first column scaled to standard deviation 1e-4
// Reductions have a fixed order (lane-strided partial sums, xor butterfly, blocks / splits in index order), float64 wherever many terms meet.  The
// only atomics are integer ones (counts and list cursors) whose effect is removed by a sort: every output is bit-identical run to run.
#include "common.h"
#include <math.h>

#define TSNE_MAXK 1024       // neighbours per row (perplexity <= 341)
#define TSNE_MAXD 1024       // feature width of the PCA initialisation (two float64 D x 2 panels live in LDS)
#define TSNE_SLAB 512        // rows of one distance slab
#define TSNE_KC 32
#define TSNE_LDT (64 + 4)
#define TSNE_UROWS 16        // rows per workgroup of the update kernel (4 per wave)
#define TSNE_PCA_SWEEPS 500
#define TSNE_PCA_TOL 1e-10

static inline size_t tsne_up(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int tsne_cdiv(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ double tsne_wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < ACT_WAVE; o <<= 1) v += __shfl_xor(v, o, ACT_WAVE);
    return v;                                        // the same bits in every lane
}
__device__ __forceinline__ int tsne_wave_sum_i(int v) {
#pragma unroll
    for (int o = 1; o < ACT_WAVE; o <<= 1) v += __shfl_xor(v, o, ACT_WAVE);
    return v;
}
// sum over a 256-thread workgroup, waves in index order; red: 8 doubles, slots alternate with `pass` so that one barrier per call is enough
__device__ __forceinline__ double tsne_block_sum(double v, double* red, int pass) {
    v = tsne_wave_sum(v);
    double* r = red + (pass & 1) * 4;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((r[0] + r[1]) + r[2]) + r[3];
}
__device__ __forceinline__ int tsne_block_sum_i(int v, int* red, int pass) {
    v = tsne_wave_sum_i(v);
    int* r = red + (pass & 1) * 4;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    return r[0] + r[1] + r[2] + r[3];
}
// sum of n doubles by one wave: lane l owns l, l + 64, ...
__device__ __forceinline__ double tsne_list_sum(const double* __restrict__ p, int n, int stride, int lane) {
    double s = 0.0;
    for (int i = lane; i < n; i += ACT_WAVE) s += p[(size_t)i * stride];
    return tsne_wave_sum(s);
}

// ---- a. cosine kNN graph ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_normalize_kernel(const float* __restrict__ X, int N, int D, float* __restrict__ Xh) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* x = X + (size_t)row * D;
    double ss = 0.0;
    for (int d = lane; d < D; d += ACT_WAVE) ss += (double)x[d] * (double)x[d];
    ss = tsne_wave_sum(ss);
    const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
    for (int d = lane; d < D; d += ACT_WAVE) Xh[(size_t)row * D + d] = (float)((double)x[d] * inv);
}

template <bool VEC>
__device__ __forceinline__ float4 tsne_load4(const float* __restrict__ src, int r, int rows, int k, int D) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) {
        const float* p = src + (size_t)r * D + k;
        if (VEC) {
            if (k < D) v = *reinterpret_cast<const float4*>(p);
        } else {
            if (k < D) v.x = p[0];
            if (k + 1 < D) v.y = p[1];
            if (k + 2 < D) v.z = p[2];
            if (k + 3 < D) v.w = p[3];
        }
    }
    return v;
}

// slab[r - row0, j] = 1 - x^_r . x^_j for r in [row0, row0 + rows), j in [0, N): 64 x 64 tile per workgroup, 4 x 4 per lane
template <bool VEC>
__global__ __launch_bounds__(256) void tsne_dist_kernel(const float* __restrict__ Xh, int N, int D, int row0, int rows, float* __restrict__ slab) {
    __shared__ __attribute__((aligned(16))) float As[TSNE_KC][TSNE_LDT];      // [k][row]
    __shared__ __attribute__((aligned(16))) float Bs[TSNE_KC][TSNE_LDT];      // [k][column]
    const int tid = threadIdx.x, r0 = row0 + blockIdx.y * 64, c0 = blockIdx.x * 64, rend = row0 + rows;
    const int cg = tid & 15, rg = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    const int kq = (tid & 7) * 4;
    for (int k0 = 0; k0 < D; k0 += TSNE_KC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = (tid >> 3) + 32 * h;
            const float4 av = tsne_load4<VEC>(Xh, r0 + r, rend, k0 + kq, D);
            const float4 bv = tsne_load4<VEC>(Xh, c0 + r, N, k0 + kq, D);
            As[kq][r] = av.x; As[kq + 1][r] = av.y; As[kq + 2][r] = av.z; As[kq + 3][r] = av.w;
            Bs[kq][r] = bv.x; Bs[kq + 1][r] = bv.y; Bs[kq + 2][r] = bv.z; Bs[kq + 3][r] = bv.w;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < TSNE_KC; ++k) {
            const float4 xa = *reinterpret_cast<const float4*>(&As[k][rg * 4]);
            const float4 xb = *reinterpret_cast<const float4*>(&Bs[k][cg * 4]);
            const float ar[4] = {xa.x, xa.y, xa.z, xa.w}, bc[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], bc[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gi = r0 + rg * 4 + i;
        if (gi >= rend) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + cg * 4 + j;
            if (c < N) slab[(size_t)(gi - row0) * N + c] = 1.f - acc[i][j];
        }
    }
}

// floats in increasing order <-> unsigned keys in increasing order
__device__ __forceinline__ uint32_t tsne_key(float d) {
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// one workgroup per row of the slab: the k smallest keys (ties: the lowest indices), then a rank sort by (key, index)
__global__ __launch_bounds__(256) void tsne_select_kernel(const float* __restrict__ slab, int row0, int N, int k, int32_t* __restrict__ idx,
                                                          float* __restrict__ dist) {
    __shared__ int red[8];
    __shared__ uint32_t skey[TSNE_MAXK];
    __shared__ int sidx[TSNE_MAXK];
    __shared__ int scount;
    const int tid = threadIdx.x, i = row0 + blockIdx.x;
    const float* __restrict__ d = slab + (size_t)blockIdx.x * N;
    int pass = 0;
    uint32_t T = 0;                                           // the largest T with #(key < T) < k is the k-th smallest key
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        int c = 0;
        for (int j = tid; j < N; j += 256) {
            const uint32_t key = j == i ? 0xFFFFFFFFu : tsne_key(d[j]);
            c += key < cand;
        }
        if (tsne_block_sum_i(c, red, pass++) < k) T = cand;
    }
    int c = 0;
    for (int j = tid; j < N; j += 256) c += (j == i ? 0xFFFFFFFFu : tsne_key(d[j])) < T;
    const int need = k - tsne_block_sum_i(c, red, pass++);    // >= 1 entries come from the keys equal to T: those of the lowest indices
    int I = 0;
    for (int bit = 31 - __clz(N | 1); bit >= 0; --bit) {
        const int cand = I | (1 << bit);
        c = 0;
        for (int j = tid; j < N; j += 256) c += (j != i && j < cand && tsne_key(d[j]) == T);
        if (tsne_block_sum_i(c, red, pass++) < need) I = cand;
    }
    if (tid == 0) scount = 0;
    __syncthreads();
    for (int j = tid; j < N; j += 256) {
        if (j == i) continue;
        const uint32_t key = tsne_key(d[j]);
        if (key < T || (key == T && j <= I)) {
            const int s = atomicAdd(&scount, 1);                  // integer slot counter; the order is fixed by the sort below
            if (s < TSNE_MAXK) { skey[s] = key; sidx[s] = j; }
        }
    }
    __syncthreads();
    for (int e = tid; e < k; e += 256) {
        const uint32_t ke = skey[e];
        const int je = sidx[e];
        int rank = 0;
        for (int f = 0; f < k; ++f) rank += (skey[f] < ke) || (skey[f] == ke && sidx[f] < je);
        idx[(size_t)i * k + rank] = je;
        dist[(size_t)i * k + rank] = d[je];
    }
}

// ---- b. perplexity search ---------------------------------------------------------------------------------------------------------------------
// one wave per row; float64 throughout.  beta doubles while the upper bound is open, halves while the lower one is, else bisects.
__global__ __launch_bounds__(256) void tsne_cond_p_kernel(const float* __restrict__ dist, int N, int k, double log_perp, float* __restrict__ p,
                                                          float* __restrict__ beta_out) {
    __shared__ double sd[4][TSNE_MAXK];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * 4 + w;
    if (row >= N) return;
    const float* dr = dist + (size_t)row * k;
    float m = INFINITY;
    for (int a = lane; a < k; a += ACT_WAVE) m = fminf(m, dr[a]);
#pragma unroll
    for (int o = 1; o < ACT_WAVE; o <<= 1) m = fminf(m, __shfl_xor(m, o, ACT_WAVE));
    for (int a = lane; a < k; a += ACT_WAVE) sd[w][a] = (double)dr[a] - (double)m;
    double beta = 1.0, lo = -INFINITY, hi = INFINITY, sumP = 1.0;
    for (int step = 0; step < 100; ++step) {
        double sp = 0.0, sdp = 0.0;
        for (int a = lane; a < k; a += ACT_WAVE) {
            const double dd = sd[w][a], pv = exp(-beta * dd);
            sp += pv;
            sdp += dd * pv;
        }
        sumP = tsne_wave_sum(sp);                             // >= 1: the nearest neighbour contributes exp(0)
        const double H = log(sumP) + beta * tsne_wave_sum(sdp) / sumP;
        const double diff = H - log_perp;
        if (fabs(diff) < 1e-5 || step == 99) break;           // wave-uniform: every lane holds the same sums
        if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : 0.5 * (beta + hi);
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5 : 0.5 * (beta + lo);
        }
    }
    for (int a = lane; a < k; a += ACT_WAVE) p[(size_t)row * k + a] = (float)(exp(-beta * sd[w][a]) / sumP);
    if (beta_out && lane == 0) beta_out[row] = (float)beta;
}

// ---- c. symmetrisation to CSR -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_indeg_kernel(const int32_t* __restrict__ idx, int E, int N, int* __restrict__ cnt) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int j = idx[e];
    if (j >= 0 && j < N) atomicAdd(&cnt[j], 1);
}
// exclusive scan of n ints by one workgroup; out[n] = the total
__global__ __launch_bounds__(1024) void tsne_scan_kernel(const int* __restrict__ in, int n, int* __restrict__ out) {
    __shared__ int part[1024];
    const int t = threadIdx.x, chunk = (n + 1023) / 1024, b = min(n, t * chunk), e = min(n, b + chunk);
    int s = 0;
    for (int i = b; i < e; ++i) s += in[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int j = 0; j < 1024; ++j) { const int v = part[j]; part[j] = acc; acc += v; }
        out[n] = acc;
    }
    __syncthreads();
    int acc = part[t];
    for (int i = b; i < e; ++i) { const int v = in[i]; out[i] = acc; acc += v; }
}
__global__ __launch_bounds__(256) void tsne_infill_kernel(const int32_t* __restrict__ idx, int E, int N, const int* __restrict__ off,
                                                          int* __restrict__ cursor, int* __restrict__ tmp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int j = idx[e];
    if (j >= 0 && j < N) tmp[off[j] + atomicAdd(&cursor[j], 1)] = e;
}
// one workgroup per list: the edges e = source * k + slot that point at j, in increasing e (every e occurs once: the rank is a permutation)
__global__ __launch_bounds__(256) void tsne_insort_kernel(const int* __restrict__ off, const int* __restrict__ tmp, int* __restrict__ ent) {
    __shared__ int chunk[1024];
    const int j = blockIdx.x, tid = threadIdx.x, b = off[j], L = off[j + 1] - b;
    for (int a0 = 0; a0 < L; a0 += 256) {
        const int a = a0 + tid;
        const int va = a < L ? tmp[b + a] : 0;
        int rank = 0;
        for (int c0 = 0; c0 < L; c0 += 1024) {
            const int m = min(1024, L - c0);
            __syncthreads();
            for (int q = tid; q < m; q += 256) chunk[q] = tmp[b + c0 + q];
            __syncthreads();
            for (int q = 0; q < m; ++q) rank += chunk[q] < va;
        }
        if (a < L) ent[b + rank] = va;
    }
}
__device__ __forceinline__ int tsne_lower_bound_ent(const int* __restrict__ In, int L, int k, int j) {       // # entries whose source is < j
    int lo = 0, hi = L;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (In[m] / k < j) lo = m + 1; else hi = m; }
    return lo;
}
__device__ __forceinline__ int tsne_lower_bound_lds(const int* s, int n, int j) {
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (s[m] < j) lo = m + 1; else hi = m; }
    return lo;
}
// one workgroup per row i: the union of the neighbours of i (sorted here) and the sorted in-list of i.  FILL = false: the row's length only
template <bool FILL>
__global__ __launch_bounds__(256) void tsne_csr_kernel(const int32_t* __restrict__ idx, const float* __restrict__ p, int N, int k,
                                                       const int* __restrict__ off, const int* __restrict__ ent, int* __restrict__ rowcnt,
                                                       const int* __restrict__ indptr, int32_t* __restrict__ indices, float* __restrict__ values) {
    __shared__ int sraw[TSNE_MAXK], sj[TSNE_MAXK], sslot[TSNE_MAXK], slb[TSNE_MAXK], spos[TSNE_MAXK], spre[TSNE_MAXK + 1];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int* In = ent + off[i];
    const int L = off[i + 1] - off[i];
    for (int a = tid; a < k; a += 256) sraw[a] = idx[(size_t)i * k + a];
    __syncthreads();
    for (int a = tid; a < k; a += 256) {
        const int j = sraw[a];
        int rank = 0;
        for (int f = 0; f < k; ++f) rank += sraw[f] < j || (sraw[f] == j && f < a);
        sj[rank] = j; sslot[rank] = a;
    }
    __syncthreads();
    for (int a = tid; a < k; a += 256) {
        const int lb = tsne_lower_bound_ent(In, L, k, sj[a]);
        slb[a] = lb;
        spos[a] = (lb < L && In[lb] / k == sj[a]) ? lb : -1;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int a = 0; a < k; ++a) { spre[a] = acc; acc += spos[a] >= 0; }
        spre[k] = acc;
    }
    __syncthreads();
    if (!FILL) {
        if (tid == 0) rowcnt[i] = k + L - spre[k];
        return;
    }
    const int base = indptr[i];
    const double inv2n = 1.0 / (2.0 * (double)N);
    for (int a = tid; a < k; a += 256) {
        const int pos = base + a + slb[a] - spre[a];
        const double pa = (double)p[(size_t)i * k + sslot[a]], pb = spos[a] >= 0 ? (double)p[In[spos[a]]] : 0.0;
        indices[pos] = sj[a];
        values[pos] = (float)((pa + pb) * inv2n);
    }
    for (int t = tid; t < L; t += 256) {
        const int e = In[t], j = e / k;
        const int lb = tsne_lower_bound_lds(sj, k, j);
        if (lb < k && sj[lb] == j) continue;
        const int pos = base + lb + t - spre[lb];
        indices[pos] = j;
        values[pos] = (float)((double)p[e] * inv2n);
    }
}

// ---- d. one optimisation step -----------------------------------------------------------------------------------------------------------------
// j range of a split (a multiple of 64) so that about 1024 workgroups run
static inline int tsne_split_len(int N) {
    const int nib = tsne_cdiv(N, 256), want = tsne_cdiv(1024, nib);
    const int L = tsne_cdiv(tsne_cdiv(N, want), 64) * 64;
    return L < 64 ? 64 : L;
}
static inline int tsne_splits(int N) { return tsne_cdiv(N, tsne_split_len(N)); }

// the all-pairs sweep: thread = one i, workgroup = 256 i x one j split.  part[split][i] = sum_j w^2 (y_i - y_j), zpart[split][i block] = sum w over the
// block's pairs (the diagonal's exact 1.0 per row included; the reader subtracts N).  fp32 inside a 64-pair chunk, float64 across chunks.
__global__ __launch_bounds__(256) void tsne_repulse_kernel(const float2* __restrict__ Y, int N, int L, float2* __restrict__ part,
                                                           double* __restrict__ zpart) {
    __shared__ float2 ys[256];
    __shared__ double red[8];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid, split = blockIdx.y;
    const int jbeg = split * L, jend = min(N, jbeg + L);
    const float2 yi = i < N ? Y[i] : make_float2(0.f, 0.f);
    double dsw = 0.0, dfx = 0.0, dfy = 0.0;
    for (int c0 = jbeg; c0 < jend; c0 += 256) {
        const int m = min(256, jend - c0);
        __syncthreads();
        if (tid < m) ys[tid] = Y[c0 + tid];
        __syncthreads();
        for (int q0 = 0; q0 < m; q0 += 64) {
            const int n = min(64, m - q0);
            float sw = 0.f, fx = 0.f, fy = 0.f;
#pragma unroll 8
            for (int q = 0; q < n; ++q) {
                const float2 yj = ys[q0 + q];
                const float dx = yi.x - yj.x, dy = yi.y - yj.y;
                const float w = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
                const float w2 = w * w;
                sw += w;
                fx = fmaf(w2, dx, fx);
                fy = fmaf(w2, dy, fy);
            }
            dsw += (double)sw; dfx += (double)fx; dfy += (double)fy;
        }
    }
    if (i < N) part[(size_t)split * N + i] = make_float2((float)dfx, (float)dfy);
    const double z = tsne_block_sum(i < N ? dsw : 0.0, red, 0);
    if (tid == 0) zpart[(size_t)split * gridDim.x + blockIdx.x] = z;
}

struct TsneStepArgs {
    const int32_t *indptr, *indices;
    const float* values;
    const float2* Y;
    int N, S, nzp;
    const float2* part;
    const double* zpart;
    float ex, mom, lr;
    float2 *upd, *gains, *Ytmp;
    double2* cpart;
};
__device__ __forceinline__ float tsne_sign(float v) { return (float)((v > 0.f) - (v < 0.f)); }
__device__ __forceinline__ void tsne_gain_update(double g, float& gain, float& upd, float mom, float lr) {
    const float gf = (float)g;
    gain = tsne_sign(gf) != tsne_sign(upd) ? gain + 0.2f : gain * 0.8f;
    gain = fmaxf(gain, 0.01f);
    upd = (float)((double)mom * (double)upd - (double)lr * (double)gain * g);
}
// wave = 4 rows, one after the other: gradient, gains, update, Ytmp = Y + update; cpart[block] = the block's column sums of Ytmp (float64)
__global__ __launch_bounds__(256) void tsne_update_kernel(TsneStepArgs a) {
    __shared__ double2 wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double Z = tsne_list_sum(a.zpart, a.nzp, 1, lane) - (double)a.N;         // sum over i != j; the same bits in every wave of the grid
    const double invZ = 1.0 / Z;
    double cx = 0.0, cy = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int i = blockIdx.x * TSNE_UROWS + w * 4 + q;
        if (i >= a.N) break;
        const float2 yi = a.Y[i];
        double ax = 0.0, ay = 0.0;
        for (int e = a.indptr[i] + lane; e < a.indptr[i + 1]; e += ACT_WAVE) {
            const float2 yj = a.Y[a.indices[e]];
            const double dx = (double)yi.x - (double)yj.x, dy = (double)yi.y - (double)yj.y;
            const double pw = (double)a.values[e] / (1.0 + dx * dx + dy * dy);
            ax += pw * dx; ay += pw * dy;
        }
        double rx = 0.0, ry = 0.0;
        for (int s = lane; s < a.S; s += ACT_WAVE) {
            const float2 v = a.part[(size_t)s * a.N + i];
            rx += (double)v.x; ry += (double)v.y;
        }
        ax = tsne_wave_sum(ax); ay = tsne_wave_sum(ay); rx = tsne_wave_sum(rx); ry = tsne_wave_sum(ry);
        const double gx = (double)a.ex * ax - rx * invZ, gy = (double)a.ex * ay - ry * invZ;
        float2 gain = a.gains[i], upd = a.upd[i];
        tsne_gain_update(gx, gain.x, upd.x, a.mom, a.lr);
        tsne_gain_update(gy, gain.y, upd.y, a.mom, a.lr);
        const float2 yn = make_float2(yi.x + upd.x, yi.y + upd.y);
        if (lane == 0) { a.gains[i] = gain; a.upd[i] = upd; a.Ytmp[i] = yn; }
        cx += (double)yn.x; cy += (double)yn.y;
    }
    if (lane == 0) wsum[w] = make_double2(cx, cy);
    __syncthreads();
    if (threadIdx.x == 0)
        a.cpart[blockIdx.x] = make_double2(((wsum[0].x + wsum[1].x) + wsum[2].x) + wsum[3].x, ((wsum[0].y + wsum[1].y) + wsum[2].y) + wsum[3].y);
}
__global__ __launch_bounds__(256) void tsne_centre_kernel(const float2* __restrict__ Ytmp, const double2* __restrict__ cpart, int ncp, int N,
                                                          float2* __restrict__ Y) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 256 + threadIdx.x;
    const double* c = reinterpret_cast<const double*>(cpart);
    const double mx = tsne_list_sum(c, ncp, 2, lane) / (double)N, my = tsne_list_sum(c + 1, ncp, 2, lane) / (double)N;
    if (i >= N) return;
    const float2 v = Ytmp[i];
    Y[i] = make_float2((float)((double)v.x - mx), (float)((double)v.y - my));
}

// ---- e. KL divergence -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_kl_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const float* __restrict__ values, const float2* __restrict__ Y, int N,
                                                      const double* __restrict__ zpart, int nzp, double* __restrict__ kpart) {
    __shared__ double wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double logZ = log(tsne_list_sum(zpart, nzp, 1, lane) - (double)N);
    double acc = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int i = blockIdx.x * TSNE_UROWS + w * 4 + q;
        if (i >= N) break;
        const float2 yi = Y[i];
        double s = 0.0;
        for (int e = indptr[i] + lane; e < indptr[i + 1]; e += ACT_WAVE) {
            const double P = (double)values[e];
            if (!(P > 0.0)) continue;
            const float2 yj = Y[indices[e]];
            const double dx = (double)yi.x - (double)yj.x, dy = (double)yi.y - (double)yj.y;
            s += P * (log(P) + log(1.0 + dx * dx + dy * dy) + logZ);                     // log P - log w + log Z
        }
        acc += tsne_wave_sum(s);
    }
    if (lane == 0) wsum[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) kpart[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
__global__ __launch_bounds__(ACT_WAVE) void tsne_kl_finish_kernel(const double* __restrict__ kpart, int n, double* __restrict__ out) {
    const double s = tsne_list_sum(kpart, n, 1, threadIdx.x);
    if (threadIdx.x == 0) out[0] = s;
}

// ---- f. PCA initialisation --------------------------------------------------------------------------------------------------------------------
// part[split][d] = sum of column d over the rows of the split (float64, rows in order)
__global__ __launch_bounds__(256) void tsne_colsum_kernel(const float* __restrict__ X, int N, int D, int rows_per_split, double* __restrict__ part) {
    __shared__ double red[4][ACT_WAVE];
    const int c = threadIdx.x & 63, ry = threadIdx.x >> 6, d = blockIdx.x * 64 + c;
    const int rbeg = blockIdx.y * rows_per_split, rend = min(N, rbeg + rows_per_split);
    double s = 0.0;
    if (d < D)
        for (int r = rbeg + ry; r < rend; r += 4) s += (double)X[(size_t)r * D + d];
    red[ry][c] = s;
    __syncthreads();
    if (ry == 0 && d < D) part[(size_t)blockIdx.y * D + d] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}
__global__ __launch_bounds__(256) void tsne_colmean_kernel(const double* __restrict__ part, int nsplit, int N, int D, double* __restrict__ mean) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) s += part[(size_t)sp * D + d];
    mean[d] = s / (double)N;
}
__global__ __launch_bounds__(256) void tsne_centre_rows_kernel(const float* __restrict__ X, const double* __restrict__ mean, size_t total, int D,
                                                               float* __restrict__ Xc) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) Xc[e] = (float)((double)X[e] - mean[e % D]);
}
// two leading eigenvectors of the symmetric C [D,D] (fp32) by orthogonal iteration in float64, one workgroup.  vec [2][D], info [4]: the two Ritz
// values, the sweeps run, the last subspace change |(I - V V^T) V_new|_F
__global__ __launch_bounds__(256) void tsne_eig2_kernel(const float* __restrict__ C, int D, double* __restrict__ vec, double* __restrict__ info) {
    __shared__ double V[2][TSNE_MAXD], W[2][TSNE_MAXD];
    __shared__ double red[8];
    const int tid = threadIdx.x;
    int pass = 0;
    auto bsum = [&](double v) { return tsne_block_sum(v, red, pass++); };
    auto product = [&]() {                                    // W = C V; C is symmetric: column r is read as row-major C[d][r] (coalesced over r)
        for (int r = tid; r < D; r += 256) {
            double s0 = 0.0, s1 = 0.0;
            for (int d = 0; d < D; ++d) {
                const double c = (double)C[(size_t)d * D + r];
                s0 += c * V[0][d]; s1 += c * V[1][d];
            }
            W[0][r] = s0; W[1][r] = s1;
        }
        __syncthreads();
    };
    auto orthonormalise = [&](double (*A)[TSNE_MAXD]) {       // Gram-Schmidt, a vanishing column stays zero
        double s = 0.0;
        for (int d = tid; d < D; d += 256) s += A[0][d] * A[0][d];
        const double n0 = sqrt(bsum(s)), i0 = n0 > 0.0 ? 1.0 / n0 : 0.0;
        s = 0.0;
        for (int d = tid; d < D; d += 256) { A[0][d] *= i0; s += A[0][d] * A[1][d]; }
        const double dot = bsum(s);
        s = 0.0;
        for (int d = tid; d < D; d += 256) { A[1][d] -= dot * A[0][d]; s += A[1][d] * A[1][d]; }
        const double n1 = sqrt(bsum(s)), i1 = n1 > 0.0 ? 1.0 / n1 : 0.0;
        for (int d = tid; d < D; d += 256) A[1][d] *= i1;
        __syncthreads();
    };
    for (int d = tid; d < D; d += 256) {                      // a fixed start with a component along every direction
        V[0][d] = 1.0 + 0.5 * sin(1.0 + (double)d);
        V[1][d] = cos(2.0 + 1.7 * (double)d);
    }
    __syncthreads();
    orthonormalise(V);
    int sweeps = 0;
    double change = 0.0;
    for (; sweeps < TSNE_PCA_SWEEPS;) {
        product();
        orthonormalise(W);
        double m[4] = {0.0, 0.0, 0.0, 0.0};
        for (int d = tid; d < D; d += 256) {
            m[0] += V[0][d] * W[0][d]; m[1] += V[0][d] * W[1][d]; m[2] += V[1][d] * W[0][d]; m[3] += V[1][d] * W[1][d];
        }
        for (int q = 0; q < 4; ++q) m[q] = bsum(m[q]);
        double s = 0.0;
        for (int d = tid; d < D; d += 256) {
            const double r0 = W[0][d] - (V[0][d] * m[0] + V[1][d] * m[2]), r1 = W[1][d] - (V[0][d] * m[1] + V[1][d] * m[3]);
            s += r0 * r0 + r1 * r1;
        }
        change = sqrt(bsum(s));
        __syncthreads();
        for (int d = tid; d < D; d += 256) { V[0][d] = W[0][d]; V[1][d] = W[1][d]; }
        __syncthreads();
        ++sweeps;
        if (change < TSNE_PCA_TOL) break;                     // the same value in every thread
    }
    product();                                                // Rayleigh-Ritz inside the subspace: H = V^T C V, rotate V onto its eigenvectors
    double h[3] = {0.0, 0.0, 0.0};
    for (int d = tid; d < D; d += 256) { h[0] += V[0][d] * W[0][d]; h[1] += V[0][d] * W[1][d]; h[2] += V[1][d] * W[1][d]; }
    for (int q = 0; q < 3; ++q) h[q] = bsum(h[q]);
    const double th = 0.5 * atan2(2.0 * h[1], h[0] - h[2]), cs = cos(th), sn = sin(th);
    double l0 = cs * cs * h[0] + 2.0 * cs * sn * h[1] + sn * sn * h[2], l1 = sn * sn * h[0] - 2.0 * cs * sn * h[1] + cs * cs * h[2];
    const bool swap = l1 > l0;
    __syncthreads();
    for (int d = tid; d < D; d += 256) {
        const double u0 = cs * V[0][d] + sn * V[1][d], u1 = -sn * V[0][d] + cs * V[1][d];
        W[0][d] = swap ? u1 : u0; W[1][d] = swap ? u0 : u1;
    }
    __syncthreads();
    if (tid < 2) {                                            // the sign that makes the largest-magnitude entry (the first of equals) positive
        double best = -1.0, val = 1.0;
        for (int d = 0; d < D; ++d) {
            const double v = W[tid][d];
            if (fabs(v) > best) { best = fabs(v); val = v; }
        }
        red[tid] = val < 0.0 ? -1.0 : 1.0;
    }
    __syncthreads();
    for (int d = tid; d < D; d += 256) { vec[d] = red[0] * W[0][d]; vec[D + d] = red[1] * W[1][d]; }
    if (tid == 0) { info[0] = swap ? l1 : l0; info[1] = swap ? l0 : l1; info[2] = (double)sweeps; info[3] = change; }
}
// Yd[r] = Xc[r] . vec (float64); spart[block] = (sum y0, sum y0^2) over the block's 16 rows, in order
__global__ __launch_bounds__(256) void tsne_project_kernel(const float* __restrict__ Xc, const double* __restrict__ vec, int N, int D,
                                                           double2* __restrict__ Yd, double2* __restrict__ spart) {
    __shared__ double2 wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int r = blockIdx.x * TSNE_UROWS + w * 4 + q;
        if (r >= N) break;
        double a = 0.0, b = 0.0;
        for (int d = lane; d < D; d += ACT_WAVE) {
            const double x = (double)Xc[(size_t)r * D + d];
            a += x * vec[d]; b += x * vec[D + d];
        }
        a = tsne_wave_sum(a); b = tsne_wave_sum(b);
        if (lane == 0) Yd[r] = make_double2(a, b);
        s1 += a; s2 += a * a;
    }
    if (lane == 0) wsum[w] = make_double2(s1, s2);
    __syncthreads();
    if (threadIdx.x == 0)
        spart[blockIdx.x] = make_double2(((wsum[0].x + wsum[1].x) + wsum[2].x) + wsum[3].x, ((wsum[0].y + wsum[1].y) + wsum[2].y) + wsum[3].y);
}
__global__ __launch_bounds__(256) void tsne_rescale_kernel(const double2* __restrict__ Yd, const double2* __restrict__ spart, int nsp, int N,
                                                           float2* __restrict__ Y) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 256 + threadIdx.x;
    const double* c = reinterpret_cast<const double*>(spart);
    const double mean = tsne_list_sum(c, nsp, 2, lane) / (double)N, msq = tsne_list_sum(c + 1, nsp, 2, lane) / (double)N;
    const double var = msq - mean * mean, scale = var > 0.0 ? 1e-4 / sqrt(var) : 0.0;
    if (i >= N) return;
    const double2 v = Yd[i];
    Y[i] = make_float2((float)(v.x * scale), (float)(v.y * scale));
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------------
static inline bool tsne_vec_ok(const void* p, int D) { return (D % 4) == 0 && (((uintptr_t)p) & 15) == 0; }
static inline bool tsne_graph_ok(int N, int k) { return N >= 2 && N <= (1 << 24) && k >= 1 && k <= TSNE_MAXK && k < N && (long long)N * k < (1LL << 30); }
static inline int tsne_slab_rows(int N) { return N < TSNE_SLAB ? tsne_cdiv(N, 64) * 64 : TSNE_SLAB; }

extern "C" size_t act_tsne_knn_workspace(int N, int D) {
    if (N <= 0 || D <= 0) return 0;
    return tsne_up(sizeof(float) * (size_t)N * D) + tsne_up(sizeof(float) * (size_t)tsne_slab_rows(N) * N);
}

extern "C" int act_tsne_knn_cosine_f32(const float* X, int N, int D, int k, int32_t* idx, float* dist, void* workspace, size_t workspace_bytes,
                                       act_stream_t stream) {
    if (!X || !idx || !dist || !workspace) return ACT_E_NULLPTR;
    if (!tsne_graph_ok(N, k) || D < 1 || D > (1 << 16) || (long long)N * D >= (1LL << 31)) return ACT_E_BADARG;
    if (workspace_bytes < act_tsne_knn_workspace(N, D) || (((uintptr_t)workspace) & 15) != 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    float* Xh = (float*)workspace;
    float* slab = (float*)((char*)workspace + tsne_up(sizeof(float) * (size_t)N * D));
    hipLaunchKernelGGL(tsne_normalize_kernel, dim3(tsne_cdiv(N, 4)), dim3(256), 0, s, X, N, D, Xh);
    ACT_LAUNCH_CHECK();
    const int R = tsne_slab_rows(N);
    for (int row0 = 0; row0 < N; row0 += R) {
        const int rows = N - row0 < R ? N - row0 : R;
        const dim3 grid(tsne_cdiv(N, 64), tsne_cdiv(rows, 64));
        if (tsne_vec_ok(Xh, D))
            hipLaunchKernelGGL(tsne_dist_kernel<true>, grid, dim3(256), 0, s, (const float*)Xh, N, D, row0, rows, slab);
        else
            hipLaunchKernelGGL(tsne_dist_kernel<false>, grid, dim3(256), 0, s, (const float*)Xh, N, D, row0, rows, slab);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(tsne_select_kernel, dim3(rows), dim3(256), 0, s, (const float*)slab, row0, N, k, idx, dist);
        ACT_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int act_tsne_conditional_p_f32(const float* dist, int N, int k, float perplexity, float* p, float* beta, act_stream_t stream) {
    if (!dist || !p) return ACT_E_NULLPTR;
    if (N < 1 || N > (1 << 24) || k < 1 || k > TSNE_MAXK || !(perplexity >= 1.f) || (long long)N * k >= (1LL << 30)) return ACT_E_BADARG;
    hipLaunchKernelGGL(tsne_cond_p_kernel, dim3(tsne_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, dist, N, k, log((double)perplexity), p, beta);
    ACT_LAUNCH_CHECK();
    return 0;
}

// workspace of the symmetrisation: int32 cnt [N], cursor [N], off [N + 1], rowcnt [N], tmp [N k], ent [N k]
struct TsneSymCarve { int *cnt, *cursor, *off, *rowcnt, *tmp, *ent; size_t bytes; };
static TsneSymCarve tsne_sym_carve(void* base, int N, int k) {
    TsneSymCarve w;
    char* p = (char*)base;
    size_t o = 0;
    auto take = [&](size_t n) { void* q = p + o; o += tsne_up(n); return q; };
    w.cnt = (int*)take(4 * (size_t)N); w.cursor = (int*)take(4 * (size_t)N); w.off = (int*)take(4 * ((size_t)N + 1));
    w.rowcnt = (int*)take(4 * (size_t)N); w.tmp = (int*)take(4 * (size_t)N * k); w.ent = (int*)take(4 * (size_t)N * k);
    w.bytes = o;
    return w;
}
extern "C" size_t act_tsne_symmetrize_workspace(int N, int k) {
    if (N <= 0 || k <= 0) return 0;
    return tsne_sym_carve(nullptr, N, k).bytes;
}

extern "C" int act_tsne_symmetrize_f32(const int32_t* idx, const float* p, int N, int k, int32_t* indptr, int32_t* indices, float* values,
                                       long long capacity, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!idx || !p || !indptr || !indices || !values || !workspace) return ACT_E_NULLPTR;
    if (!tsne_graph_ok(N, k) || capacity < 2LL * N * k) return ACT_E_BADARG;
    if (workspace_bytes < act_tsne_symmetrize_workspace(N, k) || (((uintptr_t)workspace) & 15) != 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const TsneSymCarve w = tsne_sym_carve(workspace, N, k);
    const int E = N * k;
    hipError_t e = hipMemsetAsync(w.cnt, 0, (size_t)((char*)w.off - (char*)w.cnt), s);              // cnt and cursor
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(tsne_indeg_kernel, dim3(tsne_cdiv(E, 256)), dim3(256), 0, s, idx, E, N, w.cnt);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)w.cnt, N, w.off);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_infill_kernel, dim3(tsne_cdiv(E, 256)), dim3(256), 0, s, idx, E, N, (const int*)w.off, w.cursor, w.tmp);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_insort_kernel, dim3(N), dim3(256), 0, s, (const int*)w.off, (const int*)w.tmp, w.ent);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_csr_kernel<false>, dim3(N), dim3(256), 0, s, idx, p, N, k, (const int*)w.off, (const int*)w.ent, w.rowcnt,
                       (const int*)nullptr, (int32_t*)nullptr, (float*)nullptr);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)w.rowcnt, N, (int*)indptr);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_csr_kernel<true>, dim3(N), dim3(256), 0, s, idx, p, N, k, (const int*)w.off, (const int*)w.ent, w.rowcnt,
                       (const int*)indptr, indices, values);
    ACT_LAUNCH_CHECK();
    return 0;
}

// workspace of a step: part float2 [S][N], zpart float64 [S * i blocks], Ytmp float2 [N], cpart double2 [update blocks], kpart float64 [update blocks]
struct TsneStepCarve { float2 *part, *Ytmp; double *zpart, *kpart; double2* cpart; int S, L, nib, nub; size_t bytes; };
static TsneStepCarve tsne_step_carve(void* base, int N) {
    TsneStepCarve w;
    w.L = tsne_split_len(N); w.S = tsne_splits(N); w.nib = tsne_cdiv(N, 256); w.nub = tsne_cdiv(N, TSNE_UROWS);
    char* p = (char*)base;
    size_t o = 0;
    auto take = [&](size_t n) { void* q = p + o; o += tsne_up(n); return q; };
    w.part = (float2*)take(8 * (size_t)w.S * N); w.Ytmp = (float2*)take(8 * (size_t)N);
    w.zpart = (double*)take(8 * (size_t)w.S * w.nib); w.kpart = (double*)take(8 * (size_t)w.nub); w.cpart = (double2*)take(16 * (size_t)w.nub);
    w.bytes = o;
    return w;
}
extern "C" size_t act_tsne_step_workspace(int N) { return N > 0 ? tsne_step_carve(nullptr, N).bytes : 0; }

static inline bool tsne_csr_args_ok(const void* a, const void* b, const void* c, const void* y, const void* ws) { return a && b && c && y && ws; }

extern "C" int act_tsne_steps_f32(const int32_t* indptr, const int32_t* indices, const float* values, int N, int n_steps, float exaggeration,
                                  float momentum, float lr, float* Y, float* update, float* gains, void* workspace, size_t workspace_bytes,
                                  act_stream_t stream) {
    if (!tsne_csr_args_ok(indptr, indices, values, Y, workspace) || !update || !gains) return ACT_E_NULLPTR;
    if (N < 2 || N > (1 << 24) || n_steps < 0 || !(exaggeration > 0.f) || !(momentum >= 0.f) || !(lr > 0.f)) return ACT_E_BADARG;
    if (workspace_bytes < act_tsne_step_workspace(N) || (((uintptr_t)workspace) & 15) != 0 || (((uintptr_t)Y) & 7) != 0 ||
        (((uintptr_t)update) & 7) != 0 || (((uintptr_t)gains) & 7) != 0)
        return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const TsneStepCarve w = tsne_step_carve(workspace, N);
    TsneStepArgs a;
    a.indptr = indptr; a.indices = indices; a.values = values; a.Y = (const float2*)Y; a.N = N; a.S = w.S; a.nzp = w.S * w.nib;
    a.part = w.part; a.zpart = w.zpart; a.ex = exaggeration; a.mom = momentum; a.lr = lr;
    a.upd = (float2*)update; a.gains = (float2*)gains; a.Ytmp = w.Ytmp; a.cpart = w.cpart;
    for (int it = 0; it < n_steps; ++it) {
        hipLaunchKernelGGL(tsne_repulse_kernel, dim3(w.nib, w.S), dim3(256), 0, s, (const float2*)Y, N, w.L, w.part, w.zpart);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(tsne_update_kernel, dim3(w.nub), dim3(256), 0, s, a);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(tsne_centre_kernel, dim3(w.nib), dim3(256), 0, s, (const float2*)w.Ytmp, (const double2*)w.cpart, w.nub, N, (float2*)Y);
        ACT_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int act_tsne_step_f32(const int32_t* indptr, const int32_t* indices, const float* values, int N, float exaggeration, float momentum,
                                 float lr, float* Y, float* update, float* gains, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    return act_tsne_steps_f32(indptr, indices, values, N, 1, exaggeration, momentum, lr, Y, update, gains, workspace, workspace_bytes, stream);
}

extern "C" int act_tsne_kl_f32(const int32_t* indptr, const int32_t* indices, const float* values, const float* Y, int N, double* out,
                               void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!tsne_csr_args_ok(indptr, indices, values, Y, workspace) || !out) return ACT_E_NULLPTR;
    if (N < 2 || N > (1 << 24) || workspace_bytes < act_tsne_step_workspace(N) || (((uintptr_t)workspace) & 15) != 0 || (((uintptr_t)Y) & 7) != 0 ||
        (((uintptr_t)out) & 7) != 0)
        return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const TsneStepCarve w = tsne_step_carve(workspace, N);
    hipLaunchKernelGGL(tsne_repulse_kernel, dim3(w.nib, w.S), dim3(256), 0, s, (const float2*)Y, N, w.L, w.part, w.zpart);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_kl_kernel, dim3(w.nub), dim3(256), 0, s, indptr, indices, values, (const float2*)Y, N, (const double*)w.zpart,
                       w.S * w.nib, w.kpart);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_kl_finish_kernel, dim3(1), dim3(ACT_WAVE), 0, s, (const double*)w.kpart, w.nub, out);
    ACT_LAUNCH_CHECK();
    return 0;
}

// workspace of the PCA initialisation: Xc fp32 [N,D], C fp32 [D,D], column partials float64 [splits][D], mean [D], vec [2][D], Yd double2 [N],
// spart double2 [blocks], then the split-K scratch of the covariance product
struct TsnePcaCarve { float *Xc, *C, *gemm; double *part, *mean, *vec; double2 *Yd, *spart; int rsplit, rows_per_split, ksplit, nub; size_t gemm_bytes, bytes; };
static TsnePcaCarve tsne_pca_carve(void* base, int N, int D) {
    TsnePcaCarve w;
    w.rsplit = tsne_cdiv(N, 256) < 64 ? tsne_cdiv(N, 256) : 64;
    w.rows_per_split = tsne_cdiv(N, w.rsplit);
    w.rsplit = tsne_cdiv(N, w.rows_per_split);
    w.ksplit = N / 512 < 1 ? 1 : (N / 512 > 8 ? 8 : N / 512);
    w.nub = tsne_cdiv(N, TSNE_UROWS);
    char* p = (char*)base;
    size_t o = 0;
    auto take = [&](size_t n) { void* q = p + o; o += tsne_up(n); return q; };
    w.Xc = (float*)take(4 * (size_t)N * D); w.C = (float*)take(4 * (size_t)D * D);
    w.part = (double*)take(8 * (size_t)w.rsplit * D); w.mean = (double*)take(8 * (size_t)D); w.vec = (double*)take(16 * (size_t)D);
    w.Yd = (double2*)take(16 * (size_t)N); w.spart = (double2*)take(16 * (size_t)w.nub);
    w.gemm_bytes = tsne_up(4 * (size_t)D * D * w.ksplit + (1u << 20));
    w.gemm = (float*)take(w.gemm_bytes);
    w.bytes = o;
    return w;
}
extern "C" size_t act_tsne_pca_workspace(int N, int D) { return (N > 0 && D > 0) ? tsne_pca_carve(nullptr, N, D).bytes : 0; }

extern "C" int act_tsne_pca_init_f32(const float* X, int N, int D, float* Y, double* info, void* workspace, size_t workspace_bytes,
                                     act_stream_t stream) {
    if (!X || !Y || !info || !workspace) return ACT_E_NULLPTR;
    if (N < 2 || N > (1 << 24) || D < 2 || D > TSNE_MAXD || (long long)N * D >= (1LL << 31)) return ACT_E_BADARG;
    if (workspace_bytes < act_tsne_pca_workspace(N, D) || (((uintptr_t)workspace) & 15) != 0 || (((uintptr_t)Y) & 7) != 0 ||
        (((uintptr_t)info) & 7) != 0)
        return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const TsnePcaCarve w = tsne_pca_carve(workspace, N, D);
    hipLaunchKernelGGL(tsne_colsum_kernel, dim3(tsne_cdiv(D, 64), w.rsplit), dim3(256), 0, s, X, N, D, w.rows_per_split, w.part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_colmean_kernel, dim3(tsne_cdiv(D, 256)), dim3(256), 0, s, (const double*)w.part, w.rsplit, N, D, w.mean);
    ACT_LAUNCH_CHECK();
    const size_t total = (size_t)N * D;
    hipLaunchKernelGGL(tsne_centre_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, X, (const double*)w.mean, total, D, w.Xc);
    ACT_LAUNCH_CHECK();
    act_gemm_epilogue_t epi = {};
    epi.alpha = 1.0f;
    // C = Xc^T Xc: the TN layout (both operands stored [rows][D]), a fixed tile and split so that the sum order does not depend on the tuning table
    const int rc = act_sgemm_ex_f32(0, 0, D, D, N, w.Xc, D, w.Xc, D, w.C, D, &epi, w.gemm, w.gemm_bytes, 3, w.ksplit, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(tsne_eig2_kernel, dim3(1), dim3(256), 0, s, (const float*)w.C, D, w.vec, info);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_project_kernel, dim3(w.nub), dim3(256), 0, s, (const float*)w.Xc, (const double*)w.vec, N, D, w.Yd, w.spart);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(tsne_rescale_kernel, dim3(tsne_cdiv(N, 256)), dim3(256), 0, s, (const double2*)w.Yd, (const double2*)w.spart, w.nub, N,
                       (float2*)Y);
    ACT_LAUNCH_CHECK();
    return 0;
}
