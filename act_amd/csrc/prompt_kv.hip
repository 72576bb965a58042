// prompt_kv.hip -- keys / values of the frozen teacher's prompt rows without the dense [B*P, D] x [D, N] product.
//
// For cloud b and prompt p the row is v = keep o tok[p]/(1-q) + ppos[p], LayerNorm'd and multiplied with the K,V rows W [N][D] of the qkv Linear.
// tok, ppos, gamma, beta and W do not depend on the cloud; only the dropout mask does.  With s_j = tok[p][j]/(1-q), v0 = s + ppos[p] (the undropped
// row), mu0 its mean and (mu, rstd) the statistics of the real row:
//     kv[b,p,n] = rstd * ( base[p][n] - sum_{j dropped in (b,p)} s_j gamma_j W[n][j] - (mu - mu0) g[n] ) + c[n]
//     base[p][n] = sum_j (v0_j - mu0) gamma_j W[n][j],   g[n] = sum_j gamma_j W[n][j],   c[n] = sum_j beta_j W[n][j] + bias[n]
// (centred on mu0, so a large common offset of the row cancels before anything is multiplied).  base, g and c are one (P+2) x N x D product
// (composite.hip launches it on the dense GEMM); the kernels here are
//   1. the row pass: statistics + dropped channels of every row (the mask of prompt_layernorm_fwd_kernel: both call dropout.h, domain 1) and the P+2
//      operand rows of the base product;
//   2. the correction: one workgroup per (32-column tile of W, band of prompts) holds the tile in LDS as [j][n] and walks the dropped channels of its
//      rows in increasing j -- no atomics, so runs are bit-identical.
#include "dropout.h"
#include "ln_row.h"

#define PKV_TN 32             // columns of W per workgroup
#define PKV_THREADS 1024
#define PKV_LDS_BYTES (160 * 1024)

namespace {

inline size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }

// rows 0 .. T-1: statistics + dropped-channel list of prompt row (b, p); rows T .. T+P+1: the operand rows of the base product
// ((v0 - mu0) o gamma for every prompt, then gamma, then beta).  One wave per row.
// list of row r: lst[r*LD ..], channel indices in increasing order, padded with the index D (a zero row of the weight tile) to a multiple of 8;
// steps[r] = its length / 8.  dmu[r] = mu - mu0 = -(sum of the dropped s_j) / D.
__global__ __launch_bounds__(256) void prompt_kv_rows_kernel(const float* __restrict__ tok, const float* __restrict__ ppos, int P, float drop_p,
                                                             uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, int T, int D, float eps,
                                                             int LD, float* __restrict__ rstd_out, float* __restrict__ dmu_out,
                                                             int* __restrict__ steps_out, unsigned short* __restrict__ lst,
                                                             float* __restrict__ arows) {
    const DropoutKey key = dropout_key(drop_p, seed, seed_dev);
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T + P + 2) return;
    const int nv = D >> 2;
    const float inv_keep = key.inv_keep;
    if (row >= T) {
        const int r = row - T;
        float4* __restrict__ o4 = reinterpret_cast<float4*>(arows + (size_t)r * D);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(gamma);
        if (r >= P) {
            const float4* __restrict__ src = r == P ? g4 : reinterpret_cast<const float4*>(beta);
            for (int c = lane; c < nv; c += 64) o4[c] = src[c];
            return;
        }
        const float4* __restrict__ xr = reinterpret_cast<const float4*>(tok + (size_t)r * D);
        const float4* __restrict__ qr = reinterpret_cast<const float4*>(ppos + (size_t)r * D);
        float4 v[LN_ROW_MAXV];
#pragma unroll
        for (int i = 0; i < LN_ROW_MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                float4 a = xr[c];
                const float4 b = qr[c];
                if (drop_p > 0.f) { a.x = __fmul_rn(a.x, inv_keep); a.y = __fmul_rn(a.y, inv_keep); a.z = __fmul_rn(a.z, inv_keep); a.w = __fmul_rn(a.w, inv_keep); }
                a.x = __fadd_rn(a.x, b.x); a.y = __fadd_rn(a.y, b.y); a.z = __fadd_rn(a.z, b.z); a.w = __fadd_rn(a.w, b.w);
                v[i] = a;
            } else v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float mean0 = ln_row_mean<LN_ROW_MAXV>(v, lane, nv, D);
#pragma unroll
        for (int i = 0; i < LN_ROW_MAXV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                const float4 g = g4[c];
                o4[c] = make_float4((v[i].x - mean0) * g.x, (v[i].y - mean0) * g.y, (v[i].z - mean0) * g.z, (v[i].w - mean0) * g.w);
            }
        }
        return;
    }
    const int pr = row % P;
    const float4* __restrict__ xr = reinterpret_cast<const float4*>(tok + (size_t)pr * D);
    const float4* __restrict__ qr = reinterpret_cast<const float4*>(ppos + (size_t)pr * D);
    float4 v[LN_ROW_MAXV];
    float s = 0.f, ds = 0.f;                                            // the row sum rides along with the dropped sum (ln_row_mean here moves the register count)
    uint32_t dm = 0;                                                    // bit 4 i + k: channel 4 (lane + 64 i) + k is dropped
#pragma unroll
    for (int i = 0; i < LN_ROW_MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            float4 a = xr[c];
            if (drop_p > 0.f) {
                const Dropped4 dr = dropout_dropped4(key, (uint32_t)row, (uint32_t)c);
                const float sx = a.x * inv_keep, sy = a.y * inv_keep, sz = a.z * inv_keep, sw = a.w * inv_keep;
                a.x = dr.x ? 0.f : sx; a.y = dr.y ? 0.f : sy; a.z = dr.z ? 0.f : sz; a.w = dr.w ? 0.f : sw;
                ds += ((dr.x ? sx : 0.f) + (dr.y ? sy : 0.f)) + ((dr.z ? sz : 0.f) + (dr.w ? sw : 0.f));
                dm |= ((uint32_t)dr.x | ((uint32_t)dr.y << 1) | ((uint32_t)dr.z << 2) | ((uint32_t)dr.w << 3)) << (4 * i);
            }
            const float4 b = qr[c];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            v[i] = a;
            s += (a.x + a.y) + (a.z + a.w);
        } else v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float mean = wave_sum_f32(s) / (float)D;
    const float rstd = ln_row_rstd<LN_ROW_MAXV>(v, mean, lane, nv, D, eps);
    const float dsum = wave_sum_f32(ds);
    // compact list, increasing channel: chunk i holds channels 4 (64 i + lane) + k, so the order is i, lane, k
    unsigned short* __restrict__ lr = lst + (size_t)row * LD;
    int cnt = 0;
    if (drop_p > 0.f) {
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int i = 0; i < LN_ROW_MAXV; ++i) {
            if (64 * i < nv) {                                         // uniform over the wave: every lane votes
                const uint32_t bits = (dm >> (4 * i)) & 15u;
                const unsigned long long b0 = __ballot(bits & 1u), b1 = __ballot(bits & 2u), b2 = __ballot(bits & 4u), b3 = __ballot(bits & 8u);
                int off = cnt + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below);
                const int ch = 4 * (lane + 64 * i);
                if (bits & 1u) lr[off++] = (unsigned short)ch;
                if (bits & 2u) lr[off++] = (unsigned short)(ch + 1);
                if (bits & 4u) lr[off++] = (unsigned short)(ch + 2);
                if (bits & 8u) lr[off++] = (unsigned short)(ch + 3);
                cnt += __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
            }
        }
    }
    const int padded = (cnt + 7) & ~7;                                 // <= LD = D rounded up to 8
    if (lane < padded - cnt) lr[cnt + lane] = (unsigned short)D;
    if (lane == 0) { rstd_out[row] = rstd; dmu_out[row] = -dsum / (float)D; steps_out[row] = padded >> 3; }
}

typedef float pkv_f2 __attribute__((ext_vector_type(2)));

// grid (column tiles, prompt bands), PKV_THREADS threads.  LDS: wt [(D+1)][32] (row D = zeros, the target of list padding), then coef [PC][D+1] =
// -s_j gamma_j of up to PC prompts of the band (entry D = 0).  A wave serves 8 rows (clouds) of one prompt at a time, 8 lanes x 4 columns per row.
__global__ __launch_bounds__(PKV_THREADS) void prompt_kv_correct_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                                        const float* __restrict__ tok, const float* __restrict__ gamma,
                                                                        const float* __restrict__ base, const float* __restrict__ rstd,
                                                                        const float* __restrict__ dmu, const int* __restrict__ steps,
                                                                        const unsigned short* __restrict__ lst, float* __restrict__ kvp, int B, int P,
                                                                        int D, int N, int LD, float inv_keep, int PC, int vec_store) {
    extern __shared__ __align__(16) float pkv_smem[];
    float* __restrict__ wt = pkv_smem;
    float* __restrict__ coef = pkv_smem + (size_t)(D + 1) * PKV_TN;
    const int tid = threadIdx.x, n0 = blockIdx.x * PKV_TN;
    const int p_lo = (int)((long long)blockIdx.y * P / gridDim.y), p_hi = (int)((long long)(blockIdx.y + 1) * P / gridDim.y);
    // the tile, transposed on the way in: 32 consecutive lanes = 32 rows of W (one bank each), the workgroup covers 128 consecutive j per pass
    const int nq = D >> 2;
    for (int f = tid; f < nq * PKV_TN; f += PKV_THREADS) {
        const int nl = f & (PKV_TN - 1), jq = f >> 5, n = n0 + nl;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < N) w = *reinterpret_cast<const float4*>(W + (size_t)n * D + 4 * jq);
        float* o = wt + (size_t)(4 * jq) * PKV_TN + nl;
        o[0] = w.x; o[PKV_TN] = w.y; o[2 * PKV_TN] = w.z; o[3 * PKV_TN] = w.w;
    }
    if (tid < PKV_TN) wt[(size_t)D * PKV_TN + tid] = 0.f;
    const int lane = tid & 63, wave = tid >> 6, slot = lane >> 3, sub = lane & 7;
    const int n = n0 + 4 * sub;
    float gq[4], cq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool in = n + k < N;
        gq[k] = in ? base[(size_t)P * N + n + k] : 0.f;
        cq[k] = in ? base[(size_t)(P + 1) * N + n + k] + (bias ? bias[n + k] : 0.f) : 0.f;
    }
    const int CB = (B + 7) >> 3;
    const uint32_t pad2 = (uint32_t)D | ((uint32_t)D << 16);
    const uint4 pad8 = make_uint4(pad2, pad2, pad2, pad2);
    const float* __restrict__ wl = wt + 4 * sub;
    for (int pc = p_lo; pc < p_hi; pc += PC) {
        const int np = min(PC, p_hi - pc);
        __syncthreads();                                               // the previous prompts' walkers are done with coef (first pass: nothing)
        for (int f = tid; f < np * (D + 1); f += PKV_THREADS) {
            const int pl = f / (D + 1), j = f - pl * (D + 1);
            coef[f] = j < D ? -(__fmul_rn(tok[(size_t)(pc + pl) * D + j], inv_keep) * gamma[j]) : 0.f;
        }
        __syncthreads();                                               // coef (and, first pass, the tile) visible
        for (int u = wave; u < np * CB; u += PKV_THREADS / 64) {
            const int pl = u / CB, cb = u - pl * CB, p = pc + pl, b = cb * 8 + slot;
            const bool live = b < B;
            const size_t row = live ? (size_t)b * P + p : 0;
            const int st = live ? steps[row] : 0;
            const int mx = wave_max_i32(st, 0);
            const uint4* __restrict__ lp = reinterpret_cast<const uint4*>(lst + row * LD);
            const float* __restrict__ cf = coef + (size_t)pl * (D + 1);
            pkv_f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
            // (loads always in range -- entry 0 of a list exists even when it is empty -- and the padding is selected by value)
            uint4 cur = lp[0];
            if (st <= 0) cur = pad8;
for (int s = 0; s < mx; ++s) {
                const bool more = s + 1 < st;
                const uint4 nxt = lp[more ? s + 1 : 0];                // the next 8 indices are in flight while these 8 are walked
                const uint32_t j[8] = {cur.x & 0xffffu, cur.x >> 16, cur.y & 0xffffu, cur.y >> 16, cur.z & 0xffffu, cur.z >> 16, cur.w & 0xffffu, cur.w >> 16};
                float4 w8[8]; float c8[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) { w8[k] = *reinterpret_cast<const float4*>(wl + j[k] * PKV_TN); c8[k] = cf[j[k]]; }      // all 16 reads issued first
#pragma unroll
                for (int k = 0; k < 8; ++k) {                          // ... then the multiply-adds, in list order
                    const pkv_f2 cc = {c8[k], c8[k]}, w01 = {w8[k].x, w8[k].y}, w23 = {w8[k].z, w8[k].w};
                    a01 = __builtin_elementwise_fma(cc, w01, a01); a23 = __builtin_elementwise_fma(cc, w23, a23);
                }
                cur.x = more ? nxt.x : pad2; cur.y = more ? nxt.y : pad2; cur.z = more ? nxt.z : pad2; cur.w = more ? nxt.w : pad2;
            }
            if (live && n < N) {
                const float rs = rstd[row], dm = dmu[row];
                const float* __restrict__ bp = base + (size_t)p * N + n;
                float* __restrict__ o = kvp + row * N + n;
                const float acc[4] = {a01.x, a01.y, a23.x, a23.y};
                if (vec_store) {                                       // N % 4 == 0: the four columns are in range together
                    const float4 b4 = *reinterpret_cast<const float4*>(bp);
                    float4 r4;
                    r4.x = fmaf(rs, fmaf(-dm, gq[0], b4.x + acc[0]), cq[0]); r4.y = fmaf(rs, fmaf(-dm, gq[1], b4.y + acc[1]), cq[1]);
                    r4.z = fmaf(rs, fmaf(-dm, gq[2], b4.z + acc[2]), cq[2]); r4.w = fmaf(rs, fmaf(-dm, gq[3], b4.w + acc[3]), cq[3]);
                    *reinterpret_cast<float4*>(o) = r4;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (n + k < N) o[k] = fmaf(rs, fmaf(-dm, gq[k], bp[k] + acc[k]), cq[k]);
                }
            }
        }
    }
}

int cu_count() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    return n;
}

}  // namespace

bool act_prompt_kv_shape_ok(int B, int P, int D, int N) {
    if (B <= 0 || P <= 0 || D <= 0 || N <= 0 || (D & 3) || D > 64 * 4 * LN_ROW_MAXV) return false;
    return (size_t)(D + 1) * (PKV_TN + 1) * sizeof(float) <= (size_t)PKV_LDS_BYTES;       // the tile and one prompt's coefficients
}

void act_prompt_kv_carve(float* ws, int B, int P, int D, int N, ActPromptKvWs& w) {
    const size_t T = (size_t)B * P, LD = (size_t)((D + 7) & ~7);
    size_t used = 0;
    auto take = [&](size_t n) { float* r = ws ? ws + used : nullptr; used += pad4(n); return r; };
    w.arows = take((size_t)(P + 2) * D); w.base = take((size_t)(P + 2) * N); w.rstd = take(T); w.dmu = take(T);
    w.steps = reinterpret_cast<int*>(take(T)); w.lst = reinterpret_cast<unsigned short*>(take((T * LD + 1) / 2));
    w.floats = used;
}

int act_prompt_kv_rows(const float* tok, const float* ppos, int B, int P, int D, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                       const float* gamma, const float* beta, float eps, const ActPromptKvWs& w, hipStream_t s) {
    const int T = B * P, LD = (D + 7) & ~7;
    ActProfScope ps(KID_LAYERNORM_FWD, s, 0.0, 4.0 * (double)(3 * P + 2) * D + 2.0 * T * (double)D * drop_p + 12.0 * T);
    hipLaunchKernelGGL(prompt_kv_rows_kernel, dim3((T + P + 2 + 3) / 4), dim3(256), 0, s, tok, ppos, P, drop_p, seed, seed_dev, gamma, beta, T, D, eps, LD,
                       w.rstd, w.dmu, w.steps, w.lst, w.arows);
    ACT_LAUNCH_CHECK(); return 0;
}

int act_prompt_kv_correct(const float* tok, int B, int P, int D, int N, float drop_p, const float* gamma, const float* W, const float* bias,
                          const ActPromptKvWs& w, float* kvp, hipStream_t s) {
    const int T = B * P, LD = (D + 7) & ~7;
    const int tiles = (N + PKV_TN - 1) / PKV_TN;
    int bands = cu_count() / tiles;                                    // about one workgroup per CU
    bands = bands < 1 ? 1 : (bands > P ? P : bands);
    const size_t tile_bytes = (size_t)(D + 1) * PKV_TN * sizeof(float), row_bytes = (size_t)(D + 1) * sizeof(float);
    int PC = (P + bands - 1) / bands;
    const int fit = (int)(((size_t)PKV_LDS_BYTES - tile_bytes) / row_bytes);
    if (PC > fit) PC = fit;
    const size_t smem = tile_bytes + (size_t)PC * row_bytes;
    // executed work: every dropped channel of every row is one multiply-add per column (the expected count; the drawn one is within a per mille of it)
    const double nnz = (double)T * D * (double)dropout_thr(drop_p) / DROPOUT_THR_SCALE;
    ActProfScope ps(KID_PROMPT_KV, s, 2.0 * nnz * N, 4.0 * ((double)tiles * bands * (D + 1) * PKV_TN + (double)T * N) + 2.0 * nnz * tiles);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(prompt_kv_correct_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return (int)e;
    const int vec_store = (N % 4 == 0) && ((reinterpret_cast<uintptr_t>(kvp) | reinterpret_cast<uintptr_t>(w.base)) & 15) == 0;
    hipLaunchKernelGGL(prompt_kv_correct_kernel, dim3(tiles, bands), dim3(PKV_THREADS), smem, s, W, bias, tok, gamma, w.base, w.rstd, w.dmu, w.steps, w.lst,
                       kvp, B, P, D, N, LD, dropout_inv_keep(drop_p), PC, vec_store);
    ACT_LAUNCH_CHECK(); return 0;
}
