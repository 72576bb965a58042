// seg.hip -- dense per-point prediction (semantic segmentation head, semantic_segmentation/models/pt.py + pointnet2_utils.py:262-315):
// three-nearest-centre search with inverse weights, row interpolation forward / backward (deterministic gather over the inverse adjacency),
// the xyz / bias column reduction of the restructured first propagation conv, row log-softmax, weighted-mean NLL, confusion matrix.
//
// Conventions: distances are the DIFFERENCE form (dx*dx + dy*dy) + dz*dz in fp32, never contracted (file built with -ffp-contract=off);
// the reference's expansion form |p|^2 + |c|^2 - 2 p.c is a documented deviation.  Every reduction runs in a fixed order:
// per-block partials, then one ordered pass.  The only atomics are integer ones (confusion-matrix counts), which are exact.
#include "common.h"

static inline unsigned cdiv(long long a, int b) { return (unsigned)((a + b - 1) / b); }

// ---- three nearest centres ------------------------------------------------------------------------------------------
// one lane per point, the cloud's G centres staged in LDS; ascending (distance, index) order: strict '<' keeps the lower index on ties
// (centres are visited in increasing index).  weight = (1 / (d + 1e-8)) / sum of the three.
#define SEG_MAX_G 512
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ xyz, const float* __restrict__ ctr, int N, int G,
                                                       int32_t* __restrict__ idx, float* __restrict__ wout) {
    __shared__ float sc[SEG_MAX_G * 3];
    const int b = blockIdx.y;
    const float* cb = ctr + (size_t)b * G * 3;
    for (int i = threadIdx.x; i < G * 3; i += blockDim.x) sc[i] = cb[i];
    __syncthreads();
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const size_t p = (size_t)b * N + n;
    const float px = xyz[p * 3 + 0], py = xyz[p * 3 + 1], pz = xyz[p * 3 + 2];
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int g = 0; g < G; ++g) {
        const float d = sqdist3(px, py, pz, sc[g * 3 + 0], sc[g * 3 + 1], sc[g * 3 + 2]);
        if (d < d2) {
            if (d < d1) {
                d2 = d1; i2 = i1;
                if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = g; }
                else { d1 = d; i1 = g; }
            } else { d2 = d; i2 = g; }
        }
    }
    const float r0 = __fdiv_rn(1.0f, __fadd_rn(d0, 1e-8f)), r1 = __fdiv_rn(1.0f, __fadd_rn(d1, 1e-8f)), r2 = __fdiv_rn(1.0f, __fadd_rn(d2, 1e-8f));
    const float s = __fadd_rn(__fadd_rn(r0, r1), r2);
    idx[p * 3 + 0] = i0; idx[p * 3 + 1] = i1; idx[p * 3 + 2] = i2;
    wout[p * 3 + 0] = __fdiv_rn(r0, s); wout[p * 3 + 1] = __fdiv_rn(r1, s); wout[p * 3 + 2] = __fdiv_rn(r2, s);
}

// inverse adjacency per cloud by a counting sort: thread g counts the entries e = 3n+k with idx[e] == g (pass 1), an exclusive scan over the
// centres gives the offsets, pass 2 lists the entries of every centre in increasing e.  No atomics: the lists are a function of idx alone.
#define SEG_ADJ_CHUNK 2048
__global__ __launch_bounds__(SEG_MAX_G) void three_nn_adj_kernel(const int32_t* __restrict__ idx, int N, int G, int32_t* __restrict__ off,
                                                                  int32_t* __restrict__ ent) {
    __shared__ int32_t chunk[SEG_ADJ_CHUNK];
    __shared__ int32_t cnt[SEG_MAX_G + 1];
    const int b = blockIdx.x, g = threadIdx.x, E = 3 * N;
    const int32_t* ib = idx + (size_t)b * E;
    int c = 0;
    for (int e0 = 0; e0 < E; e0 += SEG_ADJ_CHUNK) {
        const int m = min(SEG_ADJ_CHUNK, E - e0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += blockDim.x) chunk[i] = ib[e0 + i];
        __syncthreads();
        for (int i = 0; i < m; ++i) c += (chunk[i] == g);
    }
    if (g < G) cnt[g] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int j = 0; j < G; ++j) { const int t = cnt[j]; cnt[j] = acc; acc += t; }
        cnt[G] = acc;
    }
    __syncthreads();
    int32_t* ob = off + (size_t)b * (G + 1);
    if (g < G) ob[g] = cnt[g];
    if (g == 0) ob[G] = cnt[G];
    int pos = g < G ? cnt[g] : 0;
    int32_t* eb = ent + (size_t)b * E;
    for (int e0 = 0; e0 < E; e0 += SEG_ADJ_CHUNK) {
        const int m = min(SEG_ADJ_CHUNK, E - e0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += blockDim.x) chunk[i] = ib[e0 + i];
        __syncthreads();
        if (g < G)
            for (int i = 0; i < m; ++i)
                if (chunk[i] == g) eb[pos++] = e0 + i;
    }
}

extern "C" int act_three_nn_f32(const float* xyz, const float* centers, int B, int N, int G, int32_t* idx, float* weight, int32_t* adj_off,
                                int32_t* adj_ent, act_stream_t stream) {
    if (!xyz || !centers || !idx || !weight) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || G < 3 || G > SEG_MAX_G) return ACT_E_BADARG;
    if ((adj_off == nullptr) != (adj_ent == nullptr)) return ACT_E_NULLPTR;
    hipStream_t s = (hipStream_t)stream;
    {
        ActProfScope ps(KID_ELTWISE, s, 9.0 * B * (double)N * G, 4.0 * B * ((double)N * 9 + G * 3));
        hipLaunchKernelGGL(three_nn_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, s, xyz, centers, N, G, idx, weight);
        ACT_LAUNCH_CHECK();
    }
    if (adj_off) {
        ActProfScope ps(KID_ELTWISE, s, 0.0, 4.0 * B * ((double)N * 6 + G + 1));
        hipLaunchKernelGGL(three_nn_adj_kernel, dim3(B), dim3(SEG_MAX_G), 0, s, idx, N, G, adj_off, adj_ent);
        ACT_LAUNCH_CHECK();
    }
    return 0;
}

// ---- row interpolation ----------------------------------------------------------------------------------------------
// Y[b*N+n, :] = sum_k w[n,k] * P[b*G + idx[n,k], :]  (+ xyz[n] . wxyz[c,:] + bias[c]); one float4 of a row per lane, 4 rows per block
__global__ __launch_bounds__(256) void interp_fwd_kernel(const float4* __restrict__ P, const int32_t* __restrict__ idx, const float* __restrict__ w,
                                                         const float* __restrict__ xyz, const float* __restrict__ wxyz, const float* __restrict__ bias,
                                                         int N, int G, int C4, long long R, float4* __restrict__ Y) {
    const long long r = (long long)blockIdx.y * 4 + threadIdx.y;
    const int c4 = blockIdx.x * 64 + threadIdx.x;
    if (r >= R || c4 >= C4) return;
    const long long base = (r / N) * G;
    const int j0 = idx[r * 3 + 0], j1 = idx[r * 3 + 1], j2 = idx[r * 3 + 2];
    const float w0 = w[r * 3 + 0], w1 = w[r * 3 + 1], w2 = w[r * 3 + 2];
    const float4 a = P[(base + j0) * C4 + c4], bb = P[(base + j1) * C4 + c4], cc = P[(base + j2) * C4 + c4];
    float4 y;
    y.x = fmaf(w2, cc.x, fmaf(w1, bb.x, w0 * a.x));
    y.y = fmaf(w2, cc.y, fmaf(w1, bb.y, w0 * a.y));
    y.z = fmaf(w2, cc.z, fmaf(w1, bb.z, w0 * a.z));
    y.w = fmaf(w2, cc.w, fmaf(w1, bb.w, w0 * a.w));
    if (wxyz) {
        const float px = xyz[r * 3 + 0], py = xyz[r * 3 + 1], pz = xyz[r * 3 + 2];
        const float* wc = wxyz + (size_t)c4 * 12;
        y.x += fmaf(pz, wc[2], fmaf(py, wc[1], px * wc[0]));
        y.y += fmaf(pz, wc[5], fmaf(py, wc[4], px * wc[3]));
        y.z += fmaf(pz, wc[8], fmaf(py, wc[7], px * wc[6]));
        y.w += fmaf(pz, wc[11], fmaf(py, wc[10], px * wc[9]));
    }
    if (bias) {
        const float4 bv = reinterpret_cast<const float4*>(bias)[c4];
        y.x += bv.x; y.y += bv.y; y.z += bv.z; y.w += bv.w;
    }
    Y[r * C4 + c4] = y;
}

extern "C" int act_interp_rows_fwd_f32(const float* P, const int32_t* idx, const float* weight, const float* xyz, const float* wxyz,
                                       const float* bias, int B, int N, int G, int C, float* Y, act_stream_t stream) {
    if (!P || !idx || !weight || !Y) return ACT_E_NULLPTR;
    if (wxyz && !xyz) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || G <= 0 || C <= 0 || (C & 3)) return ACT_E_BADARG;
    if (((uintptr_t)P | (uintptr_t)Y | (uintptr_t)bias) & 15) return ACT_E_BADARG;
    const long long R = (long long)B * N;
    const int C4 = C / 4;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 6.0 * R * C, 4.0 * (R * (double)C * 4 + R * 9));
    hipLaunchKernelGGL(interp_fwd_kernel, dim3(cdiv(C4, 64), cdiv(R, 4)), dim3(64, 4), 0, s, reinterpret_cast<const float4*>(P), idx, weight, xyz,
                       wxyz, bias, N, G, C4, R, reinterpret_cast<float4*>(Y));
    ACT_LAUNCH_CHECK(); return 0;
}

// dP[b*G+g, :] = sum over the entries e of centre g (increasing e) of w[e] * dY[b*N + e/3, :]
__global__ __launch_bounds__(256) void interp_bwd_kernel(const float4* __restrict__ dY, const int32_t* __restrict__ off, const int32_t* __restrict__ ent,
                                                         const float* __restrict__ w, int N, int G, int C4, long long RG, float4* __restrict__ dP) {
    const long long rg = (long long)blockIdx.y * 4 + threadIdx.y;
    const int c4 = blockIdx.x * 64 + threadIdx.x;
    if (rg >= RG || c4 >= C4) return;
    const long long b = rg / G;
    const int g = (int)(rg - b * G);
    const int32_t* ob = off + b * (G + 1);
    const int32_t* eb = ent + b * 3LL * N;
    const float* wb = w + b * 3LL * N;
    const float4* yb = dY + b * (long long)N * C4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int e1 = ob[g + 1];
    for (int i = ob[g]; i < e1; ++i) {
        const int e = eb[i];
        const float wt = wb[e];
        const float4 v = yb[(long long)(e / 3) * C4 + c4];
        acc.x = fmaf(wt, v.x, acc.x); acc.y = fmaf(wt, v.y, acc.y); acc.z = fmaf(wt, v.z, acc.z); acc.w = fmaf(wt, v.w, acc.w);
    }
    dP[rg * C4 + c4] = acc;
}

extern "C" int act_interp_rows_bwd_f32(const float* dY, const int32_t* adj_off, const int32_t* adj_ent, const float* weight, int B, int N, int G,
                                       int C, float* dP, act_stream_t stream) {
    if (!dY || !adj_off || !adj_ent || !weight || !dP) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || G <= 0 || C <= 0 || (C & 3)) return ACT_E_BADARG;
    if (((uintptr_t)dY | (uintptr_t)dP) & 15) return ACT_E_BADARG;
    const long long RG = (long long)B * G;
    const int C4 = C / 4;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 6.0 * B * (double)N * C, 4.0 * ((double)B * N * C * 3 + RG * C + B * (double)N * 6));
    hipLaunchKernelGGL(interp_bwd_kernel, dim3(cdiv(C4, 64), cdiv(RG, 4)), dim3(64, 4), 0, s, reinterpret_cast<const float4*>(dY), adj_off, adj_ent,
                       weight, N, G, C4, RG, reinterpret_cast<float4*>(dP));
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- gradient of the xyz columns and the bias of the restructured first propagation conv -----------------------------
// dwxyz[c, j] = sum_r dY[r, c] * xyz[r, j], dbias[c] = sum_r dY[r, c]: per block of SEG_XYZ_ROWS rows a partial [4, C], then one ordered pass
#define SEG_XYZ_ROWS 512
__global__ __launch_bounds__(256) void xyz_grad_partial_kernel(const float* __restrict__ dY, const float* __restrict__ xyz, long long R, int C,
                                                               float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const long long r0 = (long long)blockIdx.y * SEG_XYZ_ROWS, r1 = min(R, r0 + SEG_XYZ_ROWS);
    if (c >= C) return;
    float sx = 0.f, sy = 0.f, sz = 0.f, sb = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const float g = dY[r * C + c];
        sx = fmaf(g, xyz[r * 3 + 0], sx); sy = fmaf(g, xyz[r * 3 + 1], sy); sz = fmaf(g, xyz[r * 3 + 2], sz); sb += g;
    }
    float* pb = part + (size_t)blockIdx.y * 4 * C;
    pb[c] = sx; pb[C + c] = sy; pb[2 * C + c] = sz; pb[3 * C + c] = sb;
}
__global__ __launch_bounds__(256) void xyz_grad_final_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ dwxyz,
                                                             float* __restrict__ dbias) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float sx = 0.f, sy = 0.f, sz = 0.f, sb = 0.f;
    for (int p = 0; p < nparts; ++p) {
        const float* pb = part + (size_t)p * 4 * C;
        sx += pb[c]; sy += pb[C + c]; sz += pb[2 * C + c]; sb += pb[3 * C + c];
    }
    if (dwxyz) { dwxyz[c * 3 + 0] = sx; dwxyz[c * 3 + 1] = sy; dwxyz[c * 3 + 2] = sz; }
    if (dbias) dbias[c] = sb;
}

extern "C" size_t act_interp_xyz_grad_workspace(long long R, int C) {
    return (size_t)((R + SEG_XYZ_ROWS - 1) / SEG_XYZ_ROWS) * 4 * (size_t)C * sizeof(float);
}

extern "C" int act_interp_xyz_grad_f32(const float* dY, const float* xyz, long long R, int C, float* dwxyz, float* dbias, float* workspace,
                                       size_t workspace_bytes, act_stream_t stream) {
    if (!dY || !xyz || !workspace || (!dwxyz && !dbias)) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0) return ACT_E_BADARG;
    if (workspace_bytes < act_interp_xyz_grad_workspace(R, C)) return ACT_E_BADARG;
    const int nparts = (int)((R + SEG_XYZ_ROWS - 1) / SEG_XYZ_ROWS);
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 8.0 * R * C, 4.0 * ((double)R * C + R * 3 + 8.0 * nparts * C));
    hipLaunchKernelGGL(xyz_grad_partial_kernel, dim3(cdiv(C, 256), nparts), dim3(256), 0, s, dY, xyz, R, C, workspace);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(xyz_grad_final_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, workspace, nparts, C, dwxyz, dbias);
    ACT_LAUNCH_CHECK(); return 0;
}

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
