// edgeconv.hip -- the DGCNN classifier's kernels (Wang et al. 2019): a batched Euclidean kNN in feature space, the fused EdgeConv tail with
// BatchNorm (forward + backward, no edge tensor in memory) and the LeakyReLU form of the row BatchNorm.  Built with -ffp-contract=off: the
// search is bit-exact against its restatement (tests/edgeconv_ref.py), and a forward and its backward must agree on the sign of every z.
#include "edge_bn.h"


// ================================================================================================================================ kNN
// Block (x, b) owns KF_Q = 16 consecutive queries of cloud b; the cloud streams past in tiles of KF_T = 256 candidates, one per thread.
//   distances: the 16 query rows sit transposed in LDS (sq[c][q], so a channel's 16 values are four broadcast 16-byte reads); thread t walks
//              its candidate's row once per tile and carries 16 accumulators: per channel one global word, 4 LDS reads, 48 VALU.  The
//              difference form, channels ascending, every operation rounded: d(i,i) = 0, d(i,j) = d(j,i).
//   selection: the tile's [16][256] distances go through LDS to the waves; wave w owns queries w, w+4, w+8, w+12 and keeps each one's k best
//              as a sorted list ACROSS its lanes (lane l = l-th best), one 64-bit key (distance bits << 32 | index) per lane.  Distances are
//              >= +0 or NaN, so their bit patterns order as unsigned integers; NaN becomes 0x7fffffff (after +inf), an empty slot is all
//              ones.  A candidate enters only if its key is below the list's k-th: ballot, then one insertion per set bit in ascending
//              lane (= index) order -- position by popcount of the lanes below it, the tail shifted up one lane.
// Total order (d2, index), no atomics, nothing depends on B; N x N never leaves the block.
#define KF_Q 16
#define KF_T 256
#define KF_MAXC 512
#define KF_EMPTY 0xffffffffffffffffull

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_up1_u64(unsigned long long v) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, 1), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), 1);
    return ((unsigned long long)hi << 32) | lo;
}

template <bool VEC>
__global__ __launch_bounds__(256) void knn_feat_kernel(const float* __restrict__ x, int N, int C, int k, int32_t* __restrict__ idx,
                                                       float* __restrict__ d2out) {
    __shared__ __attribute__((aligned(16))) float sq[KF_MAXC * KF_Q];            // [c][q]
    __shared__ float sd[KF_Q * KF_T];                                            // [q][t]
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int q0 = blockIdx.x * KF_Q;
    const float* xb = x + (size_t)b * N * C;
    for (int e = t; e < KF_Q * C; e += 256) {
        const int q = e / C, c = e - q * C;
        sq[c * KF_Q + q] = xb[(size_t)min(q0 + q, N - 1) * C + c];              // queries past N repeat the last point and are not written
    }
    unsigned long long list[KF_Q / 4];
#pragma unroll
    for (int u = 0; u < KF_Q / 4; ++u) list[u] = KF_EMPTY;
    for (int t0 = 0; t0 < N; t0 += KF_T) {
        __syncthreads();                                                          // sq is staged / the previous tile has been selected from
        const float* row = xb + (size_t)min(t0 + t, N - 1) * C;                  // candidates past N: a valid row, masked at selection
        float acc[KF_Q];
#pragma unroll
        for (int q = 0; q < KF_Q; ++q) acc[q] = 0.f;
        auto channel = [&](int c, float xj) {
            const float4* qv = reinterpret_cast<const float4*>(sq + c * KF_Q);
#pragma unroll
            for (int g = 0; g < KF_Q / 4; ++g) {
                const float4 q4 = qv[g];
                float d;
                d = __fsub_rn(q4.x, xj); acc[4 * g + 0] = __fadd_rn(acc[4 * g + 0], __fmul_rn(d, d));
                d = __fsub_rn(q4.y, xj); acc[4 * g + 1] = __fadd_rn(acc[4 * g + 1], __fmul_rn(d, d));
                d = __fsub_rn(q4.z, xj); acc[4 * g + 2] = __fadd_rn(acc[4 * g + 2], __fmul_rn(d, d));
                d = __fsub_rn(q4.w, xj); acc[4 * g + 3] = __fadd_rn(acc[4 * g + 3], __fmul_rn(d, d));
            }
        };
        if (VEC) {
            for (int c = 0; c < C; c += 4) {
                const float4 v = *reinterpret_cast<const float4*>(row + c);
                channel(c, v.x); channel(c + 1, v.y); channel(c + 2, v.z); channel(c + 3, v.w);
            }
        } else {
            for (int c = 0; c < C; ++c) channel(c, row[c]);
        }
#pragma unroll
        for (int q = 0; q < KF_Q; ++q) sd[q * KF_T + t] = acc[q];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < KF_Q / 4; ++u) {
            const int q = wave + 4 * u;
            unsigned long long mine = list[u];
            unsigned long long kth = shfl_u64(mine, k - 1);
            for (int s = 0; s < KF_T; s += 64) {
                const int j = t0 + s + lane;
                if (t0 + s >= N) break;
                const float d = sd[q * KF_T + s + lane];
                const unsigned bits = (d != d) ? 0x7fffffffu : __float_as_uint(d);
                const unsigned long long key = j < N ? (((unsigned long long)bits << 32) | (unsigned)j) : KF_EMPTY;
                unsigned long long pend = __ballot(key < kth);
                while (pend) {
                    const int src = first_lane(pend);
                    const unsigned long long cand = shfl_u64(key, src);
                    const int pos = __popcll(__ballot(mine < cand));                  // the list is sorted: the lanes below cand are lanes 0 .. pos-1
                    const unsigned long long up = shfl_up1_u64(mine);
                    mine = lane < pos ? mine : (lane == pos ? cand : up);
                    kth = shfl_u64(mine, k - 1);
                    pend &= pend - 1;
                    pend &= __ballot(key < kth);                                      // the bar has dropped: some of the waiting ones no longer pass
                }
            }
            list[u] = mine;
        }
    }
#pragma unroll
    for (int u = 0; u < KF_Q / 4; ++u) {
        const int q = q0 + wave + 4 * u;
        if (q < N && lane < k) {
            const size_t o = ((size_t)b * N + q) * k + lane;
            idx[o] = (int32_t)(unsigned)(list[u] & 0xffffffffull);
            if (d2out) d2out[o] = __uint_as_float((unsigned)(list[u] >> 32));        // 0x7fffffff is itself a NaN
        }
    }
}

extern "C" int act_knn_feat_f32(const float* x, int B, int N, int C, int k, int32_t* idx, float* d2, act_stream_t stream) {
    if (!x || !idx) return ACT_E_NULLPTR;
    if (B <= 0 || B > 65535 || N <= 0 || C <= 0 || C > KF_MAXC || k <= 0 || k > 64 || k > N) return ACT_E_BADARG;
    if ((long long)N * k > 0x7fffffffLL || (long long)N + KF_T > 0x7fffffffLL) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 3.0 * B * (double)N * N * C, 4.0 * B * ((double)N * C * (1.0 + cdiv(N, KF_Q)) + 2.0 * N * k));
    const dim3 grid(cdiv(N, KF_Q), B);
    if (!(C & 3) && !((uintptr_t)x & 15))
        hipLaunchKernelGGL(knn_feat_kernel<true>, grid, dim3(256), 0, s, x, N, C, k, idx, d2);
    else
        hipLaunchKernelGGL(knn_feat_kernel<false>, grid, dim3(256), 0, s, x, N, C, k, idx, d2);
    ACT_LAUNCH_CHECK(); return 0;
}


// ==================================================================================================================== EdgeConv forward
__device__ __forceinline__ float lrelu_affine(float v, float scale, float shift, float slope, float& z) {
    z = __fadd_rn(__fmul_rn(scale, v), shift);
    return z > 0.f ? z : __fmul_rn(slope, z);
}




// ---- workspace --------------------------------------------------------------------------------------------------------------------------
// forward : vmax [R,C] | vmin [R,C] | scale [C] | partials
// backward: dy [R,C] | coef [2,C] (m1 | m2 * rstd) | clamped idx [B,N*k] | adjacency (off [B,N+1] | ent [B,N*k]) | partials
struct EdgeWs { size_t a, b, c, d, e, part, total; };
static EdgeWs edge_ws_fwd(long long R, int C) {
    EdgeWs w{};
    w.a = 0;
    w.b = align16((size_t)R * C * 4);
    w.c = w.b + align16((size_t)R * C * 4);
    w.part = w.c + align16((size_t)C * 4);
    w.total = w.part + part_bytes(C, 2);
    return w;
}
static EdgeWs edge_ws_bwd(int B, int N, int k, int C) {
    EdgeWs w{};
    const size_t R = (size_t)B * N, E = (size_t)N * k;
    w.a = 0;
    w.b = align16(R * C * 4);
    w.c = w.b + align16((size_t)2 * C * 4);
    w.d = w.c + align16((size_t)B * E * 4);
    w.e = w.d + align16((size_t)B * ((size_t)N + 1) * 4);
    w.part = w.e + align16((size_t)B * E * 4);
    w.total = w.part + part_bytes(C, 2);
    return w;
}
static bool edge_dims_ok(int B, int N, int k, int C) {
    if (B <= 0 || B > 65535 || N <= 0 || k <= 0 || k > 65535 || C <= 0 || (C & 3)) return false;
    const long long R = (long long)B * N;
    return (long long)N * k <= 0x7fffffffLL && R * k <= 0x7fffffffLL && R * C <= (0x7fffffffLL - 256) * 256;
}

extern "C" size_t act_edge_bn_workspace(int B, int N, int k, int C) {
    if (!edge_dims_ok(B, N, k, C)) return 0;
    const size_t f = edge_ws_fwd((long long)B * N, C).total, b = edge_ws_bwd(B, N, k, C).total;
    return f > b ? f : b;
}

extern "C" int act_edge_bn_lrelu_max_fwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C, const float* gamma,
                                             const float* beta, float* running_mean, float* running_var, int training, float momentum, float eps,
                                             float slope, float* out, int ldo, int ooff, int32_t* arg, float* vsum, float* mean, float* mean_lo,
                                             float* rstd, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!pq || !idx || !gamma || !beta || !out || !arg || !vsum || !mean || !mean_lo || !rstd || !workspace) return ACT_E_NULLPTR;
    if ((running_mean == nullptr) != (running_var == nullptr)) return ACT_E_NULLPTR;
    if (!training && !running_mean) return ACT_E_NULLPTR;
    if (!edge_dims_ok(B, N, k, C)) return ACT_E_BADARG;
    if (qoff < 0 || ld < C || qoff + C > ld || ooff < 0 || ooff + C > ldo) return ACT_E_BADARG;
    const long long R = (long long)B * N;
    const EdgeWs w = edge_ws_fwd(R, C);
    if (workspace_bytes < w.total) return ACT_E_BADARG;
    char* ws = reinterpret_cast<char*>(workspace);
    float *vmax = (float*)(ws + w.a), *vmin = (float*)(ws + w.b), *scale = (float*)(ws + w.c);
    double* part = (double*)(ws + w.part);
    const ColShape g = col_shape(R, C);
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GN_LRELU_MAX, s, 4.0 * R * k * C, 4.0 * (R * (double)k * (C + 1) + R * (double)C * 9));
    if (training)
        hipLaunchKernelGGL(edge_bn_pass1_kernel<true>, dim3(g.nblk), dim3(256), 0, s, pq, ld, qoff, idx, N, k, C, R, g.rpb, g.tx_log, vmax, vmin, arg,
                           vsum, part);
    else
        hipLaunchKernelGGL(edge_bn_pass1_kernel<false>, dim3(g.nblk), dim3(256), 0, s, pq, ld, qoff, idx, N, k, C, R, g.rpb, g.tx_log, vmax, vmin, arg,
                           vsum, part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(edge_bn_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, pq, ld, qoff, idx, N, part, g.nblk, C, (double)R * k,
                       training ? 1 : 0, gamma, beta, eps, momentum, running_mean, running_var, mean, mean_lo, rstd, scale);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(edge_bn_apply_kernel, dim3(cdiv(R * C, 256)), dim3(256), 0, s, vmax, vmin, C, R * C, scale, beta, mean, mean_lo, slope, out,
                       ldo, ooff, arg);
    ACT_LAUNCH_CHECK(); return 0;
}

// =================================================================================================================== EdgeConv backward
// With dy_i = dout_i * (z_i > 0 ? 1 : slope), xhat*_i = (v*_i - mean) * rstd and M = B*N*k, the BatchNorm backward of the materialised form
// collapses to
//   dbeta = sum_i dy_i, dgamma = sum_i dy_i xhat*_i, m1 = dbeta / M, m2 = dgamma / M
//   dQ[i] = scale (dy_i - k m1 - m2 rstd (vsum_i - k mean))
//   dP[m] = scale (sum_{(i,j)->m, arg_i = j} dy_i - deg(m) m1 - m2 rstd sum_{(i,j)->m} (v_ij - mean))
// where (i,j)->m walks the inverse adjacency of the clamped idx with multiplicity, in ascending (i,j).  The last sum is the issue's
// deg(m) (P_m - mean) + sum Q_i, taken edge by edge on the forward's own v so that a common offset of P + Q cancels inside every term.
__global__ __launch_bounds__(256) void edge_bn_bwd_dy_kernel(const float* __restrict__ pq, int ld, int qoff, const int32_t* __restrict__ idx, int N,
                                                             int k, int C, long long R, int rpb, int tx_log, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ mean,
                                                             const float* __restrict__ mean_lo, const float* __restrict__ rstd, float slope,
                                                             const int32_t* __restrict__ arg, const float* __restrict__ dout, int ldd,
                                                             float* __restrict__ dy,
                                                             double* __restrict__ part) {
    __shared__ double sh[2 * 256];
    const int TX = 1 << tx_log, TY = 256 >> tx_log, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(R, r0 + rpb);
    for (int c0 = 0; c0 < C; c0 += TX) {
        const int c = c0 + tx;
        const bool act = c < C;
        double s[2] = {0.0, 0.0};
        if (act) {
            const float mu = mean[c], lo = mean_lo[c], rs = rstd[c], sc = __fmul_rn(gamma[c], rs), be = beta[c];
            for (long long r = r0 + ty; r < r1; r += TY) {
                const long long base = (r / N) * N;
                const int j = min(max(arg[r * C + c], 0), k - 1);
                const float v = __fadd_rn(pq[(base + clampi(idx[r * k + j], N)) * ld + c], pq[r * ld + qoff + c]);
                float z;
                lrelu_centred(v, mu, lo, sc, be, slope, z);
                const float g = z > 0.f ? dout[r * ldd + c] : __fmul_rn(slope, dout[r * ldd + c]);
                dy[r * C + c] = g;
                s[0] += (double)g;
                s[1] += (double)g * ((double)__fmul_rn(centred(v, mu, lo), rs));
            }
        }
        col_reduce_store<2>(s, sh, tx, ty, TX, TY, act, c, C, part);
    }
}

__global__ __launch_bounds__(256) void edge_bn_bwd_finalize_kernel(const double* __restrict__ part, int nblk, int C, double M,
                                                                   const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < nblk; ++p) { s1 += part[((size_t)p * 2 + 0) * C + c]; s2 += part[((size_t)p * 2 + 1) * C + c]; }
    dbeta[c] = (float)s1; dgamma[c] = (float)s2;
    coef[c] = (float)(s1 / M);
    coef[C + c] = (float)(s2 / M * (double)rstd[c]);
}


__global__ __launch_bounds__(256) void edge_bn_bwd_dpq_kernel(const float* __restrict__ pq, int ld, int qoff, int N, int k, int C, long long total,
                                                              const float* __restrict__ gamma, const float* __restrict__ mean,
                                                              const float* __restrict__ mean_lo, const float* __restrict__ rstd,
                                                              const float* __restrict__ coef,
                                                              const int32_t* __restrict__ arg, const float* __restrict__ vsum,
                                                              const float* __restrict__ dy, const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ ent, float* __restrict__ dpq) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long r = e / C, b = r / N;
    const int c = (int)(e - r * C), n = (int)(r - b * N);
    const float mu = mean[c], lo = mean_lo[c], sc = __fmul_rn(gamma[c], rstd[c]), m1 = coef[c], m2r = coef[C + c], kf = (float)k;
    // dQ
    const float cen = (float)((double)vsum[e] - (double)k * ((double)mu + (double)lo));
    dpq[r * ld + qoff + c] = __fmul_rn(sc, __fsub_rn(__fsub_rn(dy[e], __fmul_rn(kf, m1)), __fmul_rn(m2r, cen)));
    // dP
    const int32_t* ob = off + b * ((long long)N + 1);
    const int32_t* eb = ent + b * (long long)N * k;
    const float p = pq[r * ld + c];
    const int i0 = ob[n], i1 = ob[n + 1];
    float hit = 0.f, cs = 0.f;
    for (int i = i0; i < i1; ++i) {
        const int en = eb[i], src = en / k, j = en - src * k;
        const long long rs = b * N + src;
        if (arg[rs * C + c] == j) hit = __fadd_rn(hit, dy[rs * C + c]);
        cs = __fadd_rn(cs, centred(__fadd_rn(p, pq[rs * ld + qoff + c]), mu, lo));
    }
    dpq[r * ld + c] = __fmul_rn(sc, __fsub_rn(__fsub_rn(hit, __fmul_rn((float)(i1 - i0), m1)), __fmul_rn(m2r, cs)));
}

extern "C" int act_edge_bn_lrelu_max_bwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C, const float* gamma,
                                             const float* beta, const float* mean, const float* mean_lo, const float* rstd, float slope,
                                             const int32_t* arg, const float* vsum, const float* dout, int ldd, float* dpq, float* dgamma,
                                             float* dbeta, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!pq || !idx || !gamma || !beta || !mean || !mean_lo || !rstd || !arg || !vsum || !dout || !dpq || !dgamma || !dbeta || !workspace) return ACT_E_NULLPTR;
    if (!edge_dims_ok(B, N, k, C)) return ACT_E_BADARG;
    if (qoff < C || ld < 2 * C || qoff + C > ld || ldd < C) return ACT_E_BADARG;      // P and Q must not overlap: both get a gradient
    const long long R = (long long)B * N, E = (long long)N * k;
    const EdgeWs w = edge_ws_bwd(B, N, k, C);
    if (workspace_bytes < w.total) return ACT_E_BADARG;
    char* ws = reinterpret_cast<char*>(workspace);
    float *dy = (float*)(ws + w.a), *coef = (float*)(ws + w.b);
    int32_t *idxc = (int32_t*)(ws + w.c), *off = (int32_t*)(ws + w.d), *ent = (int32_t*)(ws + w.e);
    double* part = (double*)(ws + w.part);
    const ColShape g = col_shape(R, C);
    hipStream_t s = (hipStream_t)stream;
    {
        ActProfScope ps(KID_BN_BWD, s, 8.0 * R * C, 4.0 * R * (double)C * 6);
        hipLaunchKernelGGL(edge_bn_bwd_dy_kernel, dim3(g.nblk), dim3(256), 0, s, pq, ld, qoff, idx, N, k, C, R, g.rpb, g.tx_log, gamma, beta, mean, mean_lo,
                           rstd, slope, arg, dout, ldd, dy, part);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(edge_bn_bwd_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, part, g.nblk, C, (double)R * k, rstd, dgamma, dbeta, coef);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(clamp_idx_kernel, dim3(cdiv(R * k, 256)), dim3(256), 0, s, idx, R * k, N, idxc);
        ACT_LAUNCH_CHECK();
    }
    const int rc = act_sa_build_adjacency(idxc, B, N, (int)E, off, ent, s);
    if (rc) return rc;
    ActProfScope ps(KID_ROW_SCATTER, s, 6.0 * R * k * C, 4.0 * (R * (double)k * (3.0 * C + 1) + R * (double)C * 6));
    hipLaunchKernelGGL(edge_bn_bwd_dpq_kernel, dim3(cdiv(R * C, 256)), dim3(256), 0, s, pq, ld, qoff, N, k, C, R * C, gamma, mean, mean_lo, rstd, coef, arg,
                       vsum, dy, off, ent, dpq);
    ACT_LAUNCH_CHECK(); return 0;
}

// ============================================================================================== row BatchNorm with LeakyReLU (conv5, head)
// y = LeakyReLU_slope(x * scale + shift) on rows [R,C]; the backward is the ReLU one of pointnet.hip with the slope on the closed side:
// g = dy (z > 0 ? 1 : slope), dbeta = sum g, dgamma = sum g xhat, dx = scale (g - dbeta / R - xhat dgamma / R).
__global__ __launch_bounds__(256) void affine_lrelu_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, float slope, int C, long long total,
                                                           float* __restrict__ y) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    float z;
    y[e] = lrelu_affine(x[e], scale[c], shift[c], slope, z);
}

extern "C" int act_affine_lrelu_f32(const float* x, const float* scale, const float* shift, float slope, int R, int C, float* y,
                                    act_stream_t stream) {
    if (!x || !scale || !shift || !y) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || (long long)R * C > (0x7fffffffLL - 256) * 256) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_BN_APPLY, s, 3.0 * R * C, 8.0 * R * C);
    hipLaunchKernelGGL(affine_lrelu_kernel, dim3(cdiv((long long)R * C, 256)), dim3(256), 0, s, x, scale, shift, slope, C, (long long)R * C, y);
    ACT_LAUNCH_CHECK(); return 0;
}

__global__ __launch_bounds__(256) void bn_lrelu_bwd_sums_kernel(const float* __restrict__ x, const float* __restrict__ dy, int C, long long R, int rpb,
                                                                int tx_log, const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd, float slope,
                                                                double* __restrict__ part) {
    __shared__ double sh[2 * 256];
    const int TX = 1 << tx_log, TY = 256 >> tx_log, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(R, r0 + rpb);
    for (int c0 = 0; c0 < C; c0 += TX) {
        const int c = c0 + tx;
        const bool act = c < C;
        double s[2] = {0.0, 0.0};
        if (act) {
            const float sc = scale[c], sf = shift[c], mu = mean[c], rs = rstd[c];
            for (long long r = r0 + ty; r < r1; r += TY) {
                const float v = x[r * C + c];
                float z;
                lrelu_affine(v, sc, sf, slope, z);
                const float g = z > 0.f ? dy[r * C + c] : __fmul_rn(slope, dy[r * C + c]);
                s[0] += (double)g;
                s[1] += (double)g * ((double)__fmul_rn(__fsub_rn(v, mu), rs));
            }
        }
        col_reduce_store<2>(s, sh, tx, ty, TX, TY, act, c, C, part);
    }
}

__global__ __launch_bounds__(256) void bn_lrelu_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy, int C, long long total,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd, float slope,
                                                                 const float* __restrict__ coef, float* __restrict__ dx) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const float v = x[e], sc = scale[c];
    float z;
    lrelu_affine(v, sc, shift[c], slope, z);
    const float g = z > 0.f ? dy[e] : __fmul_rn(slope, dy[e]);
    const float xhat = __fmul_rn(__fsub_rn(v, mean[c]), rstd[c]);
    dx[e] = __fmul_rn(sc, __fsub_rn(__fsub_rn(g, coef[c]), __fmul_rn(xhat, coef[C + c])));
}

__global__ __launch_bounds__(256) void bn_lrelu_bwd_finalize_kernel(const double* __restrict__ part, int nblk, int C, double R,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                    float* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < nblk; ++p) { s1 += part[((size_t)p * 2 + 0) * C + c]; s2 += part[((size_t)p * 2 + 1) * C + c]; }
    dbeta[c] = (float)s1; dgamma[c] = (float)s2;
    coef[c] = (float)(s1 / R);
    coef[C + c] = (float)(s2 / R);
}

extern "C" size_t act_bn_lrelu_bwd_workspace(int R, int C) {
    if (R <= 0 || C <= 0) return 0;
    return align16((size_t)2 * C * 4) + part_bytes(C, 2);
}

extern "C" int act_bn_lrelu_bwd_f32(const float* x, const float* dy, const float* scale, const float* shift, const float* mean, const float* rstd,
                                    float slope, int R, int C, float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                    act_stream_t stream) {
    if (!x || !dy || !scale || !shift || !mean || !rstd || !dx || !dgamma || !dbeta || !workspace) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || (long long)R * C > (0x7fffffffLL - 256) * 256) return ACT_E_BADARG;
    if (workspace_bytes < act_bn_lrelu_bwd_workspace(R, C)) return ACT_E_BADARG;
    char* ws = reinterpret_cast<char*>(workspace);
    float* coef = (float*)ws;
    double* part = (double*)(ws + align16((size_t)2 * C * 4));
    const ColShape g = col_shape(R, C);
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_BN_BWD, s, 14.0 * R * C, 20.0 * R * C);
    hipLaunchKernelGGL(bn_lrelu_bwd_sums_kernel, dim3(g.nblk), dim3(256), 0, s, x, dy, C, (long long)R, g.rpb, g.tx_log, scale, shift, mean, rstd, slope,
                       part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_lrelu_bwd_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, part, g.nblk, C, (double)R, dgamma, dbeta, coef);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_lrelu_bwd_apply_kernel, dim3(cdiv((long long)R * C, 256)), dim3(256), 0, s, x, dy, C, (long long)R * C, scale, shift, mean,
                       rstd, slope, coef, dx);
    ACT_LAUNCH_CHECK(); return 0;
}
