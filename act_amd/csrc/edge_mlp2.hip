// edge_mlp2.hip -- the EdgeConv of the DGCNN segmentation networks and of their spatial transformer: TWO convolutions ahead of the max over the
// neighbours, conv -> BatchNorm -> LeakyReLU -> conv -> BatchNorm -> LeakyReLU -> max_j.  The first collapses to v = P[idx] + Q as in edgeconv.hip;
// the second, y = w2 . h over all E = B*N*k edges, is formed here tile by tile on the f32 matrix cores from an h tile built in LDS, forward and
// backward: no [E, C] tensor is written by the forward, one (dpre1) by the backward.  Also the 3x3 transform of a cloud.  Built with
// -ffp-contract=off: the backward recomputes h and y with the forward's own instruction sequence and reads the signs of z1 and z2 off them.
#include "edge_bn.h"

#define M2_MAXC 128
#define M2_MAXK 64
#define M2_PAD 4                         // floats between LDS rows: a 16-row x 4-quad read of 16-byte words then touches every bank once at widths 64, 128
#define M2_LDS_MAX (160 * 1024)
#define M2_MAX_BLOCKS 256                // the backward keeps one [C2, C1] partial of dw2 per workgroup

typedef float v4f __attribute__((ext_vector_type(4)));

// ---- tile geometry ------------------------------------------------------------------------------------------------------------------------------------
// A workgroup of 4 waves owns TM = 64 * RB consecutive edge rows, which are PT = TM / k WHOLE points (k <= 64, so PT >= 1; the rows past PT * k are
// zero).  Wave w owns rows [16 RB w, 16 RB (w + 1)) and all of the C2 columns.  Widths are padded with zeros: C1p, C2p = the power of two >= 16.
//   hs  [TM][C1p + 4]   h = LeakyReLU(BN1(v)), built by all 256 threads: thread t owns the four channels 4 (t % (C1p / 4)) of every (256 / (C1p / 4))-th row
//   w2s [C2p][C1p + 4]  resident for the whole kernel
//   ys  [TM][C2p + 4]   y (forward: overlays hs, which is dead by then) / dy (backward)
// The product walks K in steps of 16: lane (i = lane % 16, q = lane / 16) reads ONE 16-byte word hs[row i][16 s + 4 q ..] and w2s[col i][16 s + 4 q ..]
// and feeds its four floats to four v_mfma_f32_16x16x4_f32 -- the MFMA's k index q then stands for channel 16 s + 4 q + t in step t, on both
// operands alike.  The order of the sum (s ascending, t ascending, q inside the instruction) is the same wherever a row sits, in every kernel here.
struct M2Geo { int C1p, C2p, S1, S2, KS; };
__host__ __device__ static inline int pow2_16(int c) { int p = 16; while (p < c) p <<= 1; return p; }
static M2Geo m2_geo(int C1, int C2) {
    M2Geo g;
    g.C1p = pow2_16(C1); g.C2p = pow2_16(C2);
    g.S1 = g.C1p + M2_PAD; g.S2 = g.C2p + M2_PAD;
    g.KS = (C1 + 15) & ~15;
    return g;
}
static size_t m2_lds_fwd(const M2Geo& g, int TM) {
    return ((size_t)g.C2p * g.S1 + (size_t)TM * (g.S1 > g.S2 ? g.S1 : g.S2)) * 4 + (size_t)TM * 8;
}
static size_t m2_lds_bwd(const M2Geo& g, int TM) {
    return ((size_t)g.C2p * g.S1 + (size_t)TM * g.S1 + (size_t)TM * g.S2 + 5 * (size_t)g.C2p) * 4 + (size_t)TM * 8;
}

struct M2Args {
    const float* pq; int ld, qoff; const int32_t* idx; int N, k, C1, C2; long long R;
    const float *mean1, *lo1, *scale1, *beta1, *w2; float slope;
    int PT, tpb, vec; long long ntiles;
};

__device__ __forceinline__ float4 ld4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// w2 [C2, C1] -> w2s [C2p][S1], zero outside
__device__ __forceinline__ void m2_stage_w2(const M2Args& a, int C1p, int C2p, int S1, float* w2s) {
    for (int e = threadIdx.x; e < C2p * C1p; e += 256) {
        const int n = e / C1p, c = e - n * C1p;
        w2s[n * S1 + c] = (n < a.C2 && c < a.C1) ? a.w2[(size_t)n * a.C1 + c] : 0.f;
    }
}

struct M2Bn1 { float4 mean, lo, scale, beta; bool act; int c4; };
__device__ __forceinline__ M2Bn1 m2_bn1_of_thread(const M2Args& a, int C1p) {
    M2Bn1 p;
    p.c4 = 4 * (threadIdx.x & (C1p / 4 - 1));
    p.act = p.c4 < a.C1;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    p.mean = p.act ? ld4(a.mean1 + p.c4, false) : z; p.lo = p.act ? ld4(a.lo1 + p.c4, false) : z;
    p.scale = p.act ? ld4(a.scale1 + p.c4, false) : z; p.beta = p.act ? ld4(a.beta1 + p.c4, false) : z;
    return p;
}

// rows of the tile that starts at point p0: rowm[row] = the row of pq that holds P of the edge's neighbour (-1 past the tile's last edge),
// rowr[row] = the row of pq that holds its Q (the point itself)
template <int TM>
__device__ __forceinline__ void m2_tile_rows(const M2Args& a, long long p0, int npts, int* rowm, int* rowr) {
    const int t = threadIdx.x;
    if (t < TM) {
        int m = -1, rr = -1;
        if (t < npts * a.k) {
            const int p = t / a.k;
            const long long r = p0 + p;
            rr = (int)r;
            m = (int)((r / a.N) * a.N + clampi(a.idx[p0 * a.k + t], a.N));
        }
        rowm[t] = m; rowr[t] = rr;
    }
}

template <int TM>
__device__ __forceinline__ void m2_build_h(const M2Args& a, const M2Bn1& b, int C1p, int S1, const int* rowm, const int* rowr, float* hs) {
    const int cq = C1p / 4, rstep = 256 / cq;
    for (int row = threadIdx.x / cq; row < TM; row += rstep) {
        float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
        const int m = rowm[row];
        if (m >= 0 && b.act) {
            const float4 p = ld4(a.pq + (size_t)m * a.ld + b.c4, a.vec), q = ld4(a.pq + (size_t)rowr[row] * a.ld + a.qoff + b.c4, a.vec);
            float z;
            h.x = lrelu_centred(__fadd_rn(p.x, q.x), b.mean.x, b.lo.x, b.scale.x, b.beta.x, a.slope, z);
            h.y = lrelu_centred(__fadd_rn(p.y, q.y), b.mean.y, b.lo.y, b.scale.y, b.beta.y, a.slope, z);
            h.z = lrelu_centred(__fadd_rn(p.z, q.z), b.mean.z, b.lo.z, b.scale.z, b.beta.z, a.slope, z);
            h.w = lrelu_centred(__fadd_rn(p.w, q.w), b.mean.w, b.lo.w, b.scale.w, b.beta.w, a.slope, z);
        }
        *reinterpret_cast<float4*>(hs + row * S1 + b.c4) = h;
    }
}

// y tile = h tile . w2^T: acc[rb][nb][r] = y[row wrow + 16 rb + 4 q + r][channel 16 nb + i]
template <int RB, int NB2>
__device__ __forceinline__ void m2_product_y(const float* hs, const float* w2s, int S1, int KS, int wrow, int i, int q, v4f (&acc)[RB][NB2]) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int nb = 0; nb < NB2; ++nb) acc[rb][nb] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < KS; s += 16) {
        float4 af[RB], bf[NB2];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) af[rb] = *reinterpret_cast<const float4*>(hs + (wrow + 16 * rb + i) * S1 + s + 4 * q);
#pragma unroll
        for (int nb = 0; nb < NB2; ++nb) bf[nb] = *reinterpret_cast<const float4*>(w2s + (16 * nb + i) * S1 + s + 4 * q);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int nb = 0; nb < NB2; ++nb) {
                acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rb].x, bf[nb].x, acc[rb][nb], 0, 0, 0);
                acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rb].y, bf[nb].y, acc[rb][nb], 0, 0, 0);
                acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rb].z, bf[nb].z, acc[rb][nb], 0, 0, 0);
                acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rb].w, bf[nb].w, acc[rb][nb], 0, 0, 0);
            }
    }
}

// ==================================================================================================================================== forward
// The pivot of BN2's moments: y of edge 0, summed channel by channel in one thread -- of the size of y, which is all a pivot has to be (the tile
// kernel's own y of that edge differs from it by the order of the sum).
__global__ __launch_bounds__(128) void m2_pivot_kernel(M2Args a, float* __restrict__ ypiv) {
    __shared__ float h0[M2_MAXC];
    const int t = threadIdx.x;
    if (t < a.C1) {
        float z;
        const float v = __fadd_rn(a.pq[(size_t)clampi(a.idx[0], a.N) * a.ld + t], a.pq[a.qoff + t]);
        h0[t] = lrelu_centred(v, a.mean1[t], a.lo1[t], a.scale1[t], a.beta1[t], a.slope, z);
    }
    __syncthreads();
    if (t < a.C2) {
        float y = 0.f;
        for (int c = 0; c < a.C1; ++c) y = __fadd_rn(y, __fmul_rn(a.w2[(size_t)t * a.C1 + c], h0[c]));
        ypiv[t] = y;
    }
}

// Per tile: rows, h, y (matrix cores), y through LDS to one thread per (point, channel): over its k values in ascending j the largest and the smallest
// y with their first j, and the float64 moments of y - pivot.  The moments stay in the thread over the workgroup's tiles (ascending), the threads of
// a channel are added in ascending order at the end, the workgroups by the finalize kernel: fixed order, no atomics.
template <int NB2, bool STATS>
__global__ __launch_bounds__(256) void m2_fwd_kernel(M2Args a, const float* __restrict__ ypiv, float* __restrict__ ymax, float* __restrict__ ymin,
                                                     int32_t* __restrict__ arg2, double* __restrict__ part) {
    constexpr int RB = 2, TM = 64 * RB, C2p = 16 * NB2, S2 = C2p + M2_PAD;
    extern __shared__ __attribute__((aligned(16))) float m2_smem[];
    __shared__ double sh[2 * 256];
    const int C1p = pow2_16(a.C1), S1 = C1p + M2_PAD, KS = (a.C1 + 15) & ~15;
    float* w2s = m2_smem;
    float* hs = w2s + C2p * S1;
    float* ys = hs;                                                               // overlay
    int* rowm = reinterpret_cast<int*>(hs + TM * (S1 > S2 ? S1 : S2));
    int* rowr = rowm + TM;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = lane & 15, q = lane >> 4, wrow = wave * 16 * RB;
    m2_stage_w2(a, C1p, C2p, S1, w2s);
    const M2Bn1 bn1 = m2_bn1_of_thread(a, C1p);
    const int c = t & (C2p - 1), part_id = t / C2p, parts = 256 / C2p;
    const bool cact = c < a.C2;
    const float piv = (STATS && cact) ? ypiv[c] : 0.f;
    double s[2] = {0.0, 0.0};
    const long long t0 = (long long)blockIdx.x * a.tpb, t1 = min(a.ntiles, t0 + a.tpb);
    for (long long tile = t0; tile < t1; ++tile) {
        const long long p0 = tile * a.PT;
        const int npts = (int)min((long long)a.PT, a.R - p0);
        __syncthreads();                                                          // the previous tile's ys (= hs) and rows have been read
        m2_tile_rows<TM>(a, p0, npts, rowm, rowr);
        __syncthreads();
        m2_build_h<TM>(a, bn1, C1p, S1, rowm, rowr, hs);
        __syncthreads();
        v4f acc[RB][NB2];
        m2_product_y<RB, NB2>(hs, w2s, S1, KS, wrow, i, q, acc);
        __syncthreads();                                                          // every wave is done with hs
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int nb = 0; nb < NB2; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) ys[(wrow + 16 * rb + 4 * q + r) * S2 + 16 * nb + i] = acc[rb][nb][r];
        __syncthreads();
        if (cact) {
            for (int p = part_id; p < npts; p += parts) {
                const float* yr = ys + p * a.k * S2 + c;
                float mx = yr[0], mn = mx;
                int jx = 0, jn = 0;
                if (STATS) { const double d = (double)mx - (double)piv; s[0] += d; s[1] += d * d; }
                for (int j = 1; j < a.k; ++j) {
                    const float y = yr[j * S2];
                    if (y > mx) { mx = y; jx = j; }
                    if (y < mn) { mn = y; jn = j; }
                    if (STATS) { const double d = (double)y - (double)piv; s[0] += d; s[1] += d * d; }
                }
                const long long o = (p0 + p) * a.C2 + c;
                ymax[o] = mx; ymin[o] = mn; arg2[o] = jx | (jn << 16);
            }
        }
    }
    if (STATS) col_reduce_store<2>(s, sh, c, part_id, C2p, parts, cact, c, a.C2, part);
}

// ---- workspace -------------------------------------------------------------------------------------------------------------------------------------------
// forward : ymax [R,C2] | ymin [R,C2] | scale1 [C1] | scale2 [C2] | ypiv [C2] | partials (2 sums, max(C1,C2) channels)
// backward: gsel [R,C2] | coef2 [2,C2] | coef1 [2,C1] | scale1 [C1] | prm2 [5,C2] | dpre1 [E,C1] | clamped idx [B,N*k] | off [B,N+1] | ent [B,N*k] |
//           dw2 partials [blocks, C2, C1] | partials
struct M2Ws { size_t ymax, ymin, scale1, scale2, ypiv, gsel, coef2, coef1, prm2, dpre1, idxc, off, ent, dw2p, part, total; };
static M2Ws m2_ws_fwd(long long R, int C1, int C2) {
    M2Ws w{};
    w.ymax = 0;
    w.ymin = align16((size_t)R * C2 * 4);
    w.scale1 = w.ymin + align16((size_t)R * C2 * 4);
    w.scale2 = w.scale1 + align16((size_t)C1 * 4);
    w.ypiv = w.scale2 + align16((size_t)C2 * 4);
    w.part = w.ypiv + align16((size_t)C2 * 4);
    w.total = w.part + part_bytes(C1 > C2 ? C1 : C2, 2);
    return w;
}
static M2Ws m2_ws_bwd(int B, int N, int k, int C1, int C2) {
    M2Ws w{};
    const size_t R = (size_t)B * N, E = (size_t)N * k;
    w.gsel = 0;
    w.coef2 = align16(R * C2 * 4);
    w.coef1 = w.coef2 + align16((size_t)2 * C2 * 4);
    w.scale1 = w.coef1 + align16((size_t)2 * C1 * 4);
    w.prm2 = w.scale1 + align16((size_t)C1 * 4);
    w.dpre1 = w.prm2 + align16((size_t)5 * C2 * 4);
    w.idxc = w.dpre1 + align16(R * k * C1 * 4);
    w.off = w.idxc + align16((size_t)B * E * 4);
    w.ent = w.off + align16((size_t)B * ((size_t)N + 1) * 4);
    w.dw2p = w.ent + align16((size_t)B * E * 4);
    w.part = w.dw2p + align16((size_t)M2_MAX_BLOCKS * C2 * C1 * 4);
    w.total = w.part + part_bytes(C1 > C2 ? C1 : C2, 2);
    return w;
}
static bool m2_dims_ok(int B, int N, int k, int C1, int C2) {
    if (B <= 0 || B > 65535 || N <= 0 || k <= 0 || k > M2_MAXK) return false;
    if (C1 < 4 || C1 > M2_MAXC || (C1 & 3) || C2 < 4 || C2 > M2_MAXC || (C2 & 3)) return false;
    const long long R = (long long)B * N;
    return (long long)N * k <= 0x7fffffffLL && R * k <= 0x7fffffffLL && R * k * C1 <= (0x7fffffffLL - 256) * 256;
}

extern "C" size_t act_edge_mlp2_workspace(int B, int N, int k, int C1, int C2) {
    if (!m2_dims_ok(B, N, k, C1, C2)) return 0;
    const size_t f = m2_ws_fwd((long long)B * N, C1, C2).total, b = m2_ws_bwd(B, N, k, C1, C2).total;
    return f > b ? f : b;
}

static void m2_tiling(M2Args& a, int TM, int max_blocks, int& nblk) {
    a.PT = TM / a.k;
    a.ntiles = (a.R + a.PT - 1) / a.PT;
    long long nb = a.ntiles < max_blocks ? a.ntiles : max_blocks;
    a.tpb = (int)((a.ntiles + nb - 1) / nb);
    nblk = (int)((a.ntiles + a.tpb - 1) / a.tpb);
}

template <int NB2>
static int m2_launch_fwd(const M2Args& a, int nblk, size_t lds, bool stats, const float* ypiv, float* ymax, float* ymin, int32_t* arg2, double* part,
                         hipStream_t s) {
    auto kt = m2_fwd_kernel<NB2, true>;
    auto kf = m2_fwd_kernel<NB2, false>;
    auto k = stats ? kt : kf;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3(nblk), dim3(256), lds, s, a, ypiv, ymax, ymin, arg2, part);
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_edge_mlp2_fwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C1, int C2, const float* gamma1,
                                     const float* beta1, float* running_mean1, float* running_var1, const float* w2, const float* gamma2,
                                     const float* beta2, float* running_mean2, float* running_var2, int training, float momentum1, float eps1,
                                     float momentum2, float eps2, float slope, float* out, int32_t* arg, float* ysel, float* stats1, float* stats2,
                                     void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!pq || !idx || !gamma1 || !beta1 || !w2 || !gamma2 || !beta2 || !out || !arg || !ysel || !stats1 || !stats2 || !workspace) return ACT_E_NULLPTR;
    if ((running_mean1 == nullptr) != (running_var1 == nullptr) || (running_mean2 == nullptr) != (running_var2 == nullptr)) return ACT_E_NULLPTR;
    if (!training && (!running_mean1 || !running_mean2)) return ACT_E_NULLPTR;
    if (!m2_dims_ok(B, N, k, C1, C2)) return ACT_E_BADARG;
    if (qoff < 0 || ld < C1 || qoff + C1 > ld || !(slope >= 0.f)) return ACT_E_BADARG;
    const long long R = (long long)B * N;
    const M2Ws w = m2_ws_fwd(R, C1, C2);
    if (workspace_bytes < w.total) return ACT_E_BADARG;
    const M2Geo g = m2_geo(C1, C2);
    const size_t lds = m2_lds_fwd(g, 128);
    if (lds > M2_LDS_MAX) return ACT_E_BADARG;
    char* ws = reinterpret_cast<char*>(workspace);
    float *ymax = (float*)(ws + w.ymax), *ymin = (float*)(ws + w.ymin), *scale1 = (float*)(ws + w.scale1), *scale2 = (float*)(ws + w.scale2);
    float* ypiv = (float*)(ws + w.ypiv);
    double* part = (double*)(ws + w.part);
    // stats1 / stats2 [3, C]: mean | mean_lo | rstd, what the backward needs of each BatchNorm
    float *mean1 = stats1, *lo1 = stats1 + C1, *rstd1 = stats1 + 2 * C1, *mean2 = stats2, *lo2 = stats2 + C2, *rstd2 = stats2 + 2 * C2;
    hipStream_t s = (hipStream_t)stream;
    const double M = (double)R * k;
    ActProfScope ps(KID_GN_LRELU_MAX, s, 2.0 * M * C1 * C2 + 12.0 * M * C1, 4.0 * (M * (2.0 * C1 + 1) + R * (double)C2 * 6));
    if (training) {
        const ColShape cs = col_shape(R, C1);
        hipLaunchKernelGGL((edge_bn_pass1_kernel<true, false>), dim3(cs.nblk), dim3(256), 0, s, pq, ld, qoff, idx, N, k, C1, R, cs.rpb, cs.tx_log,
                           (float*)nullptr, (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, part);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(edge_bn_finalize_kernel, dim3(cdiv(C1, 256)), dim3(256), 0, s, pq, ld, qoff, idx, N, part, cs.nblk, C1, M, 1, gamma1, beta1,
                           eps1, momentum1, running_mean1, running_var1, mean1, lo1, rstd1, scale1, (const float*)nullptr);
    } else {
        hipLaunchKernelGGL(edge_bn_finalize_kernel, dim3(cdiv(C1, 256)), dim3(256), 0, s, pq, ld, qoff, idx, N, part, 0, C1, M, 0, gamma1, beta1, eps1,
                           momentum1, running_mean1, running_var1, mean1, lo1, rstd1, scale1, (const float*)nullptr);
    }
    ACT_LAUNCH_CHECK();
    M2Args a{pq, ld, qoff, idx, N, k, C1, C2, R, mean1, lo1, scale1, beta1, w2, slope, 0, 0, 0, 0};
    a.vec = (!(ld & 3) && !(qoff & 3) && !((uintptr_t)pq & 15)) ? 1 : 0;
    int nblk = 0;
    m2_tiling(a, 128, CS_MAX_BLOCKS, nblk);
    if (training) {
        hipLaunchKernelGGL(m2_pivot_kernel, dim3(1), dim3(128), 0, s, a, ypiv);
        ACT_LAUNCH_CHECK();
    }
    int rc;
    switch (g.C2p) {
        case 16: rc = m2_launch_fwd<1>(a, nblk, lds, training != 0, ypiv, ymax, ymin, arg, part, s); break;
        case 32: rc = m2_launch_fwd<2>(a, nblk, lds, training != 0, ypiv, ymax, ymin, arg, part, s); break;
        case 64: rc = m2_launch_fwd<4>(a, nblk, lds, training != 0, ypiv, ymax, ymin, arg, part, s); break;
        default: rc = m2_launch_fwd<8>(a, nblk, lds, training != 0, ypiv, ymax, ymin, arg, part, s); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(edge_bn_finalize_kernel, dim3(cdiv(C2, 256)), dim3(256), 0, s, pq, ld, qoff, idx, N, part, nblk, C2, M, training ? 1 : 0, gamma2,
                       beta2, eps2, momentum2, running_mean2, running_var2, mean2, lo2, rstd2, scale2, (const float*)ypiv);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(edge_bn_apply_kernel, dim3(cdiv(R * C2, 256)), dim3(256), 0, s, ymax, ymin, C2, R * C2, scale2, beta2, mean2, lo2, slope, out, C2, 0,
                       arg, ysel);
    ACT_LAUNCH_CHECK(); return 0;
}

// =================================================================================================================================== backward
// dz2 is sparse -- per (point, channel) the one selected edge carries g = dout (z2 > 0 ? 1 : slope) -- so BN2's sums come from [R, C2] data:
//   dbeta2 = sum g, dgamma2 = sum g xhat2(ysel), m1 = dbeta2 / M, m2r = dgamma2 / M * rstd2
//   dy[e,c] = scale2 ((arg[r,c] == j ? g[r,c] : 0) - m1 - (y[e,c] - mean2) m2r)                       dense from here on
__global__ __launch_bounds__(256) void m2_bwd_sel_kernel(const float* __restrict__ ysel, const float* __restrict__ dout, int ldd, int C, long long R,
                                                         int rpb, int tx_log, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ mean, const float* __restrict__ mean_lo,
                                                         const float* __restrict__ rstd, float slope, float* __restrict__ gsel,
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
                const float y = ysel[r * C + c];
                float z;
                lrelu_centred(y, mu, lo, sc, be, slope, z);
                const float g = z > 0.f ? dout[r * ldd + c] : __fmul_rn(slope, dout[r * ldd + c]);
                gsel[r * C + c] = g;
                s[0] += (double)g;
                s[1] += (double)g * ((double)__fmul_rn(centred(y, mu, lo), rs));
            }
        }
        col_reduce_store<2>(s, sh, tx, ty, TX, TY, act, c, C, part);
    }
}

// dbeta | dgamma and the two coefficients of the BatchNorm backward from the block partials; scale_out (optional) = gamma * rstd
__global__ __launch_bounds__(256) void m2_bwd_coef_kernel(const double* __restrict__ part, int nblk, int C, double M, const float* __restrict__ gamma,
                                                          const float* __restrict__ rstd, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                          float* __restrict__ coef, float* __restrict__ scale_out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < nblk; ++p) { s1 += part[((size_t)p * 2 + 0) * C + c]; s2 += part[((size_t)p * 2 + 1) * C + c]; }
    dbeta[c] = (float)s1; dgamma[c] = (float)s2;
    coef[c] = (float)(s1 / M);
    coef[C + c] = (float)(s2 / M * (double)rstd[c]);
    if (scale_out) scale_out[c] = __fmul_rn(gamma[c], rstd[c]);
}

// prm2 [5, C2]: scale2 | m1 | m2r | mean2 | mean_lo2, what the tile kernel needs per column of dy
__global__ __launch_bounds__(128) void m2_bwd_prm2_kernel(int C2, const float* __restrict__ gamma2, const float* __restrict__ stats2,
                                                          const float* __restrict__ coef2, float* __restrict__ prm2) {
    const int c = threadIdx.x;
    if (c >= C2) return;
    prm2[c] = __fmul_rn(gamma2[c], stats2[2 * C2 + c]);
    prm2[C2 + c] = coef2[c]; prm2[2 * C2 + c] = coef2[C2 + c];
    prm2[3 * C2 + c] = stats2[c]; prm2[4 * C2 + c] = stats2[C2 + c];
}

// The dense pass.  Per tile: rows, h and y exactly as the forward forms them; dy in the accumulators' own layout, through LDS (ds); then on the matrix
// cores dh = dy . w2 (K = C2: dy read as 16-byte words along its row, w2s down its column) and dw2 += dy^T h (K = the tile's rows).  dpre1 = dh (z1 > 0 ?
// 1 : slope) -- slope >= 0, so the sign of h is the sign of z1 -- goes to the workspace, the one edge tensor the backward writes, and into BN1's two
// float64 column sums, xhat1 from a second gather of v (L2).  dw2 stays in registers over the workgroup's tiles.  RB = 2 (128 rows) where hs, ds and
// w2s fit the LDS together, else 1: a row's y does not depend on the tile it sits in.
template <int NB1, int NB2>
struct M2Bwd {
    static constexpr int C1p = 16 * NB1, C2p = 16 * NB2, S1 = C1p + M2_PAD, S2 = C2p + M2_PAD;
    static constexpr size_t lds(int TM) { return ((size_t)C2p * S1 + (size_t)TM * S1 + (size_t)TM * S2 + 5 * (size_t)C2p) * 4 + (size_t)TM * 8; }
    static constexpr int RB = lds(128) <= M2_LDS_MAX ? 2 : 1;
    // dw2 blocks of a wave: NB2 >= 4: m-blocks w, w + 4, ... and every n-block; NB2 < 4: m-block w % NB2 and n-blocks w / NB2, w / NB2 + 4 / NB2, ...
    static constexpr int MW = NB2 >= 4 ? NB2 / 4 : 1;
    static constexpr int NSTEP = NB2 >= 4 ? 1 : 4 / NB2;
    static constexpr int NW = (NB1 + NSTEP - 1) / NSTEP;
};

template <int NB1, int NB2>
__global__ __launch_bounds__(256) void m2_bwd_tile_kernel(M2Args a, const float* __restrict__ rstd1, const float* __restrict__ prm2g,
                                                          const int32_t* __restrict__ arg, const float* __restrict__ gsel,
                                                          float* __restrict__ dpre1, float* __restrict__ dw2p, double* __restrict__ part) {
    using G = M2Bwd<NB1, NB2>;
    constexpr int RB = G::RB, TM = 64 * RB, C1p = G::C1p, C2p = G::C2p, S1 = G::S1, S2 = G::S2, MW = G::MW, NSTEP = G::NSTEP, NW = G::NW;
    extern __shared__ __attribute__((aligned(16))) float m2_smem[];
    float* w2s = m2_smem;
    float* hs = w2s + C2p * S1;
    float* ds = hs + TM * S1;
    float* prm2 = ds + TM * S2;
    int* rowm = reinterpret_cast<int*>(prm2 + 5 * C2p);
    int* rowr = rowm + TM;
    const int KS = (a.C1 + 15) & ~15;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = lane & 15, q = lane >> 4, wrow = wave * 16 * RB;
    m2_stage_w2(a, C1p, C2p, S1, w2s);
    for (int e = t; e < 5 * C2p; e += 256) {
        const int w = e / C2p, c = e - w * C2p;
        prm2[e] = c < a.C2 ? prm2g[w * a.C2 + c] : 0.f;
    }
    const M2Bn1 bn1 = m2_bn1_of_thread(a, C1p);
    // BN1's per-column constants of this lane's columns 16 cb + i
    float mu1[NB1], lo1[NB1], rs1[NB1];
#pragma unroll
    for (int cb = 0; cb < NB1; ++cb) {
        const int c = 16 * cb + i;
        const bool ok = c < a.C1;
        mu1[cb] = ok ? a.mean1[c] : 0.f; lo1[cb] = ok ? a.lo1[c] : 0.f; rs1[cb] = ok ? rstd1[c] : 0.f;
    }
    double s0[NB1], s1[NB1];
#pragma unroll
    for (int cb = 0; cb < NB1; ++cb) s0[cb] = s1[cb] = 0.0;
    v4f dw[MW][NW];
#pragma unroll
    for (int u = 0; u < MW; ++u)
#pragma unroll
        for (int n = 0; n < NW; ++n) dw[u][n] = (v4f){0.f, 0.f, 0.f, 0.f};
    const int mb0 = NB2 >= 4 ? wave : wave % NB2, nb0 = NB2 >= 4 ? 0 : wave / NB2;

    const long long t0 = (long long)blockIdx.x * a.tpb, t1 = min(a.ntiles, t0 + a.tpb);
    for (long long tile = t0; tile < t1; ++tile) {
        const long long p0 = tile * a.PT;
        const int npts = (int)min((long long)a.PT, a.R - p0);
        const int nrows = npts * a.k;
        __syncthreads();                                                          // the previous tile's hs, ds and rows have been read
        m2_tile_rows<TM>(a, p0, npts, rowm, rowr);
        __syncthreads();
        m2_build_h<TM>(a, bn1, C1p, S1, rowm, rowr, hs);
        __syncthreads();
        {
            v4f acc[RB][NB2];
            m2_product_y<RB, NB2>(hs, w2s, S1, KS, wrow, i, q, acc);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wrow + 16 * rb + 4 * q + r;
                    const bool rok = row < nrows;
                    const int pt = rok ? rowr[row] : 0;
                    const int j = rok ? row - (int)(pt - p0) * a.k : 0;
#pragma unroll
                    for (int nb = 0; nb < NB2; ++nb) {
                        const int c = 16 * nb + i;
                        float dy = 0.f;
                        if (rok && c < a.C2) {
                            const long long o = (long long)pt * a.C2 + c;
                            const float g = arg[o] == j ? gsel[o] : 0.f;
                            const float cen = centred(acc[rb][nb][r], prm2[3 * C2p + c], prm2[4 * C2p + c]);
                            dy = __fmul_rn(prm2[c], __fsub_rn(__fsub_rn(g, prm2[C2p + c]), __fmul_rn(cen, prm2[2 * C2p + c])));
                        }
                        ds[row * S2 + c] = dy;
                    }
                }
        }
        __syncthreads();
        {   // dh = dy . w2: channel 16 s + 4 qq + tt of dy against row 16 s + 4 qq + tt of w2s
            v4f dh[RB][NB1];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int cb = 0; cb < NB1; ++cb) dh[rb][cb] = (v4f){0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < C2p; s += 16) {
                float4 af[RB];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) af[rb] = *reinterpret_cast<const float4*>(ds + (wrow + 16 * rb + i) * S2 + s + 4 * q);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    float bf[NB1];
#pragma unroll
                    for (int cb = 0; cb < NB1; ++cb) bf[cb] = w2s[(s + 4 * q + tt) * S1 + 16 * cb + i];
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        const float av = tt == 0 ? af[rb].x : tt == 1 ? af[rb].y : tt == 2 ? af[rb].z : af[rb].w;
#pragma unroll
                        for (int cb = 0; cb < NB1; ++cb) dh[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bf[cb], dh[rb][cb], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wrow + 16 * rb + 4 * q + r;
                    if (row >= nrows) continue;
                    const size_t pm = (size_t)rowm[row] * a.ld, qm = (size_t)rowr[row] * a.ld + a.qoff;
                    float* drow = dpre1 + (size_t)(p0 * a.k + row) * a.C1;
#pragma unroll
                    for (int cb = 0; cb < NB1; ++cb) {
                        const int c = 16 * cb + i;
                        if (c >= a.C1) continue;
                        const float d = dh[rb][cb][r];
                        const float dp = hs[row * S1 + c] > 0.f ? d : __fmul_rn(a.slope, d);
                        drow[c] = dp;
                        const float xhat = __fmul_rn(centred(__fadd_rn(a.pq[pm + c], a.pq[qm + c]), mu1[cb], lo1[cb]), rs1[cb]);
                        s0[cb] += (double)dp;
                        s1[cb] += (double)dp * (double)xhat;
                    }
                }
        }
        // dw2 += dy^T h over the tile's rows (rows past nrows are zero in ds)
        for (int kk = 0; kk < TM; kk += 4) {
            float af[MW], bf[NW];
#pragma unroll
            for (int u = 0; u < MW; ++u) af[u] = ds[(kk + q) * S2 + 16 * (mb0 + 4 * u) + i];
#pragma unroll
            for (int n = 0; n < NW; ++n) {
                const int nb = nb0 + NSTEP * n;
                bf[n] = nb < NB1 ? hs[(kk + q) * S1 + 16 * nb + i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < MW; ++u)
#pragma unroll
                for (int n = 0; n < NW; ++n) dw[u][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u], bf[n], dw[u][n], 0, 0, 0);
        }
    }
    // the workgroup's dw2: element (16 mb + 4 q + r, 16 nb + i)
    float* mine = dw2p + (size_t)blockIdx.x * a.C2 * a.C1;
#pragma unroll
    for (int u = 0; u < MW; ++u)
#pragma unroll
        for (int n = 0; n < NW; ++n) {
            const int mb = mb0 + 4 * u, nb = nb0 + NSTEP * n;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c2 = 16 * mb + 4 * q + r, c1 = 16 * nb + i;
                if (mb < NB2 && nb < NB1 && c2 < a.C2 && c1 < a.C1) mine[(size_t)c2 * a.C1 + c1] = dw[u][n][r];
            }
        }
    // BN1's sums: the 16 (wave, q) owners of a column, added in ascending order through LDS (hs and ds are free: 2 * 16 * C1p doubles <= TM * S1 floats)
    __syncthreads();
    double* red = reinterpret_cast<double*>(hs);
#pragma unroll
    for (int cb = 0; cb < NB1; ++cb) {
        red[(0 * 16 + wave * 4 + q) * C1p + 16 * cb + i] = s0[cb];
        red[(1 * 16 + wave * 4 + q) * C1p + 16 * cb + i] = s1[cb];
    }
    __syncthreads();
    for (int e = t; e < 2 * C1p; e += 256) {
        const int w = e / C1p, c = e - w * C1p;
        if (c < a.C1) {
            double acc = 0.0;
            for (int y = 0; y < 16; ++y) acc += red[(w * 16 + y) * C1p + c];
            part[((size_t)blockIdx.x * 2 + w) * a.C1 + c] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void m2_bwd_dw2_kernel(const float* __restrict__ dw2p, int nblk, int total, float* __restrict__ dw2) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float acc = 0.f;
    for (int p = 0; p < nblk; ++p) acc = __fadd_rn(acc, dw2p[(size_t)p * total + e]);
    dw2[e] = acc;
}

// dv[e,c] = scale1 (dpre1[e,c] - n1 - (v[e,c] - mean1) n2r); dQ[i] = sum_j dv, dP[m] = the sum over the inverse adjacency of m in ascending (i, j)
__global__ __launch_bounds__(256) void m2_bwd_dpq_kernel(const float* __restrict__ pq, int ld, int qoff, int N, int k, int C, long long total,
                                                         const float* __restrict__ scale, const float* __restrict__ mean,
                                                         const float* __restrict__ mean_lo, const float* __restrict__ coef,
                                                         const float* __restrict__ dpre1, const int32_t* __restrict__ idxc,
                                                         const int32_t* __restrict__ off, const int32_t* __restrict__ ent, float* __restrict__ dpq) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long r = e / C, b = r / N;
    const int c = (int)(e - r * C), n = (int)(r - b * N);
    const float mu = mean[c], lo = mean_lo[c], sc = scale[c], n1 = coef[c], n2r = coef[C + c];
    const float p = pq[r * ld + c], qv = pq[r * ld + qoff + c];
    float dq = 0.f;
    for (int j = 0; j < k; ++j) {
        const long long ed = r * k + j;
        const float v = __fadd_rn(pq[(b * N + idxc[ed]) * ld + c], qv);
        dq = __fadd_rn(dq, __fmul_rn(sc, __fsub_rn(__fsub_rn(dpre1[ed * C + c], n1), __fmul_rn(centred(v, mu, lo), n2r))));
    }
    dpq[r * ld + qoff + c] = dq;
    const int32_t* ob = off + b * ((long long)N + 1);
    const int32_t* eb = ent + b * (long long)N * k;
    float dp = 0.f;
    for (int x = ob[n]; x < ob[n + 1]; ++x) {
        const int en = eb[x], src = en / k;
        const float v = __fadd_rn(p, pq[(b * N + src) * ld + qoff + c]);
        dp = __fadd_rn(dp, __fmul_rn(sc, __fsub_rn(__fsub_rn(dpre1[(b * N * k + en) * C + c], n1), __fmul_rn(centred(v, mu, lo), n2r))));
    }
    dpq[r * ld + c] = dp;
}

template <int NB1, int NB2>
static int m2_launch_bwd(M2Args a, const float* rstd1, const float* prm2, const int32_t* arg, const float* gsel, float* dpre1, float* dw2p, double* part,
                         int& nblk, hipStream_t s) {
    using G = M2Bwd<NB1, NB2>;
    m2_tiling(a, 64 * G::RB, M2_MAX_BLOCKS, nblk);
    const size_t lds = G::lds(64 * G::RB);
    auto k = m2_bwd_tile_kernel<NB1, NB2>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3(nblk), dim3(256), lds, s, a, rstd1, prm2, arg, gsel, dpre1, dw2p, part);
    ACT_LAUNCH_CHECK(); return 0;
}

template <int NB1>
static int m2_launch_bwd_n2(int C2p, const M2Args& a, const float* rstd1, const float* prm2, const int32_t* arg, const float* gsel, float* dpre1,
                            float* dw2p, double* part, int& nblk, hipStream_t s) {
    switch (C2p) {
        case 16: return m2_launch_bwd<NB1, 1>(a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s);
        case 32: return m2_launch_bwd<NB1, 2>(a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s);
        case 64: return m2_launch_bwd<NB1, 4>(a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s);
        default: return m2_launch_bwd<NB1, 8>(a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s);
    }
}

extern "C" int act_edge_mlp2_bwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C1, int C2, const float* gamma1,
                                     const float* beta1, const float* w2, const float* gamma2, const float* beta2, const float* stats1,
                                     const float* stats2, float slope, const int32_t* arg, const float* ysel, const float* dout, int ldd, float* dpq,
                                     float* dgamma1, float* dbeta1, float* dw2, float* dgamma2, float* dbeta2, void* workspace, size_t workspace_bytes,
                                     act_stream_t stream) {
    if (!pq || !idx || !gamma1 || !beta1 || !w2 || !gamma2 || !beta2 || !stats1 || !stats2 || !arg || !ysel || !dout || !dpq || !dgamma1 || !dbeta1 ||
        !dw2 || !dgamma2 || !dbeta2 || !workspace)
        return ACT_E_NULLPTR;
    if (!m2_dims_ok(B, N, k, C1, C2)) return ACT_E_BADARG;
    if (qoff < C1 || ld < 2 * C1 || qoff + C1 > ld || ldd < C2 || !(slope >= 0.f)) return ACT_E_BADARG;   // P and Q must not overlap: both get a gradient
    const long long R = (long long)B * N, E = (long long)N * k;
    const M2Ws w = m2_ws_bwd(B, N, k, C1, C2);
    if (workspace_bytes < w.total) return ACT_E_BADARG;
    const M2Geo g = m2_geo(C1, C2);
    char* ws = reinterpret_cast<char*>(workspace);
    float *gsel = (float*)(ws + w.gsel), *coef2 = (float*)(ws + w.coef2), *coef1 = (float*)(ws + w.coef1), *scale1 = (float*)(ws + w.scale1);
    float *prm2 = (float*)(ws + w.prm2), *dpre1 = (float*)(ws + w.dpre1), *dw2p = (float*)(ws + w.dw2p);
    int32_t *idxc = (int32_t*)(ws + w.idxc), *off = (int32_t*)(ws + w.off), *ent = (int32_t*)(ws + w.ent);
    double* part = (double*)(ws + w.part);
    const float *mean1 = stats1, *lo1 = stats1 + C1, *rstd1 = stats1 + 2 * C1, *mean2 = stats2, *lo2 = stats2 + C2, *rstd2 = stats2 + 2 * C2;
    const double M = (double)R * k;
    hipStream_t s = (hipStream_t)stream;
    int nblk = 0;
    {
        ActProfScope ps(KID_BN_BWD, s, 6.0 * M * C1 * C2 + 20.0 * M * C1, 4.0 * (M * (5.0 * C1 + 1) + R * (double)C2 * 6));
        const ColShape cs = col_shape(R, C2);
        hipLaunchKernelGGL(m2_bwd_sel_kernel, dim3(cs.nblk), dim3(256), 0, s, ysel, dout, ldd, C2, R, cs.rpb, cs.tx_log, gamma2, beta2, mean2, lo2, rstd2,
                           slope, gsel, part);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(m2_bwd_coef_kernel, dim3(1), dim3(256), 0, s, part, cs.nblk, C2, M, gamma2, rstd2, dgamma2, dbeta2, coef2, (float*)nullptr);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(m2_bwd_prm2_kernel, dim3(1), dim3(128), 0, s, C2, gamma2, stats2, coef2, prm2);
        ACT_LAUNCH_CHECK();
        // scale1 = gamma1 * rstd1, as the forward's finalize formed it
        hipLaunchKernelGGL(m2_bwd_coef_kernel, dim3(1), dim3(256), 0, s, part, 0, C1, M, gamma1, rstd1, dgamma1, dbeta1, coef1, scale1);
        ACT_LAUNCH_CHECK();
        M2Args a{pq, ld, qoff, idx, N, k, C1, C2, R, mean1, lo1, scale1, beta1, w2, slope, 0, 0, 0, 0};
        a.vec = (!(ld & 3) && !(qoff & 3) && !((uintptr_t)pq & 15)) ? 1 : 0;
        int rc;
        switch (g.C1p) {
            case 16: rc = m2_launch_bwd_n2<1>(g.C2p, a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s); break;
            case 32: rc = m2_launch_bwd_n2<2>(g.C2p, a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s); break;
            case 64: rc = m2_launch_bwd_n2<4>(g.C2p, a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s); break;
            default: rc = m2_launch_bwd_n2<8>(g.C2p, a, rstd1, prm2, arg, gsel, dpre1, dw2p, part, nblk, s); break;
        }
        if (rc) return rc;
        hipLaunchKernelGGL(m2_bwd_coef_kernel, dim3(1), dim3(256), 0, s, part, nblk, C1, M, gamma1, rstd1, dgamma1, dbeta1, coef1, (float*)nullptr);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(m2_bwd_dw2_kernel, dim3(cdiv((long long)C1 * C2, 256)), dim3(256), 0, s, dw2p, nblk, C1 * C2, dw2);
        ACT_LAUNCH_CHECK();
        hipLaunchKernelGGL(clamp_idx_kernel, dim3(cdiv(R * k, 256)), dim3(256), 0, s, idx, R * k, N, idxc);
        ACT_LAUNCH_CHECK();
    }
    const int rc = act_sa_build_adjacency(idxc, B, N, (int)E, off, ent, s);
    if (rc) return rc;
    ActProfScope ps(KID_ROW_SCATTER, s, 14.0 * M * C1, 4.0 * (M * (6.0 * C1 + 2) + R * (double)C1 * 4));
    hipLaunchKernelGGL(m2_bwd_dpq_kernel, dim3(cdiv(R * C1, 256)), dim3(256), 0, s, pq, ld, qoff, N, k, C1, R * C1, scale1, mean1, lo1, coef1, dpre1, idxc,
                       off, ent, dpq);
    ACT_LAUNCH_CHECK(); return 0;
}

// ============================================================================================================== the 3x3 transform of a cloud
// y[b,n,:] = x[b,n,:] . T[b]; dx = dy . T[b]^T; dT[b] = sum_n x_n^T dy_n: one workgroup per cloud, thread t adds its points n = t, t + 256, ... in
// float64, the 256 threads are added in ascending order.
__global__ __launch_bounds__(256) void transform3_fwd_kernel(const float* __restrict__ x, const float* __restrict__ T, int N, long long total,
                                                             float* __restrict__ y) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float* t = T + (e / N) * 9;
    const float a = x[3 * e], b = x[3 * e + 1], c = x[3 * e + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) y[3 * e + j] = __fadd_rn(__fadd_rn(__fmul_rn(a, t[j]), __fmul_rn(b, t[3 + j])), __fmul_rn(c, t[6 + j]));
}

__global__ __launch_bounds__(256) void transform3_bwd_kernel(const float* __restrict__ x, const float* __restrict__ T, const float* __restrict__ dy,
                                                             int N, float* __restrict__ dx, float* __restrict__ dT) {
    __shared__ double sh[9 * 256];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* tb = T + (size_t)b * 9;
    float tm[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) tm[u] = tb[u];
    double acc[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) acc[u] = 0.0;
    for (int n = t; n < N; n += 256) {
        const size_t o = 3 * ((size_t)b * N + n);
        const float xv[3] = {x[o], x[o + 1], x[o + 2]}, g[3] = {dy[o], dy[o + 1], dy[o + 2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dx[o + i] = __fadd_rn(__fadd_rn(__fmul_rn(g[0], tm[3 * i]), __fmul_rn(g[1], tm[3 * i + 1])), __fmul_rn(g[2], tm[3 * i + 2]));
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 * i + j] += (double)xv[i] * (double)g[j];
        }
    }
#pragma unroll
    for (int u = 0; u < 9; ++u) sh[u * 256 + t] = acc[u];
    __syncthreads();
    if (t < 9) {
        double a = 0.0;
        for (int y = 0; y < 256; ++y) a += sh[t * 256 + y];
        dT[(size_t)b * 9 + t] = (float)a;
    }
}

extern "C" int act_cloud_transform3_fwd_f32(const float* x, const float* T, int B, int N, float* y, act_stream_t stream) {
    if (!x || !T || !y) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || (long long)B * N > 0x7fffffffLL / 3) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 15.0 * B * N, 24.0 * B * N);
    hipLaunchKernelGGL(transform3_fwd_kernel, dim3(cdiv((long long)B * N, 256)), dim3(256), 0, s, x, T, N, (long long)B * N, y);
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_cloud_transform3_bwd_f32(const float* x, const float* T, const float* dy, int B, int N, float* dx, float* dT, act_stream_t stream) {
    if (!x || !T || !dy || !dx || !dT) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || (long long)B * N > 0x7fffffffLL / 3) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 33.0 * B * N, 36.0 * B * N);
    hipLaunchKernelGGL(transform3_bwd_kernel, dim3(B), dim3(256), 0, s, x, T, dy, N, dx, dT);
    ACT_LAUNCH_CHECK(); return 0;
}
