// offset_attn.hip -- PCT's offset attention (Guo et al., CVM 2021) on the f32 matrix cores, forward and backward, without an [N,N] tensor in memory.
//
//   E[i,j] = q_i . k_j      P[i,j] = exp(E[i,j] - lse_i)      c_j = sum_i P[i,j]      s_j = 1 / (1e-9f + c_j)      x_r[j] = s_j sum_i P[i,j] v_i
//
// Every product is v_mfma_f32_16x16x4_f32 on 16 x 16 tiles of (i, j).  A tile of E comes in one of two forms, chosen by which side the workgroup owns:
//   "column form" (the workgroup owns 16 columns j, walks the i tiles)   lane (n, g) register r holds E[i0 + 4g + r][j0 + n]
//   "row form"    (the workgroup owns 16 rows i, walks the j tiles)      lane (n, g) register r holds E[i0 + n][j0 + 4g + r]
// with n = lane % 16, g = lane / 16.  Either way register r of lane (n, g) is what the NEXT product wants from that lane as its A operand in step r
// (the MFMA's k index g then stands for the walked index 4g + r, on both operands alike), so P and dE go from the accumulators straight back into
// the matrix pipe: no LDS round trip, no shuffle.  The reductions over the head width Dq and the value width C split the width in four contiguous
// quarters, one per g, so a lane reads one contiguous piece of its row (float4 loads when the quarter is a multiple of 4 floats).
// The 4 waves of a workgroup split the walked tiles (wave w takes tiles w, w + 4, ..); their partial sums meet in LDS and are added in wave order.
// Fixed order everywhere, no atomics: a cloud's result does not depend on B and is bit-identical run to run.
//
// Forward: oa_stats_kernel (row form; online max / sum -> m_i, the row maximum, an element of E, and ll_i = log2 l_i, both kept in the workspace
// for the second pass, and lse_i = m_i + ln l_i for the caller), oa_out_kernel (column form; weights exp2((E - m_i) log2e - ll_i) <= 1, a plain
// running c_j).  The weight is formed from the PAIR (m_i, ll_i), not from the rounded lse_i: at energies of 144 the rounding of lse alone is a
// common factor of up to 1 +- 7.6e-6 on a whole row of P, the row then no longer sums to 1, and with |k_j| = 12 that was measured as 1.1e-4 of dq.
// E - m_i is exact near the maximum, so the pair keeps every weight to a few ulps.  With q = 0 the pair is (0, log2 N), for N a power of two the
// weights are exactly 1 / N and the output is the exact mean.
// Backward: oa_stats_kernel again (the pair is not saved: one Dq-deep sweep gives it back bit for bit), oa_bwd_prep_kernel (gs_j = s_j g_j,
// ds_j = s_j g_j . x_r[j]), oa_bwd_rows_kernel<false> (row form: R_i and dv), oa_bwd_rows_kernel<true> (row form: dq, needs R),
// oa_bwd_cols_kernel (column form: dk).  dP[i,j] = v_i . gs_j - ds_j is recomputed in each.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define OA_LOG2E 1.4426950408889634f
#define OA_LN2 0.6931471805599453f
#define OA_TILE 16
#define OA_Q4 16                 // Dq / 4 at most
#define OA_C4 64                 // C / 4 at most
#define OA_CT 16                 // 16-wide tiles of C at most
#define OA_DT 4                  // 16-wide tiles of Dq at most
#define OA_RED (3 * 64 * 64)     // floats: the accumulators of waves 1..3

struct OaArgs {
    const float *q, *k, *v;
    int N, Dq, C, dq4, c4, nct, ndt, vq, vc;
};

__device__ __forceinline__ f32x4 oa_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float oa_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// x[0 .. n) = p[0 .. n), n <= MAXN (wave-uniform); vec: n % 4 == 0 and p 16-byte aligned
template <int MAXN>
__device__ __forceinline__ void oa_chunk(const float* __restrict__ p, int n, int vec, float* x) {
    if (vec) {
#pragma unroll
        for (int u = 0; u < MAXN / 4; ++u)
            if (4 * u < n) {
                const float4 t = *reinterpret_cast<const float4*>(p + 4 * u);
                x[4 * u] = t.x; x[4 * u + 1] = t.y; x[4 * u + 2] = t.z; x[4 * u + 3] = t.w;
            }
    } else {
#pragma unroll
        for (int u = 0; u < MAXN; ++u)
            if (u < n) x[u] = p[u];
    }
}

// sum_u a[u] (x) b[u] over u < n on two accumulators (even and odd u), added at the end: the same order wherever it is called
template <int MAXN>
__device__ __forceinline__ f32x4 oa_dot(const float* a, const float* b, int n) {
    f32x4 e = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < MAXN; u += 2)
        if (u < n) {
            e = oa_mfma(a[u], b[u], e);
            if (u + 1 < n) o = oa_mfma(a[u + 1], b[u + 1], o);
        }
    return e + o;
}

// the accumulators of waves 1..3 are added to wave 0's in wave order
template <int NT>
__device__ __forceinline__ void oa_reduce(f32x4* acc, int nt, float* red, int w, int lane) {
    if (w > 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < nt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(((w - 1) * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
            }
    }
    __syncthreads();
    if (w == 0) {
        for (int ww = 0; ww < 3; ++ww) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (t < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t][r] += red[((ww * NT + t) * 4 + r) * 64 + lane];
                }
        }
    }
}

// ---- forward, first pass: lse_i, m_i and ll_i ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void oa_stats_kernel(OaArgs a, float* __restrict__ lse, float* __restrict__ mrow, float* __restrict__ ll) {
    const int b = blockIdx.y, i0 = blockIdx.x * OA_TILE, lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    const float* q = a.q + (size_t)b * a.N * a.Dq;
    const float* k = a.k + (size_t)b * a.N * a.Dq;
    float qf[OA_Q4], kf[OA_Q4];
    oa_chunk<OA_Q4>(q + (size_t)min(i0 + n, a.N - 1) * a.Dq + g * a.dq4, a.dq4, a.vq, qf);
    float m = -3e38f, l = 0.f;                                         // of row i0 + n over the columns j = 4g + r (mod 16) this lane meets
    for (int j0 = 0; j0 < a.N; j0 += OA_TILE) {
        oa_chunk<OA_Q4>(k + (size_t)min(j0 + n, a.N - 1) * a.Dq + g * a.dq4, a.dq4, a.vq, kf);
        const f32x4 e = oa_dot<OA_Q4>(kf, qf, a.dq4);                 // row form
        float t[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = (j0 + 4 * g + r < a.N) ? e[r] : -INFINITY;
        const float mn = fmaxf(m, fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3])));
        l = l * oa_exp2((m - mn) * OA_LOG2E) + (((oa_exp2((t[0] - mn) * OA_LOG2E) + oa_exp2((t[1] - mn) * OA_LOG2E)) +
                                                 oa_exp2((t[2] - mn) * OA_LOG2E)) + oa_exp2((t[3] - mn) * OA_LOG2E));
        m = mn;
    }
    float mg[4], lg[4];
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) { mg[gg] = __shfl(m, n + 16 * gg); lg[gg] = __shfl(l, n + 16 * gg); }
    const float M = fmaxf(fmaxf(mg[0], mg[1]), fmaxf(mg[2], mg[3]));
    float L = 0.f;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) L += lg[gg] * oa_exp2((mg[gg] - M) * OA_LOG2E);
    if (g == 0 && i0 + n < a.N) {
        const float v = __builtin_amdgcn_logf(L);                      // v_log_f32: log2
        mrow[(size_t)b * a.N + i0 + n] = M;
        ll[(size_t)b * a.N + i0 + n] = v;
        lse[(size_t)b * a.N + i0 + n] = M + v * OA_LN2;
    }
}

// ---- forward, second pass: c_j and x_r[j] (or x[j] - x_r[j]) -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void oa_out_kernel(OaArgs a, const float* __restrict__ mrow, const float* __restrict__ ll,
                                                     const float* __restrict__ x, float* __restrict__ out, float* __restrict__ colsum,
                                                     float* __restrict__ xr) {
    __shared__ float red[OA_RED];
    __shared__ float cred[4 * 64];
    const int b = blockIdx.y, j0 = blockIdx.x * OA_TILE, lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const size_t row0 = (size_t)b * a.N;
    const float* q = a.q + row0 * a.Dq;
    const float* v = a.v + row0 * a.C;
    const float* mb = mrow + row0;
    const float* llb = ll + row0;
    float kf[OA_Q4], qf[OA_Q4];
    oa_chunk<OA_Q4>(a.k + (row0 + min(j0 + n, a.N - 1)) * a.Dq + g * a.dq4, a.dq4, a.vq, kf);
    f32x4 acc[OA_CT];
#pragma unroll
    for (int t = 0; t < OA_CT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float cp = 0.f;
    const int ntile = (a.N + OA_TILE - 1) / OA_TILE;
    for (int it = w; it < ntile; it += 4) {
        const int i0 = it * OA_TILE;
        oa_chunk<OA_Q4>(q + (size_t)min(i0 + n, a.N - 1) * a.Dq + g * a.dq4, a.dq4, a.vq, qf);
        const f32x4 e = oa_dot<OA_Q4>(qf, kf, a.dq4);                 // column form
        float p[4];
        const float* vrow[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ii = i0 + 4 * g + r, ic = min(ii, a.N - 1);
            const float L = ii < a.N ? llb[ic] : INFINITY;
            p[r] = oa_exp2(__builtin_fmaf(e[r] - mb[ic], OA_LOG2E, -L));
            cp += p[r];
            vrow[r] = v + (size_t)ic * a.C;
        }
#pragma unroll
        for (int t = 0; t < OA_CT; ++t)
            if (t < a.nct) {
                const int col = min(t * 16 + n, a.C - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t] = oa_mfma(p[r], vrow[r][col], acc[t]);
            }
    }
    cred[w * 64 + lane] = cp;
    oa_reduce<OA_CT>(acc, a.nct, red, w, lane);                        // (its barrier covers cred)
    if (w != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int jl = 4 * g + r, j = j0 + jl;
        float c = 0.f;
        for (int ww = 0; ww < 4; ++ww)
            for (int gg = 0; gg < 4; ++gg) c += cred[ww * 64 + gg * 16 + jl];
        if (j >= a.N) continue;
        const float s = 1.0f / (1e-9f + c);
        if (n == 0) colsum[row0 + j] = c;
#pragma unroll
        for (int t = 0; t < OA_CT; ++t)
            if (t < a.nct) {
                const int col = t * 16 + n;
                if (col < a.C) {
                    const size_t at = (row0 + j) * a.C + col;
                    const float val = acc[t][r] * s;
                    if (xr) xr[at] = val;
                    out[at] = x ? x[at] - val : val;
                }
            }
    }
}

// ---- backward: gs_j = s_j g_j, ds_j = s_j (g_j . x_r[j]); g = sign * dout ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void oa_bwd_prep_kernel(const float* __restrict__ dout, const float* __restrict__ xr,
                                                          const float* __restrict__ colsum, long long rows, int C, float sign, float* __restrict__ gs,
                                                          float* __restrict__ ds) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                           // (whole waves)
    const float s = 1.0f / (1e-9f + colsum[row]);
    float d = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float gv = sign * dout[row * C + c];
        d = __builtin_fmaf(gv, xr[row * C + c], d);
        gs[row * C + c] = s * gv;
    }
    d = wave_sum_f32(d);
    if (lane == 0) ds[row] = s * d;
}

// ---- backward, row form: the workgroup owns rows i0 .. i0 + 15.  DQ == false: R_i = sum_j P dP and dv_i = sum_j P[i,j] gs_j;  DQ == true:
// dq_i = sum_j P (dP - R_i) k_j ---------------------------------------------------------------------------------------------------------------------------
template <bool DQ>
__global__ __launch_bounds__(256) void oa_bwd_rows_kernel(OaArgs a, const float* __restrict__ gs, const float* __restrict__ ds,
                                                          const float* __restrict__ mrow, const float* __restrict__ ll, float* __restrict__ R,
                                                          float* __restrict__ dst) {
    constexpr int NT = DQ ? OA_DT : OA_CT;
    __shared__ float red[3 * NT * 4 * 64];
    __shared__ float sred[4 * 64];
    const int b = blockIdx.y, i0 = blockIdx.x * OA_TILE, lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const size_t row0 = (size_t)b * a.N;
    const float* k = a.k + row0 * a.Dq;
    const float* gsb = gs + row0 * a.C;
    const float* dsb = ds + row0;
    const int i = min(i0 + n, a.N - 1);
    float qf[OA_Q4], kf[OA_Q4], vf[OA_C4], gf[OA_C4];
    oa_chunk<OA_Q4>(a.q + (row0 + i) * a.Dq + g * a.dq4, a.dq4, a.vq, qf);
    oa_chunk<OA_C4>(a.v + (row0 + i) * a.C + g * a.c4, a.c4, a.vc, vf);
    const float Mi = mrow[row0 + i], Li = ll[row0 + i], Ri = DQ ? R[row0 + i] : 0.f;
    const int nt = DQ ? a.ndt : a.nct, wid = DQ ? a.Dq : a.C;
    const float* src = DQ ? k : gsb;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float rp = 0.f;
    const int ntile = (a.N + OA_TILE - 1) / OA_TILE;
    for (int jt = w; jt < ntile; jt += 4) {
        const int j0 = jt * OA_TILE, jr = min(j0 + n, a.N - 1);
        oa_chunk<OA_Q4>(k + (size_t)jr * a.Dq + g * a.dq4, a.dq4, a.vq, kf);
        oa_chunk<OA_C4>(gsb + (size_t)jr * a.C + g * a.c4, a.c4, a.vc, gf);
        const f32x4 e = oa_dot<OA_Q4>(kf, qf, a.dq4);                 // row form
        const f32x4 dp = oa_dot<OA_C4>(gf, vf, a.c4);
        float op[4];
        const float* srow[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jj = j0 + 4 * g + r, jc = min(jj, a.N - 1);
            const float p = jj < a.N ? oa_exp2(__builtin_fmaf(e[r] - Mi, OA_LOG2E, -Li)) : 0.f;
            const float d = dp[r] - dsb[jc];
            if (DQ) op[r] = p * (d - Ri);
            else { rp = __builtin_fmaf(p, d, rp); op[r] = p; }
            srow[r] = src + (size_t)jc * wid;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < nt) {
                const int col = min(t * 16 + n, wid - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t] = oa_mfma(op[r], srow[r][col], acc[t]);
            }
    }
    if (!DQ) sred[w * 64 + lane] = rp;
    oa_reduce<NT>(acc, nt, red, w, lane);
    if (w != 0) return;
    if (!DQ && g == 0 && i0 + n < a.N) {
        float s = 0.f;
        for (int ww = 0; ww < 4; ++ww)
            for (int gg = 0; gg < 4; ++gg) s += sred[ww * 64 + gg * 16 + n];
        R[row0 + i0 + n] = s;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ii = i0 + 4 * g + r;
        if (ii >= a.N) continue;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < nt) {
                const int col = t * 16 + n;
                if (col < wid) dst[(row0 + ii) * wid + col] = acc[t][r];
            }
    }
}

// ---- backward, column form: the workgroup owns columns j0 .. j0 + 15: dk_j = sum_i P (dP - R_i) q_i --------------------------------------------------------
__global__ __launch_bounds__(256) void oa_bwd_cols_kernel(OaArgs a, const float* __restrict__ gs, const float* __restrict__ ds,
                                                          const float* __restrict__ mrow, const float* __restrict__ ll, const float* __restrict__ R,
                                                          float* __restrict__ dk) {
    __shared__ float red[3 * OA_DT * 4 * 64];
    const int b = blockIdx.y, j0 = blockIdx.x * OA_TILE, lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const size_t row0 = (size_t)b * a.N;
    const float* q = a.q + row0 * a.Dq;
    const float* v = a.v + row0 * a.C;
    const float* mb = mrow + row0;
    const float* llb = ll + row0;
    const float* Rb = R + row0;
    const int j = min(j0 + n, a.N - 1);
    float qf[OA_Q4], kf[OA_Q4], vf[OA_C4], gf[OA_C4];
    oa_chunk<OA_Q4>(a.k + (row0 + j) * a.Dq + g * a.dq4, a.dq4, a.vq, kf);
    oa_chunk<OA_C4>(gs + (row0 + j) * a.C + g * a.c4, a.c4, a.vc, gf);
    const float dsj = ds[row0 + j];
    f32x4 acc[OA_DT];
#pragma unroll
    for (int t = 0; t < OA_DT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntile = (a.N + OA_TILE - 1) / OA_TILE;
    for (int it = w; it < ntile; it += 4) {
        const int i0 = it * OA_TILE, ir = min(i0 + n, a.N - 1);
        oa_chunk<OA_Q4>(q + (size_t)ir * a.Dq + g * a.dq4, a.dq4, a.vq, qf);
        oa_chunk<OA_C4>(v + (size_t)ir * a.C + g * a.c4, a.c4, a.vc, vf);
        const f32x4 e = oa_dot<OA_Q4>(qf, kf, a.dq4);                 // column form
        const f32x4 dp = oa_dot<OA_C4>(vf, gf, a.c4);
        float op[4];
        const float* srow[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ii = i0 + 4 * g + r, ic = min(ii, a.N - 1);
            const float p = ii < a.N ? oa_exp2(__builtin_fmaf(e[r] - mb[ic], OA_LOG2E, -llb[ic])) : 0.f;
            op[r] = p * ((dp[r] - dsj) - Rb[ic]);
            srow[r] = q + (size_t)ic * a.Dq;
        }
#pragma unroll
        for (int t = 0; t < OA_DT; ++t)
            if (t < a.ndt) {
                const int col = min(t * 16 + n, a.Dq - 1);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t] = oa_mfma(op[r], srow[r][col], acc[t]);
            }
    }
    oa_reduce<OA_DT>(acc, a.ndt, red, w, lane);
    if (w != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int jj = j0 + 4 * g + r;
        if (jj >= a.N) continue;
#pragma unroll
        for (int t = 0; t < OA_DT; ++t)
            if (t < a.ndt) {
                const int col = t * 16 + n;
                if (col < a.Dq) dk[(row0 + jj) * a.Dq + col] = acc[t][r];
            }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
static bool oa_shape_ok(int B, int N, int Dq, int C) {
    return B >= 1 && B <= 65535 && N >= 1 && N <= 1024 && Dq >= 4 && Dq <= 64 && Dq % 4 == 0 && C >= 4 && C <= 256 && C % 4 == 0;
}
static size_t oa_rows(int B, int N) { return ((size_t)B * N + 63) & ~(size_t)63; }          // floats per [B,N] array of the workspace
static bool oa_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" size_t act_offset_attn_workspace(int B, int N, int Dq, int C) {
    if (!oa_shape_ok(B, N, Dq, C)) return 0;
    return (5 * oa_rows(B, N) + (size_t)B * N * C) * sizeof(float);
}

static OaArgs oa_args(const float* q, const float* k, const float* v, const float* extra, int N, int Dq, int C) {
    OaArgs a;
    a.q = q; a.k = k; a.v = v; a.N = N; a.Dq = Dq; a.C = C; a.dq4 = Dq / 4; a.c4 = C / 4; a.nct = (C + 15) / 16; a.ndt = (Dq + 15) / 16;
    a.vq = (a.dq4 % 4 == 0 && oa_al16(q) && oa_al16(k)) ? 1 : 0;
    a.vc = (a.c4 % 4 == 0 && oa_al16(v) && oa_al16(extra)) ? 1 : 0;
    return a;
}

extern "C" int act_offset_attn_fwd_f32(const float* q, const float* k, const float* v, const float* x, int B, int N, int Dq, int C, float* out,
                                       float* lse, float* colsum, float* xr, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!oa_shape_ok(B, N, Dq, C)) return ACT_E_BADARG;
    if (!q || !k || !v || !out || !lse || !colsum || !workspace) return ACT_E_NULLPTR;
    if (workspace_bytes < act_offset_attn_workspace(B, N, Dq, C) || !oa_al16(workspace)) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    float *mrow = (float*)workspace, *ll = mrow + oa_rows(B, N);
    const OaArgs a = oa_args(q, k, v, v, N, Dq, C);
    const dim3 grid((N + OA_TILE - 1) / OA_TILE, B);
    hipLaunchKernelGGL(oa_stats_kernel, grid, dim3(64), 0, s, a, lse, mrow, ll);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(oa_out_kernel, grid, dim3(256), 0, s, a, (const float*)mrow, (const float*)ll, x, out, colsum, xr);
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" int act_offset_attn_bwd_f32(const float* q, const float* k, const float* v, const float* colsum, const float* xr, const float* dout,
                                       int negate, int B, int N, int Dq, int C, float* dq, float* dk, float* dv, void* workspace,
                                       size_t workspace_bytes, act_stream_t stream) {
    if (!oa_shape_ok(B, N, Dq, C)) return ACT_E_BADARG;
    if (!q || !k || !v || !colsum || !xr || !dout || !dq || !dk || !dv || !workspace) return ACT_E_NULLPTR;
    if (dq == dk) return ACT_E_BADARG;
    if (workspace_bytes < act_offset_attn_workspace(B, N, Dq, C) || !oa_al16(workspace)) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t nr = oa_rows(B, N);
    float *mrow = (float*)workspace, *ll = mrow + nr, *ds = ll + nr, *R = ds + nr, *lse = R + nr, *gs = lse + nr;
    const long long rows = (long long)B * N;
    const OaArgs a = oa_args(q, k, v, gs, N, Dq, C);
    const dim3 grid((N + OA_TILE - 1) / OA_TILE, B);
    hipLaunchKernelGGL(oa_stats_kernel, grid, dim3(64), 0, s, a, lse, mrow, ll);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(oa_bwd_prep_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, dout, xr, colsum, rows, C, negate ? -1.f : 1.f, gs, ds);
    ACT_LAUNCH_CHECK();
    const float *cm = mrow, *cl = ll, *cg = gs, *cd = ds;
    hipLaunchKernelGGL(oa_bwd_rows_kernel<false>, grid, dim3(256), 0, s, a, cg, cd, cm, cl, R, dv);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(oa_bwd_rows_kernel<true>, grid, dim3(256), 0, s, a, cg, cd, cm, cl, R, dq);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(oa_bwd_cols_kernel, grid, dim3(256), 0, s, a, cg, cd, cm, cl, (const float*)R, dk);
    ACT_LAUNCH_CHECK();
    return 0;
}
