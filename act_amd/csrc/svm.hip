// svm.hip -- linear-SVM validation of pretrained features (tools/runner_pretrain.py:47-51, 228-287: sklearn.svm.LinearSVC() on extracted features),
// solved on the device.  Objective per class c (liblinear's L2-regularised L2-loss SVC, one-vs-rest, the bias regularised as liblinear's appended
// constant feature but carried as a separate scalar):
//     f_c(w, b) = 1/2 (|w|^2 + b^2) + C sum_i max(0, 1 - y_ic (x_i . w + b))^2,      y_ic = +1 if labels[i] == classes[c] else -1
// All K <= 64 classes are solved together by Newton-CG on the generalised Hessian H_c = I + 2C X_A^T X_A (A: rows with positive hinge).
//
// One Newton iteration (act_svm_newton_f32) is a fixed sequence of launches; every decision (CG scalars, CG stop, step length, Armijo test,
// convergence flag) is taken per class on the device, and a kernel whose classes are all frozen returns at once:
//     scores  M = X W^T + b                     svm_scores_kernel   (64 x 64 output tile per workgroup, 4 x 4 per lane, X streamed with 16-byte loads)
//     hinge   R = y max(0, 1 - y m), sum h^2    svm_hinge_kernel    (per-row-block float64 partials, no atomics)
//     X^T R                                     svm_tprod_kernel    (256 rows per workgroup -> fp32 partial [K, D] tiles, summed in float64 by the reader)
//     g = w - 2C X^T R, CG start, stop test     svm_grad_kernel     (one wave per class)
//     max_cg x { Z = A o (X D^T + d_b) ; X^T Z ; alpha, s, r, beta, d }     scores (masked) / tprod / svm_cg_kernel (one wave per class)
//     Z = X S^T + s_b ; loss(alpha) for alpha = 0, 1, 1/2, ... 2^-15 ; largest alpha that passes Armijo, W += alpha S     scores / svm_ls_eval / svm_ls_pick
// The line search evaluates the TRUE objective along the step (scores are linear in alpha: m + alpha z, in float64) for all candidates in one pass,
// so a step that increases the objective cannot be accepted; no candidate accepted = "no progress" = the class ends.
//
// Reductions: fixed order everywhere (lane-strided partial sums, xor butterfly, partial blocks in index order), float64 wherever a sum runs over the
// N rows.  No atomics: every output is bit-identical run to run.
#include "common.h"
#include <math.h>

#define SVM_MAXK 64
#define SVM_RB 64            // rows per workgroup of the row-parallel passes (scores, hinge, line search)
#define SVM_TROWS 256        // rows per workgroup of the transposed product
#define SVM_KC 32            // reduction chunk staged in LDS
#define SVM_LDT (64 + 4)     // LDS row stride of a 64-wide tile (16-byte aligned rows)
#define SVM_NLS 16           // step lengths 2^0 .. 2^-15; slot SVM_NLS holds alpha = 0
#define SVM_XI 0.05          // CG ends at |r| <= SVM_XI |g|
#define SVM_SIGMA 0.01       // Armijo constant (liblinear's eta)

enum { IS_DONE = 0, IS_NEWTON, IS_CG, IS_ROWS };                 // istate int32 [IS_ROWS, K]
enum { DS_F = 0, DS_GNORM, DS_ROWS };                               // dstate float64 [DS_ROWS, K]

static inline size_t svm_up(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int svm_row_blocks(int N) { return (N + SVM_RB - 1) / SVM_RB; }
static inline int svm_splits(int N) { return (N + SVM_TROWS - 1) / SVM_TROWS; }

__device__ __forceinline__ double svm_wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < ACT_WAVE; o <<= 1) v += __shfl_xor(v, o, ACT_WAVE);
    return v;                                        // the same bits in every lane
}
// flags int32 [K]: true when every class is frozen (the same answer in every wave of the grid: nothing writes flags while this kernel runs)
__device__ __forceinline__ bool svm_all_frozen(const int* __restrict__ flags, int K) {
    const int lane = threadIdx.x & (ACT_WAVE - 1);
    const int v = lane < K ? flags[lane] : 1;
    return __all(v != 0);
}
// sum over the partial blocks of one class column, blocks in index order: lane l owns blocks l, l + 64, ...
__device__ __forceinline__ double svm_block_sum(const double* __restrict__ part, int nblk, int stride, int lane) {
    double s = 0.0;
    for (int bI = lane; bI < nblk; bI += ACT_WAVE) s += part[(size_t)bI * stride];
    return svm_wave_sum(s);
}
// element (c, d) of sum_split part[split][c][d], in float64, splits in index order
__device__ __forceinline__ double svm_split_sum(const float* __restrict__ part, int nsplit, int K, int D, int c, int d) {
    double s = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) s += (double)part[((size_t)sp * K + c) * D + d];
    return s;
}
__device__ __forceinline__ double svm_split_sum_b(const double* __restrict__ partb, int nsplit, int K, int c) {
    double s = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) s += partb[(size_t)sp * K + c];
    return s;
}

// four consecutive floats of row-major src [rows, D] at (r, k); zero outside.  VEC: D % 4 == 0 and a 16-byte aligned base, k % 4 == 0
template <bool VEC>
__device__ __forceinline__ float4 svm_load4(const float* __restrict__ src, int r, int rows, int k, int D) {
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

// out[N,K] = X[N,D] . W[K,D]^T + b (b may be NULL); mask (may be NULL, [N,K]): out = 0 where mask == 0
template <bool VEC>
__global__ __launch_bounds__(256) void svm_scores_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ b,
                                                         const float* __restrict__ mask, const int* __restrict__ frozen, int N, int D, int K,
                                                         float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float Xs[SVM_KC][SVM_LDT];      // [k][row]
    __shared__ __attribute__((aligned(16))) float Ws[SVM_KC][SVM_LDT];      // [k][class]
    if (frozen && svm_all_frozen(frozen, K)) return;
    const int tid = threadIdx.x, row0 = blockIdx.x * SVM_RB;
    const int cg = tid & 15, rg = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    const int kq = (tid & 7) * 4;
    for (int k0 = 0; k0 < D; k0 += SVM_KC) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = (tid >> 3) + 32 * h;
            const float4 xv = svm_load4<VEC>(X, row0 + r, N, k0 + kq, D);
            const float4 wv = svm_load4<VEC>(W, r, K, k0 + kq, D);
            Xs[kq][r] = xv.x; Xs[kq + 1][r] = xv.y; Xs[kq + 2][r] = xv.z; Xs[kq + 3][r] = xv.w;
            Ws[kq][r] = wv.x; Ws[kq + 1][r] = wv.y; Ws[kq + 2][r] = wv.z; Ws[kq + 3][r] = wv.w;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < SVM_KC; ++k) {
            const float4 xa = *reinterpret_cast<const float4*>(&Xs[k][rg * 4]);
            const float4 wb = *reinterpret_cast<const float4*>(&Ws[k][cg * 4]);
            const float xr[4] = {xa.x, xa.y, xa.z, xa.w}, wc[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(xr[i], wc[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gi = row0 + rg * 4 + i;
        if (gi >= N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = cg * 4 + j;
            if (c >= K) continue;
            float v = acc[i][j];
            if (b) v += b[c];
            if (mask && mask[(size_t)gi * K + c] == 0.f) v = 0.f;
            out[(size_t)gi * K + c] = v;
        }
    }
}

// R = y max(0, 1 - y m); part [row blocks][K] = the block's sum of h^2 (float64), rows in a fixed order
__global__ __launch_bounds__(256) void svm_hinge_kernel(const float* __restrict__ M, const int64_t* __restrict__ labels,
                                                        const int64_t* __restrict__ classes, int N, int K, float* __restrict__ R,
                                                        double* __restrict__ part) {
    __shared__ double red[4][ACT_WAVE];
    const int c = threadIdx.x & 63, ry = threadIdx.x >> 6;
    double acc = 0.0;
    if (c < K) {
        const int64_t cls = classes[c];
        for (int r = ry; r < SVM_RB; r += 4) {
            const int i = blockIdx.x * SVM_RB + r;
            if (i >= N) break;
            const float y = labels[i] == cls ? 1.f : -1.f;
            const float h = fmaxf(0.f, 1.f - y * M[(size_t)i * K + c]);         // y m is exact: one rounding whether or not this contracts
            R[(size_t)i * K + c] = y * h;
            acc += (double)h * (double)h;
        }
    }
    red[ry][c] = acc;
    __syncthreads();
    if (ry == 0 && c < K) part[(size_t)blockIdx.x * K + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

__global__ __launch_bounds__(ACT_WAVE) void svm_hinge_finish_kernel(const double* __restrict__ part, int nblk, int K, double* __restrict__ sums) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const double s = svm_block_sum(part + c, nblk, K, lane);
    if (lane == 0) sums[c] = s;
}

// part[split][K][D] = P[rows of the split, K]^T . X[rows, D] (fp32, rows in order); partb[split][K] = column sums of P over the rows (float64)
template <bool VEC>
__global__ __launch_bounds__(256) void svm_tprod_kernel(const float* __restrict__ P, const float* __restrict__ X, const int* __restrict__ frozen, int N,
                                                        int D, int K, float* __restrict__ part, double* __restrict__ partb) {
    __shared__ __attribute__((aligned(16))) float Ps[SVM_KC][SVM_LDT];      // [row][class]
    __shared__ __attribute__((aligned(16))) float Xs[SVM_KC][SVM_LDT];      // [row][d]
    if (frozen && svm_all_frozen(frozen, K)) return;
    const int tid = threadIdx.x, d0 = blockIdx.x * 64, split = blockIdx.y;
    const int rbeg = split * SVM_TROWS, rend = min(N, rbeg + SVM_TROWS);
    const int dg = tid & 15, cgp = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int n0 = rbeg; n0 < rend; n0 += SVM_KC) {
#pragma unroll
        for (int e = tid; e < SVM_KC * 64; e += 256) {
            const int n = e >> 6, c = e & 63, gi = n0 + n;
            Ps[n][c] = (gi < rend && c < K) ? P[(size_t)gi * K + c] : 0.f;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int n = (tid >> 4) + 16 * h, gi = n0 + n;
            *reinterpret_cast<float4*>(&Xs[n][dg * 4]) = svm_load4<VEC>(X, gi, rend, d0 + dg * 4, D);
        }
        __syncthreads();
#pragma unroll 8
        for (int n = 0; n < SVM_KC; ++n) {
            const float4 pa = *reinterpret_cast<const float4*>(&Ps[n][cgp * 4]);
            const float4 xb = *reinterpret_cast<const float4*>(&Xs[n][dg * 4]);
            const float pr[4] = {pa.x, pa.y, pa.z, pa.w}, xc[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(pr[i], xc[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = cgp * 4 + i;
        if (c >= K) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = d0 + dg * 4 + j;
            if (d < D) part[((size_t)split * K + c) * D + d] = acc[i][j];
        }
    }
    if (blockIdx.x == 0 && tid < K) {
        double s = 0.0;
        for (int gi = rbeg; gi < rend; ++gi) s += (double)P[(size_t)gi * K + tid];
        partb[(size_t)split * K + tid] = s;
    }
}

// out [K,D] / colsum [K] = the split partials summed in float64, rounded once
__global__ __launch_bounds__(ACT_WAVE) void svm_tprod_finish_kernel(const float* __restrict__ part, const double* __restrict__ partb, int nsplit, int D,
                                                                    int K, float* __restrict__ out, float* __restrict__ colsum) {
    const int c = blockIdx.x, lane = threadIdx.x;
    for (int d = lane; d < D; d += ACT_WAVE) out[(size_t)c * D + d] = (float)svm_split_sum(part, nsplit, K, D, c, d);
    if (colsum && lane == 0) colsum[c] = (float)svm_split_sum_b(partb, nsplit, K, c);
}

// device-resident vectors of the solver ([K,D] fp32 with the bias component in a [K] array beside it)
struct SvmVec {
    float *G, *gb, *S, *sb, *Rr, *rb, *Dd, *db, *Hd;
    double* rr;          // [K] CG residual norm squared
    int* cg_done;        // [K]
};

// gradient, objective, stopping test and CG start of one class per wave
__global__ __launch_bounds__(ACT_WAVE) void svm_grad_kernel(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ part,
                                                            const double* __restrict__ partb, const double* __restrict__ hpart, int nsplit, int nrb,
                                                            int D, int K, double C, double tol, SvmVec v, int* __restrict__ istate,
                                                            double* __restrict__ dstate) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (istate[IS_DONE * K + c] != 0) {
        if (lane == 0) v.cg_done[c] = 1;
        return;
    }
    const double loss = svm_block_sum(hpart + c, nrb, K, lane);
    double gg = 0.0, ww = 0.0;
    for (int d = lane; d < D; d += ACT_WAVE) {
        const size_t o = (size_t)c * D + d;
        const float w = W[o];
        const float g = (float)((double)w - 2.0 * C * svm_split_sum(part, nsplit, K, D, c, d));
        v.G[o] = g; v.S[o] = 0.f; v.Rr[o] = -g; v.Dd[o] = -g;
        gg += (double)g * (double)g;
        ww += (double)w * (double)w;
    }
    if (lane == 0) {
        const float bb = b[c];
        const float g = (float)((double)bb - 2.0 * C * svm_split_sum_b(partb, nsplit, K, c));
        v.gb[c] = g; v.sb[c] = 0.f; v.rb[c] = -g; v.db[c] = -g;
        gg += (double)g * (double)g;
        ww += (double)bb * (double)bb;
    }
    gg = svm_wave_sum(gg);
    ww = svm_wave_sum(ww);
    if (lane == 0) {
        const double gnorm = sqrt(gg);
        dstate[DS_F * K + c] = 0.5 * ww + C * loss;
        dstate[DS_GNORM * K + c] = gnorm;
        const int done = gnorm <= tol ? 1 : 0;
        istate[IS_DONE * K + c] = done;
        v.cg_done[c] = done != 0;
        v.rr[c] = gg;
    }
}

// one CG iteration of one class per wave: Hd = d + 2C X^T (A o (X d + d_b)) from the split partials, alpha, s, r, stop test, beta, d
__global__ __launch_bounds__(ACT_WAVE) void svm_cg_kernel(const float* __restrict__ part, const double* __restrict__ partb, int nsplit, int D, int K,
                                                          double C, SvmVec v, int* __restrict__ istate, const double* __restrict__ dstate) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (v.cg_done[c] != 0) return;
    double dHd = 0.0;
    for (int d = lane; d < D; d += ACT_WAVE) {
        const size_t o = (size_t)c * D + d;
        const float dd = v.Dd[o];
        const float hd = (float)((double)dd + 2.0 * C * svm_split_sum(part, nsplit, K, D, c, d));
        v.Hd[o] = hd;
        dHd += (double)dd * (double)hd;
    }
    float hdb = 0.f;
    if (lane == 0) {
        const float dd = v.db[c];
        hdb = (float)((double)dd + 2.0 * C * svm_split_sum_b(partb, nsplit, K, c));
        dHd += (double)dd * (double)hdb;
    }
    dHd = svm_wave_sum(dHd);
    const double rr = v.rr[c];
    if (!(dHd > 0.0)) {                                     // H >= I: only rounding of a vanishing direction gets here
        if (lane == 0) v.cg_done[c] = 1;
        return;
    }
    const float alpha = (float)(rr / dHd);
    double rn = 0.0;
    for (int d = lane; d < D; d += ACT_WAVE) {              // a lane re-reads only what it wrote itself
        const size_t o = (size_t)c * D + d;
        v.S[o] = fmaf(alpha, v.Dd[o], v.S[o]);
        const float r = fmaf(-alpha, v.Hd[o], v.Rr[o]);
        v.Rr[o] = r;
        rn += (double)r * (double)r;
    }
    float rbn = 0.f;
    if (lane == 0) {
        v.sb[c] = fmaf(alpha, v.db[c], v.sb[c]);
        rbn = fmaf(-alpha, hdb, v.rb[c]);
        v.rb[c] = rbn;
        rn += (double)rbn * (double)rbn;
    }
    rn = svm_wave_sum(rn);
    if (lane == 0) { v.rr[c] = rn; istate[IS_CG * K + c] += 1; }
    if (sqrt(rn) <= SVM_XI * dstate[DS_GNORM * K + c]) {
        if (lane == 0) v.cg_done[c] = 1;
        return;
    }
    const float beta = (float)(rn / rr);
    for (int d = lane; d < D; d += ACT_WAVE) {
        const size_t o = (size_t)c * D + d;
        v.Dd[o] = fmaf(beta, v.Dd[o], v.Rr[o]);
    }
    if (lane == 0) v.db[c] = fmaf(beta, v.db[c], rbn);
}

// lpart [row blocks][SVM_NLS + 1][K] = the block's sum of max(0, 1 - y (m + alpha z))^2 in float64 for alpha = 2^-t (t < SVM_NLS) and alpha = 0
__global__ __launch_bounds__(256) void svm_ls_eval_kernel(const float* __restrict__ M, const float* __restrict__ Z, const int64_t* __restrict__ labels,
                                                          const int64_t* __restrict__ classes, const int* __restrict__ done, int N, int K,
                                                          double* __restrict__ lpart) {
    __shared__ double red[SVM_NLS + 1][4][ACT_WAVE];
    if (svm_all_frozen(done, K)) return;
    const int c = threadIdx.x & 63, ry = threadIdx.x >> 6;
    double acc[SVM_NLS + 1];
#pragma unroll
    for (int t = 0; t <= SVM_NLS; ++t) acc[t] = 0.0;
    if (c < K && done[c] == 0) {
        const int64_t cls = classes[c];
        for (int r = ry; r < SVM_RB; r += 4) {
            const int i = blockIdx.x * SVM_RB + r;
            if (i >= N) break;
            const double y = labels[i] == cls ? 1.0 : -1.0;
            const double u = 1.0 - y * (double)M[(size_t)i * K + c], w = y * (double)Z[(size_t)i * K + c];
            double alpha = 1.0;
#pragma unroll
            for (int t = 0; t < SVM_NLS; ++t) {
                const double a = fmax(0.0, u - alpha * w);
                acc[t] += a * a;
                alpha *= 0.5;
            }
            const double a0 = fmax(0.0, u);
            acc[SVM_NLS] += a0 * a0;
        }
    }
#pragma unroll
    for (int t = 0; t <= SVM_NLS; ++t) red[t][ry][c] = acc[t];
    __syncthreads();
    for (int e = threadIdx.x; e < (SVM_NLS + 1) * ACT_WAVE; e += 256) {
        const int t = e >> 6, cc = e & 63;
        if (cc < K) lpart[((size_t)blockIdx.x * (SVM_NLS + 1) + t) * K + cc] = ((red[t][0][cc] + red[t][1][cc]) + red[t][2][cc]) + red[t][3][cc];
    }
}

// one wave per class: the largest alpha = 2^-t with f(alpha) - f(0) <= sigma alpha g.s, then W += alpha S.  No candidate passes, or the accepted
// decrease is below fp32 epsilon times the objective -- the scores are fp32, so the objective recomputed at the new point is known no better than
// that, and the gradient of the fp32 products sits on its noise floor there: the class ends ("no progress")
__global__ __launch_bounds__(ACT_WAVE) void svm_ls_pick_kernel(const double* __restrict__ lpart, int nrb, int N, int D, int K, double C, SvmVec v,
                                                               float* __restrict__ W, float* __restrict__ b, int* __restrict__ istate,
                                                               double* __restrict__ dstate) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (istate[IS_DONE * K + c] != 0) return;
    double gs = 0.0, ws = 0.0, ss = 0.0;
    for (int d = lane; d < D; d += ACT_WAVE) {
        const size_t o = (size_t)c * D + d;
        const double s = (double)v.S[o];
        gs += (double)v.G[o] * s;
        ws += (double)W[o] * s;
        ss += s * s;
    }
    if (lane == 0) {
        const double s = (double)v.sb[c];
        gs += (double)v.gb[c] * s;
        ws += (double)b[c] * s;
        ss += s * s;
    }
    gs = svm_wave_sum(gs);
    ws = svm_wave_sum(ws);
    ss = svm_wave_sum(ss);
    const double L0 = svm_block_sum(lpart + (size_t)SVM_NLS * K + c, nrb, (SVM_NLS + 1) * K, lane);
    double alpha = 1.0, delta = 0.0;
    bool ok = false;
    if (gs < 0.0) {
        for (int t = 0; t < SVM_NLS; ++t) {                  // wave-uniform: every lane holds the same sums
            const double Lt = svm_block_sum(lpart + (size_t)t * K + c, nrb, (SVM_NLS + 1) * K, lane);
            delta = alpha * ws + 0.5 * alpha * alpha * ss + C * (Lt - L0);
            if (delta <= SVM_SIGMA * alpha * gs) { ok = true; break; }
            alpha *= 0.5;
        }
    }
    if (!ok) {
        if (lane == 0) istate[IS_DONE * K + c] = 2;
        return;
    }
    const float af = (float)alpha;                            // a power of two: exact
    for (int d = lane; d < D; d += ACT_WAVE) {
        const size_t o = (size_t)c * D + d;
        W[o] = fmaf(af, v.S[o], W[o]);
    }
    if (lane == 0) {
        b[c] = fmaf(af, v.sb[c], b[c]);
        istate[IS_NEWTON * K + c] += 1;
        if (-delta <= 0x1p-24 * fabs(dstate[DS_F * K + c])) istate[IS_DONE * K + c] = 2;
    }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------------
static inline bool svm_vec_ok(const void* p, int D) { return (D % 4) == 0 && (((uintptr_t)p) & 15) == 0; }

static int svm_launch_scores(const float* X, const float* W, const float* b, const float* mask, const int* frozen, int N, int D, int K, float* out,
                             hipStream_t s) {
    const dim3 grid(svm_row_blocks(N)), block(256);
    if (svm_vec_ok(X, D) && svm_vec_ok(W, D))
        hipLaunchKernelGGL(svm_scores_kernel<true>, grid, block, 0, s, X, W, b, mask, frozen, N, D, K, out);
    else
        hipLaunchKernelGGL(svm_scores_kernel<false>, grid, block, 0, s, X, W, b, mask, frozen, N, D, K, out);
    ACT_LAUNCH_CHECK();
    return 0;
}

static int svm_launch_tprod(const float* P, const float* X, const int* frozen, int N, int D, int K, float* part, double* partb, hipStream_t s) {
    const dim3 grid((D + 63) / 64, svm_splits(N)), block(256);
    if (svm_vec_ok(X, D))
        hipLaunchKernelGGL(svm_tprod_kernel<true>, grid, block, 0, s, P, X, frozen, N, D, K, part, partb);
    else
        hipLaunchKernelGGL(svm_tprod_kernel<false>, grid, block, 0, s, P, X, frozen, N, D, K, part, partb);
    ACT_LAUNCH_CHECK();
    return 0;
}

static inline bool svm_dims_ok(int N, int D, int K) {
    return N > 0 && D > 0 && K > 0 && K <= SVM_MAXK && (long long)N * (D > K ? D : K) < (1LL << 31) && N <= (1 << 24) && D <= (1 << 16);
}

extern "C" int act_svm_scores_f32(const float* X, const float* W, const float* b, const float* mask, int N, int D, int K, float* out,
                                  act_stream_t stream) {
    if (!X || !W || !out) return ACT_E_NULLPTR;
    if (!svm_dims_ok(N, D, K)) return ACT_E_BADARG;
    return svm_launch_scores(X, W, b, mask, nullptr, N, D, K, out, (hipStream_t)stream);
}

extern "C" size_t act_svm_hinge_workspace(int N, int K) { return svm_up(sizeof(double) * (size_t)svm_row_blocks(N > 0 ? N : 1) * (size_t)(K > 0 ? K : 1)); }

extern "C" int act_svm_hinge_f32(const float* M, const int64_t* labels, const int64_t* classes, int N, int K, float* R, double* sums, void* workspace,
                                 size_t workspace_bytes, act_stream_t stream) {
    if (!M || !labels || !classes || !R || !sums || !workspace) return ACT_E_NULLPTR;
    if (!svm_dims_ok(N, 1, K) || workspace_bytes < act_svm_hinge_workspace(N, K) || (((uintptr_t)workspace) & 7) != 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(svm_hinge_kernel, dim3(svm_row_blocks(N)), dim3(256), 0, s, M, labels, classes, N, K, R, part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(svm_hinge_finish_kernel, dim3(K), dim3(ACT_WAVE), 0, s, (const double*)part, svm_row_blocks(N), K, sums);
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t act_svm_tprod_workspace(int N, int D, int K) {
    if (N <= 0 || D <= 0 || K <= 0) return 0;
    const size_t ns = (size_t)svm_splits(N);
    return svm_up(sizeof(float) * ns * K * D) + svm_up(sizeof(double) * ns * K);
}

extern "C" int act_svm_tprod_f32(const float* P, const float* X, int N, int D, int K, float* out, float* colsum, void* workspace, size_t workspace_bytes,
                                 act_stream_t stream) {
    if (!P || !X || !out || !workspace) return ACT_E_NULLPTR;
    if (!svm_dims_ok(N, D, K) || workspace_bytes < act_svm_tprod_workspace(N, D, K) || (((uintptr_t)workspace) & 15) != 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int ns = svm_splits(N);
    float* part = (float*)workspace;
    double* partb = (double*)((char*)workspace + svm_up(sizeof(float) * (size_t)ns * K * D));
    const int rc = svm_launch_tprod(P, X, nullptr, N, D, K, part, partb, s);
    if (rc) return rc;
    hipLaunchKernelGGL(svm_tprod_finish_kernel, dim3(K), dim3(ACT_WAVE), 0, s, (const float*)part, (const double*)partb, ns, D, K, out, colsum);
    ACT_LAUNCH_CHECK();
    return 0;
}

// workspace of one Newton iteration, carved in this order (every piece 256-byte aligned)
struct SvmCarve {
    float *M, *R, *Z, *part;
    double *partb, *hpart, *lpart;
    SvmVec v;
    size_t bytes;
};
static SvmCarve svm_carve(void* base, int N, int D, int K) {
    SvmCarve w;
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t n) { void* q = p + off; off += svm_up(n); return q; };
    const size_t nk = (size_t)N * K, kd = (size_t)K * D, ns = (size_t)svm_splits(N), nrb = (size_t)svm_row_blocks(N);
    w.M = (float*)take(4 * nk); w.R = (float*)take(4 * nk); w.Z = (float*)take(4 * nk);
    w.part = (float*)take(4 * ns * kd);
    w.partb = (double*)take(8 * ns * K);
    w.hpart = (double*)take(8 * nrb * K);
    w.lpart = (double*)take(8 * nrb * (SVM_NLS + 1) * K);
    w.v.G = (float*)take(4 * kd); w.v.S = (float*)take(4 * kd); w.v.Rr = (float*)take(4 * kd); w.v.Dd = (float*)take(4 * kd); w.v.Hd = (float*)take(4 * kd);
    w.v.gb = (float*)take(4 * K); w.v.sb = (float*)take(4 * K); w.v.rb = (float*)take(4 * K); w.v.db = (float*)take(4 * K);
    w.v.rr = (double*)take(8 * K);
    w.v.cg_done = (int*)take(4 * K);
    w.bytes = off;
    return w;
}

extern "C" size_t act_svm_newton_workspace(int N, int D, int K) {
    if (N <= 0 || D <= 0 || K <= 0) return 0;
    return svm_carve(nullptr, N, D, K).bytes;
}

extern "C" int act_svm_newton_f32(const float* X, const int64_t* labels, const int64_t* classes, int N, int D, int K, float C, float tol, int max_cg,
                                  float* W, float* b, int32_t* istate, double* dstate, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!X || !labels || !classes || !W || !b || !istate || !dstate || !workspace) return ACT_E_NULLPTR;
    if (!svm_dims_ok(N, D, K) || !(C > 0.f) || !(tol >= 0.f) || max_cg < 1 || max_cg > 4096) return ACT_E_BADARG;
    if (workspace_bytes < act_svm_newton_workspace(N, D, K) || (((uintptr_t)workspace) & 15) != 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const SvmCarve w = svm_carve(workspace, N, D, K);
    const int ns = svm_splits(N), nrb = svm_row_blocks(N);
    int* done = istate + IS_DONE * K;
    int rc;
    if ((rc = svm_launch_scores(X, W, b, nullptr, nullptr, N, D, K, w.M, s))) return rc;
    hipLaunchKernelGGL(svm_hinge_kernel, dim3(nrb), dim3(256), 0, s, (const float*)w.M, labels, classes, N, K, w.R, w.hpart);
    ACT_LAUNCH_CHECK();
    if ((rc = svm_launch_tprod(w.R, X, nullptr, N, D, K, w.part, w.partb, s))) return rc;
    hipLaunchKernelGGL(svm_grad_kernel, dim3(K), dim3(ACT_WAVE), 0, s, (const float*)W, (const float*)b, (const float*)w.part, (const double*)w.partb,
                       (const double*)w.hpart, ns, nrb, D, K, (double)C, (double)tol, w.v, istate, dstate);
    ACT_LAUNCH_CHECK();
    for (int it = 0; it < max_cg; ++it) {                    // launches of an iteration in which every class is frozen return at once
        if ((rc = svm_launch_scores(X, w.v.Dd, w.v.db, w.R, w.v.cg_done, N, D, K, w.Z, s))) return rc;
        if ((rc = svm_launch_tprod(w.Z, X, w.v.cg_done, N, D, K, w.part, w.partb, s))) return rc;
        hipLaunchKernelGGL(svm_cg_kernel, dim3(K), dim3(ACT_WAVE), 0, s, (const float*)w.part, (const double*)w.partb, ns, D, K, (double)C, w.v, istate,
                           (const double*)dstate);
        ACT_LAUNCH_CHECK();
    }
    if ((rc = svm_launch_scores(X, w.v.S, w.v.sb, nullptr, done, N, D, K, w.Z, s))) return rc;
    hipLaunchKernelGGL(svm_ls_eval_kernel, dim3(nrb), dim3(256), 0, s, (const float*)w.M, (const float*)w.Z, labels, classes, (const int*)done, N, K,
                       w.lpart);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(svm_ls_pick_kernel, dim3(K), dim3(ACT_WAVE), 0, s, (const double*)w.lpart, nrb, N, D, K, (double)C, w.v, W, b, istate, dstate);
    ACT_LAUNCH_CHECK();
    return 0;
}
