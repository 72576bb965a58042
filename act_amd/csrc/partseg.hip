// partseg.hip -- ShapeNetPart part segmentation (part_segmentation/models/pt.py, main.py:235-299): the 16-way category label branch
// (Conv1d(16, 64, bias=False) + BatchNorm1d(64) over the B clouds + LeakyReLU(0.2)) forward / backward, and the category-masked evaluation
// (arg-max over the shape's part range, per-shape part intersection / union counts, per-part seen / correct counts).
//
// Conventions: every float reduction runs in a fixed order (one lane per channel walks the B rows in increasing order), so results are
// bit-identical run to run; the only atomics are integer ones (LDS histograms, the int64 seen / correct counters), which are exact.
#include "common.h"

#define PS_LABELS 16          // categories (one-hot width)
#define PS_FEAT 64            // label-branch output channels
#define PS_MAX_LOCAL 6        // parts of the largest category (Motorbike)
#define PS_MAX_PARTS 64
#define PS_COUNT_STRIDE 16    // per-shape int32 record: [0,6) intersections, [6,12) unions, [12] category, [13] parts in the category

// ---- label branch --------------------------------------------------------------------------------------------------------------
// one lane per output channel c: z[b] = sum_k cl[b,k] * W[c,k] (k ascending), then BatchNorm over the B rows and LeakyReLU(slope).
// train: biased batch variance for the normalisation, running stats updated with momentum and the unbiased variance (count B), as
// nn.BatchNorm1d does; eval: running statistics.  The branch moves about 10 KB and is launch-bound, so every lane computes in float64
// and rounds once per output: the results are within half an fp32 ulp of the float64 function of the fp32 inputs.  The backward
// recomputes the batch statistics the same way (nothing is saved between the two launches).
__device__ __forceinline__ void ps_load_w(const float* __restrict__ W, int c, double* w) {
#pragma unroll
    for (int k = 0; k < PS_LABELS; ++k) w[k] = (double)W[c * PS_LABELS + k];
}
__device__ __forceinline__ double ps_dot16(const float* __restrict__ a, const double* w) {
    double z = 0.0;
#pragma unroll
    for (int k = 0; k < PS_LABELS; ++k) z = fma((double)a[k], w[k], z);
    return z;
}
// batch mean and centred sum of squares of z over the B rows (b ascending)
__device__ __forceinline__ void ps_batch_stats(const float* __restrict__ cl, const double* w, int B, double& mean, double& q) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += ps_dot16(cl + (size_t)b * PS_LABELS, w);
    mean = s / (double)B;
    q = 0.0;
    for (int b = 0; b < B; ++b) {
        const double d = ps_dot16(cl + (size_t)b * PS_LABELS, w) - mean;
        q = fma(d, d, q);
    }
}

__global__ __launch_bounds__(PS_FEAT) void label_branch_fwd_kernel(const float* __restrict__ cl, const float* __restrict__ W, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, int B, int training, float eps, float momentum,
                                                                  float slope, float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                  float* __restrict__ y) {
    const int c = threadIdx.x;
    double w[PS_LABELS];
    ps_load_w(W, c, w);
    double mean, rstd;
    if (training) {
        double q;
        ps_batch_stats(cl, w, B, mean, q);
        rstd = 1.0 / sqrt(q / (double)B + (double)eps);
        const double m = (double)momentum;
        running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
        running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (q / (double)(B - 1)));
    } else {
        mean = (double)running_mean[c];
        rstd = 1.0 / sqrt((double)running_var[c] + (double)eps);
    }
    const double g = (double)gamma[c], bt = (double)beta[c];
    for (int b = 0; b < B; ++b) {
        const double u = fma(g, (ps_dot16(cl + (size_t)b * PS_LABELS, w) - mean) * rstd, bt);
        y[(size_t)b * PS_FEAT + c] = (float)(u > 0.0 ? u : u * (double)slope);
    }
}

// backward of the train-mode branch, one lane per channel: du = dy * lrelu'(u); dbeta = sum_b du; dgamma = sum_b du * xh;
// dz = gamma * rstd * (du - dbeta / B - xh * dgamma / B); dW[c, :] = sum_b dz[b] * cl[b, :] (b ascending, 16 accumulators per lane)
__global__ __launch_bounds__(PS_FEAT) void label_branch_bwd_kernel(const float* __restrict__ cl, const float* __restrict__ W, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const float* __restrict__ dy, int B, float eps,
                                                                  float slope, float* __restrict__ dW, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = threadIdx.x;
    double w[PS_LABELS];
    ps_load_w(W, c, w);
    double mean, q;
    ps_batch_stats(cl, w, B, mean, q);
    const double rstd = 1.0 / sqrt(q / (double)B + (double)eps), g = (double)gamma[c], bt = (double)beta[c], sl = (double)slope;
    double sb = 0.0, sg = 0.0;
    for (int b = 0; b < B; ++b) {
        const double xh = (ps_dot16(cl + (size_t)b * PS_LABELS, w) - mean) * rstd;
        const double d = (double)dy[(size_t)b * PS_FEAT + c];
        const double du = fma(g, xh, bt) > 0.0 ? d : d * sl;
        sb += du;
        sg = fma(du, xh, sg);
    }
    const double invB = 1.0 / (double)B, k0 = g * rstd;
    double acc[PS_LABELS];
#pragma unroll
    for (int k = 0; k < PS_LABELS; ++k) acc[k] = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* a = cl + (size_t)b * PS_LABELS;
        const double xh = (ps_dot16(a, w) - mean) * rstd;
        const double d = (double)dy[(size_t)b * PS_FEAT + c];
        const double du = fma(g, xh, bt) > 0.0 ? d : d * sl;
        const double dz = k0 * (du - sb * invB - xh * sg * invB);
#pragma unroll
        for (int k = 0; k < PS_LABELS; ++k) acc[k] = fma(dz, (double)a[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < PS_LABELS; ++k) dW[c * PS_LABELS + k] = (float)acc[k];
    dgamma[c] = (float)sg;
    dbeta[c] = (float)sb;
}

extern "C" int act_label_branch_fwd_f32(const float* cls, const float* W, const float* gamma, const float* beta, int B, int training, float eps,
                                        float momentum, float slope, float* running_mean, float* running_var, float* y, act_stream_t stream) {
    if (!cls || !W || !gamma || !beta || !running_mean || !running_var || !y) return ACT_E_NULLPTR;
    if (B <= 0 || (training && B < 2)) return ACT_E_BADARG;          // nn.BatchNorm1d: more than one value per channel when training
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 2.0 * 3 * B * PS_LABELS * PS_FEAT, 4.0 * (B * PS_LABELS + PS_FEAT * PS_LABELS + B * PS_FEAT + 6 * PS_FEAT));
    hipLaunchKernelGGL(label_branch_fwd_kernel, dim3(1), dim3(PS_FEAT), 0, s, cls, W, gamma, beta, B, training, eps, momentum, slope, running_mean,
                       running_var, y);
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_label_branch_bwd_f32(const float* cls, const float* W, const float* gamma, const float* beta, const float* dy, int B, float eps,
                                        float slope, float* dW, float* dgamma, float* dbeta, act_stream_t stream) {
    if (!cls || !W || !gamma || !beta || !dy || !dW || !dgamma || !dbeta) return ACT_E_NULLPTR;
    if (B < 2) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 2.0 * 5 * B * PS_LABELS * PS_FEAT, 4.0 * (B * PS_LABELS + 2 * PS_FEAT * PS_LABELS + B * PS_FEAT + 4 * PS_FEAT));
    hipLaunchKernelGGL(label_branch_bwd_kernel, dim3(1), dim3(PS_FEAT), 0, s, cls, W, gamma, beta, dy, B, eps, slope, dW, dgamma, dbeta);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- category-masked part evaluation -----------------------------------------------------------------------------------------
// one workgroup per shape.  The shape's category is part2cat[target[first point]]; its parts are [cat_first[cat], cat_first[cat + 1]).
// The log-prob rows are staged through LDS in chunks of `rows` rows (256 at P = 50; fewer for wider rows, so that a tile stays within
// PS_EVAL_TILE floats = 50 KiB) with 16-byte loads (VEC: every chunk start is 16-byte aligned,
// i.e. N * P % 4 == 0 and logp 16-byte aligned), then one lane per row takes the arg-max over the part range (strict '>': ties to the first
// index, as np.argmax).  Per-shape intersections / unions and the per-part seen / correct counts are LDS histograms; the shape's record is
// written once, seen / correct are added to the int64 totals with integer atomics.
#define PS_EVAL_ROWS 256      // at most one row per lane
#define PS_EVAL_TILE 12800    // LDS floats of the staging tile
#define PS_EVAL_THREADS 256

template <bool VEC>
__global__ __launch_bounds__(PS_EVAL_THREADS) void part_eval_kernel(const float* __restrict__ logp, const int64_t* __restrict__ target, int N, int P,
                                                                    const int32_t* __restrict__ part2cat, const int32_t* __restrict__ cat_first, int ncat,
                                                                    int32_t* __restrict__ pred, int32_t* __restrict__ counts, int shape_offset, int rows,
                                                                    unsigned long long* __restrict__ seen, unsigned long long* __restrict__ correct) {
    extern __shared__ float tile[];                                   // rows * P floats
    __shared__ int h_inter[PS_MAX_LOCAL], h_union[PS_MAX_LOCAL], h_seen[PS_MAX_PARTS], h_corr[PS_MAX_PARTS];
    __shared__ int s_lo, s_len, s_cat;
    const int i = blockIdx.x, t = threadIdx.x;
    const size_t row0 = (size_t)i * N;
    if (t < PS_MAX_LOCAL) { h_inter[t] = 0; h_union[t] = 0; }
    if (t < PS_MAX_PARTS) { h_seen[t] = 0; h_corr[t] = 0; }
    if (t == 0) {
        const long long t0 = target[row0];
        int cat = -1, lo = 0, len = 0;
        if (t0 >= 0 && t0 < P) {
            const int c = part2cat[t0];
            if (c >= 0 && c < ncat) {
                const int l0 = cat_first[c], n0 = cat_first[c + 1] - l0;
                if (l0 >= 0 && n0 >= 1 && n0 <= PS_MAX_LOCAL && l0 + n0 <= P) { cat = c; lo = l0; len = n0; }
            }
        }
        s_lo = lo; s_len = len; s_cat = cat;
    }
    __syncthreads();
    const int lo = s_lo, len = s_len;
    for (int r0 = 0; r0 < N; r0 += rows) {
        const int m = min(rows, N - r0);
        const float* src = logp + (row0 + r0) * (size_t)P;
        __syncthreads();                                              // every lane is done with the previous chunk
        if (VEC) {
            const int nf4 = (m * P) >> 2, rem = (m * P) & 3;
            const float4* s4 = reinterpret_cast<const float4*>(src);
            float4* d4 = reinterpret_cast<float4*>(tile);
            for (int j = t; j < nf4; j += PS_EVAL_THREADS) d4[j] = s4[j];
            if (t < rem) tile[nf4 * 4 + t] = src[nf4 * 4 + t];
        } else {
            for (int j = t; j < m * P; j += PS_EVAL_THREADS) tile[j] = src[j];
        }
        __syncthreads();
        if (t < m) {
            const size_t r = row0 + r0 + t;
            const long long tg = target[r];
            int pr = -1;
            if (len > 0) {
                const float* row = tile + t * P + lo;
                float bv = row[0];
                int bj = 0;
                for (int j = 1; j < len; ++j)
                    if (row[j] > bv) { bv = row[j]; bj = j; }
                pr = lo + bj;
                const int lt = (tg >= lo && tg < lo + len) ? (int)(tg - lo) : -1;
                if (lt == bj) atomicAdd(&h_inter[bj], 1);
                atomicAdd(&h_union[bj], 1);
                if (lt >= 0 && lt != bj) atomicAdd(&h_union[lt], 1);
            }
            if (tg >= 0 && tg < P) {
                atomicAdd(&h_seen[tg], 1);
                if (pr == (int)tg) atomicAdd(&h_corr[tg], 1);
            }
            if (pred) pred[r] = pr;
        }
    }
    __syncthreads();
    int32_t* rec = counts + (size_t)(shape_offset + i) * PS_COUNT_STRIDE;
    if (t < PS_MAX_LOCAL) rec[t] = h_inter[t];
    else if (t < 2 * PS_MAX_LOCAL) rec[t] = h_union[t - PS_MAX_LOCAL];
    else if (t == 12) rec[t] = s_cat;
    else if (t == 13) rec[t] = len;
    else if (t < PS_COUNT_STRIDE) rec[t] = 0;
    if (t < P) {
        if (h_seen[t]) atomicAdd(&seen[t], (unsigned long long)h_seen[t]);
        if (h_corr[t]) atomicAdd(&correct[t], (unsigned long long)h_corr[t]);
    }
}

extern "C" int act_part_eval_f32(const float* logp, const int64_t* target, int B, int N, int P, const int32_t* part2cat, const int32_t* cat_first,
                                 int ncat, int32_t* pred, int32_t* counts, int shape_offset, int num_shapes, int64_t* seen, int64_t* correct,
                                 act_stream_t stream) {
    if (!logp || !target || !part2cat || !cat_first || !counts || !seen || !correct) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || P <= 0 || P > PS_MAX_PARTS || ncat <= 0) return ACT_E_BADARG;
    if (shape_offset < 0 || (long long)shape_offset + B > (long long)num_shapes) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int rows = min(PS_EVAL_ROWS, (PS_EVAL_TILE / P) & ~3);          // a multiple of 4: every chunk start keeps the 16-byte alignment
    const size_t lds = (size_t)rows * P * sizeof(float);
    const bool vec = ((long long)N * P) % 4 == 0 && ((uintptr_t)logp & 15) == 0;
    ActProfScope ps(KID_ELTWISE, s, (double)B * N * PS_MAX_LOCAL, 4.0 * B * (double)N * P + 8.0 * B * N + (pred ? 4.0 * B * N : 0.0));
    if (vec)
        hipLaunchKernelGGL(part_eval_kernel<true>, dim3(B), dim3(PS_EVAL_THREADS), lds, s, logp, target, N, P, part2cat, cat_first, ncat, pred, counts,
                           shape_offset, rows, reinterpret_cast<unsigned long long*>(seen), reinterpret_cast<unsigned long long*>(correct));
    else
        hipLaunchKernelGGL(part_eval_kernel<false>, dim3(B), dim3(PS_EVAL_THREADS), lds, s, logp, target, N, P, part2cat, cat_first, ncat, pred, counts,
                           shape_offset, rows, reinterpret_cast<unsigned long long*>(seen), reinterpret_cast<unsigned long long*>(correct));
    ACT_LAUNCH_CHECK(); return 0;
}
