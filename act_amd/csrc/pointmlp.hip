// pointmlp.hip -- the two row kernels PointMLP (Ma et al., ICLR 2022) needs beyond the library's: the geometric affine module of LocalGrouper
// (normalize="anchor") and the residual block tail ReLU(BN(y) + x).  Built with -ffp-contract=off: every product and sum below is rounded once.
#include "edge_bn.h"

// A 256-thread block is TX lanes along a row (a power of two, at most 64) by TY = 256 / TX rows in flight; a lane is one float4 of a row when
// D % 4 == 0 and the operands are 16-byte aligned, one float otherwise (use_xyz gives D = 67, 131, ...).
template <typename V> struct Vn { static constexpr int n = 1; };
template <> struct Vn<float4> { static constexpr int n = 4; };
template <typename V> __device__ __forceinline__ float* fl(V& v) { return reinterpret_cast<float*>(&v); }
template <typename V> __device__ __forceinline__ const float* fl(const V& v) { return reinterpret_cast<const float*>(&v); }

template <typename V> __device__ __forceinline__ V vsub(const V& a, const V& b) {
    V o;
#pragma unroll
    for (int u = 0; u < Vn<V>::n; ++u) fl(o)[u] = __fsub_rn(fl(a)[u], fl(b)[u]);
    return o;
}
template <typename V> __device__ __forceinline__ V vadd(const V& a, const V& b) {
    V o;
#pragma unroll
    for (int u = 0; u < Vn<V>::n; ++u) fl(o)[u] = __fadd_rn(fl(a)[u], fl(b)[u]);
    return o;
}
template <typename V> __device__ __forceinline__ V vzero() {
    V o;
#pragma unroll
    for (int u = 0; u < Vn<V>::n; ++u) fl(o)[u] = 0.f;
    return o;
}

static int lane_log(int W) {
    int l = 0;
    while ((1 << l) < W && l < 6) ++l;
    return l;
}
static bool vec4(int D, const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
    return !(D & 3) && !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15);
}

// ============================================================================================ geometric affine grouping: forward
// e[(b,i,j), c] = feat[b, idx[b,i,j], c] - feat[b, fps[b,i], c]; per cloud the float64 moments of e - pivot around the pivot e[(b,0,0), 0] (a value of
// e, so a common offset of the features never reaches the sums), block partials in a fixed order, then sigma = sqrt(M2 / (n - 1)).  The split of a
// cloud's rows over blocks depends on (S, k, D) alone, so a cloud's sigma does not depend on B.  Indices are clamped into [0, N): the entry point
// range-checks them first when asked to.
#define GA_MAX_BLOCKS 1024
#define GA_BLOCK_LANES 4096

struct GaShape { int tx_log, rpb, nblk; };
static GaShape ga_shape(long long E, int W) {
    GaShape g;
    g.tx_log = lane_log(W);
    const int ty = 256 >> g.tx_log;
    long long rpb = (GA_BLOCK_LANES + W - 1) / W;
    if ((E + rpb - 1) / rpb > GA_MAX_BLOCKS) rpb = (E + GA_MAX_BLOCKS - 1) / GA_MAX_BLOCKS;
    rpb = (rpb + ty - 1) / ty * ty;
    g.rpb = (int)rpb;
    g.nblk = (int)((E + rpb - 1) / rpb);
    return g;
}

__device__ __forceinline__ float ga_pivot(const float* __restrict__ feat, const int32_t* __restrict__ fps, const int32_t* __restrict__ idx, int b, int N,
                                          int S, long long E, int D) {
    const float* fb = feat + (size_t)b * N * D;
    return __fsub_rn(fb[(size_t)clampi(idx[(size_t)b * E], N) * D], fb[(size_t)clampi(fps[(size_t)b * S], N) * D]);
}

// tree sum of the 256 values of sh (fixed shape, so a fixed order); the result is in sh[0]
__device__ __forceinline__ void block_tree(double* sh, int t) {
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) sh[t] += sh[t + s];
    }
    __syncthreads();
}

template <typename V>
__global__ __launch_bounds__(256) void ga_moments_kernel(const V* __restrict__ feat, const int32_t* __restrict__ fps, const int32_t* __restrict__ idx, int N,
                                                         int S, int k, int W, int D, int rpb, int tx_log, double* __restrict__ part) {
    __shared__ double sh[2][256];
    const int b = blockIdx.y, t = threadIdx.x, TX = 1 << tx_log, TY = 256 >> tx_log, tx = t & (TX - 1), ty = t >> tx_log;
    const long long E = (long long)S * k;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(E, r0 + rpb);
    const double piv = (double)ga_pivot(reinterpret_cast<const float*>(feat), fps, idx, b, N, S, E, D);
    const V* fb = feat + (size_t)b * N * W;
    double s1 = 0.0, s2 = 0.0;
    for (long long r = r0 + ty; r < r1; r += TY) {
        const int nb = clampi(idx[(size_t)b * E + r], N), an = clampi(fps[(size_t)b * S + r / k], N);
        for (int c = tx; c < W; c += TX) {
            const V e = vsub(fb[(size_t)nb * W + c], fb[(size_t)an * W + c]);
#pragma unroll
            for (int u = 0; u < Vn<V>::n; ++u) { const double d = (double)fl(e)[u] - piv; s1 += d; s2 += d * d; }
        }
    }
    sh[0][t] = s1; sh[1][t] = s2;
    block_tree(sh[0], t);
    block_tree(sh[1], t);
    if (t == 0) {
        part[((size_t)b * gridDim.x + blockIdx.x) * 2 + 0] = sh[0][0];
        part[((size_t)b * gridDim.x + blockIdx.x) * 2 + 1] = sh[1][0];
    }
}

__global__ __launch_bounds__(256) void ga_sigma_kernel(const float* __restrict__ feat, const int32_t* __restrict__ fps, const int32_t* __restrict__ idx, int N,
                                                       int S, int k, int D, const double* __restrict__ part, int nblk, float* __restrict__ sigma,
                                                       float* __restrict__ mean) {
    __shared__ double sh[2][256];
    const int b = blockIdx.x, t = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int p = t; p < nblk; p += 256) { s1 += part[((size_t)b * nblk + p) * 2 + 0]; s2 += part[((size_t)b * nblk + p) * 2 + 1]; }
    sh[0][t] = s1; sh[1][t] = s2;
    block_tree(sh[0], t);
    block_tree(sh[1], t);
    if (t == 0) {
        const long long E = (long long)S * k;
        const double n = (double)E * D, dm = sh[0][0] / n;
        double m2 = sh[1][0] - sh[0][0] * dm;
        if (m2 < 0.0) m2 = 0.0;
        sigma[b] = (float)sqrt(m2 / (n - 1.0));
        mean[b] = (float)((double)ga_pivot(feat, fps, idx, b, N, S, E, D) + dm);
    }
}

// out[(b,i,j), c] = alpha[c] * (e * r) + beta[c], r = 1 / (sigma_b + eps); with cat the anchor's row goes to the columns [D, 2D)
template <typename V>
__global__ __launch_bounds__(256) void ga_apply_kernel(const V* __restrict__ feat, const int32_t* __restrict__ fps, const int32_t* __restrict__ idx,
                                                       const V* __restrict__ alpha, const V* __restrict__ beta, const float* __restrict__ sigma, float eps,
                                                       int N, int S, int k, int W, long long R, int tx_log, int cat, V* __restrict__ out) {
    const int t = threadIdx.x, TX = 1 << tx_log, TY = 256 >> tx_log, tx = t & (TX - 1), ty = t >> tx_log;
    const long long r = (long long)blockIdx.x * TY + ty;
    if (r >= R) return;
    const long long bs = r / k, b = bs / S;
    const float rr = __fdiv_rn(1.0f, __fadd_rn(sigma[b], eps));
    const V* fb = feat + (size_t)b * N * W;
    const int nb = clampi(idx[r], N), an = clampi(fps[bs], N);
    const int ldo = cat ? 2 * W : W;
    for (int c = tx; c < W; c += TX) {
        const V a = fb[(size_t)an * W + c], e = vsub(fb[(size_t)nb * W + c], a), al = alpha[c], be = beta[c];
        V o;
#pragma unroll
        for (int u = 0; u < Vn<V>::n; ++u) fl(o)[u] = __fadd_rn(__fmul_rn(fl(al)[u], __fmul_rn(fl(e)[u], rr)), fl(be)[u]);
        out[(size_t)r * ldo + c] = o;
        if (cat) out[(size_t)r * ldo + W + c] = a;
    }
}

// flag[0] = 1 when an index lies outside [0, N) (every writer stores the same value)
__global__ __launch_bounds__(256) void ga_check_kernel(const int32_t* __restrict__ idx, long long total, int N, int32_t* __restrict__ flag) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < total && (unsigned)idx[e] >= (unsigned)N) flag[0] = 1;
}

static bool ga_dims_ok(int B, int N, int S, int k, int D) {
    if (B <= 0 || B > 65535 || N <= 0 || S <= 0 || k <= 0 || k > N || D <= 0) return false;
    const long long E = (long long)S * k;
    if (E > 0x7fffffffLL || (long long)B * E > 0x7fffffffLL || (long long)B * N > 0x7fffffffLL) return false;
    if ((double)E * D < 2.0 || (double)B * E * D > 9.0e15 || (double)B * N * D > 9.0e15) return false;
    return true;
}

extern "C" size_t act_geo_affine_fwd_workspace(int B, int N, int S, int k, int D) {
    if (!ga_dims_ok(B, N, S, k, D)) return 0;
    return 16 + (size_t)B * ga_shape((long long)S * k, D).nblk * 2 * sizeof(double);      // (float lanes: at least as many blocks as float4 lanes)
}

extern "C" int act_geo_affine_group_fwd_f32(const float* feat, const int32_t* fps_idx, const int32_t* idx, const float* alpha, const float* beta, float eps,
                                            int B, int N, int S, int k, int D, int cat, int validate, float* out, float* sigma, float* mean,
                                            void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!feat || !fps_idx || !idx || !alpha || !beta || !out || !sigma || !mean || !workspace) return ACT_E_NULLPTR;
    if (!ga_dims_ok(B, N, S, k, D) || !(eps >= 0.f)) return ACT_E_BADARG;
    if (workspace_bytes < act_geo_affine_fwd_workspace(B, N, S, k, D) || ((uintptr_t)workspace & 15)) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const long long E = (long long)S * k, R = (long long)B * E;
    int32_t* flag = reinterpret_cast<int32_t*>(workspace);
    double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + 16);
    if (validate) {
        int32_t bad = 0;
        if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) return (int)hipGetLastError();
        hipLaunchKernelGGL(ga_check_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, idx, R, N, flag);
        hipLaunchKernelGGL(ga_check_kernel, dim3(cdiv((long long)B * S, 256)), dim3(256), 0, s, fps_idx, (long long)B * S, N, flag);
        ACT_LAUNCH_CHECK();
        if (hipMemcpyAsync(&bad, flag, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess) return (int)hipGetLastError();
        if (hipStreamSynchronize(s) != hipSuccess) return (int)hipGetLastError();
        if (bad) return ACT_E_INDEX;
    }
    const bool v4 = vec4(D, feat, alpha, beta, out);
    const int W = v4 ? D / 4 : D;
    const GaShape g = ga_shape(E, W);
    const int ty = 256 >> g.tx_log;
    ActProfScope ps(KID_ROW_GATHER, s, 6.0 * R * D, 4.0 * R * D * (cat ? 2.0 : 1.0) + 8.0 * R);
    if (v4) hipLaunchKernelGGL(ga_moments_kernel<float4>, dim3(g.nblk, B), dim3(256), 0, s, reinterpret_cast<const float4*>(feat), fps_idx, idx, N, S, k, W,
                               D, g.rpb, g.tx_log, part);
    else    hipLaunchKernelGGL(ga_moments_kernel<float>, dim3(g.nblk, B), dim3(256), 0, s, feat, fps_idx, idx, N, S, k, W, D, g.rpb, g.tx_log, part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(ga_sigma_kernel, dim3(B), dim3(256), 0, s, feat, fps_idx, idx, N, S, k, D, part, g.nblk, sigma, mean);
    ACT_LAUNCH_CHECK();
    if (v4) hipLaunchKernelGGL(ga_apply_kernel<float4>, dim3(cdiv(R, ty)), dim3(256), 0, s, reinterpret_cast<const float4*>(feat), fps_idx, idx,
                               reinterpret_cast<const float4*>(alpha), reinterpret_cast<const float4*>(beta), sigma, eps, N, S, k, W, R, g.tx_log, cat,
                               reinterpret_cast<float4*>(out));
    else    hipLaunchKernelGGL(ga_apply_kernel<float>, dim3(cdiv(R, ty)), dim3(256), 0, s, feat, fps_idx, idx, alpha, beta, sigma, eps, N, S, k, W, R,
                               g.tx_log, cat, out);
    ACT_LAUNCH_CHECK(); return 0;
}

// ============================================================================================ geometric affine grouping: backward
// With g the cotangent of the normalised columns and h that of the anchor columns (ldd = D or 2D floats per row of dout):
//   A_b[c] = sum_{i,j} g e, G_b[c] = sum_{i,j} g (float64, block partials then blocks in ascending order)
//   dalpha[c] = sum_b r_b A_b[c], dbeta[c] = sum_b G_b[c], T_b = sum_c alpha[c] A_b[c], q_b = -r_b^2 T_b / ((n - 1) sigma_b)  (0 where sigma_b == 0)
//   de = (alpha g) r + q_b (e - mean_b)
// and every point gathers de over the inverse adjacency of idx in ascending (i, j); a point that is anchor i adds sum_j h - sum_j de of its own k
// rows (found through the inverse adjacency of fps_idx, so a repeated anchor is summed too).  No [E, D] tensor, no atomics.
#define GA_BWD_BLOCKS 32

__global__ __launch_bounds__(256) void ga_bwd_sums_kernel(const float* __restrict__ feat, const int32_t* __restrict__ fps, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ dout, int ldd, int N, int S, int k, int D, int rpb, int tx_log,
                                                          double* __restrict__ part) {
    __shared__ double sh[2 * 256];
    const int b = blockIdx.y, TX = 1 << tx_log, TY = 256 >> tx_log, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log;
    const long long E = (long long)S * k;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(E, r0 + rpb);
    const float* fb = feat + (size_t)b * N * D;
    double* pb = part + (size_t)b * gridDim.x * 2 * D;
    for (int c0 = 0; c0 < D; c0 += TX) {
        const int c = c0 + tx;
        const bool act = c < D;
        double s[2] = {0.0, 0.0};
        if (act) {
            for (long long r = r0 + ty; r < r1; r += TY) {
                const int nb = idx[(size_t)b * E + r], an = fps[(size_t)b * S + r / k];
                const float e = __fsub_rn(fb[(size_t)nb * D + c], fb[(size_t)an * D + c]);
                const float g = dout[((size_t)b * E + r) * ldd + c];
                s[0] += (double)g;
                s[1] += (double)g * (double)e;
            }
        }
        col_reduce_store<2>(s, sh, tx, ty, TX, TY, act, c, D, pb);
    }
}

// per cloud: A_b, G_b and the coefficient q_b
__global__ __launch_bounds__(256) void ga_bwd_cloud_kernel(const double* __restrict__ part, int nblk, int D, double n, const float* __restrict__ alpha,
                                                           const float* __restrict__ sigma, float eps, double* __restrict__ AG, float* __restrict__ coef) {
    __shared__ double sh[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* pb = part + (size_t)b * nblk * 2 * D;
    double T = 0.0;
    for (int c = t; c < D; c += 256) {
        double g = 0.0, a = 0.0;
        for (int p = 0; p < nblk; ++p) { g += pb[((size_t)p * 2 + 0) * D + c]; a += pb[((size_t)p * 2 + 1) * D + c]; }
        AG[((size_t)b * 2 + 0) * D + c] = g;
        AG[((size_t)b * 2 + 1) * D + c] = a;
        T += (double)alpha[c] * a;
    }
    sh[t] = T;
    block_tree(sh, t);
    if (t == 0) {
        const float sg = sigma[b];
        const double r = (double)__fdiv_rn(1.0f, __fadd_rn(sg, eps));
        coef[b] = sg > 0.f ? (float)(-(r * r) * sh[0] / ((n - 1.0) * (double)sg)) : 0.f;
    }
}

__global__ __launch_bounds__(256) void ga_bwd_params_kernel(const double* __restrict__ AG, int B, int D, const float* __restrict__ sigma, float eps,
                                                            float* __restrict__ dalpha, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    double da = 0.0, db = 0.0;
    for (int b = 0; b < B; ++b) {
        const double r = (double)__fdiv_rn(1.0f, __fadd_rn(sigma[b], eps));
        db += AG[((size_t)b * 2 + 0) * D + c];
        da += r * AG[((size_t)b * 2 + 1) * D + c];
    }
    dalpha[c] = (float)da; dbeta[c] = (float)db;
}

template <typename V>
__device__ __forceinline__ V ga_de(const V& al, const V& g, float rr, float q, const V& e, float mu) {
    V o;
#pragma unroll
    for (int u = 0; u < Vn<V>::n; ++u)
        fl(o)[u] = __fadd_rn(__fmul_rn(__fmul_rn(fl(al)[u], fl(g)[u]), rr), __fmul_rn(q, __fsub_rn(fl(e)[u], mu)));
    return o;
}

// idx and fps hold indices in [0, N) here (the entry point clamps them into the workspace); off / ent: inverse adjacency of idx over [B, E],
// aoff / aent: that of fps over [B, S]
template <typename V>
__global__ __launch_bounds__(256) void ga_bwd_points_kernel(const V* __restrict__ feat, const int32_t* __restrict__ fps, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ off, const int32_t* __restrict__ ent,
                                                            const int32_t* __restrict__ aoff, const int32_t* __restrict__ aent,
                                                            const V* __restrict__ alpha, const float* __restrict__ sigma, const float* __restrict__ mean,
                                                            const float* __restrict__ coef, float eps, const V* __restrict__ dout, int ldd, int cat, int N,
                                                            int S, int k, int W, long long RN, int tx_log, V* __restrict__ dfeat) {
    const int t = threadIdx.x, TX = 1 << tx_log, TY = 256 >> tx_log, tx = t & (TX - 1), ty = t >> tx_log;
    const long long p = (long long)blockIdx.x * TY + ty;
    if (p >= RN) return;
    const long long b = p / N, E = (long long)S * k;
    const int m = (int)(p - b * N);
    const float rr = __fdiv_rn(1.0f, __fadd_rn(sigma[b], eps)), q = coef[b], mu = mean[b];
    const V* fb = feat + (size_t)b * N * W;
    const V* gb = dout + (size_t)b * E * ldd;
    const int32_t* eb = ent + (size_t)b * E;
    const int32_t* ab = aent + (size_t)b * S;
    const int32_t* fpb = fps + (size_t)b * S;
    const int32_t* ib = idx + (size_t)b * E;
    const int e0 = max(off[b * ((long long)N + 1) + m], 0), e1 = (int)min((long long)off[b * ((long long)N + 1) + m + 1], E);
    const int a0 = max(aoff[b * ((long long)N + 1) + m], 0), a1 = min(aoff[b * ((long long)N + 1) + m + 1], S);
    for (int c = tx; c < W; c += TX) {
        const V fm = fb[(size_t)m * W + c], al = alpha[c];
        V acc = vzero<V>();
        for (int i = e0; i < e1; ++i) {
            const int en = min(max(eb[i], 0), (int)(E - 1));
            const V e = vsub(fm, fb[(size_t)fpb[en / k] * W + c]);
            acc = vadd(acc, ga_de(al, gb[(size_t)en * ldd + c], rr, q, e, mu));
        }
        for (int i = a0; i < a1; ++i) {
            const int an = min(max(ab[i], 0), S - 1);
            V hs = vzero<V>(), ds = vzero<V>();
            for (int j = 0; j < k; ++j) {
                const size_t row = (size_t)an * k + j;
                const V e = vsub(fb[(size_t)ib[row] * W + c], fm);
                ds = vadd(ds, ga_de(al, gb[row * ldd + c], rr, q, e, mu));
                if (cat) hs = vadd(hs, gb[row * ldd + W + c]);
            }
            acc = vadd(acc, vsub(hs, ds));
        }
        dfeat[(size_t)p * W + c] = acc;
    }
}

struct GaBwdWs { int32_t *idxc, *fpsc, *off, *ent, *aoff, *aent; float* coef; double *AG, *part; size_t bytes; };
static GaBwdWs ga_bwd_carve(char* ws, int B, int N, int S, int k, int D) {
    GaBwdWs w;
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = ws ? ws + o : nullptr; o += align16(bytes); return p; };
    const size_t E = (size_t)S * k;
    w.part = (double*)take((size_t)B * GA_BWD_BLOCKS * 2 * D * sizeof(double));
    w.AG = (double*)take((size_t)B * 2 * D * sizeof(double));
    w.coef = (float*)take((size_t)B * sizeof(float));
    w.idxc = (int32_t*)take((size_t)B * E * 4);
    w.fpsc = (int32_t*)take((size_t)B * S * 4);
    w.off = (int32_t*)take((size_t)B * ((size_t)N + 1) * 4);
    w.ent = (int32_t*)take((size_t)B * E * 4);
    w.aoff = (int32_t*)take((size_t)B * ((size_t)N + 1) * 4);
    w.aent = (int32_t*)take((size_t)B * S * 4);
    w.bytes = o;
    return w;
}

extern "C" size_t act_geo_affine_bwd_workspace(int B, int N, int S, int k, int D) {
    if (!ga_dims_ok(B, N, S, k, D)) return 0;
    return ga_bwd_carve(nullptr, B, N, S, k, D).bytes;
}

extern "C" int act_geo_affine_group_bwd_f32(const float* feat, const int32_t* fps_idx, const int32_t* idx, const float* alpha, const float* sigma,
                                            const float* mean, float eps, const float* dout, int B, int N, int S, int k, int D, int cat, float* dfeat,
                                            float* dalpha, float* dbeta, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!feat || !fps_idx || !idx || !alpha || !sigma || !mean || !dout || !dfeat || !dalpha || !dbeta || !workspace) return ACT_E_NULLPTR;
    if (!ga_dims_ok(B, N, S, k, D) || !(eps >= 0.f)) return ACT_E_BADARG;
    if (workspace_bytes < act_geo_affine_bwd_workspace(B, N, S, k, D) || ((uintptr_t)workspace & 15)) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const long long E = (long long)S * k, R = (long long)B * E, RN = (long long)B * N;
    const GaBwdWs w = ga_bwd_carve(reinterpret_cast<char*>(workspace), B, N, S, k, D);
    const int ldd = cat ? 2 * D : D;
    ActProfScope ps(KID_ROW_SCATTER, s, 12.0 * R * D, 4.0 * (2.0 * R * ldd + RN * D) + 24.0 * R);
    hipLaunchKernelGGL(clamp_idx_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, idx, R, N, w.idxc);
    hipLaunchKernelGGL(clamp_idx_kernel, dim3(cdiv((long long)B * S, 256)), dim3(256), 0, s, fps_idx, (long long)B * S, N, w.fpsc);
    ACT_LAUNCH_CHECK();
    // the column sums: at most GA_BWD_BLOCKS row ranges per cloud
    const int tx_log = lane_log(D), ty = 256 >> tx_log;
    long long rpb = (E + GA_BWD_BLOCKS - 1) / GA_BWD_BLOCKS;
    rpb = (rpb + ty - 1) / ty * ty;
    const int nblk = (int)((E + rpb - 1) / rpb);
    hipLaunchKernelGGL(ga_bwd_sums_kernel, dim3(nblk, B), dim3(256), 0, s, feat, w.fpsc, w.idxc, dout, ldd, N, S, k, D, (int)rpb, tx_log, w.part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(ga_bwd_cloud_kernel, dim3(B), dim3(256), 0, s, w.part, nblk, D, (double)E * D, alpha, sigma, eps, w.AG, w.coef);
    hipLaunchKernelGGL(ga_bwd_params_kernel, dim3(cdiv(D, 256)), dim3(256), 0, s, w.AG, B, D, sigma, eps, dalpha, dbeta);
    ACT_LAUNCH_CHECK();
    int rc = act_sa_build_adjacency(w.idxc, B, N, (int)E, w.off, w.ent, s);
    if (rc) return rc;
    rc = act_sa_build_adjacency(w.fpsc, B, N, S, w.aoff, w.aent, s);
    if (rc) return rc;
    const bool v4 = vec4(D, feat, alpha, dout, dfeat);
    const int W = v4 ? D / 4 : D, wl = lane_log(W), wy = 256 >> wl;
    if (v4) hipLaunchKernelGGL(ga_bwd_points_kernel<float4>, dim3(cdiv(RN, wy)), dim3(256), 0, s, reinterpret_cast<const float4*>(feat), w.fpsc, w.idxc, w.off,
                               w.ent, w.aoff, w.aent, reinterpret_cast<const float4*>(alpha), sigma, mean, w.coef, eps,
                               reinterpret_cast<const float4*>(dout), ldd / 4, cat, N, S, k, W, RN, wl, reinterpret_cast<float4*>(dfeat));
    else    hipLaunchKernelGGL(ga_bwd_points_kernel<float>, dim3(cdiv(RN, wy)), dim3(256), 0, s, feat, w.fpsc, w.idxc, w.off, w.ent, w.aoff, w.aent, alpha,
                               sigma, mean, w.coef, eps, dout, ldd, cat, N, S, k, W, RN, wl, dfeat);
    ACT_LAUNCH_CHECK(); return 0;
}

// ============================================================================================ residual BatchNorm tail: ReLU(BN(y) + res)
// out = max((y * scale + shift) + res, 0) on rows [R,C].  The sign of BN(y) + res cannot be rebuilt from scale * y + shift alone, so the backward
// takes its mask from the saved output: g = dout where out > 0, dres = g, dbeta = sum g, dgamma = sum g xhat (float64 column sums in a fixed order),
// dy = scale * (g - dbeta / R - xhat * dgamma / R).
template <typename V>
__global__ __launch_bounds__(256) void affine_add_relu_kernel(const V* __restrict__ y, const V* __restrict__ res, const V* __restrict__ scale,
                                                              const V* __restrict__ shift, long long total, int CV, V* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % CV);
        const V v = y[i], rv = res[i], sc = scale[c], sf = shift[c];
        V o;
#pragma unroll
        for (int u = 0; u < Vn<V>::n; ++u)
            fl(o)[u] = fmaxf(__fadd_rn(__fadd_rn(__fmul_rn(fl(v)[u], fl(sc)[u]), fl(sf)[u]), fl(rv)[u]), 0.f);
        out[i] = o;
    }
}

static unsigned flat_grid(long long total) {
    long long g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    return (unsigned)(g < 1 ? 1 : g);
}

extern "C" int act_affine_add_relu_f32(const float* y, const float* res, const float* scale, const float* shift, int R, int C, float* out,
                                       act_stream_t stream) {
    if (!y || !res || !scale || !shift || !out) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)R * C;
    ActProfScope ps(KID_BN_APPLY, s, 4.0 * total, 12.0 * total);
    if (vec4(C, y, res, out) && vec4(C, scale, shift))
        hipLaunchKernelGGL(affine_add_relu_kernel<float4>, dim3(flat_grid(total / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(y),
                           reinterpret_cast<const float4*>(res), reinterpret_cast<const float4*>(scale), reinterpret_cast<const float4*>(shift), total / 4,
                           C / 4, reinterpret_cast<float4*>(out));
    else
        hipLaunchKernelGGL(affine_add_relu_kernel<float>, dim3(flat_grid(total)), dim3(256), 0, s, y, res, scale, shift, total, C, out);
    ACT_LAUNCH_CHECK(); return 0;
}

// The column sums of the backward, and with them the moments of y around the forward's mean once more, in float64: the forward's mean and rstd are
// float32 statistics a few ulps off, which is what the gradient would otherwise inherit.  s = {sum g, sum g (y - mu), sum (y - mu), sum (y - mu)^2}.
__global__ __launch_bounds__(256) void bn_add_relu_bwd_sums_kernel(const float* __restrict__ y, const float* __restrict__ out, const float* __restrict__ dout,
                                                                   int C, long long R, int rpb, int tx_log, const float* __restrict__ mean,
                                                                   double* __restrict__ part) {
    __shared__ double sh[4 * 256];
    const int TX = 1 << tx_log, TY = 256 >> tx_log, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log;
    const long long r0 = (long long)blockIdx.x * rpb, r1 = min(R, r0 + rpb);
    const int c = blockIdx.y * TX + tx;                                   // one strip of TX columns per block: C / TX times the blocks in flight
    const bool act = c < C;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (act) {
        const double mu = (double)mean[c];
        for (long long r = r0 + ty; r < r1; r += TY) {
            const double g = out[r * C + c] > 0.f ? (double)dout[r * C + c] : 0.0, d = (double)y[r * C + c] - mu;
            s[0] += g;
            s[1] += g * d;
            s[2] += d;
            s[3] += d * d;
        }
    }
    col_reduce_store<4>(s, sh, tx, ty, TX, TY, act, c, C, part);
}

// coef [5, C]: dbeta / R, dgamma / R, gamma * rstd, the correction of the mean, rstd -- the last three from the float64 moments
__global__ __launch_bounds__(256) void bn_add_relu_bwd_finalize_kernel(const double* __restrict__ part, int nblk, int C, double R, const float* __restrict__ gamma,
                                                                       float eps, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                       float* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = 0; p < nblk; ++p)
        for (int q = 0; q < 4; ++q) s[q] += part[((size_t)p * 4 + q) * C + c];
    const double dm = s[2] / R;
    double var = s[3] / R - dm * dm;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps), dg = rstd * (s[1] - dm * s[0]);
    dbeta[c] = (float)s[0]; dgamma[c] = (float)dg;
    coef[c] = (float)(s[0] / R);
    coef[C + c] = (float)(dg / R);
    coef[2 * C + c] = (float)((double)gamma[c] * rstd);
    coef[3 * C + c] = (float)dm;
    coef[4 * C + c] = (float)rstd;
}

template <typename V>
__global__ __launch_bounds__(256) void bn_add_relu_bwd_apply_kernel(const V* __restrict__ y, const V* __restrict__ out, const V* __restrict__ dout,
                                                                    const V* __restrict__ mean, const V* __restrict__ coef, long long total, int CV,
                                                                    V* __restrict__ dy, V* __restrict__ dres) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % CV);
        const V v = y[i], o = out[i], d = dout[i], mu = mean[c], k1 = coef[c], k2 = coef[CV + c], sc = coef[2 * CV + c], dm = coef[3 * CV + c],
                rs = coef[4 * CV + c];
        V g, dx;
#pragma unroll
        for (int u = 0; u < Vn<V>::n; ++u) {
            fl(g)[u] = fl(o)[u] > 0.f ? fl(d)[u] : 0.f;
            const float xhat = __fmul_rn(__fsub_rn(__fsub_rn(fl(v)[u], fl(mu)[u]), fl(dm)[u]), fl(rs)[u]);
            fl(dx)[u] = __fmul_rn(fl(sc)[u], __fsub_rn(__fsub_rn(fl(g)[u], fl(k1)[u]), __fmul_rn(xhat, fl(k2)[u])));
        }
        dy[i] = dx;
        dres[i] = g;
    }
}

extern "C" size_t act_bn_add_relu_bwd_workspace(int R, int C) {
    if (R <= 0 || C <= 0) return 0;
    return align16((size_t)5 * C * 4) + part_bytes(C, 4);
}

extern "C" int act_bn_add_relu_bwd_f32(const float* y, const float* out, const float* dout, const float* gamma, const float* mean, float eps, int R, int C,
                                       float* dy, float* dres, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                       act_stream_t stream) {
    if (!y || !out || !dout || !gamma || !mean || !dy || !dres || !dgamma || !dbeta || !workspace) return ACT_E_NULLPTR;
    if (R <= 0 || C <= 0 || C > 65535 * 64 || !(eps >= 0.f)) return ACT_E_BADARG;
    if (workspace_bytes < act_bn_add_relu_bwd_workspace(R, C) || ((uintptr_t)workspace & 15)) return ACT_E_BADARG;
    char* ws = reinterpret_cast<char*>(workspace);
    float* coef = (float*)ws;
    double* part = (double*)(ws + align16((size_t)5 * C * 4));
    const ColShape g = col_shape(R, C);
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)R * C;
    ActProfScope ps(KID_BN_BWD, s, 14.0 * total, 32.0 * total);
    hipLaunchKernelGGL(bn_add_relu_bwd_sums_kernel, dim3(g.nblk, cdiv(C, 1 << g.tx_log)), dim3(256), 0, s, y, out, dout, C, (long long)R, g.rpb, g.tx_log, mean, part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_add_relu_bwd_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, part, g.nblk, C, (double)R, gamma, eps, dgamma, dbeta, coef);
    ACT_LAUNCH_CHECK();
    if (vec4(C, y, out, dout, dy) && vec4(C, dres, mean))
        hipLaunchKernelGGL(bn_add_relu_bwd_apply_kernel<float4>, dim3(flat_grid(total / 4)), dim3(256), 0, s, reinterpret_cast<const float4*>(y),
                           reinterpret_cast<const float4*>(out), reinterpret_cast<const float4*>(dout), reinterpret_cast<const float4*>(mean),
                           reinterpret_cast<const float4*>(coef), total / 4, C / 4, reinterpret_cast<float4*>(dy), reinterpret_cast<float4*>(dres));
    else
        hipLaunchKernelGGL(bn_add_relu_bwd_apply_kernel<float>, dim3(flat_grid(total)), dim3(256), 0, s, y, out, dout, mean, coef, total, C, dy, dres);
    ACT_LAUNCH_CHECK(); return 0;
}
