// recon_eval.hip -- Stage-I reconstruction evaluation (tools/runner_autoencoder.py:219-323 validate, utils/metrics.py): for every cloud of a
// batch, in ONE launch, the four whole-cloud Chamfer losses (sparse / dense, L1 / L2), the ignore_zeros Chamfer metrics CDL1 / CDL2
// (chamfer_dist/__init__.py:37-41,73-77 at batch size 1) and the F-Score@th counts (metrics.py:57-76).
//
// One workgroup per cloud runs the four nearest-neighbour scans dense->gt, gt->dense, coarse->gt, gt->coarse:
//  * resident path (the Stage-I geometry, 512 + 2048 + 1024 points = 54 KB): the three clouds are staged ONCE into LDS as x[] y[] z[] arrays
//    (plus w[] = 0 / +inf, the zero-point mask as an additive penalty).  In the inner loop every lane reads the same candidate address, so a
//    ds_read_b128 of four candidates' x (y, z, w) is a broadcast: no bank conflicts by construction.
//  * tiled path (clouds that do not fit): the candidates stream through a 1024-point LDS tile per block of 512 queries, as chamfer_large_fwd.
// The dense<->gt scans carry two running minima (all candidates; non-zero candidates: d + w), so the ignore_zeros variants cost no second pass.
//
// Arithmetic: squared distances are sqdist3 (every product and sum rounded; the file is built with -ffp-contract=off), so the per-point minima
// are bit-identical to act_chamfer_fwd_f32's dist1 / dist2.  Sums run in float64: one lane owns queries tid, tid + 512, ... in increasing
// order, the wave sum is a fixed xor butterfly, the 8 wave sums are added in wave order by lane 0.  No atomics: a row is bit-identical run to
// run.  The '< th' decision is taken on the float64 distance between the query and the neighbour the fp32 scan selected (strict '<': lowest
// index on ties, as chamfer.hip).
#include "common.h"
#include <math.h>

#define RE_THREADS 512
#define RE_WAVES (RE_THREADS / ACT_WAVE)
#define RE_TILE 1024              // candidates per LDS tile of the tiled path
#define RE_NACC 16                // per-cloud sums (see the enum)
#define RE_LDS_MAX (60 * 1024)    // resident path: staged bytes (the default 64 KB dynamic-LDS limit less the static reduction buffer)

enum { A_S1 = 0, A_S2, A_M1, A_M2, A_NZ, A_HIT,          // dense -> gt: sum sqrt(d), sum d, the same over non-zero points, their count, hits
       B_S1, B_S2, B_M1, B_M2, B_NZ, B_HIT,              // gt -> dense
       C_S1, C_S2, D_S1, D_S2 };                         // coarse -> gt, gt -> coarse

__device__ __forceinline__ int re_pad4(int n) { return (n + 3) & ~3; }
// torch.sum(xyz, dim=2).ne(0) of one point, in fp32: (x + y) + z
__device__ __forceinline__ bool re_is_zero(float x, float y, float z) { return __fadd_rn(__fadd_rn(x, y), z) == 0.0f; }

// points [n,3] -> x[] y[] z[] (w[] = +inf for a zero point, else 0) for indices [0, npad): the padding is at +inf, never the nearest
__device__ __forceinline__ void re_stage(const float* __restrict__ src, int n, int npad, float* sx, float* sy, float* sz, float* sw) {
    for (int t = threadIdx.x; t < npad; t += RE_THREADS) {
        float x = INFINITY, y = INFINITY, z = INFINITY;
        if (t < n) { const float* p = src + (size_t)t * 3; x = p[0]; y = p[1]; z = p[2]; }
        sx[t] = x; sy[t] = y; sz[t] = z;
        if (sw) sw[t] = (t < n && !re_is_zero(x, y, z)) ? 0.0f : INFINITY;
    }
}

#define RE_STEP(J, BX, BY, BZ, BW)                                             \
    {                                                                          \
        const float d = sqdist3(BX, BY, BZ, qx, qy, qz);                       \
        if (d < best) { best = d; bi = base + k + J; }                         \
        if (MASK) bnz = fminf(bnz, __fadd_rn(d, BW));                          \
    }

// scan cnt4 (a multiple of 4) staged candidates; every lane reads the same addresses (LDS broadcast)
template <bool MASK>
__device__ __forceinline__ void re_scan(const float* sx, const float* sy, const float* sz, const float* sw, int cnt4, int base, float qx, float qy,
                                        float qz, float& best, int& bi, float& bnz) {
#pragma unroll 2
    for (int k = 0; k < cnt4; k += 4) {
        const float4 X = *reinterpret_cast<const float4*>(sx + k), Y = *reinterpret_cast<const float4*>(sy + k),
                     Z = *reinterpret_cast<const float4*>(sz + k);
        float4 W = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MASK) W = *reinterpret_cast<const float4*>(sw + k);
        RE_STEP(0, X.x, Y.x, Z.x, W.x)
        RE_STEP(1, X.y, Y.y, Z.y, W.y)
        RE_STEP(2, X.z, Y.z, Z.z, W.z)
        RE_STEP(3, X.w, Y.w, Z.w, W.w)
    }
}

// one direction: every query of q [nq,3] against the candidates c [ncand,3].  RES: the candidates are already staged at rx / ry / rz / rw;
// else they stream through the tile at lds.  acc[0..1] += sqrt(min), min; MASK: acc[2..4] += the same over non-zero queries against non-zero
// candidates and the count of non-zero queries; acc[5] += queries whose float64 distance to the selected neighbour is < th.
template <bool RES, bool MASK>
__device__ __forceinline__ void re_pass(const float* __restrict__ q, int nq, const float* __restrict__ c, int ncand, const float* rx, const float* ry,
                                        const float* rz, const float* rw, float* lds, double th, double* acc) {
    for (int q0 = 0; q0 < nq; q0 += RE_THREADS) {                    // uniform trip count: the tiled path has barriers inside
        const int j = q0 + threadIdx.x;
        const bool valid = j < nq;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (valid) { const float* p = q + (size_t)j * 3; qx = p[0]; qy = p[1]; qz = p[2]; }
        float best = INFINITY, bnz = INFINITY;
        int bi = 0;
        if (RES) {
            if (valid) re_scan<MASK>(rx, ry, rz, rw, re_pad4(ncand), 0, qx, qy, qz, best, bi, bnz);       // no barrier inside: idle waves skip the scan
        } else {
            float *tx = lds, *ty = lds + RE_TILE, *tz = lds + 2 * RE_TILE, *tw = lds + 3 * RE_TILE;
            for (int k2 = 0; k2 < ncand; k2 += RE_TILE) {
                const int cnt = min(RE_TILE, ncand - k2);
                __syncthreads();                                     // every lane is done with the previous tile
                re_stage(c + (size_t)k2 * 3, cnt, re_pad4(cnt), tx, ty, tz, MASK ? tw : nullptr);
                __syncthreads();
                re_scan<MASK>(tx, ty, tz, tw, re_pad4(cnt), k2, qx, qy, qz, best, bi, bnz);
            }
        }
        if (valid) {
            acc[0] += sqrt((double)best);
            acc[1] += (double)best;
            if (MASK) {
                if (!re_is_zero(qx, qy, qz)) { acc[2] += sqrt((double)bnz); acc[3] += (double)bnz; acc[4] += 1.0; }
                const float* p = c + (size_t)bi * 3;                 // bi < ncand always (0 when nothing compared below +inf)
                const double dx = (double)qx - (double)p[0], dy = (double)qy - (double)p[1], dz = (double)qz - (double)p[2];
                if (sqrt(dx * dx + dy * dy + dz * dz) < th) acc[5] += 1.0;
            }
        }
    }
}

template <bool RES>
__global__ __launch_bounds__(RE_THREADS) void recon_eval_kernel(const float* __restrict__ coarse, const float* __restrict__ dense,
                                                               const float* __restrict__ gt, int nc, int nd, int N, float th,
                                                               double* __restrict__ out, int row0) {
    extern __shared__ float4 re_lds4[];
    __shared__ double red[RE_WAVES][RE_NACC];
    float* lds = reinterpret_cast<float*>(re_lds4);
    const int b = blockIdx.x;
    const float* pc = coarse + (size_t)b * nc * 3;
    const float* pd = dense + (size_t)b * nd * 3;
    const float* pg = gt + (size_t)b * N * 3;
    const int Np = re_pad4(N), ndp = re_pad4(nd), ncp = re_pad4(nc);
    float *gx = lds, *gy = gx + Np, *gz = gy + Np, *gw = gz + Np;
    float *dx = gw + Np, *dy = dx + ndp, *dz = dy + ndp, *dw = dz + ndp;
    float *cx = dw + ndp, *cy = cx + ncp, *cz = cy + ncp;
    if (RES) {
        re_stage(pg, N, Np, gx, gy, gz, gw);
        re_stage(pd, nd, ndp, dx, dy, dz, dw);
        re_stage(pc, nc, ncp, cx, cy, cz, nullptr);
        __syncthreads();
    }
    double acc[RE_NACC];
#pragma unroll
    for (int i = 0; i < RE_NACC; ++i) acc[i] = 0.0;
    const double thd = (double)th;
    re_pass<RES, true>(pd, nd, pg, N, gx, gy, gz, gw, lds, thd, acc + A_S1);
    re_pass<RES, true>(pg, N, pd, nd, dx, dy, dz, dw, lds, thd, acc + B_S1);
    re_pass<RES, false>(pc, nc, pg, N, gx, gy, gz, nullptr, lds, thd, acc + C_S1);
    re_pass<RES, false>(pg, N, pc, nc, cx, cy, cz, nullptr, lds, thd, acc + D_S1);
    // fixed-order reduction: xor butterfly within the wave, then the waves in order
#pragma unroll
    for (int i = 0; i < RE_NACC; ++i) {
        double v = acc[i];
#pragma unroll
        for (int o = 1; o < ACT_WAVE; o <<= 1) v += __shfl_xor(v, o, ACT_WAVE);
        acc[i] = v;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < RE_NACC; ++i) red[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[RE_NACC];
        for (int i = 0; i < RE_NACC; ++i) {
            double v = red[0][i];
            for (int w = 1; w < RE_WAVES; ++w) v += red[w][i];
            s[i] = v;
        }
        const double fnc = (double)nc, fnd = (double)nd, fN = (double)N, qnan = __longlong_as_double(0x7ff8000000000000LL);
        const bool some = s[A_NZ] > 0.0 && s[B_NZ] > 0.0;            // torch.mean of an empty tensor is NaN
        const double p = s[A_HIT] / fnd, r = s[B_HIT] / fN;
        double* o = out + (size_t)(row0 + b) * ACT_RECON_FIELDS;
        o[0] = (s[C_S1] / fnc + s[D_S1] / fN) / 2.0;
        o[1] = s[C_S2] / fnc + s[D_S2] / fN;
        o[2] = (s[A_S1] / fnd + s[B_S1] / fN) / 2.0;
        o[3] = s[A_S2] / fnd + s[B_S2] / fN;
        o[4] = some ? (s[A_M1] / s[A_NZ] + s[B_M1] / s[B_NZ]) / 2.0 : qnan;
        o[5] = some ? s[A_M2] / s[A_NZ] + s[B_M2] / s[B_NZ] : qnan;
        o[6] = s[A_HIT];
        o[7] = s[B_HIT];
        o[8] = (r + p) > 0.0 ? 2.0 * r * p / (r + p) : 0.0;
        o[9] = s[A_NZ];
        o[10] = s[B_NZ];
        o[11] = 0.0;
    }
}

extern "C" int act_recon_eval_f32(const float* coarse, const float* dense, const float* gt, int B, int nc, int nd, int N, float th, double* out,
                                  int row0, int num_rows, act_stream_t stream) {
    if (B == 0) return 0;
    if (!coarse || !dense || !gt || !out) return ACT_E_NULLPTR;
    if (B < 0 || nc <= 0 || nd <= 0 || N <= 0 || nc > (1 << 24) || nd > (1 << 24) || N > (1 << 24)) return ACT_E_BADARG;   // counts exact, indices int
    if (row0 < 0 || (long long)row0 + B > (long long)num_rows) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const double evals = (double)B * 2.0 * ((double)nd * N + (double)nc * N);
    ActProfScope ps(KID_CHAMFER_FWD, s, 8.0 * evals, (double)B * (12.0 * ((double)nc + nd + N) + 8.0 * ACT_RECON_FIELDS));
    const size_t resident = sizeof(float) * (4 * (size_t)((N + 3) & ~3) + 4 * (size_t)((nd + 3) & ~3) + 3 * (size_t)((nc + 3) & ~3));
    if (resident <= RE_LDS_MAX)
        hipLaunchKernelGGL(recon_eval_kernel<true>, dim3(B), dim3(RE_THREADS), resident, s, coarse, dense, gt, nc, nd, N, th, out, row0);
    else
        hipLaunchKernelGGL(recon_eval_kernel<false>, dim3(B), dim3(RE_THREADS), sizeof(float) * 4 * RE_TILE, s, coarse, dense, gt, nc, nd, N, th, out,
                           row0);
    ACT_LAUNCH_CHECK();
    return 0;
}
