// emd.hip -- Earth Mover's Distance between two clouds of N points each: the exact assignment problem min_a sum_i |x1[i] - x2[a(i)]|^2,
// solved by a forward auction with eps-scaling (Bertsekas 1988), entirely on the device, for gfx950.
//
// The extensions/emd module of the code bases ACT grew from (models/dvae.py:302,701 keep its commented call) is an approximate auction with a
// fixed iteration count that may leave points unassigned and differs from run to run.  Here:
//  * ONE WORKGROUP PER PAIR for the whole solve, one launch per batch.  Both clouds, the prices, owner[j], assign[i], the per-object bid slots
//    and the two lists of unassigned bidders live in LDS (52 bytes per point: 3,072 points fill the 160 KiB of a CU).
//  * Jacobi rounds.  After the first rounds of a phase only a handful of bidders are unassigned, so the unassigned bidders are kept as a
//    compacted list and EACH BIDDER GETS A WAVE: its scan of the N objects is N / 64 steps plus three DPP reductions (best value, its lowest
//    index, second-best value).
//  * bids meet in one 64-bit LDS atomicMax per bid on the key (bid bits << 32) | ~bidder: bids are positive floats, so their bit patterns
//    order like the values, equal bids go to the lower bidder, and the maximum does not depend on arrival order.  A new bid on an object is
//    strictly above its price, which is the object's last winning bid, so a slot never has to be cleared.
//  * every cost is (dx*dx + dy*dy) + dz*dz with each operation rounded (sqdist3), every value d + price one rounded sum: a host restatement
//    reproduces dist bit for bit, and on lattice inputs with a power-of-two eps_final every bid and price is exact.
//  * the round loop has a hard cap; past it the unassigned bidders get the free objects in ascending order, so the result is always a bijection.
#include <math.h>
#include "common.h"

#define EMD_MAX_POINTS 3072
#define EMD_WAVE_MAX_POINTS 64                       // emd_wave_kernel: one object per lane
#define EMD_THETA 4.0f
#define EMD_HDR 16                                   // bytes: cnt[2], max-distance bits, pad
#define EMD_BYTES_PER_POINT 52

typedef unsigned long long emd_u64;

__global__ __launch_bounds__(1024) void emd_auction_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2, int N,
                                                           float eps_final, int max_rounds, float* __restrict__ dist,
                                                           int32_t* __restrict__ assignment, int32_t* __restrict__ info,
                                                           emd_u64* __restrict__ evals) {
    extern __shared__ __align__(16) unsigned char emd_smem[];
    int* cnt = reinterpret_cast<int*>(emd_smem);                             // cnt[0], cnt[1]: lengths of the two lists; cnt[2]: max d_ij bits
    emd_u64* bidkey = reinterpret_cast<emd_u64*>(emd_smem + EMD_HDR);
    float* bx = reinterpret_cast<float*>(bidkey + N);
    float *by = bx + N, *bz = by + N, *ax = bz + N, *ay = ax + N, *az = ay + N, *price = az + N;
    int* owner = reinterpret_cast<int*>(price + N);
    int *assign = owner + N, *want = assign + N;
    unsigned short* list0 = reinterpret_cast<unsigned short*>(want + N);
    unsigned short* list1 = list0 + N;

    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const size_t base = (size_t)blockIdx.x * N;
    const float INF = __builtin_inff();

    for (int i = tid; i < N; i += nt) {
        const float* p = xyz1 + (base + i) * 3; ax[i] = p[0]; ay[i] = p[1]; az[i] = p[2];
        const float* q = xyz2 + (base + i) * 3; bx[i] = q[0]; by[i] = q[1]; bz[i] = q[2];
        price[i] = 0.f; bidkey[i] = 0ull;
    }
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();

    // max_ij d_ij: non-negative floats order like their bit patterns
    {
        float m = 0.f;
        for (int i = tid; i < N; i += nt) {
            const float x = ax[i], y = ay[i], z = az[i];
            for (int j = 0; j < N; ++j) m = fmaxf(m, sqdist3(x, y, z, bx[j], by[j], bz[j]));
        }
        m = wave_max_f32(m, -1.f);
        if (lane == 0) atomicMax(&cnt[2], __float_as_int(m));
    }
    __syncthreads();
    // the ladder eps_final * theta^k: start at the smallest rung >= max d / 4 (at most 64 rungs: an infinite distance must not spin here)
    float eps = eps_final;
    {
        const float first = __int_as_float(cnt[2]) * 0.25f;
        for (int k = 0; k < 64 && eps < first; ++k) eps *= EMD_THETA;
    }

    int cur = 0, rounds = 0;
    bool capped = false;
    emd_u64 bids = 0;
    for (;;) {                                                               // one phase
        __syncthreads();                                                     // everybody has read cnt[cur] == 0 of the phase before
        for (int i = tid; i < N; i += nt) { assign[i] = -1; owner[i] = -1; (cur ? list1 : list0)[i] = (unsigned short)i; }
        if (tid == 0) cnt[cur] = N;
        __syncthreads();
        for (;;) {                                                           // one round
            const int c = cnt[cur];
            if (c == 0) break;
            if (rounds >= max_rounds) { capped = true; break; }
            ++rounds; bids += (emd_u64)c;
            const unsigned short* lst = cur ? list1 : list0;
            unsigned short* nxt = cur ? list0 : list1;
            if (tid == 0) cnt[cur ^ 1] = 0;
            // bidding: one wave per unassigned bidder
            for (int t = wave; t < c; t += nw) {
                const int i = lst[t];
                const float x = ax[i], y = ay[i], z = az[i];
                float u1 = INF, u2 = INF; int j1 = 0x7fffffff;               // u = d + price = -value: smallest and second smallest of this lane
                for (int j = lane; j < N; j += 64) {
                    const float u = __fadd_rn(sqdist3(x, y, z, bx[j], by[j], bz[j]), price[j]);
                    const bool lt = u < u1;                                  // branch-free: (u1, j1) = best so far, u2 = best of the rest
                    u2 = lt ? u1 : fminf(u2, u);
                    j1 = lt ? j : j1;
                    u1 = lt ? u : u1;
                }
                const float m1 = wave_min_f32(u1, INF);
                int jb = -wave_max_i32(u1 == m1 ? -j1 : -0x7fffffff, (int)0x80000000);      // lowest index among the best
                const float m2 = wave_min_f32(j1 == jb ? u2 : u1, INF);      // best of everything else
                if (lane == 0) {
                    if (jb >= N) jb = 0;                                     // no finite value at all (inf / NaN coordinates): any object, the cap ends it
                    const float p = price[jb];
                    float bid = m2 < INF ? __fadd_rn(__fadd_rn(p, __fsub_rn(m2, m1)), eps) : __fadd_rn(p, eps);
                    if (!(bid > p)) bid = __int_as_float(__float_as_int(p) + 1);            // eps below half an ulp of the price: still strictly up
                    want[t] = jb;
                    atomicMax(&bidkey[jb], ((emd_u64)__float_as_uint(bid) << 32) | (emd_u64)(~(unsigned)i));
                }
            }
            __syncthreads();
            // resolution: one thread per bidder
            for (int t = tid; t < c; t += nt) {
                const int i = lst[t], j = want[t];
                const emd_u64 key = bidkey[j];
                if (~(unsigned)key == (unsigned)i) {
                    const int prev = owner[j];
                    owner[j] = i; assign[i] = j; price[j] = __uint_as_float((unsigned)(key >> 32));
                    if (prev >= 0) { assign[prev] = -1; nxt[atomicAdd(&cnt[cur ^ 1], 1)] = (unsigned short)prev; }
                } else {
                    nxt[atomicAdd(&cnt[cur ^ 1], 1)] = (unsigned short)i;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        if (capped || !(eps > eps_final)) break;
        eps = fmaxf(eps / EMD_THETA, eps_final);
    }

    if (capped) {                                                            // unassigned bidders take the free objects, both ascending
        __syncthreads();
        if (tid == 0) {
            int j = 0;
            for (int i = 0; i < N; ++i) {
                if (assign[i] >= 0) continue;
                while (j < N && owner[j] >= 0) ++j;
                if (j < N) { assign[i] = j; owner[j] = i; ++j; }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < N; i += nt) {
        int a = assign[i];
        if ((unsigned)a >= (unsigned)N) a = 0;                               // unreachable: assign is a bijection here
        assignment[base + i] = a;
        dist[base + i] = sqdist3(ax[i], ay[i], az[i], bx[a], by[a], bz[a]);
    }
    if (tid == 0) {
        info[blockIdx.x] = capped ? -rounds : rounds;
        if (evals) evals[blockIdx.x] = bids;
    }
}

// ---- one wave per pair (N <= 64): the Stage-I loss regime, thousands of group patches of 32 points --------------------------------------------
// Lane j < N holds object j (xyz2[j], price[j], owner[j]) and, as lane i, the coordinates of bidder i; everything lives in registers: no LDS is
// allocated, there is no barrier and no atomic (the cross-lane traffic is DPP, readlane and, once at the end, a bpermute).  Lanes >= N hold
// price = +inf, so their value d + price is +inf and they never win.  Gauss-Seidel: ONE bid at a time, by the lowest unassigned bidder.  The set
// of unassigned bidders is what a ballot over assign[i] < 0 would return; it is kept as that 64-bit mask in scalar registers and updated with
// the (wave-uniform) bidder and evicted owner, so the bidder index is uniform and its coordinates are three readlanes.
// Costs and values are rounded exactly as in emd_auction_kernel (sqdist3, one __fadd_rn): tests/emd_wave_ref.py restates the solve bit for bit.
__global__ __launch_bounds__(256) void emd_wave_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2, int B, int N,
                                                       float eps_final, float eps_rel, int max_bids, float* __restrict__ dist,
                                                       int32_t* __restrict__ assignment, int32_t* __restrict__ info,
                                                       float* __restrict__ eps_used_out) {
    const int lane = threadIdx.x & 63;
    const long long pair = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pair >= B) return;                                                   // wave-uniform: the ragged last workgroup
    const size_t base = (size_t)pair * N;
    const float INF = __builtin_inff();
    const bool valid = lane < N;

    float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
    if (valid) {
        const float* p = xyz1 + (base + lane) * 3; ax = p[0]; ay = p[1]; az = p[2];
        const float* q = xyz2 + (base + lane) * 3; bx = q[0]; by = q[1]; bz = q[2];
    }
    float price = valid ? 0.f : INF;

    // max_ij d_ij (exact, any order); NaN costs are dropped by fmaxf as in emd_auction_kernel
    float dmax = 0.f;
    for (int i = 0; i < N; ++i) {
        const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ax), i));
        const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ay), i));
        const float z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(az), i));
        dmax = fmaxf(dmax, sqdist3(x, y, z, bx, by, bz));
    }
    dmax = wave_max_f32(valid ? dmax : 0.f, -1.f);
    const float eps_used = fmaxf(eps_final, __fmul_rn(eps_rel, dmax));
    float eps = eps_used;
    {
        const float first = dmax * 0.25f;
        for (int k = 0; k < 64 && eps < first; ++k) eps *= EMD_THETA;
    }

    const emd_u64 all = N >= 64 ? ~0ull : ((1ull << N) - 1ull);
    emd_u64 un = all;                                                        // bit i: bidder i is unassigned
    int owner = -1, bids = 0;
    bool capped = false;
    for (;;) {                                                               // one phase: everything unassigned, prices kept
        un = all; owner = -1;
        while (un) {
            if (bids >= max_bids) { capped = true; break; }
            ++bids;
            const int i = first_lane(un);
            const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ax), i));
            const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ay), i));
            const float z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(az), i));
            const float u = __fadd_rn(sqdist3(x, y, z, bx, by, bz), price);  // lanes >= N: +inf
            const float m1 = wave_min_f32(u, INF);
            const emd_u64 eq = __ballot(valid && u == m1);
            const int jb = eq ? first_lane(eq) : 0;                          // nothing compares equal (NaN coordinates): any object, the cap ends it
            const float m2 = wave_min_f32(lane == jb ? INF : u, INF);        // best of everything else; +inf when N == 1
            const float p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(price), jb));
            float bid = m2 < INF ? __fadd_rn(__fadd_rn(p, __fsub_rn(m2, m1)), eps) : __fadd_rn(p, eps);
            if (!(bid > p)) bid = __int_as_float(__float_as_int(p) + 1);     // eps below half an ulp of the price: still strictly up
            const int prev = __builtin_amdgcn_readlane(owner, jb);
            price = lane == jb ? bid : price;
            owner = lane == jb ? i : owner;
            un &= ~(1ull << i);
            if (prev >= 0) un |= 1ull << prev;
        }
        if (capped || !(eps > eps_used)) break;
        eps = fmaxf(eps / EMD_THETA, eps_used);
    }

    if (capped) {                                                            // unassigned bidders take the free objects, both ascending
        emd_u64 fr = all & ~__ballot(owner >= 0);
        while (un && fr) {
            const int i = first_lane(un), j = first_lane(fr);
            owner = lane == j ? i : owner;
            un &= un - 1; fr &= fr - 1;
        }
    }
    // object lane j writes the row of its owner: dist[owner] = d(owner, j), assignment[owner] = j (owner is a bijection here)
    const int src = (unsigned)owner < (unsigned)N ? owner : 0;
    const float ox = __shfl(ax, src, 64), oy = __shfl(ay, src, 64), oz = __shfl(az, src, 64);
    if (valid && (unsigned)owner < (unsigned)N) {
        assignment[base + owner] = lane;
        dist[base + owner] = sqdist3(ox, oy, oz, bx, by, bz);
    }
    if (lane == 0) {
        info[pair] = capped ? -bids : bids;
        if (eps_used_out) eps_used_out[pair] = eps_used;
    }
}

__global__ __launch_bounds__(256) void emd_bwd_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                      const int32_t* __restrict__ assignment, const float* __restrict__ g, long long total,
                                                      int N, float* __restrict__ gx1, float* __restrict__ gx2) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long b = t / N;
    const int a = assignment[t];
    const bool ok = (unsigned)a < (unsigned)N;
    const float* p = xyz1 + t * 3;
    const float* q = xyz2 + (b * N + (ok ? a : 0)) * 3;
    const float gi = g[t];
    const float rx = ok ? __fmul_rn(__fmul_rn(2.0f, __fsub_rn(p[0], q[0])), gi) : 0.f;
    const float ry = ok ? __fmul_rn(__fmul_rn(2.0f, __fsub_rn(p[1], q[1])), gi) : 0.f;
    const float rz = ok ? __fmul_rn(__fmul_rn(2.0f, __fsub_rn(p[2], q[2])), gi) : 0.f;
    float* o = gx1 + t * 3; o[0] = rx; o[1] = ry; o[2] = rz;
    if (ok) { float* r = gx2 + (b * N + a) * 3; r[0] = -rx; r[1] = -ry; r[2] = -rz; }
}

extern "C" int act_emd_max_points(void) { return EMD_MAX_POINTS; }

extern "C" int act_emd_fwd_ex_f32(const float* xyz1, const float* xyz2, int B, int N, float eps_final, int max_rounds, float* dist,
                                  int32_t* assignment, int32_t* info, uint64_t* evals, act_stream_t stream) {
    if (B == 0) return 0;
    if (!xyz1 || !xyz2 || !dist || !assignment || !info) return ACT_E_NULLPTR;
    if (B < 0 || N <= 0 || N > EMD_MAX_POINTS || !(eps_final > 0.f) || __builtin_isinf(eps_final) || max_rounds < 1) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t smem = EMD_HDR + (size_t)EMD_BYTES_PER_POINT * N;
    const int threads = N > 1024 ? 1024 : N > 256 ? 512 : 256;
    if (smem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(emd_auction_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(emd_auction_kernel, dim3(B), dim3(threads), smem, s, xyz1, xyz2, N, eps_final, max_rounds, dist, assignment, info,
                       reinterpret_cast<emd_u64*>(evals));
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" int act_emd_fwd_f32(const float* xyz1, const float* xyz2, int B, int N, float eps_final, int max_rounds, float* dist,
                               int32_t* assignment, int32_t* info, act_stream_t stream) {
    return act_emd_fwd_ex_f32(xyz1, xyz2, B, N, eps_final, max_rounds, dist, assignment, info, nullptr, stream);
}

extern "C" int act_emd_wave_max_points(void) { return EMD_WAVE_MAX_POINTS; }

extern "C" int act_emd_wave_fwd_f32(const float* xyz1, const float* xyz2, int B, int N, float eps_final, float eps_rel, int max_bids,
                                    float* dist, int32_t* assignment, int32_t* info, float* eps_used, act_stream_t stream) {
    if (B == 0) return 0;
    if (!xyz1 || !xyz2 || !dist || !assignment || !info) return ACT_E_NULLPTR;
    if (B < 0 || N <= 0 || N > EMD_WAVE_MAX_POINTS || !(eps_final > 0.f) || __builtin_isinf(eps_final) || !(eps_rel >= 0.f) ||
        __builtin_isinf(eps_rel) || max_bids < 1) return ACT_E_BADARG;
    const long long blocks = ((long long)B + 3) / 4;                         // four waves, four pairs, per workgroup
    if (blocks > 0x7fffffffLL) return ACT_E_BADARG;
    hipLaunchKernelGGL(emd_wave_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xyz1, xyz2, B, N, eps_final, eps_rel,
                       max_bids, dist, assignment, info, eps_used);
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" int act_emd_bwd_f32(const float* xyz1, const float* xyz2, const int32_t* assignment, const float* grad_dist, int B, int N,
                               float* gx1, float* gx2, act_stream_t stream) {
    if (B == 0) return 0;
    if (!xyz1 || !xyz2 || !assignment || !grad_dist || !gx1 || !gx2) return ACT_E_NULLPTR;
    if (B < 0 || N <= 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)B * N;
    if ((total + 255) / 256 > 0x7fffffffLL) return ACT_E_BADARG;
    hipError_t e = hipMemsetAsync(gx2, 0, (size_t)total * 3 * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(emd_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, xyz1, xyz2, assignment, grad_dist, total, N,
                       gx1, gx2);
    ACT_LAUNCH_CHECK();
    return 0;
}
