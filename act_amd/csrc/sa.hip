// sa.hip -- PointNet++ set abstraction (reference: {part,semantic}_segmentation/models/pointnet2_utils.py:84-155; upstream pointnet2_ops
// ball_query / group_points): radius search that keeps the first nsample hits in index order, the fused gather that writes the grouped rows
// in the row-major layout the row GEMMs read, and the deterministic backward of that gather over an inverse adjacency; and the library's one
// three-NN feature propagation (PointNet++ networks and the Transformer segmentation head): search, inverse adjacency, row interpolation.
//
// Conventions: distances are the DIFFERENCE form (dx*dx + dy*dy) + dz*dz in fp32, never contracted (file built with -ffp-contract=off, and
// sqdist3 rounds every product and sum); radius^2 is the fp32 product of the fp32 radius, as in upstream's kernel.  No float atomics and no
// atomics at all: the adjacency lists are a function of idx alone and every sum runs in ascending (s, j) order, so the backward is
// bit-identical from run to run.
#include "common.h"

static inline unsigned cdiv(long long a, int b) { return (unsigned)((a + b - 1) / b); }

// ---- ball query -------------------------------------------------------------------------------------------------------------------------
// One wave per query, SA_BQ_WAVES queries per workgroup.  The cloud is staged in LDS in chunks of SA_BQ_CHUNK points (x | y | z planes: lane l
// of a wave reads word base + l of a plane, conflict-free) and every wave walks the chunk 64 points per step: one distance per lane, a ballot
// of the hits, and the lane prefix count of the ballot gives every hit its output slot -- the output order is the index order with no sort.
// A wave stops walking once nsample hits are out; the workgroup stops staging once all its waves have.
#define SA_BQ_WAVES 4
#define SA_BQ_CHUNK 1024
#define SA_BQ_PAD 11            // plane stride CHUNK + 11: the AoS -> plane scatter of the staging (words 3p+c -> plane c, slot p) spreads over the banks

template <bool INCLUSIVE>
__global__ __launch_bounds__(SA_BQ_WAVES * 64) void ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ qxyz, int N, int S,
                                                                      float r2, int nsample, int32_t* __restrict__ idx,
                                                                      int32_t* __restrict__ cnt_out) {
    __shared__ float sp[3 * (SA_BQ_CHUNK + SA_BQ_PAD)];
    __shared__ int sdone[SA_BQ_WAVES];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * SA_BQ_WAVES + wave;
    const bool live = s < S;                                             // wave-uniform
    const float* xb = xyz + (size_t)b * N * 3;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
        const float* q = qxyz + ((size_t)b * S + s) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    int32_t* out = idx + ((size_t)b * S + (live ? s : 0)) * nsample;
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0, first = 0;
    bool done = !live;
    for (int c0 = 0; c0 < N; c0 += SA_BQ_CHUNK) {
        const int m = min(SA_BQ_CHUNK, N - c0);
        if (lane == 0) sdone[wave] = done;
        __syncthreads();                                                 // the previous chunk has been read; the flags are visible
        bool all = true;
#pragma unroll
        for (int w = 0; w < SA_BQ_WAVES; ++w) all = all && (sdone[w] != 0);
        if (all) break;                                                  // block-uniform
        for (int e = threadIdx.x; e < 3 * m; e += SA_BQ_WAVES * 64) {
            const int p = e / 3, c = e - 3 * p;
            sp[c * (SA_BQ_CHUNK + SA_BQ_PAD) + p] = xb[(size_t)c0 * 3 + e];
        }
        __syncthreads();
        if (!done) {
            for (int p0 = 0; p0 < m; p0 += 64) {
                const int p = p0 + lane;
                bool hit = false;
                if (p < m) {
                    const float d2 = sqdist3(qx, qy, qz, sp[p], sp[(SA_BQ_CHUNK + SA_BQ_PAD) + p], sp[2 * (SA_BQ_CHUNK + SA_BQ_PAD) + p]);
                    hit = INCLUSIVE ? (d2 <= r2) : (d2 < r2);
                }
                const unsigned long long mask = __ballot(hit);
                if (mask) {
                    if (cnt == 0) first = c0 + p0 + first_lane(mask);
                    const int pos = cnt + __popcll(mask & below);
                    if (hit && pos < nsample) out[pos] = c0 + p;
                    cnt += __popcll(mask);
                    if (cnt >= nsample) { done = true; break; }          // wave-uniform
                }
            }
        }
    }
    if (!live) return;
    const int kept = min(cnt, nsample);
    for (int j = kept + lane; j < nsample; j += 64) out[j] = first;      // no hit: first == 0, the row of zeros upstream leaves
    if (cnt_out && lane == 0) cnt_out[(size_t)b * S + s] = kept;
}

extern "C" int act_ball_query_f32(const float* xyz, const float* new_xyz, int B, int N, int S, float radius, int nsample, int inclusive,
                                  int32_t* idx, int32_t* cnt, act_stream_t stream) {
    if (!xyz || !new_xyz || !idx) return ACT_E_NULLPTR;
    if (B <= 0 || B > 65535 || N <= 0 || S <= 0 || nsample <= 0 || !(radius >= 0.f)) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const float r2 = radius * radius;
    ActProfScope ps(KID_KNN_GROUP, s, 9.0 * B * (double)S * N, 4.0 * B * ((double)cdiv(S, SA_BQ_WAVES) * N * 3 + (double)S * (nsample + 4)));
    if (inclusive)
        hipLaunchKernelGGL(ball_query_kernel<true>, dim3(cdiv(S, SA_BQ_WAVES), B), dim3(SA_BQ_WAVES * 64), 0, s, xyz, new_xyz, N, S, r2, nsample,
                           idx, cnt);
    else
        hipLaunchKernelGGL(ball_query_kernel<false>, dim3(cdiv(S, SA_BQ_WAVES), B), dim3(SA_BQ_WAVES * 64), 0, s, xyz, new_xyz, N, S, r2, nsample,
                           idx, cnt);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- grouped rows: forward ------------------------------------------------------------------------------------------------------------------
// rows[(b*S + s)*ns + j, :] = (xyz[b, i] - new_xyz[b, s] if use_xyz) | feat[b, i, :], i = idx[b, s, j]; one row per wave, 4 rows per block.
// An index outside [0, N) writes a row of zeros (never read out of the cloud).
__global__ __launch_bounds__(256) void group_rows_fwd_kernel(const float* __restrict__ xyz, const float* __restrict__ qxyz, const float* __restrict__ feat,
                                                             const int32_t* __restrict__ idx, int N, int S, int ns, int D, int X, long long R,
                                                             float* __restrict__ rows) {
    const long long r = (long long)blockIdx.x * 4 + threadIdx.y;
    if (r >= R) return;
    const int C = X + D;
    const long long bs = r / ns, b = bs / S;
    const int i = idx[r];
    float* o = rows + r * C;
    if ((unsigned)i >= (unsigned)N) {
        for (int c = threadIdx.x; c < C; c += 64) o[c] = 0.f;
        return;
    }
    const long long p = b * N + i;
    if ((int)threadIdx.x < X) o[threadIdx.x] = __fsub_rn(xyz[p * 3 + threadIdx.x], qxyz[bs * 3 + threadIdx.x]);
    const float* f = feat + p * D;
    for (int c = threadIdx.x; c < D; c += 64) o[X + c] = f[c];
}

extern "C" int act_group_rows_fwd_f32(const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx, int B, int N, int S,
                                      int nsample, int D, int use_xyz, float* rows, act_stream_t stream) {
    if (!idx || !rows) return ACT_E_NULLPTR;
    if (use_xyz && (!xyz || !new_xyz)) return ACT_E_NULLPTR;
    if (D > 0 && !feat) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || S <= 0 || nsample <= 0 || D < 0 || (!use_xyz && D == 0)) return ACT_E_BADARG;
    const long long R = (long long)B * S * nsample;
    if ((R + 3) / 4 > 0x7fffffffLL) return ACT_E_BADARG;
    const int X = use_xyz ? 3 : 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ROW_GATHER, s, 0.0, 4.0 * R * (2.0 * (X + D) + 1));
    hipLaunchKernelGGL(group_rows_fwd_kernel, dim3(cdiv(R, 4)), dim3(64, 4), 0, s, xyz, new_xyz, feat, idx, N, S, nsample, D, X, R, rows);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- inverse adjacency of idx [B, E] (E = S * nsample) over the N points of every cloud ---------------------------------------------------------
// A counting sort without atomics.  Block (x, b) owns the points [256 x, 256 x + 256) of cloud b, one per thread.  The entries are staged in
// chunks of SA_ADJ_CHUNK; the ones that fall into the block's range are compacted IN ORDER (ballot + lane prefix inside each 64-entry segment,
// the 32 segment counts of a chunk prefixed in LDS), and every thread scans the compacted list for its own point -- 256 compares per entry
// instead of N.  Pass 1 counts, an exclusive scan per cloud gives the offsets, pass 2 repeats the walk and lists the entries of every point
// in increasing e.  Entries outside [0, N) belong to no point.
#define SA_ADJ_CHUNK 2048
#define SA_ADJ_SEGS (SA_ADJ_CHUNK / 64)
template <bool FILL>
__global__ __launch_bounds__(256) void group_adj_kernel(const int32_t* __restrict__ idx, int N, int E, int32_t* __restrict__ off,
                                                        int32_t* __restrict__ ent) {
    __shared__ int32_t ckey[SA_ADJ_CHUNK];
    __shared__ int32_t cent[SA_ADJ_CHUNK];
    __shared__ int32_t scnt[SA_ADJ_SEGS];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n0 = blockIdx.x * 256, n = n0 + t;
    const int32_t* ib = idx + (size_t)b * E;
    int32_t* ob = off + (size_t)b * (N + 1);
    int32_t* eb = FILL ? ent + (size_t)b * E : nullptr;
    const unsigned long long below = (1ull << lane) - 1ull;
    int acc = (FILL && n < N) ? ob[n] : 0;                             // FILL: write cursor; else: count
    for (int e0 = 0; e0 < E; e0 += SA_ADJ_CHUNK) {
        const int m = min(SA_ADJ_CHUNK, E - e0);
        int key[SA_ADJ_CHUNK / 256], pre[SA_ADJ_CHUNK / 256];
        __syncthreads();                                                 // the previous chunk's lists have been scanned
#pragma unroll
        for (int k = 0; k < SA_ADJ_CHUNK / 256; ++k) {
            const int i = k * 256 + t;
            const int v = i < m ? ib[e0 + i] - n0 : -1;
            const bool in = (unsigned)v < 256u && v + n0 < N;
            const unsigned long long mask = __ballot(in);
            key[k] = in ? v : -1;
            pre[k] = __popcll(mask & below);
            if (lane == 0) scnt[k * 4 + wave] = __popcll(mask);
        }
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int k = 0; k < SA_ADJ_CHUNK / 256; ++k) {
            const int seg = k * 4 + wave;
            int base = 0;
            for (int q = 0; q < seg; ++q) base += scnt[q];
            if (key[k] >= 0) { ckey[base + pre[k]] = key[k]; cent[base + pre[k]] = e0 + k * 256 + t; }
        }
        for (int q = 0; q < SA_ADJ_SEGS; ++q) total += scnt[q];
        __syncthreads();
        if (n < N) {
            for (int j = 0; j < total; ++j) {
                if (ckey[j] == t) {
                    if (FILL) eb[acc] = cent[j];
                    ++acc;
                }
            }
        }
    }
    if (!FILL && n < N) ob[n] = acc;
}

// in-place exclusive scan of the N counts of every cloud, off[b, N] = total; thread t owns a contiguous range of the cloud
__global__ __launch_bounds__(256) void group_adj_scan_kernel(int N, int32_t* __restrict__ off) {
    __shared__ int part[256];
    int32_t* ob = off + (size_t)blockIdx.x * (N + 1);
    const int per = (N + 255) / 256, lo = min(N, (int)threadIdx.x * per), hi = min(N, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += ob[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int j = 0; j < 256; ++j) { const int v = part[j]; part[j] = acc; acc += v; }
        ob[N] = acc;
    }
    __syncthreads();
    int acc = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { const int v = ob[i]; ob[i] = acc; acc += v; }
}

static size_t adj_bytes(int B, int N, long long E) { return ((size_t)B * ((size_t)N + 1) + (size_t)B * (size_t)E) * sizeof(int32_t); }

static int build_adjacency(const int32_t* idx, int B, int N, int E, int32_t* off, int32_t* ent, hipStream_t s) {
    ActProfScope ps(KID_ELTWISE, s, 0.0, 4.0 * B * (2.0 * cdiv(N, 256) * E + 3.0 * N + E));
    hipLaunchKernelGGL(group_adj_kernel<false>, dim3(cdiv(N, 256), B), dim3(256), 0, s, idx, N, E, off, ent);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_adj_scan_kernel, dim3(B), dim3(256), 0, s, N, off);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(group_adj_kernel<true>, dim3(cdiv(N, 256), B), dim3(256), 0, s, idx, N, E, off, ent);
    ACT_LAUNCH_CHECK();
    return 0;
}

// the same adjacency for the other files of the library (edgeconv.hip); declared in common.h
int act_sa_build_adjacency(const int32_t* idx, int B, int N, int E, int32_t* off, int32_t* ent, hipStream_t s) {
    return build_adjacency(idx, B, N, E, off, ent, s);
}

extern "C" size_t act_group_rows_bwd_workspace(int B, int N, int S, int nsample) {
    if (B <= 0 || N <= 0 || S <= 0 || nsample <= 0) return 0;
    return adj_bytes(B, N, (long long)S * nsample);
}

// ---- grouped rows: backward -----------------------------------------------------------------------------------------------------------------
// dfeat[b, n, :] = sum over the entries e of point n (increasing e = ascending (s, j)) of drows[b*E + e, X : X + D]; one point per wave
__global__ __launch_bounds__(256) void group_rows_bwd_kernel(const float* __restrict__ drows, const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ ent, int N, int E, int D, int X, long long RN,
                                                             float* __restrict__ dfeat) {
    const long long rn = (long long)blockIdx.x * 4 + threadIdx.y;
    if (rn >= RN) return;
    const long long b = rn / N;
    const int n = (int)(rn - b * N), C = X + D;
    const int32_t* ob = off + b * (N + 1);
    const int32_t* eb = ent + b * E;
    const float* rb = drows + b * (long long)E * C + X;
    const int i0 = ob[n], i1 = ob[n + 1];
    for (int c = threadIdx.x; c < D; c += 64) {
        float acc = 0.f;
        for (int i = i0; i < i1; ++i) acc = __fadd_rn(acc, rb[(long long)eb[i] * C + c]);
        dfeat[rn * D + c] = acc;
    }
}

extern "C" int act_group_rows_bwd_f32(const float* drows, const int32_t* idx, int B, int N, int S, int nsample, int D, int use_xyz, float* dfeat,
                                      void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!drows || !idx || !dfeat || !workspace) return ACT_E_NULLPTR;
    if (B <= 0 || B > 65535 || N <= 0 || S <= 0 || nsample <= 0 || D <= 0) return ACT_E_BADARG;
    const long long E = (long long)S * nsample, RN = (long long)B * N;
    if (E > 0x7fffffffLL || (long long)B * E > 0x7fffffffLL || (RN + 3) / 4 > 0x7fffffffLL) return ACT_E_BADARG;
    if (workspace_bytes < adj_bytes(B, N, E)) return ACT_E_BADARG;
    int32_t* off = reinterpret_cast<int32_t*>(workspace);
    int32_t* ent = off + (size_t)B * (N + 1);
    hipStream_t s = (hipStream_t)stream;
    const int rc = build_adjacency(idx, B, N, (int)E, off, ent, s);
    if (rc) return rc;
    ActProfScope ps(KID_ROW_SCATTER, s, (double)B * E * D, 4.0 * ((double)B * E * (D + 1) + RN * (D + 2.0)));
    hipLaunchKernelGGL(group_rows_bwd_kernel, dim3(cdiv(RN, 4)), dim3(64, 4), 0, s, drows, off, ent, N, (int)E, D, use_xyz ? 3 : 0, RN, dfeat);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- channel-first grouping (upstream group_points): features [B,C,N], idx [B,S,ns] -> out [B,C,S,ns] ---------------------------------------
__global__ __launch_bounds__(256) void group_gather_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx, int C, int N, int E,
                                                           float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const size_t b = blockIdx.z, c = blockIdx.y;
    const int i = idx[b * E + e];
    out[(b * C + c) * E + e] = (unsigned)i < (unsigned)N ? feat[(b * C + c) * N + i] : 0.f;
}

extern "C" int act_group_gather_f32(const float* features, const int32_t* idx, int B, int C, int N, int S, int nsample, float* out,
                                    act_stream_t stream) {
    if (!features || !idx || !out) return ACT_E_NULLPTR;
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || N <= 0 || S <= 0 || nsample <= 0) return ACT_E_BADARG;
    const long long E = (long long)S * nsample;
    if (E > 0x7fffffffLL - 256) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ROW_GATHER, s, 0.0, 4.0 * B * (double)E * (2.0 * C + 1));
    hipLaunchKernelGGL(group_gather_kernel, dim3(cdiv(E, 256), C, B), dim3(256), 0, s, features, idx, C, N, (int)E, out);
    ACT_LAUNCH_CHECK(); return 0;
}

// dfeatures[b, c, n] = sum over the entries e of point n (increasing e) of dout[b, c, e]; one point per lane (coalesced along n)
__global__ __launch_bounds__(256) void group_gather_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ off,
                                                               const int32_t* __restrict__ ent, int C, int N, int E, float* __restrict__ dfeat) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const size_t b = blockIdx.z, c = blockIdx.y;
    const int32_t* ob = off + b * ((size_t)N + 1);
    const int32_t* eb = ent + b * E;
    const float* gb = dout + (b * C + c) * E;
    float acc = 0.f;
    const int i1 = ob[n + 1];
    for (int i = ob[n]; i < i1; ++i) acc = __fadd_rn(acc, gb[eb[i]]);
    dfeat[(b * C + c) * N + n] = acc;
}

extern "C" int act_group_gather_bwd_f32(const float* dout, const int32_t* idx, int B, int C, int N, int S, int nsample, float* dfeatures,
                                        void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!dout || !idx || !dfeatures || !workspace) return ACT_E_NULLPTR;
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || N <= 0 || S <= 0 || nsample <= 0) return ACT_E_BADARG;
    const long long E = (long long)S * nsample;
    if (E > 0x7fffffffLL || (long long)B * E > 0x7fffffffLL) return ACT_E_BADARG;
    if (workspace_bytes < adj_bytes(B, N, E)) return ACT_E_BADARG;
    int32_t* off = reinterpret_cast<int32_t*>(workspace);
    int32_t* ent = off + (size_t)B * (N + 1);
    hipStream_t s = (hipStream_t)stream;
    const int rc = build_adjacency(idx, B, N, (int)E, off, ent, s);
    if (rc) return rc;
    ActProfScope ps(KID_ROW_SCATTER, s, (double)B * E * C, 4.0 * B * ((double)E * (C + 1) + (double)N * (C + 2)));
    hipLaunchKernelGGL(group_gather_bwd_kernel, dim3(cdiv(N, 256), C, B), dim3(256), 0, s, dout, off, ent, C, N, (int)E, dfeatures);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- three-NN feature propagation (reference pointnet2_utils.py:262-312; upstream pointnet2_ops three_nn / three_interpolate) ------------------
// Three nearest known points of every unknown point.  One lane per unknown point; the known cloud streams through LDS in tiles of SA_NN_TILE
// points (every lane reads the same words: broadcast, no bank conflicts), the three best (d2, index) pairs stay in registers: ascending
// (distance, index) order, strict '<' keeps the lower index on ties (the known points are visited in increasing index).
// weight = (1 / (d2 + 1e-8)) / sum of the three.  m < 3: the slots that never fill keep idx 0 and d2 = +inf, so r = 1 / (inf + 1e-8) = 0 and
// their weight is exactly 0 while the others are normalised over what exists (m == 1: r0 / r0 = 1).
#define SA_NN_TILE 1024
__global__ __launch_bounds__(256) void three_nn_kernel(const float* __restrict__ unknown, const float* __restrict__ known, int n, int m,
                                                       int32_t* __restrict__ idx, float* __restrict__ wout, float* __restrict__ d2out) {
    __shared__ float sc[SA_NN_TILE * 3];
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const size_t p = (size_t)b * n + (live ? i : n - 1);               // idle lanes of the last block walk the last point and write nothing
    const float px = unknown[p * 3 + 0], py = unknown[p * 3 + 1], pz = unknown[p * 3 + 2];
    const float* kb = known + (size_t)b * m * 3;
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int t0 = 0; t0 < m; t0 += SA_NN_TILE) {
        const int cnt = min(SA_NN_TILE, m - t0);
        __syncthreads();                                                 // the previous tile has been walked
        for (int j = threadIdx.x; j < cnt * 3; j += 256) sc[j] = kb[(size_t)t0 * 3 + j];
        __syncthreads();
        // one point per step.  (Four points per step behind one compare of their minimum measured 30 - 50 % SLOWER: the branch is per wave,
        // and with 64 lanes some lane has a candidate in almost every group of four, so the wave ran all four insertions almost every time.)
#pragma unroll 4
        for (int g = 0; g < cnt; ++g) {
            const float d = sqdist3(px, py, pz, sc[g * 3 + 0], sc[g * 3 + 1], sc[g * 3 + 2]);
            if (d < d2) {
                const int gi = t0 + g;
                if (d < d1) {
                    d2 = d1; i2 = i1;
                    if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = gi; }
                    else { d1 = d; i1 = gi; }
                } else { d2 = d; i2 = gi; }
            }
        }
    }
    if (!live) return;
    const float r0 = __fdiv_rn(1.0f, __fadd_rn(d0, 1e-8f)), r1 = __fdiv_rn(1.0f, __fadd_rn(d1, 1e-8f)), r2 = __fdiv_rn(1.0f, __fadd_rn(d2, 1e-8f));
    const float s = __fadd_rn(__fadd_rn(r0, r1), r2);
    idx[p * 3 + 0] = i0; idx[p * 3 + 1] = i1; idx[p * 3 + 2] = i2;
    wout[p * 3 + 0] = __fdiv_rn(r0, s); wout[p * 3 + 1] = __fdiv_rn(r1, s); wout[p * 3 + 2] = __fdiv_rn(r2, s);
    if (d2out) { d2out[p * 3 + 0] = d0; d2out[p * 3 + 1] = d1; d2out[p * 3 + 2] = d2; }
}

// The inverse adjacency of idx [B, 3n] over m <= SA_ADJ3_MAX_M known points in ONE launch, one workgroup per cloud: thread g counts the entries
// e = 3i+k with idx[e] == g (pass 1), an exclusive scan over the known points gives the offsets, pass 2 lists the entries of every known point in
// increasing e.  No atomics, and an index outside [0, m) matches no thread that writes: the same off / ent as build_adjacency.
#define SA_ADJ3_MAX_M 256
#define SA_ADJ3_CHUNK 2048
__global__ __launch_bounds__(SA_ADJ3_MAX_M) void three_adj_kernel(const int32_t* __restrict__ idx, int n, int m, int32_t* __restrict__ off,
                                                                   int32_t* __restrict__ ent) {
    __shared__ int32_t chunk[SA_ADJ3_CHUNK];
    __shared__ int32_t cnt[SA_ADJ3_MAX_M + 1];
    const int b = blockIdx.x, g = threadIdx.x, E = 3 * n;
    const int32_t* ib = idx + (size_t)b * E;
    int c = 0;
    for (int e0 = 0; e0 < E; e0 += SA_ADJ3_CHUNK) {
        const int len = min(SA_ADJ3_CHUNK, E - e0);
        __syncthreads();
        for (int i = threadIdx.x; i < len; i += blockDim.x) chunk[i] = ib[e0 + i];
        __syncthreads();
        for (int i = 0; i < len; ++i) c += (chunk[i] == g);
    }
    if (g < m) cnt[g] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int j = 0; j < m; ++j) { const int t = cnt[j]; cnt[j] = acc; acc += t; }
        cnt[m] = acc;
    }
    __syncthreads();
    int32_t* ob = off + (size_t)b * (m + 1);
    if (g < m) ob[g] = cnt[g];
    if (g == 0) ob[m] = cnt[m];
    int pos = g < m ? cnt[g] : 0;
    int32_t* eb = ent + (size_t)b * E;
    for (int e0 = 0; e0 < E; e0 += SA_ADJ3_CHUNK) {
        const int len = min(SA_ADJ3_CHUNK, E - e0);
        __syncthreads();
        for (int i = threadIdx.x; i < len; i += blockDim.x) chunk[i] = ib[e0 + i];
        __syncthreads();
        if (g < m)
            for (int i = 0; i < len; ++i)
                if (chunk[i] == g) eb[pos++] = e0 + i;
    }
}

// off [B,m+1] / ent [B,3n] of idx [B,3n]: the one-launch kernel while a workgroup holds a thread per known point, else the shared builder (three
// launches that spread a cloud's known points over several workgroups).  Both give the same lists, so the choice does not show in the output.
static int three_adjacency(const int32_t* idx, int B, int n, int m, int32_t* off, int32_t* ent, hipStream_t s) {
    if (m > SA_ADJ3_MAX_M) return build_adjacency(idx, B, m, 3 * n, off, ent, s);
    ActProfScope ps(KID_ELTWISE, s, 0.0, 4.0 * B * ((double)n * 6 + m + 1));
    hipLaunchKernelGGL(three_adj_kernel, dim3(B), dim3(SA_ADJ3_MAX_M), 0, s, idx, n, m, off, ent);
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_three_nn_f32(const float* unknown, const float* known, int B, int n, int m, int32_t* idx, float* weight, float* d2,
                                int32_t* adj_off, int32_t* adj_ent, act_stream_t stream) {
    if (!unknown || !known || !idx || !weight) return ACT_E_NULLPTR;
    if ((adj_off == nullptr) != (adj_ent == nullptr)) return ACT_E_NULLPTR;
    if (B <= 0 || B > 65535 || n <= 0 || m <= 0) return ACT_E_BADARG;
    if (3LL * n > 0x7fffffffLL) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    {
        ActProfScope ps(KID_ELTWISE, s, 9.0 * B * (double)n * m, 4.0 * B * ((double)n * 9 + (double)m * 3));
        hipLaunchKernelGGL(three_nn_kernel, dim3(cdiv(n, 256), B), dim3(256), 0, s, unknown, known, n, m, idx, weight, d2);
        ACT_LAUNCH_CHECK();
    }
    return adj_off ? three_adjacency(idx, B, n, m, adj_off, adj_ent, s) : 0;
}

// the inverse adjacency alone, for caller-supplied indices (three_interpolate): off [B,m+1], ent [B,3n]; an index outside [0,m) is in no list
extern "C" int act_three_adj_i32(const int32_t* idx, int B, int n, int m, int32_t* adj_off, int32_t* adj_ent, act_stream_t stream) {
    if (!idx || !adj_off || !adj_ent) return ACT_E_NULLPTR;
    if (B <= 0 || B > 65535 || n <= 0 || m <= 0 || 3LL * n > 0x7fffffffLL) return ACT_E_BADARG;
    return three_adjacency(idx, B, n, m, adj_off, adj_ent, (hipStream_t)stream);
}

// ---- row interpolation ----------------------------------------------------------------------------------------------------------------------
// Y[b*N+n, :] = sum over the slots k with w[n,k] != 0 and idx[n,k] in [0,G) of w[n,k] * P[b*G + idx[n,k], :]  (+ xyz[n] . wxyz[c,:], then + bias[c]),
// the sum in slot order as w0*a, then fma, then fma.  A skipped slot is never read, so a non-finite row behind a weight of exactly 0 cannot
// reach the result.  One row per wave, 4 rows per block; V = float4 when C % 4 == 0 and the rows are 16-byte aligned, else float.
__device__ __forceinline__ float vmul(float w, float v) { return w * v; }
__device__ __forceinline__ float vfma(float w, float v, float a) { return fmaf(w, v, a); }
__device__ __forceinline__ float vadd(float a, float v) { return a + v; }
__device__ __forceinline__ float4 vmul(float w, float4 v) { return make_float4(w * v.x, w * v.y, w * v.z, w * v.w); }
__device__ __forceinline__ float4 vfma(float w, float4 v, float4 a) {
    return make_float4(fmaf(w, v.x, a.x), fmaf(w, v.y, a.y), fmaf(w, v.z, a.z), fmaf(w, v.w, a.w));
}
__device__ __forceinline__ float4 vadd(float4 a, float4 v) { return make_float4(a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w); }
__device__ __forceinline__ float vsel(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ float4 vsel(bool c, float4 a, float4 b) { return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w); }
__device__ __forceinline__ void vzero(float& v) { v = 0.f; }
__device__ __forceinline__ void vzero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
// p . wxyz[c,:] for the channels of lane element c: wc = wxyz + 3 * (first channel)
__device__ __forceinline__ float xyz_dot(float px, float py, float pz, const float* wc) { return fmaf(pz, wc[2], fmaf(py, wc[1], px * wc[0])); }
__device__ __forceinline__ void vxyz(float px, float py, float pz, const float* wc, float& v) { v = xyz_dot(px, py, pz, wc); }
__device__ __forceinline__ void vxyz(float px, float py, float pz, const float* wc, float4& v) {
    v = make_float4(xyz_dot(px, py, pz, wc), xyz_dot(px, py, pz, wc + 3), xyz_dot(px, py, pz, wc + 6), xyz_dot(px, py, pz, wc + 9));
}

template <typename V>
__global__ __launch_bounds__(256) void interp_fwd_kernel(const V* __restrict__ P, const int32_t* __restrict__ idx, const float* __restrict__ w,
                                                         const float* __restrict__ xyz, const float* __restrict__ wxyz,
                                                         const float* __restrict__ bias, int N, int G, int CV, long long R, V* __restrict__ Y) {
    const long long r = (long long)blockIdx.x * 4 + threadIdx.y;        // a one-dimensional grid of row blocks; the wave walks its row's channels
    if (r >= R) return;
    const long long base = (r / N) * G;
    int j[3];
    float wk[3];
    bool live[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        j[k] = idx[r * 3 + k];
        wk[k] = w[r * 3 + k];
        live[k] = wk[k] != 0.f && (unsigned)j[k] < (unsigned)G;
    }
    float px = 0.f, py = 0.f, pz = 0.f;
    if (wxyz) { px = xyz[r * 3 + 0]; py = xyz[r * 3 + 1]; pz = xyz[r * 3 + 2]; }
    for (int c = threadIdx.x; c < CV; c += 64) {
        V y;
        if (live[0] && live[1] && live[2]) {                             // wave-uniform (a wave holds one row): the three loads are in flight together
            const V a = P[(base + j[0]) * CV + c], bb = P[(base + j[1]) * CV + c], cc = P[(base + j[2]) * CV + c];
            y = vfma(wk[2], cc, vfma(wk[1], bb, vmul(wk[0], a)));
        } else {
            vzero(y);
            bool first = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (live[k]) {
                    const V v = P[(base + j[k]) * CV + c];
                    y = first ? vmul(wk[k], v) : vfma(wk[k], v, y);
                    first = false;
                }
            }
        }
        if (wxyz) {
            V t;
            vxyz(px, py, pz, wxyz + (size_t)c * 3 * (sizeof(V) / sizeof(float)), t);
            y = vadd(y, t);
        }
        if (bias) y = vadd(y, reinterpret_cast<const V*>(bias)[c]);
        Y[r * CV + c] = y;
    }
}

static bool vec4_ok(int C, const void* a, const void* b, const void* c = nullptr) {
    return !(C & 3) && !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15);
}

extern "C" int act_interp_rows_fwd_f32(const float* P, const int32_t* idx, const float* weight, const float* xyz, const float* wxyz,
                                       const float* bias, int B, int N, int G, int C, float* Y, act_stream_t stream) {
    if (!P || !idx || !weight || !Y) return ACT_E_NULLPTR;
    if (wxyz && !xyz) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || G <= 0 || C <= 0) return ACT_E_BADARG;
    const long long R = (long long)B * N;
    if (R > (1LL << 27)) return ACT_E_BADARG;                           // 2^25 row blocks of 64 x 4 threads
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 6.0 * R * C, 4.0 * (R * (double)C * 4 + R * 9));
    if (vec4_ok(C, P, Y, bias))
        hipLaunchKernelGGL(interp_fwd_kernel<float4>, dim3(cdiv(R, 4)), dim3(64, 4), 0, s, reinterpret_cast<const float4*>(P), idx,
                           weight, xyz, wxyz, bias, N, G, C / 4, R, reinterpret_cast<float4*>(Y));
    else
        hipLaunchKernelGGL(interp_fwd_kernel<float>, dim3(cdiv(R, 4)), dim3(64, 4), 0, s, P, idx, weight, xyz, wxyz, bias, N, G, C, R, Y);
    ACT_LAUNCH_CHECK(); return 0;
}

// dP[b*G+g, :] = sum over the entries e of known point g (increasing e) with w[e] != 0 of w[e] * dY[b*N + e/3, :].  Entries are bounded by the
// adjacency builder (0 <= e < 3N).
template <typename V>
__global__ __launch_bounds__(256) void interp_bwd_kernel(const V* __restrict__ dY, const int32_t* __restrict__ off, const int32_t* __restrict__ ent,
                                                         const float* __restrict__ w, int N, int G, int CV, int CB, long long RG, V* __restrict__ dP) {
    // grid.x = row blocks x CB channel blocks, the channel blocks of a row block next to each other: neighbouring workgroups read neighbouring
    // pieces of the same dY rows
    const long long rg = (long long)(blockIdx.x / CB) * 4 + threadIdx.y;
    const int c = (blockIdx.x % CB) * 64 + threadIdx.x;
    if (rg >= RG || c >= CV) return;
    const long long b = rg / G;
    const int g = (int)(rg - b * G);
    const int32_t* ob = off + b * ((long long)G + 1);
    const int32_t* eb = ent + b * 3LL * N;
    const float* wb = w + b * 3LL * N;
    const V* yb = dY + b * (long long)N * CV;
    const int e0 = max(ob[g], 0), e1 = min(ob[g + 1], 3 * N);          // a caller's adjacency is never followed out of its arrays
    V acc;
    vzero(acc);
    // no branch in the walk, so that the row loads of several entries are in flight together: an entry outside [0, 3N) reads entry 0 and, like
    // an entry of weight 0, leaves acc as it is.  A wave holds one known point, so the list bounds and the entry are the same in all its
    // lanes: read once per wave, the index arithmetic runs on the scalar unit (measured 203 against 208 us at 32 x 2,048 <- 128, C = 1,536).
    const int s0 = __builtin_amdgcn_readfirstlane(e0), s1 = __builtin_amdgcn_readfirstlane(e1);
    for (int i = s0; i < s1; ++i) {
        const int e = __builtin_amdgcn_readfirstlane(eb[i]);
        const bool in = (unsigned)e < 3u * (unsigned)N;
        const int es = in ? e : 0;
        const float wt = wb[es];
        acc = vsel(in && wt != 0.f, vfma(wt, yb[(long long)(es / 3) * CV + c], acc), acc);
    }
    dP[rg * CV + c] = acc;
}

extern "C" int act_interp_rows_bwd_f32(const float* dY, const int32_t* adj_off, const int32_t* adj_ent, const float* weight, int B, int N, int G,
                                       int C, float* dP, act_stream_t stream) {
    if (!dY || !adj_off || !adj_ent || !weight || !dP) return ACT_E_NULLPTR;
    if (B <= 0 || N <= 0 || G <= 0 || C <= 0 || 3LL * N > 0x7fffffffLL) return ACT_E_BADARG;
    const long long RG = (long long)B * G;
    const bool v4 = vec4_ok(C, dY, dP);
    const int CV = v4 ? C / 4 : C, CB = (CV + 63) / 64;
    if (RG > (1LL << 27) || ((RG + 3) / 4) * CB > 0x7fffffffLL) return ACT_E_BADARG;      // row blocks x channel blocks on grid.x
    const unsigned blocks = (unsigned)(((RG + 3) / 4) * CB);
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 6.0 * B * (double)N * C, 4.0 * ((double)B * N * C * 3 + RG * C + B * (double)N * 6));
    if (v4)
        hipLaunchKernelGGL(interp_bwd_kernel<float4>, dim3(blocks), dim3(64, 4), 0, s, reinterpret_cast<const float4*>(dY), adj_off, adj_ent, weight,
                           N, G, CV, CB, RG, reinterpret_cast<float4*>(dP));
    else
        hipLaunchKernelGGL(interp_bwd_kernel<float>, dim3(blocks), dim3(64, 4), 0, s, dY, adj_off, adj_ent, weight, N, G, CV, CB, RG, dP);
    ACT_LAUNCH_CHECK(); return 0;
}

// ---- gradient of the xyz columns and the bias of the interpolation epilogue (the restructured first propagation conv) ----
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
