// sa.hip -- PointNet++ set abstraction (reference: {part,semantic}_segmentation/models/pointnet2_utils.py:84-155; upstream pointnet2_ops
// ball_query / group_points): radius search that keeps the first nsample hits in index order, the fused gather that writes the grouped rows
// in the row-major layout the row GEMMs read, and the deterministic backward of that gather over an inverse adjacency.
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
