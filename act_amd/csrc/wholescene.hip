// wholescene.hip -- S3DIS whole-room sliding-window testing (semantic_segmentation/main_test.py, dataset.py ScannetDatasetWholeScene): block
// membership, keyed row-index build (fill + shuffle), gather + centre, voting, and the per-room finish (arg-max of the votes, confusion matrix).
//
// Membership is exactly the reference's np.where: a point is in block (ix, iy) iff lo_x <= x <= hi_x and lo_y <= y <= hi_y, the thresholds
// computed on the host in the room file's dtype and compared here in float64 (a float32 threshold and a float32 coordinate promote exactly).
// The block intervals of one axis are non-decreasing in the block index (every operation that forms them is monotone), so the blocks of a point
// are a product of two index ranges found by binary search: one O(P log grid) pass, never blocks x points.  Member lists are in increasing point
// order by construction (per-tile counts, scans, ordered writes); no atomics decide an order.  Votes and confusion counts are integer atomics,
// which are exact and order-independent.  Built with -ffp-contract=off.
#include "common.h"
#include "ws_hash.h"

#define WS_C_MAX 64                 // classes per row (vote / finish)
#define WS_TILE_MIN 1024            // points per membership tile (one wave walks its tile in chunks of 64)
#define WS_TILE_CELLS (1ll << 24)   // cap on tiles x blocks of the membership count matrix (int32)
#define WS_MAX_P (1ll << 27)        // points per room (at most 16 blocks per point: member offsets stay int32)

static inline unsigned wcdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

static long long ws_tile(long long P, int nblk) {
    long long tile = WS_TILE_MIN;
    const long long need = (P * (long long)nblk + WS_TILE_CELLS - 1) / WS_TILE_CELLS;
    if (need > tile) tile = (need + 63) / 64 * 64;
    return tile;
}

// ---- block membership ----------------------------------------------------------------------------------------------
// table [gy*gx, 6] float64: lo_x, hi_x, lo_y, hi_y, cx, cy of block iy*gx + ix.  The x intervals are those of row 0, the y intervals those of
// column 0.  -> the blocks of (x, y) are [ax, bx] x [ay, by] (empty when ax > bx or ay > by; NaN coordinates belong to none).
__device__ __forceinline__ void ws_ranges(const double* __restrict__ tab, int gx, int gy, double x, double y, int& ax, int& bx, int& ay, int& by) {
    int lo = 0, hi = gx;                                                    // first ix with hi_x >= x
    while (lo < hi) { const int m = (lo + hi) >> 1; if (tab[(size_t)m * 6 + 1] >= x) hi = m; else lo = m + 1; }
    ax = lo;
    lo = 0; hi = gx;                                                        // first ix with lo_x > x
    while (lo < hi) { const int m = (lo + hi) >> 1; if (!(tab[(size_t)m * 6 + 0] <= x)) hi = m; else lo = m + 1; }
    bx = lo - 1;
    lo = 0; hi = gy;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (tab[(size_t)m * gx * 6 + 3] >= y) hi = m; else lo = m + 1; }
    ay = lo;
    lo = 0; hi = gy;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (!(tab[(size_t)m * gx * 6 + 2] <= y)) hi = m; else lo = m + 1; }
    by = lo - 1;
}

// One wave per tile of `tile` points, walked in chunks of 64 (lane = point, increasing).  For every block K of a lane: rank = lanes below it
// that are in K, last = no lane above it is in K.  MODE 0 (count): the last lane adds rank + 1 to cur[t][K].  MODE 1 (write): member position
// off[K] + cur[t][K] + rank, then (after a barrier) the last lane advances cur[t][K].  The tile owns row t of cur, so no atomics are needed; the barrier between
// chunks orders the row's updates (workgroup-scope fence).
template <int MODE>
__global__ __launch_bounds__(64) void ws_member_kernel(const double* __restrict__ xyz, long long P, const double* __restrict__ tab, int gx, int gy,
                                                       long long tile, int32_t* __restrict__ cur, const int32_t* __restrict__ off,
                                                       int32_t* __restrict__ members) {
    __shared__ int sr[4][64];
    const int lane = threadIdx.x;
    const int nblk = gx * gy;
    int32_t* row = cur + (size_t)blockIdx.x * nblk;
    const long long t0 = (long long)blockIdx.x * tile;
    const long long t1 = min(P, t0 + tile);
    for (long long c0 = t0; c0 < t1; c0 += 64) {
        const long long p = c0 + lane;
        int ax = 1, bx = 0, ay = 1, by = 0;
        if (p < t1) ws_ranges(tab, gx, gy, xyz[p * 3 + 0], xyz[p * 3 + 1], ax, bx, ay, by);
        if (ax > bx || ay > by) { ax = 1; bx = 0; ay = 1; by = 0; }
        sr[0][lane] = ax; sr[1][lane] = bx; sr[2][lane] = ay; sr[3][lane] = by;
        __syncthreads();
        // pass 0 reads the chunk's bases (write mode), pass 1 advances them: lanes walk their blocks in lockstep, so a cursor must not move
        // while another lane may still read it
        for (int pass = MODE == 1 ? 0 : 1; pass < 2; ++pass) {
            for (int ky = ay; ky <= by; ++ky)
                for (int kx = ax; kx <= bx; ++kx) {
                    int rank = 0;
                    bool last = true;
                    for (int j = 0; j < 64; ++j) {
                        const bool in = kx >= sr[0][j] && kx <= sr[1][j] && ky >= sr[2][j] && ky <= sr[3][j];
                        rank += (in && j < lane);
                        last = last && !(in && j > lane);
                    }
                    const int K = ky * gx + kx;
                    if (pass == 0) members[off[K] + row[K] + rank] = (int32_t)p;
                    else if (last) row[K] += rank + 1;
                }
            __syncthreads();
        }
    }
}

// cur [T, nblk] (per-tile counts) -> per-tile exclusive starts within each block, total[b] = the block's count
__global__ __launch_bounds__(256) void ws_tile_scan_kernel(int32_t* __restrict__ cur, int T, int nblk, int32_t* __restrict__ total) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblk) return;
    int run = 0;
    for (int t = 0; t < T; ++t) {
        const int v = cur[(size_t)t * nblk + b];
        cur[(size_t)t * nblk + b] = run;
        run += v;
    }
    total[b] = run;
}

// one workgroup: counts[b] = total[b], off = exclusive scan of total ([nblk + 1])
__global__ __launch_bounds__(1024) void ws_block_scan_kernel(const int32_t* __restrict__ total, int nblk, int32_t* __restrict__ counts,
                                                             int32_t* __restrict__ off) {
    __shared__ int s[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += 1024) {
        const int b = b0 + threadIdx.x;
        const int v = b < nblk ? total[b] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {                                // inclusive Hillis-Steele scan
            const int add = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < nblk) { counts[b] = v; off[b] = carry + s[threadIdx.x] - v; }
        __syncthreads();
        if (threadIdx.x == 1023) carry += s[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) off[nblk] = carry;
}

extern "C" size_t act_scene_member_workspace(long long P, int gx, int gy) {
    if (P <= 0 || gx <= 0 || gy <= 0) return 0;
    const int nblk = gx * gy;
    const long long T = (P + ws_tile(P, nblk) - 1) / ws_tile(P, nblk);
    return (size_t)(T * nblk + nblk) * sizeof(int32_t);
}

static int ws_member_check(const double* xyz, long long P, const double* table, int gx, int gy, void* ws, size_t ws_bytes) {
    if (!xyz || !table || !ws) return ACT_E_NULLPTR;
    if (P <= 0 || P > WS_MAX_P || gx <= 0 || gy <= 0 || (long long)gx * gy > (1 << 20)) return ACT_E_BADARG;
    if (ws_bytes < act_scene_member_workspace(P, gx, gy)) return ACT_E_BADARG;
    return 0;
}

extern "C" int act_scene_member_count(const double* xyz, long long P, const double* table, int gx, int gy, int32_t* counts, int32_t* offsets,
                                      void* ws, size_t ws_bytes, act_stream_t stream) {
    const int rc = ws_member_check(xyz, P, table, gx, gy, ws, ws_bytes);
    if (rc) return rc;
    if (!counts || !offsets) return ACT_E_NULLPTR;
    const int nblk = gx * gy;
    const long long tile = ws_tile(P, nblk);
    const int T = (int)((P + tile - 1) / tile);
    int32_t* cur = (int32_t*)ws;
    int32_t* total = cur + (size_t)T * nblk;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, 24.0 * P + 8.0 * T * nblk + 12.0 * nblk);
    if (hipMemsetAsync(cur, 0, (size_t)T * nblk * sizeof(int32_t), s) != hipSuccess) return ACT_E_BADARG;
    hipLaunchKernelGGL(ws_member_kernel<0>, dim3(T), dim3(64), 0, s, xyz, P, table, gx, gy, tile, cur, (const int32_t*)nullptr, (int32_t*)nullptr);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(ws_tile_scan_kernel, dim3(wcdiv(nblk, 256)), dim3(256), 0, s, cur, T, nblk, total);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(ws_block_scan_kernel, dim3(1), dim3(1024), 0, s, total, nblk, counts, offsets);
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" int act_scene_member_fill(const double* xyz, long long P, const double* table, int gx, int gy, const int32_t* offsets, int32_t* members,
                                     void* ws, size_t ws_bytes, act_stream_t stream) {
    const int rc = ws_member_check(xyz, P, table, gx, gy, ws, ws_bytes);
    if (rc) return rc;
    if (!offsets || !members) return ACT_E_NULLPTR;
    const int nblk = gx * gy;
    const long long tile = ws_tile(P, nblk);
    const int T = (int)((P + tile - 1) / tile);
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, 24.0 * P + 8.0 * T * nblk + 4.0 * 4 * P);
    hipLaunchKernelGGL(ws_member_kernel<1>, dim3(T), dim3(64), 0, s, xyz, P, table, gx, gy, tile, (int32_t*)ws, offsets, members);
    ACT_LAUNCH_CHECK();
    return 0;
}

// ---- keyed row-index build ------------------------------------------------------------------------------------------
// ws_mix32 (lowbias32 mixer) and ws_feistel (keyed bijection of [0, n)) live in ws_hash.h; every key and draw below is a function of
// (seed, room, vote, block, position) only.
// rows [R] (blocks back to back, block s at [roff[s], roff[s+1]), point_size = roff[s+1] - roff[s]): position j of block s holds
// pre[perm(j)], pre = the block's members followed by pad = point_size - cnt fills.  Fills: the first pad outputs of a keyed bijection of
// [0, cnt) when pad <= cnt (without replacement, dataset.py's rule), else hi32(h * cnt) of a 32-bit hash h per fill (with replacement; each
// member gets floor or ceil of 2^32 / cnt hash values: relative bias below cnt / 2^32).
__global__ __launch_bounds__(256) void ws_rows_kernel(const int32_t* __restrict__ members, const int32_t* __restrict__ moff,
                                                      const int32_t* __restrict__ bid, const int32_t* __restrict__ roff, int nb, long long R,
                                                      uint32_t seed, uint32_t room, uint32_t vote, int32_t* __restrict__ rows) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int lo = 0, hi = nb;                                                    // block s: roff[s] <= r < roff[s+1]
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (roff[m] <= r) lo = m; else hi = m; }
    const int s = lo, b = bid[s];
    const uint32_t j = (uint32_t)(r - roff[s]);
    const uint32_t ps = (uint32_t)(roff[s + 1] - roff[s]);
    const int32_t m0 = moff[b];
    const uint32_t cnt = (uint32_t)(moff[b + 1] - m0);
    const uint32_t pad = ps - cnt;
    uint32_t k = ws_mix32(seed ^ 0x243f6a88u);
    k = ws_mix32(k ^ room);
    k = ws_mix32(k ^ vote);
    k = ws_mix32(k ^ (uint32_t)b);
    const uint32_t i = ws_feistel(j, ps, ws_mix32(k ^ 1u));
    uint32_t m;
    if (i < cnt) m = i;
    else if (pad <= cnt) m = ws_feistel(i - cnt, cnt, ws_mix32(k ^ 2u));
    else m = (uint32_t)(((uint64_t)ws_mix32(ws_mix32(i - cnt) ^ ws_mix32(k ^ 3u)) * cnt) >> 32);
    rows[r] = members[m0 + m];
}

extern "C" int act_scene_rows(const int32_t* members, const int32_t* member_off, const int32_t* block_ids, const int32_t* row_off, int nb,
                              long long R, int block_points, unsigned seed, unsigned room, unsigned vote, int32_t* rows, act_stream_t stream) {
    if (!members || !member_off || !block_ids || !row_off || !rows) return ACT_E_NULLPTR;
    if (nb <= 0 || R <= 0 || block_points <= 0 || R % block_points || R > (1ll << 31) - 1) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, 8.0 * R);
    hipLaunchKernelGGL(ws_rows_kernel, dim3(wcdiv(R, 256)), dim3(256), 0, s, members, member_off, block_ids, row_off, nb, R, (uint32_t)seed,
                       (uint32_t)room, (uint32_t)vote, rows);
    ACT_LAUNCH_CHECK();
    return 0;
}

// ---- gather and centre ----------------------------------------------------------------------------------------------
// out [R, 3] float32 = (x - cx, y - cy, z) of point rows[r], cx / cy of the row's block, in float64 and rounded once (dataset.py's float32 or
// float64 arithmetic, then main_test.py's float32 tensor: one rounding either way -- a float32 difference computed in float64 is exact-then-round).
__global__ __launch_bounds__(256) void ws_gather_kernel(const double* __restrict__ xyz, const double* __restrict__ tab, const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ bid, const int32_t* __restrict__ roff, int nb, long long R,
                                                        long long P, float* __restrict__ out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int lo = 0, hi = nb;
    while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (roff[m] <= r) lo = m; else hi = m; }
    const double* t = tab + (size_t)bid[lo] * 6;
    const long long p = rows[r];
    if (p < 0 || p >= P) { out[r * 3 + 0] = out[r * 3 + 1] = out[r * 3 + 2] = NAN; return; }   // not a point of the room
    out[r * 3 + 0] = (float)(xyz[p * 3 + 0] - t[4]);
    out[r * 3 + 1] = (float)(xyz[p * 3 + 1] - t[5]);
    out[r * 3 + 2] = (float)xyz[p * 3 + 2];
}

extern "C" int act_scene_gather(const double* xyz, long long P, const double* table, const int32_t* rows, const int32_t* block_ids,
                                const int32_t* row_off, int nb, long long R, float* out, act_stream_t stream) {
    if (!xyz || !table || !rows || !block_ids || !row_off || !out) return ACT_E_NULLPTR;
    if (P <= 0 || nb <= 0 || R <= 0) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, R * (4.0 + 24.0 + 12.0));
    hipLaunchKernelGGL(ws_gather_kernel, dim3(wcdiv(R, 256)), dim3(256), 0, s, xyz, table, rows, block_ids, row_off, nb, R, P, out);
    ACT_LAUNCH_CHECK();
    return 0;
}

// ---- vote -----------------------------------------------------------------------------------------------------------
// one lane per row (rows outside [0, P) skipped): arg-max of the row's C log-probs (ties and NaN as CPU torch max: the first maximum, a NaN wins), then votes[point, class]
// += 1 when labelweights[label[point]] is non-zero and not infinite (main_test.py add_vote; labels outside [0, C) do not vote).
__global__ __launch_bounds__(256) void ws_vote_kernel(const float* __restrict__ logp, const int32_t* __restrict__ rows, long long n, long long P, int C,
                                                      const int32_t* __restrict__ label, const float* __restrict__ lw, int32_t* __restrict__ votes) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const long long p = rows[r];
    if (p < 0 || p >= P) return;
    const int l = label[p];
    if (l < 0 || l >= C) return;
    const float w = lw[l];
    if (w == 0.0f || isinf(w)) return;
    const float* z = logp + r * C;
    float best = z[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float v = z[c];
        if (!isnan(best) && (v > best || isnan(v))) { best = v; arg = c; }
    }
    atomicAdd(&votes[p * C + arg], 1);
}

extern "C" int act_scene_vote(const float* logp, const int32_t* rows, long long n, long long P, int C, const int32_t* label, const float* labelweights,
                              int32_t* votes, act_stream_t stream) {
    if (!logp || !rows || !label || !labelweights || !votes) return ACT_E_NULLPTR;
    if (n <= 0 || P <= 0 || C <= 0 || C > WS_C_MAX) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, n * (4.0 * C + 4.0 + 4.0 + 4.0));
    hipLaunchKernelGGL(ws_vote_kernel, dim3(wcdiv(n, 256)), dim3(256), 0, s, logp, rows, n, P, C, label, labelweights, votes);
    ACT_LAUNCH_CHECK();
    return 0;
}

// ---- finish ---------------------------------------------------------------------------------------------------------
// pred[p] = arg-max of votes[p, :] (ties: lowest class; no votes: class 0, as np.argmax); cm [C, C] int64 += (label, pred) counts, points with a
// label outside [0, C) skipped.  Counts gather in an LDS histogram per workgroup and reach cm with one integer atomic per non-zero bin.
#define WS_FINISH_GRID 512
__global__ __launch_bounds__(256) void ws_finish_kernel(const int32_t* __restrict__ votes, const int32_t* __restrict__ label, long long P, int C,
                                                        int32_t* __restrict__ pred, unsigned long long* __restrict__ cm) {
    __shared__ unsigned int hist[WS_C_MAX * WS_C_MAX];
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        const int32_t* v = votes + p * C;
        int best = v[0], arg = 0;
        for (int c = 1; c < C; ++c)
            if (v[c] > best) { best = v[c]; arg = c; }
        pred[p] = arg;
        const int l = label[p];
        if (cm && l >= 0 && l < C) atomicAdd(&hist[l * C + arg], 1u);
    }
    __syncthreads();
    if (cm)
        for (int i = threadIdx.x; i < C * C; i += blockDim.x)
            if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
}

extern "C" int act_scene_finish(const int32_t* votes, const int32_t* label, long long P, int C, int32_t* pred, int64_t* cm, act_stream_t stream) {
    if (!votes || !label || !pred) return ACT_E_NULLPTR;
    if (P <= 0 || C <= 0 || C > WS_C_MAX) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, P * (4.0 * C + 4.0 + 4.0));
    const unsigned grid = wcdiv(P, 256) < WS_FINISH_GRID ? wcdiv(P, 256) : WS_FINISH_GRID;
    hipLaunchKernelGGL(ws_finish_kernel, dim3(grid), dim3(256), 0, s, votes, label, P, C, pred, reinterpret_cast<unsigned long long*>(cm));
    ACT_LAUNCH_CHECK();
    return 0;
}
