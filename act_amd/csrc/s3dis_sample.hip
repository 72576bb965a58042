// s3dis_sample.hip -- S3DIS training blocks sampled on the device from resident rooms (semantic_segmentation/dataset.py:119-147, S3DISDataset.sample_block):
// a random point of the room is the centre of a block_size x block_size column, the column is taken when it holds more than min_points points, and
// num_point of its points are drawn (without replacement when it has that many, with replacement otherwise), x / y centred on the centre.
//
// One launch per batch, one workgroup per item.  The rooms are resident (float64 xyz, all rooms back to back) with a per-room uniform 2-D grid of
// square cells as a CSR (cell_off / cell_pts, cell iy * gx + ix, points ascending inside a cell): cell(v) = clamp(floor((v - o) / c), 0, g - 1) is
// monotone in v, so every point with lo <= v <= hi lies in a cell of [cell(lo), cell(hi)] and an attempt reads those cells only -- the cells
// ix0..ix1 of one grid row are one contiguous range of cell_pts.  Membership is exactly the reference's np.where (float64, both ends inclusive).
// Members are compacted in a fixed order (grid rows ascending, cells ascending, points ascending: ballot + lane prefix count, no atomics) into the
// item's slice of a workspace.  Every draw is a function of (seed, epoch, item id, attempt) through ws_mix32 / ws_feistel, so an item's result
// does not depend on the batch it is sampled in.  Built with -ffp-contract=off.
#include "common.h"
#include "ws_hash.h"

#define SS_THREADS 256
#define SS_WAVES (SS_THREADS / 64)
#define SS_MAX_TRIES (1 << 16)

struct SsArgs {
    const double* xyz; const int32_t* labels; const long long* room_off; int R;
    const double* origin; const long long* dims; const long long* cell_off; const int32_t* cell_pts;
    double half, cell; int min_points, max_tries; long long cap;
    const int32_t *room_ids, *item_ids, *center_in; int num_point; uint32_t seed, epoch;
    float* out_xyz; int64_t* out_labels; int32_t *rows, *count, *center_idx, *info, *ws;
};

__device__ __forceinline__ int ss_cell(double v, double o, double c, int g) {
    double t = floor((v - o) / c);
    const double top = (double)(g - 1);
    if (!(t >= 0.0)) t = 0.0;
    if (t > top) t = top;
    return (int)t;
}

// attempt t's centre: a point index uniform in [0, P) from a 64-bit hash (each point gets floor or ceil of 2^64 / P hash values)
__device__ __forceinline__ long long ss_center(uint32_t k0, uint32_t t, long long P) {
    const uint32_t ka = ws_mix32(k0 ^ ws_mix32(t ^ 0x85a308d3u));
    const unsigned long long h = ((unsigned long long)ws_mix32(ka ^ 1u) << 32) | ws_mix32(ka ^ 2u);
    return (long long)__umul64hi(h, (unsigned long long)P);
}

// The column of centre point ci: counts its members and writes them, in order, to ws[0, min(count, cap)).  Every thread of the workgroup calls it with
// the same arguments and gets the same count.  sw [2][SS_WAVES] holds the per-wave hit counts of a chunk; chunks alternate between its two rows
// (par), so one barrier per chunk is enough: a wave can be at most one chunk ahead of the slowest reader.
__device__ int ss_column(const SsArgs& a, const double* __restrict__ xyz, const long long* __restrict__ coff, double ox, double oy, int gx, int gy,
                         long long ci, int32_t* __restrict__ ws, int (*sw)[SS_WAVES], int& par, double& cx, double& cy) {
    cx = xyz[ci * 3 + 0];
    cy = xyz[ci * 3 + 1];
    const double lox = cx - a.half, hix = cx + a.half, loy = cy - a.half, hiy = cy + a.half;
    const int ix0 = ss_cell(lox, ox, a.cell, gx), ix1 = ss_cell(hix, ox, a.cell, gx);
    const int iy0 = ss_cell(loy, oy, a.cell, gy), iy1 = ss_cell(hiy, oy, a.cell, gy);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int total = 0;
    for (int iy = iy0; iy <= iy1; ++iy) {
        const long long s = coff[(long long)iy * gx + ix0], e = coff[(long long)iy * gx + ix1 + 1];
        for (long long c0 = s; c0 < e; c0 += SS_THREADS) {
            const long long i = c0 + threadIdx.x;
            bool in = false;
            int32_t p = 0;
            if (i < e) {
                p = a.cell_pts[i];
                const double x = xyz[(long long)p * 3 + 0], y = xyz[(long long)p * 3 + 1];
                in = x >= lox && x <= hix && y >= loy && y <= hiy;
            }
            const unsigned long long mask = __ballot(in);
            if (lane == 0) sw[par][wave] = __popcll(mask);
            __syncthreads();
            int pre = total, chunk = 0;
            for (int w = 0; w < SS_WAVES; ++w) {
                const int v = sw[par][w];
                pre += w < wave ? v : 0;
                chunk += v;
            }
            const long long pos = (long long)pre + __popcll(mask & below);
            if (in && pos < a.cap) ws[pos] = p;
            total += chunk;
            par ^= 1;
        }
    }
    __syncthreads();                                                        // the member list is complete (and visible) before anyone reads it
    return total;
}

__global__ __launch_bounds__(SS_THREADS) void ss_sample_kernel(const SsArgs a) {
    __shared__ int sw[2][SS_WAVES];
    const int b = blockIdx.x;
    const size_t o0 = (size_t)b * a.num_point;
    const int room = a.room_ids[b];
    long long P = 0, p0 = 0;
    bool bad = room < 0 || room >= a.R;
    if (!bad) { p0 = a.room_off[room]; P = a.room_off[room + 1] - p0; bad = P <= 0; }
    if (!bad && a.center_in) bad = a.center_in[b] < 0 || a.center_in[b] >= P;
    if (bad) {                                                              // not an item of these rooms (the wrapper refuses it): nothing is read
        for (int j = threadIdx.x; j < a.num_point; j += SS_THREADS) {
            a.out_xyz[(o0 + j) * 3 + 0] = a.out_xyz[(o0 + j) * 3 + 1] = a.out_xyz[(o0 + j) * 3 + 2] = NAN;
            a.out_labels[o0 + j] = -1;
            a.rows[o0 + j] = -1;
        }
        if (threadIdx.x == 0) { a.count[b] = 0; a.center_idx[b] = -1; a.info[b] = 0; }
        return;
    }
    const double* xyz = a.xyz + p0 * 3;
    const int32_t* lab = a.labels + p0;
    const double ox = a.origin[room * 2 + 0], oy = a.origin[room * 2 + 1];
    const int gx = (int)a.dims[room * 3 + 0], gy = (int)a.dims[room * 3 + 1];
    const long long* coff = a.cell_off + a.dims[room * 3 + 2];
    int32_t* ws = a.ws + (size_t)b * a.cap;

    uint32_t k0 = ws_mix32(a.seed ^ 0x13198a2eu);
    k0 = ws_mix32(k0 ^ a.epoch);
    k0 = ws_mix32(k0 ^ (uint32_t)a.item_ids[b]);

    int par = 0, cnt = 0, info = 0;
    long long ci = 0;
    double cx = 0.0, cy = 0.0;
    if (a.center_in) {                                                      // injected centre: no retries, accepted whatever its count
        ci = a.center_in[b];
        cnt = ss_column(a, xyz, coff, ox, oy, gx, gy, ci, ws, sw, par, cx, cy);
        info = 1;
    } else {
        int best_t = 0, best_cnt = -1, t = 0;
        for (; t < a.max_tries; ++t) {
            ci = ss_center(k0, (uint32_t)t, P);
            cnt = ss_column(a, xyz, coff, ox, oy, gx, gy, ci, ws, sw, par, cx, cy);
            if (cnt > a.min_points) break;
            if (cnt > best_cnt) { best_cnt = cnt; best_t = t; }             // largest count, the earliest on ties
        }
        if (t < a.max_tries) info = t + 1;
        else {
            info = -a.max_tries;
            if (best_t != a.max_tries - 1) {                                // the workspace holds the last attempt's members: list the chosen one's again
                ci = ss_center(k0, (uint32_t)best_t, P);
                cnt = ss_column(a, xyz, coff, ox, oy, gx, gy, ci, ws, sw, par, cx, cy);
            }
        }
    }
    if (threadIdx.x == 0) { a.count[b] = cnt; a.center_idx[b] = (int32_t)ci; a.info[b] = info; }

    const uint32_t n = (uint32_t)(cnt < a.cap ? cnt : a.cap);               // (count <= max_window <= cap by the index's construction)
    const uint32_t kperm = ws_mix32(k0 ^ 0x03707344u), krep = ws_mix32(k0 ^ 0xa4093822u);
    for (uint32_t j = threadIdx.x; j < (uint32_t)a.num_point; j += SS_THREADS) {
        if (n == 0) {                                                       // (cannot happen: the centre is a member of its own column)
            a.out_xyz[(o0 + j) * 3 + 0] = a.out_xyz[(o0 + j) * 3 + 1] = a.out_xyz[(o0 + j) * 3 + 2] = NAN;
            a.out_labels[o0 + j] = -1;
            a.rows[o0 + j] = -1;
            continue;
        }
        // count >= num_point: the first num_point outputs of a keyed bijection of [0, count) (without replacement, in random order);
        // else hi32(h * count) of a 32-bit hash per position (with replacement), the rule of ws_rows_kernel
        const uint32_t m = n >= (uint32_t)a.num_point ? ws_feistel(j, n, kperm)
                                                      : (uint32_t)(((uint64_t)ws_mix32(ws_mix32(j) ^ krep) * n) >> 32);
        const long long p = ws[m];
        a.rows[o0 + j] = (int32_t)p;
        a.out_labels[o0 + j] = lab[p];
        a.out_xyz[(o0 + j) * 3 + 0] = (float)(xyz[p * 3 + 0] - cx);
        a.out_xyz[(o0 + j) * 3 + 1] = (float)(xyz[p * 3 + 1] - cy);
        a.out_xyz[(o0 + j) * 3 + 2] = (float)xyz[p * 3 + 2];
    }
}

extern "C" size_t act_s3dis_sample_workspace(int B, long long max_window) {
    if (B <= 0 || max_window <= 0) return 0;
    return (size_t)B * (size_t)max_window * sizeof(int32_t);
}

extern "C" int act_s3dis_sample_f32(const double* xyz, const int32_t* labels, const long long* room_off, int R, const double* grid_origin,
                                    const long long* grid_dims, const long long* cell_off, const int32_t* cell_pts, double block_size, double cell,
                                    int min_points, int max_tries, long long max_window, const int32_t* room_ids, const int32_t* item_ids,
                                    const int32_t* center_in, int B, int num_point, unsigned seed, unsigned epoch, float* out_xyz,
                                    int64_t* out_labels, int32_t* rows, int32_t* count, int32_t* center_idx, int32_t* info, void* ws,
                                    size_t ws_bytes, act_stream_t stream) {
    if (!xyz || !labels || !room_off || !grid_origin || !grid_dims || !cell_off || !cell_pts || !room_ids || !item_ids || !out_xyz || !out_labels ||
        !rows || !count || !center_idx || !info || !ws)
        return ACT_E_NULLPTR;
    if (R <= 0 || B <= 0 || num_point <= 0 || min_points < 0 || max_tries <= 0 || max_tries > SS_MAX_TRIES || max_window <= 0) return ACT_E_BADARG;
    if (!(block_size > 0.0) || !(cell > 0.0) || block_size > 1e300 || cell > 1e300) return ACT_E_BADARG;
    if (ws_bytes < act_s3dis_sample_workspace(B, max_window)) return ACT_E_BADARG;
    SsArgs a;
    a.xyz = xyz; a.labels = labels; a.room_off = room_off; a.R = R;
    a.origin = grid_origin; a.dims = grid_dims; a.cell_off = cell_off; a.cell_pts = cell_pts;
    a.half = block_size / 2.0; a.cell = cell; a.min_points = min_points; a.max_tries = max_tries; a.cap = max_window;
    a.room_ids = room_ids; a.item_ids = item_ids; a.center_in = center_in; a.num_point = num_point; a.seed = (uint32_t)seed; a.epoch = (uint32_t)epoch;
    a.out_xyz = out_xyz; a.out_labels = out_labels; a.rows = rows; a.count = count; a.center_idx = center_idx; a.info = info; a.ws = (int32_t*)ws;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, (double)B * (36.0 * (double)max_window + 48.0 * num_point));
    hipLaunchKernelGGL(ss_sample_kernel, dim3(B), dim3(SS_THREADS), 0, s, a);
    ACT_LAUNCH_CHECK();
    return 0;
}
