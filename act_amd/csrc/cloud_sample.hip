// cloud_sample.hip -- training batches of the object datasets made on the device from a resident split (datasets/ShapeNet55Dataset.py:35-51,
// datasets/ModelNetDataset.py:120-140): clouds [M,N,C] float32 (C = 3 or 6, xyz first) stay on the device, and one launch makes a batch [B,n,C]:
// per item a keyed subset of n of its N rows without replacement in random order (the contract of permutation[:n]) and numpy's pc_norm of xyz.
//
// One workgroup per item, no atomics, no host synchronisation.  The selection of position j is ws_feistel(j, N, key) with key a function of
// (seed, epoch, draw id), so an item's result does not depend on the batch or the rank it is sampled in.  The normalisation keeps numpy's order of
// operations exactly (fp32, no contraction: built with -ffp-contract=off): np.mean(axis=0) of an [n,3] array adds the rows one by one in ascending
// order, so three lanes walk the staged rows serially, one coordinate each; the sum is divided by (float)n and subtracted; the scale is the largest
// sqrtf((x*x + y*y) + z*z); every coordinate is divided by it (IEEE division; a scale of 0 gives numpy's NaNs).  The selected xyz rows are
// staged in LDS (12 n bytes, 96 KB at n = 8192) and leave it once, normalised.  Normals (channels 3..5) go straight from source to output.
#include "common.h"
#include "ws_hash.h"

#define CS_THREADS 256
#define CS_WAVES (CS_THREADS / 64)
#define CS_MAX_POINTS 8192
#define CS_SALT 0x299f31d0u                                                 // (not the S3DIS sampler's 0x13198a2e: the two streams are unrelated)

struct CsArgs {
    const float* clouds; long long M; int N;
    const int32_t *item_ids, *draw_ids; int n; uint32_t seed, epoch; int flags;
    float* out; int32_t* rows;
};

template <int C, bool NORM>
__global__ __launch_bounds__(CS_THREADS) void cs_sample_kernel(const CsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cs_xyz[];          // [n][3], NORM only
    __shared__ float s_mean[3];
    __shared__ float s_max[CS_WAVES];
    const int b = blockIdx.x, n = a.n;
    const size_t o0 = (size_t)b * n;
    const long long item = a.item_ids[b];
    if (item < 0 || item >= a.M) {                                          // not an item of this split (the wrapper refuses it): nothing is read
        for (int j = threadIdx.x; j < n; j += CS_THREADS) {
            for (int c = 0; c < C; ++c) a.out[(o0 + j) * C + c] = NAN;
            if (a.rows) a.rows[o0 + j] = -1;
        }
        return;
    }
    const float* src = a.clouds + (size_t)item * a.N * C;
    uint32_t key = ws_mix32(a.seed ^ CS_SALT);
    key = ws_mix32(key ^ a.epoch);
    key = ws_mix32(key ^ (uint32_t)a.draw_ids[b]);
    const bool permute = a.flags & ACT_CLOUD_PERMUTE;

    for (int j = threadIdx.x; j < n; j += CS_THREADS) {
        const uint32_t r = permute ? ws_feistel((uint32_t)j, (uint32_t)a.N, key) : (uint32_t)j;
        if (a.rows) a.rows[o0 + j] = (int32_t)r;
        const float* p = src + (size_t)r * C;
        float* q = a.out + (o0 + j) * C;
        if (NORM) { cs_xyz[j * 3 + 0] = p[0]; cs_xyz[j * 3 + 1] = p[1]; cs_xyz[j * 3 + 2] = p[2]; }
        else { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; }
        if (C == 6) { q[3] = p[3]; q[4] = p[4]; q[5] = p[5]; }
    }
    if (!NORM) return;
    __syncthreads();

    if (threadIdx.x < 3) {                                                  // numpy's column sums: one fp32 add per row, rows ascending
        const float* p = cs_xyz + threadIdx.x;
        float s = 0.0f;
        int j = 0;
        for (; j + 8 <= n; j += 8) {                                        // eight loads in flight, the adds in order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(j + u) * 3];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; j < n; ++j) s += p[j * 3];
        s_mean[threadIdx.x] = s / (float)n;
    }
    __syncthreads();

    const float mx = s_mean[0], my = s_mean[1], mz = s_mean[2];
    float big = 0.0f;                                                       // (a norm is never NaN here: finite rows keep the sums free of inf - inf)
    for (int j = threadIdx.x; j < n; j += CS_THREADS) {
        const float x = cs_xyz[j * 3 + 0] - mx, y = cs_xyz[j * 3 + 1] - my, z = cs_xyz[j * 3 + 2] - mz;
        cs_xyz[j * 3 + 0] = x; cs_xyz[j * 3 + 1] = y; cs_xyz[j * 3 + 2] = z;
        big = fmaxf(big, sqrtf((x * x + y * y) + z * z));
    }
    for (int d = 32; d > 0; d >>= 1) big = fmaxf(big, __shfl_xor(big, d));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = big;
    __syncthreads();                                                        // (also: every centred row is in LDS)
    float m = s_max[0];
    for (int w = 1; w < CS_WAVES; ++w) m = fmaxf(m, s_max[w]);

    if (C == 3) {
        float* q = a.out + o0 * 3;
        for (int i = threadIdx.x; i < 3 * n; i += CS_THREADS) q[i] = cs_xyz[i] / m;
    } else {
        for (int i = threadIdx.x; i < 3 * n; i += CS_THREADS) a.out[(o0 + i / 3) * C + i % 3] = cs_xyz[i] / m;
    }
}

extern "C" int act_cloud_sample_max_points(void) { return CS_MAX_POINTS; }

template <int C, bool NORM>
static int cs_launch(const CsArgs& a, int B, hipStream_t s) {
    auto k = cs_sample_kernel<C, NORM>;
    const size_t smem = NORM ? (size_t)3 * a.n * sizeof(float) : 0;
    if (smem > 48 * 1024) {                                                 // raised once per device, to the largest staged cloud
        static bool raised[64] = {false};
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return ACT_E_BADARG;
        if (!raised[d]) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)((size_t)3 * CS_MAX_POINTS * sizeof(float)));
            if (e != hipSuccess) return (int)e;
            raised[d] = true;
        }
    }
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(CS_THREADS), smem, s, a);
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" int act_cloud_sample_f32(const float* clouds, long long M, int N, int C, const int32_t* item_ids, const int32_t* draw_ids, int B, int n,
                                    unsigned seed, unsigned epoch, int flags, float* out, int32_t* src_rows, act_stream_t stream) {
    if (B < 1 || M < 1 || N < 1 || n < 1 || n > N || n > CS_MAX_POINTS || (C != 3 && C != 6)) return ACT_E_BADARG;
    if (flags & ~(ACT_CLOUD_PERMUTE | ACT_CLOUD_NORMALIZE)) return ACT_E_BADARG;
    if (!clouds || !item_ids || !draw_ids || !out) return ACT_E_NULLPTR;
    CsArgs a;
    a.clouds = clouds; a.M = M; a.N = N; a.item_ids = item_ids; a.draw_ids = draw_ids; a.n = n;
    a.seed = (uint32_t)seed; a.epoch = (uint32_t)epoch; a.flags = flags; a.out = out; a.rows = src_rows;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, (double)B * n * (8.0 * C + 4.0));
    const bool norm = flags & ACT_CLOUD_NORMALIZE;
    if (C == 3) return norm ? cs_launch<3, true>(a, B, s) : cs_launch<3, false>(a, B, s);
    return norm ? cs_launch<6, true>(a, B, s) : cs_launch<6, false>(a, B, s);
}
