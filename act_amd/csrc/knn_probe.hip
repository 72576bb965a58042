// knn_probe.hip -- weighted k-nearest-neighbour validation of frozen features (Wu et al. 2018, "Unsupervised Feature Learning via Non-Parametric
// Instance Discrimination"; the protocol of DINO's eval_knn): for every query the kmax most similar bank rows, then per k a class vote weighted by
// exp(sim / T).  Three stages, all on the caller's stream, every one bit-identical run to run and independent of the launch geometry:
//
//   prep     knn_prep_kernel     rows copied into the workspace with a leading dimension padded to KNN_KC floats (zero fill), divided by
//                                max(|x|, 1e-12) when normalize != 0.  One wave per row; the norm is a lane-strided fmaf sum + xor butterfly.
//   search   knn_search_kernel   a workgroup owns QT queries and a range of 128-row bank tiles (the bank is split over workgroups so a few dozen
//                                query tiles fill the chip).  Per bank tile the QT x 128 similarities are formed on v_mfma_f32_16x16x4_f32 from
//                                LDS-staged 16-deep operand chunks (each similarity is ONE fmaf chain over the padded feature index, in an order
//                                that depends on nothing but that index, so its bits do not depend on tile, split or position), parked in LDS over
//                                the staging buffers, and every wave folds them into the sorted best-kmax lists of its queries, which live in LDS
//                                for the whole kernel.  The similarity matrix never reaches global memory; a split writes kmax keys per query.
//   merge    knn_merge_kernel    one workgroup per query ranks the splits' keys against each other (own position + binary searches) and writes
//                                idx / sim.  Keys are unique, so the ranks are a permutation and no two threads write one slot.
//   vote     knn_vote_kernel     one workgroup per query: weights exp(sim / T), class scores summed in rank order, arg-max, top-1 / top-5 counts.
//
// Order: larger similarity first, then lower bank index.  Both live in one 64-bit key (monotone image of the float in the high word, ~index in the
// low word), so "better" is one unsigned compare, and 0 is the key of "no entry".
//
// LDS layout of the operand chunks: [row][KNN_LD = 24 floats], 16 of them used.  A lane of the 16x16x4 MFMA reads its row's four consecutive k
// (ds_read_b128 at row * 96 + 16 * (lane >> 4) bytes) and uses component s in k-step s; with a 24-float row stride the four 16-lane groups of a
// ds_read_b128 each cover the 64 banks exactly once (strides 16, 20, 28 and 32 are 2- to 4-way).
#include "common.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

#define KNN_BT 128            // bank rows per tile
#define KNN_KC 16             // feature chunk staged per step; the workspace copies have a leading dimension that is a multiple of it
#define KNN_LD 24             // LDS row stride of a chunk, floats
#define KNN_SLD (KNN_BT + 4)  // LDS row stride of the parked similarity tile
#define KNN_MAXK 256
#define KNN_MAX_SPLITS 16
#define KNN_MAX_CLASSES 1024
#define KNN_MAX_KS 16

static inline size_t knn_up(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int knn_dp(int D) { return (D + KNN_KC - 1) / KNN_KC * KNN_KC; }
static inline int knn_qt(int kmax) { return kmax <= 128 ? 64 : 32; }
static inline int knn_bank_tiles(int Nb) { return (Nb + KNN_BT - 1) / KNN_BT; }
// number of bank ranges: the caller's, or enough workgroups for two waves of 256 CUs; never more than there are bank tiles
static int knn_splits(int Nq, int Nb, int kmax, int splits) {
    const int qt = knn_qt(kmax), tiles_q = (Nq + qt - 1) / qt, nbt = knn_bank_tiles(Nb);
    if (splits <= 0) splits = (512 + tiles_q - 1) / tiles_q;
    if (splits > KNN_MAX_SPLITS) splits = KNN_MAX_SPLITS;
    if (splits > nbt) splits = nbt;
    return splits < 1 ? 1 : splits;
}

__device__ __forceinline__ unsigned knn_ford(float f) {                 // monotone: a < b  <=>  ford(a) < ford(b)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unford(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }
__device__ __forceinline__ u64 knn_key(float sim, int idx) { return ((u64)knn_ford(sim + 0.f) << 32) | (unsigned)(~idx); }   // (+ 0: -0 and +0 tie)
__device__ __forceinline__ float knn_el(const float4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// ---- prep: out [N, Dp] = x / max(|x|, 1e-12) (normalize) or x, zero in the padding -------------------------------------------------------
__global__ __launch_bounds__(256) void knn_prep_kernel(const float* __restrict__ X, int N, int D, int Dp, int normalize, float* __restrict__ out) {
    const int lane = threadIdx.x & (ACT_WAVE - 1);
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* x = X + (size_t)row * D;
    float den = 1.f;
    if (normalize) {
        float s = 0.f;
        for (int d = lane; d < D; d += ACT_WAVE) s = fmaf(x[d], x[d], s);
#pragma unroll
        for (int o = 1; o < ACT_WAVE; o <<= 1) s += __shfl_xor(s, o, ACT_WAVE);        // the same bits in every lane
        den = fmaxf(sqrtf(s), 1e-12f);
    }
    float* o = out + (size_t)row * Dp;
    for (int d = lane; d < Dp; d += ACT_WAVE) o[d] = d < D ? (normalize ? __fdiv_rn(x[d], den) : x[d]) : 0.f;
}

// ---- search ---------------------------------------------------------------------------------------------------------------------------------
// insert key x into the descending list L (n entries, capacity kmax) of one query; the whole wave calls it with the same arguments
template <int KCAP>
__device__ __forceinline__ int knn_insert(volatile u64* L, int n, int kmax, u64 x, int lane) {
    constexpr int NJ = (KCAP + ACT_WAVE - 1) / ACT_WAVE;
    u64 e[NJ];
    int pos = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int p = lane + ACT_WAVE * j;
        e[j] = p < n ? L[p] : 0ull;
        pos += __popcll(__ballot(p < n && e[j] > x));
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {                       // every read above precedes every write below (one wave, LDS operations in order)
        const int p = lane + ACT_WAVE * j;
        if (p < n && p >= pos && p + 1 < kmax) L[p + 1] = e[j];
    }
    if (lane == 0) L[pos] = x;                           // pos < kmax: either n < kmax and pos <= n, or x beat the last entry
    return n < kmax ? n + 1 : n;
}

template <int QT, int KCAP>
__global__ __launch_bounds__(256) void knn_search_kernel(const float* __restrict__ Qn, const float* __restrict__ Bn, int Nq, int Nb, int Dp,
                                                         int kmax, int exclude_self, int splits, int tiles_q, u64* __restrict__ part) {
    constexpr int MT = QT / 16;                                       // 16-row query blocks of a wave
    constexpr int BUF = (QT + KNN_BT) * KNN_LD;                       // one staged chunk: queries then bank rows
    constexpr int STAGE = 2 * BUF > QT * KNN_SLD ? 2 * BUF : QT * KNN_SLD;
    constexpr int QPW = QT / 4;                                       // queries a wave selects for
    __shared__ u64 lists[QT * KCAP];
    __shared__ __attribute__((aligned(16))) float stage[STAGE];       // two operand chunks, or the parked similarity tile
    __shared__ int lcount[QT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ml = lane & 15, kl = lane >> 4;
    const int sp = blockIdx.x / tiles_q, qt = blockIdx.x - sp * tiles_q;
    const int q0 = qt * QT;
    const int nbt = (Nb + KNN_BT - 1) / KNN_BT;
    const int t0 = (int)((long long)sp * nbt / splits), t1 = (int)((long long)(sp + 1) * nbt / splits);
    const int nch = Dp / KNN_KC;

    if (tid < QT) lcount[tid] = 0;
    __syncthreads();

    // staging: float4 #tid of the [rows][16] chunk: row = tid / 4 (+ 64 for the second bank half), k = 4 (tid % 4); rows past the end repeat the last
    const int sr = tid >> 2, sk = (tid & 3) * 4;
    const bool stage_q = sr < QT;
    const float* gq = Qn + (size_t)min(q0 + sr, Nq - 1) * Dp + sk;
    float4 rq, rb0, rb1;
    rq = rb0 = rb1 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int t = t0; t < t1; ++t) {
        const int b0 = t * KNN_BT;
        const float* gb0 = Bn + (size_t)min(b0 + sr, Nb - 1) * Dp + sk;
        const float* gb1 = Bn + (size_t)min(b0 + sr + 64, Nb - 1) * Dp + sk;
        auto load_g = [&](int c) {
            if (stage_q) rq = *reinterpret_cast<const float4*>(gq + c * KNN_KC);
            rb0 = *reinterpret_cast<const float4*>(gb0 + c * KNN_KC);
            rb1 = *reinterpret_cast<const float4*>(gb1 + c * KNN_KC);
        };
        auto store_lds = [&](int buf) {
            float* s = stage + buf * BUF;
            if (stage_q) *reinterpret_cast<float4*>(&s[sr * KNN_LD + sk]) = rq;
            *reinterpret_cast<float4*>(&s[(QT + sr) * KNN_LD + sk]) = rb0;
            *reinterpret_cast<float4*>(&s[(QT + sr + 64) * KNN_LD + sk]) = rb1;
        };
        f32x4 acc[MT][2];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto compute = [&](int buf) {
            const float* s = stage + buf * BUF;
            float4 a[MT], b[2];
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const float4*>(&s[(16 * i + ml) * KNN_LD + 4 * kl]);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const float4*>(&s[(QT + 32 * wave + 16 * j + ml) * KNN_LD + 4 * kl]);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(knn_el(a[i], c), knn_el(b[j], c), acc[i][j], 0, 0, 0);
        };
        load_g(0);
        store_lds(0);
        __syncthreads();
        for (int c = 0; c + 1 < nch; ++c) {
            load_g(c + 1);
            compute(c & 1);
            store_lds((c & 1) ^ 1);
            __syncthreads();
        }
        compute((nch - 1) & 1);
        __syncthreads();                                              // every wave is done with the chunks: the tile goes over them
        // accumulator (i, j)[r] = query 16 i + 4 (lane / 16) + r, bank row 32 wave + 16 j + lane % 16
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) stage[(16 * i + 4 * kl + r) * KNN_SLD + 32 * wave + 16 * j + ml] = acc[i][j][r];
        __syncthreads();
        // selection: wave w owns queries w * QPW .. + QPW - 1 and their lists
        for (int qi = 0; qi < QPW; ++qi) {
            const int ql = wave * QPW + qi, gqi = q0 + ql;
            if (gqi >= Nq) break;                                     // (the same in every lane)
            volatile u64* L = lists + ql * KCAP;
            int n = lcount[ql];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int bl = lane + 64 * h, b = b0 + bl;
                const bool valid = b < Nb && !(exclude_self && b == gqi);
                const u64 key = valid ? knn_key(stage[ql * KNN_SLD + bl], b) : 0ull;
                const u64 thr = n == kmax ? L[kmax - 1] : 0ull;
                u64 m = __ballot(key > thr);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const u64 x = ((u64)(unsigned)__shfl((int)(key >> 32), src, ACT_WAVE) << 32) | (unsigned)__shfl((int)(unsigned)key, src, ACT_WAVE);
                    if (n == kmax && x <= L[kmax - 1]) continue;      // the list's last entry has risen since the ballot
                    n = knn_insert<KCAP>(L, n, kmax, x, lane);
                }
            }
            if (lane == 0) lcount[ql] = n;
        }
        __syncthreads();                                              // the next tile's chunks go over the similarity tile
    }
    for (int qi = 0; qi < QPW; ++qi) {
        const int ql = wave * QPW + qi, gqi = q0 + ql;
        if (gqi >= Nq) break;
        const int n = lcount[ql];
        u64* dst = part + ((size_t)sp * Nq + gqi) * kmax;
        for (int r = lane; r < kmax; r += ACT_WAVE) dst[r] = r < n ? lists[ql * KCAP + r] : 0ull;
    }
}

// ---- merge: the best kmax of `splits` descending lists per query ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_merge_kernel(const u64* __restrict__ part, int Nq, int kmax, int splits, int* __restrict__ idx,
                                                        float* __restrict__ sim) {
    __shared__ u64 keys[KNN_MAX_SPLITS * KNN_MAXK];
    __shared__ int nvalid[KNN_MAX_SPLITS];
    const int q = blockIdx.x, tid = threadIdx.x, total = splits * kmax;
    for (int e = tid; e < total; e += 256) keys[e] = part[((size_t)(e / kmax) * Nq + q) * kmax + e % kmax];
    __syncthreads();
    // entries of list s above x (the list is descending, its empty slots are 0 at the end)
    auto above = [&](int s, u64 x) {
        int lo = 0, hi = kmax;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[s * kmax + mid] > x) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    if (tid < splits) nvalid[tid] = above(tid, 0ull);
    __syncthreads();
    int have = 0;
    for (int s = 0; s < splits; ++s) have += nvalid[s];
    for (int e = tid; e < total; e += 256) {
        const u64 x = keys[e];
        if (x == 0ull) continue;
        const int s = e / kmax;
        int rank = e - s * kmax;
        for (int o = 0; o < splits; ++o) if (o != s) rank += above(o, x);
        if (rank < kmax) {
            if (idx) idx[(size_t)q * kmax + rank] = (int)~(unsigned)x;
            if (sim) sim[(size_t)q * kmax + rank] = knn_unford((unsigned)(x >> 32));
        }
    }
    for (int r = have + tid; r < kmax; r += 256) {                    // fewer than kmax candidates (the entry point refuses it; keep the slots defined)
        if (idx) idx[(size_t)q * kmax + r] = -1;
        if (sim) sim[(size_t)q * kmax + r] = -INFINITY;
    }
}

// ---- vote -----------------------------------------------------------------------------------------------------------------------------------
struct KnnKs { int n; int k[KNN_MAX_KS]; };

__device__ __forceinline__ u64 knn_block_max(u64 v, u64* red, int tid) {
#pragma unroll
    for (int o = 1; o < ACT_WAVE; o <<= 1) {
        const u64 w = ((u64)(unsigned)__shfl_xor((int)(v >> 32), o, ACT_WAVE) << 32) | (unsigned)__shfl_xor((int)(unsigned)v, o, ACT_WAVE);
        v = w > v ? w : v;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    u64 r = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) r = red[w] > r ? red[w] : r;
    return r;
}
__device__ __forceinline__ int knn_block_sum(int v, int* red, int tid) {
#pragma unroll
    for (int o = 1; o < ACT_WAVE; o <<= 1) v += __shfl_xor(v, o, ACT_WAVE);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void knn_vote_kernel(const float* __restrict__ sim, const int* __restrict__ idx, int kmax,
                                                       const int* __restrict__ bank_cls, int Nb, const int* __restrict__ q_cls, int C, KnnKs ks,
                                                       float T, float* __restrict__ scores, long long* __restrict__ pred,
                                                       unsigned long long* __restrict__ counts) {
    __shared__ float w[KNN_MAXK];
    __shared__ int cls[KNN_MAXK];
    __shared__ u64 red64[4];
    __shared__ int red32[4];
    __shared__ float s_true;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int kuse = ks.k[ks.n - 1];
    for (int r = tid; r < kuse; r += 256) {
        const int b = idx[(size_t)q * kmax + r];
        const bool ok = b >= 0 && b < Nb;
        const int c = ok ? bank_cls[b] : -1;
        cls[r] = c;
        w[r] = (ok && c >= 0 && c < C) ? expf(__fdiv_rn(sim[(size_t)q * kmax + r], T)) : 0.f;
    }
    __syncthreads();
    float s[4] = {0.f, 0.f, 0.f, 0.f};                                 // classes tid, tid + 256, tid + 512, tid + 768
    const int truth = q_cls ? q_cls[q] : -1;
    int r = 0;
    for (int j = 0; j < ks.n; ++j) {
        for (; r < ks.k[j]; ++r) {                                      // rank order, one rounding per neighbour
            const int c = cls[r];
            const float wr = w[r];
#pragma unroll
            for (int m = 0; m < 4; ++m) if (c == tid + 256 * m) s[m] += wr;
        }
        u64 best = 0ull;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int c = tid + 256 * m;
            if (c < C) {
                if (scores) scores[((size_t)q * ks.n + j) * C + c] = s[m];
                const u64 key = knn_key(s[m], c);
                best = key > best ? key : best;
                if (c == truth) s_true = s[m];
            }
        }
        best = knn_block_max(best, red64, tid);                         // (its barriers also publish s_true)
        if (pred && tid == 0) pred[(size_t)q * ks.n + j] = (long long)(int)~(unsigned)best;
        if (counts && truth >= 0 && truth < C) {
            const u64 mine = knn_key(s_true, truth);
            int beat = 0;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int c = tid + 256 * m;
                if (c < C && knn_key(s[m], c) > mine) ++beat;
            }
            beat = knn_block_sum(beat, red32, tid);
            if (tid == 0) {
                if (beat == 0) atomicAdd(&counts[2 * j], 1ull);
                if (beat < 5) atomicAdd(&counts[2 * j + 1], 1ull);
            }
        }
        __syncthreads();
    }
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------
extern "C" int act_knn_probe_splits(int Nq, int Nb, int kmax, int splits) {
    if (Nq < 1 || Nb < 1 || kmax < 1 || kmax > KNN_MAXK) return 0;
    return knn_splits(Nq, Nb, kmax, splits);
}

extern "C" size_t act_knn_probe_workspace(int Nq, int Nb, int D, int kmax, int splits) {
    if (Nq < 1 || Nb < 1 || D < 1 || kmax < 1 || kmax > KNN_MAXK) return 0;
    const size_t dp = (size_t)knn_dp(D);
    return knn_up((size_t)Nq * dp * 4) + knn_up((size_t)Nb * dp * 4) + knn_up((size_t)knn_splits(Nq, Nb, kmax, splits) * Nq * kmax * 8);
}

extern "C" int act_knn_probe_normalize_f32(const float* X, int N, int D, float* out, act_stream_t stream) {
    if (!X || !out) return ACT_E_NULLPTR;
    if (N < 1 || D < 1) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(knn_prep_kernel, dim3((N + 3) / 4), dim3(256), 0, s, X, N, D, D, 1, out);
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" int act_knn_probe_search_f32(const float* Q, int Nq, const float* bank, int Nb, int D, int kmax, int normalize, int exclude_self,
                                        int splits, int32_t* idx, float* sim, void* workspace, size_t workspace_bytes, act_stream_t stream) {
    if (!Q || !bank || !workspace || (!idx && !sim)) return ACT_E_NULLPTR;
    if (Nq < 1 || Nb < 1 || D < 1 || kmax < 1 || kmax > KNN_MAXK || splits < 0) return ACT_E_BADARG;
    if ((long long)kmax > (long long)Nb - (exclude_self ? 1 : 0)) return ACT_E_BADARG;
    if (workspace_bytes < act_knn_probe_workspace(Nq, Nb, D, kmax, splits) || ((uintptr_t)workspace & 15)) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const int dp = knn_dp(D), nsp = knn_splits(Nq, Nb, kmax, splits), qt = knn_qt(kmax), tiles_q = (Nq + qt - 1) / qt;
    char* p = (char*)workspace;
    float* qn = (float*)p;  p += knn_up((size_t)Nq * dp * 4);
    float* bn = (float*)p;  p += knn_up((size_t)Nb * dp * 4);
    u64* part = (u64*)p;
    hipLaunchKernelGGL(knn_prep_kernel, dim3((Nq + 3) / 4), dim3(256), 0, s, Q, Nq, D, dp, normalize, qn);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_prep_kernel, dim3((Nb + 3) / 4), dim3(256), 0, s, bank, Nb, D, dp, normalize, bn);
    ACT_LAUNCH_CHECK();
    const dim3 grid((unsigned)(tiles_q * nsp));
    if (kmax <= 32)
        hipLaunchKernelGGL((knn_search_kernel<64, 32>), grid, dim3(256), 0, s, qn, bn, Nq, Nb, dp, kmax, exclude_self, nsp, tiles_q, part);
    else if (kmax <= 128)
        hipLaunchKernelGGL((knn_search_kernel<64, 128>), grid, dim3(256), 0, s, qn, bn, Nq, Nb, dp, kmax, exclude_self, nsp, tiles_q, part);
    else
        hipLaunchKernelGGL((knn_search_kernel<32, 256>), grid, dim3(256), 0, s, qn, bn, Nq, Nb, dp, kmax, exclude_self, nsp, tiles_q, part);
    ACT_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_merge_kernel, dim3(Nq), dim3(256), 0, s, part, Nq, kmax, nsp, idx, sim);
    ACT_LAUNCH_CHECK();
    return 0;
}

extern "C" int act_knn_probe_vote_f32(const float* sim, const int32_t* idx, int Nq, int kmax, const int32_t* bank_cls, int Nb, const int32_t* q_cls,
                                      int C, const int* ks, int nk, float T, float* scores, long long* pred, long long* counts,
                                      act_stream_t stream) {
    if (!sim || !idx || !bank_cls || !ks) return ACT_E_NULLPTR;
    if (Nq < 1 || Nb < 1 || kmax < 1 || kmax > KNN_MAXK || C < 1 || C > KNN_MAX_CLASSES || nk < 1 || nk > KNN_MAX_KS || !(T > 0.f)) return ACT_E_BADARG;
    KnnKs k;
    k.n = nk;
    for (int j = 0; j < KNN_MAX_KS; ++j) k.k[j] = j < nk ? ks[j] : 0;
    for (int j = 0; j < nk; ++j)
        if (k.k[j] < 1 || k.k[j] > kmax || (j && k.k[j] <= k.k[j - 1])) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(knn_vote_kernel, dim3(Nq), dim3(256), 0, s, sim, idx, kmax, bank_cls, Nb, q_cls, C, k, T, scores, pred,
                       (unsigned long long*)counts);
    ACT_LAUNCH_CHECK();
    return 0;
}
