// gemm_bf16x3.hip -- OPT-IN NT GEMM on the bf16 matrix cores with split operands ("bf16x3"), for the FROZEN teacher only (round 5).
//
//   C[M,N] = epilogue( (A_hi + A_lo) . (B_hi + B_lo)^T )  with the lo.lo term dropped:  A_hi.B_hi + A_hi.B_lo + A_lo.B_hi, fp32 accumulation
//
// hi = bf16(x) (round to nearest even), lo = bf16(x - hi) (split_planes.h): 16 significand bits per operand instead of 24.  Every product of two planes is exact in the
// MFMA's fp32 accumulator; what is lost is the 2^-17 tail of each operand and the 2^-16 lo.lo term: 4.2e-6 relative per product against fp64, and the
// frozen teacher's features move by 6e-6 .. 7e-6 of their range when the 48 Linear layers of its ViT blocks run this way (parity bar 1e-4; measured with
// the CPU oracle, benchmarks/bf16x3_teacher_numerics.py, and on the device, tests/test_gpu_bf16x3.py).  It is NOT the default: the product path is
// f32-input MFMA and every headline number is measured on it; ACT_TEACHER_BF16X3=1 routes the teacher's five GEMMs per ViT layer here and bench.py
// reports that configuration on a separate line.
//
// Why it is fast: v_mfma_f32_16x16x32_bf16 has 16 x the rate of the f32-input MFMA, three products cost 3/16 of the matrix time, and two bf16 planes are
// the same 4 bytes per element as fp32 -- so the kernel moves exactly the bytes of the fp32 kernel and is bound by the L2 -> LDS fill path and the LDS,
// not by the matrix pipe: 128 x 128 tile, 32-deep K tiles, double-buffered LDS (ONE barrier per K tile), global prefetch two K tiles ahead in two register
// sets.  8192 x 3072 x 768: 282 TFLOP/s-equivalent (shipped f32 kernel: 135), benchmarks/micro/bf16x3_planes.hip -> profiles/r05_micro_bf16x3_planes.txt.
// A lesson kept in the code: the staging arrays are NATIVE vector types (ext_vector_type); arrays of HIP's `uint4` struct stay in scratch memory.
//
// DEFAULT for the frozen teacher's inference forward (F16 form of the same kernel, ACT_TEACHER_F16X3, notebook/teacher_f16x3.md): two f16 planes with a scaled
// low plane, x s = h1 + 2^-11 h2 (split_planes.h), keep 22 significand bits + the residual's sign instead of 16, at the same bytes, LDS traffic and MFMA count
// (v_mfma_f32_16x16x32_f16 runs at the bf16 rate).  f16's narrow exponent range is handled with exact powers of two: the weights carry one scale per output
// row (row max lifted into [2^14, 2^15)), the activations one static scale per Linear derived from a weight-only bound on the operand (composite.py), and the
// two cross terms h1.h2 + h2.h1 go to a SECOND accumulator that is folded in with 2^-11 in the epilogue, where the scales are divided out again:
//   v = (acc0 + 2^-11 acc1) * (1 / s_B[n]) * (1 / s_A)   -> bias / GELU / residual exactly as the f32 kernels.   fp32-grade: error against fp64 equal to the
// f32 kernel's on LayerNorm / GELU / attention operands (tests/test_gpu_f16x3.py holds it to 1.5 x).  Launches are counted under the same profiling id.
//
// TILE FORMS (notebook/x3_tiles.md).  The kernel is a template over the tile BM x BN and its wave grid WGM x WGN (64 WGM WGN threads, wave block BM/WGM x BN/WGN):
//   <128, 128, 2, 2>  4 waves, 64 x 64 per wave, 81,920 B LDS, two workgroups per CU            (bf16: 162 VGPRs, F16: 226 VGPRs) -- the bf16 opt-in and the default
//   <128, 192, 2, 4>  8 waves, 64 x 48 per wave, 102,400 B LDS, one workgroup per CU, F16 only  (196 VGPRs, no scratch)
// Both run two waves per SIMD.  The kernel's speed follows how its grid fills the CUs: at M = 8,192, N = 768 (the teacher's proj and fc2) 128 x 128 tiles make 384
// workgroups for 512 slots -- half of the CUs hold two, half hold one, and the launch lasts as long as the CUs that hold two -- where 128 x 192 makes 256, one per
// CU, each 1.5 tiles' worth: proj 67.6 -> 56.2 us, fc2 160.0 -> 132.0 us per launch inside the step.  act_sgemm_nt_f16x3_pick_tile (below) picks by shape alone.
// The order of accumulation of an output element does not depend on the tile (K tiles in sequence, the three products in the same order, the same epilogue):
// every form gives the same bits (tests/test_gpu_f16x3_tiles.py).
//
// THE GROUP-MAX PRODUCT (notebook/pn_f16x3.md): the last conv of the frozen tokenizer's mini-PointNet, out[g] = max over the rows of group g of
// relu(h3 * sc + sh) . W^T + b, is the F16 form with two more template flags: A32 -- A arrives as fp32 and is activated (BatchNorm-2 affine + ReLU, the activation
// scale folded in) and split while it is staged, the planes never exist in memory -- and GMAX -- the epilogue reduces over each group of 32 or 64 rows inside the
// wave's 64-row block and stores only that.  act_sgemm_nt_f16x3_gmax_f32; 254 VGPRs on 128 x 128, 196 on 128 x 192, no scratch.  The other instances are unchanged.
#include "gemm_common.h"
#include "split_planes.h"
#include <stdlib.h>

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));

namespace {

// relu(a * sc + sh), one fma per element: the A-side affine map of the group-max product, shared by its on-load form and the pass below
__device__ __forceinline__ float4 x3_affine_relu4(const float4& a, const float4& sc, const float4& sh) {
    return make_float4(fmaxf(__builtin_fmaf(a.x, sc.x, sh.x), 0.f), fmaxf(__builtin_fmaf(a.y, sc.y, sh.y), 0.f),
                       fmaxf(__builtin_fmaf(a.z, sc.z, sh.z), 0.f), fmaxf(__builtin_fmaf(a.w, sc.w, sh.w), 0.f));
}
__device__ __forceinline__ float4 x3_scale4(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// fp32 [R][K] (row stride ldx) -> two planes [R][K] (split_planes.h), four elements per thread (K % 4 == 0): (hi, lo) bf16 planes of x, or (F16) the (h1, h2)
// f16 planes of x * scale * row_scale[row]; both scales are powers of two chosen by the caller and are not read in the bf16 form.  The planes' rows are ldp
// elements apart (ldp == K: dense; wider: a column slice of a wider plane buffer, the same bytes per element)
// AFF (F16 only): the planes of relu(x * col_scale[k] + col_shift[k]) * scale instead -- the power of two folded into the affine map first, one fma per element,
// exactly what the product's on-load form computes, so the two forms give the same planes bit for bit
// kt_rows > 0: the planes leave in the K-tile-major layout of a [kt_rows][K] plane (x3_kt_index below; K % 32 == 0) instead, the same values at other places
template <bool F16, bool AFF = false>
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, int K4, int ldx, int ldp4, long long n4, float scale,
                                                           const float* __restrict__ row_scale, unsigned short* __restrict__ p1, unsigned short* __restrict__ p2,
                                                           const float* __restrict__ col_scale = nullptr, const float* __restrict__ col_shift = nullptr,
                                                           int kt_rows = 0) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / K4; const int c4 = (int)(i - row * K4);
        const float4 v = *reinterpret_cast<const float4*>(x + row * ldx + c4 * 4);
        // ldp4 = the planes' row stride in groups of four elements (K4: dense, o4 == i); K-tile-major: eight groups of four per row and K tile
        const size_t o4 = kt_rows ? ((size_t)(c4 >> 3) * kt_rows + row) * 8 + (c4 & 7) : (size_t)(row * ldp4 + c4);
        if constexpr (AFF) {
            const float4 sc = x3_scale4(*reinterpret_cast<const float4*>(col_scale + c4 * 4), scale), sh = x3_scale4(*reinterpret_cast<const float4*>(col_shift + c4 * 4), scale);
            store_planes4<F16>(p1, p2, o4, x3_affine_relu4(v, sc, sh), 1.0f);
        } else {
            store_planes4<F16>(p1, p2, o4, v, F16 && row_scale ? scale * row_scale[row] : scale);
        }
    }
}

constexpr int BK = 32;                      // bf16 per K tile = 64-byte rows

// K-TILE-MAJOR ("KT") PLANES (notebook/x3_ktile.md).  Element (r, k) of a plane [R][K] lies at ((k / BK) * R + r) * BK + k % BK: the 64-byte pieces that the
// rows of one K tile contribute are adjacent, so a workgroup's A or B tile of one K tile is ONE contiguous block of rows * 64 bytes and thread tid of a staging
// pass reads bytes 16 tid .. of it -- every wave-wide load is eight whole 128-byte lines, where the row-major plane gives sixteen half-used ones.  The product
// kernel walks either layout through two strides per operand (X3Params): row stride and K-tile stride, (ld, BK) row-major and (BK, R * BK) KT.  Same values,
// same order of summation: the same bits.
constexpr long long x3_kt_index(long long r, long long k, long long rows) { return ((k / BK) * rows + r) * BK + k % BK; }

// plane [R][K] row-major -> KT, one 16-byte chunk per thread (K8 = K / 8 chunks per row, four per K tile)
__global__ __launch_bounds__(256) void repack_ktile_kernel(const u32x4v* __restrict__ src, u32x4v* __restrict__ dst, int R, int K8, long long n8) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / K8; const int c8 = (int)(i - row * K8);
        dst[((long long)(c8 >> 2) * R + row) * 4 + (c8 & 3)] = src[i];
    }
}
constexpr int LROW = 40;                    // bf16 per LDS row: 32 + 8 pad (80-byte pitch: conflict-free ds_read_b128 / ds_write_b128)

struct X3Params {
    const unsigned short *Ah, *Al, *Bh, *Bl;   // planes of A [M][K] and B [N][K], each walked by a row stride (lda, ldb) and a K-tile stride (kta, ktb), in elements:
                                               // row-major (ld, BK) with ld >= K (a column slice of a wider plane buffer); K-tile-major (BK, rows_total * BK)
    float* C; int ldc;                         // fp32 result (nullable when the planes below are given)
    unsigned short *Oh, *Ol;                   // optional: the result ALSO / INSTEAD as (hi, lo) bf16 planes [M][N] -- the A operand of the next split-bf16 product
    int M, N, K;
    act_gemm_epilogue_t epi;
    const float* b_inv; float a_inv, o_scale;  // F16 form: 1 / s_B[n], 1 / s_A, and the scale the planes-out are split at (the next product's s_A)
    // A32 form: A arrives as fp32 [M][K] (row stride lda) and its planes are those of relu(A * a_sc[k] + a_sh[k]) * a_fold, made while the tile is staged
    const float *A32, *a_sc, *a_sh; int lda; float a_fold;   // (lda: the row stride of A in either form, in elements of that form)
    int ldb, kta, ktb;                         // (A32: kta == BK)
    int o_kt;                                  // the planes-out [M][N] leave K-tile-major: the A operand of a product that reads it so
    int group;                                 // GMAX form: rows per group (32 or 64); C = out [M / group][N] (row stride ldc), the max over each group's rows
};

// A32 staging: eight consecutive k of one row as two fp32 vectors -> affine + ReLU (sc / sh: this thread's eight (scale, shift) pairs, the activation scale
// folded in) -> split_f16x2 (split_planes.h) -> the 16 bytes of each plane that the planes-in form loads from memory
__device__ __forceinline__ void x3_affine_split8(const u32x4v& a0, const u32x4v& a1, const float* sc, const float* sh, u32x4v& h1, u32x4v& h2) {
    // one half (four k) at a time, the halves kept apart in the schedule: the 128 x 128 form has 30 registers to spare
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const float4 c = *reinterpret_cast<const float4*>(sc + half * (LROW / 2)), s = *reinterpret_cast<const float4*>(sh + half * (LROW / 2));
        const float4 v = x3_affine_relu4(__builtin_bit_cast(float4, half ? a1 : a0), c, s);
        const float e[4] = {v.x, v.y, v.z, v.w};
        unsigned h[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split_f16x2(e[j], h[j], l[j]);
        h1[2 * half] = h[0] | (h[1] << 16); h1[2 * half + 1] = h[2] | (h[3] << 16);
        h2[2 * half] = l[0] | (l[1] << 16); h2[2 * half + 1] = l[2] | (l[3] << 16);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// one MFMA of two 16-bit fragments (8 per lane), bf16 or f16 by the plane format
template <bool F16>
__device__ __forceinline__ f32x4 x3_mfma(const bf16x8& b, const bf16x8& a, const f32x4& c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b), __builtin_bit_cast(f16x8, a), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, c, 0, 0, 0);
}

// workgroups per CU the kernel is built for: two of the 4-wave form, one of the 8-wave form -- two waves per SIMD either way
constexpr int x3_wgs_per_cu(int waves) { return waves <= 4 ? 2 : 1; }

// F16: f16 planes, the two cross terms in a second accumulator set (acc[1]), scales divided out in the epilogue; otherwise bf16 planes and one accumulator set
// WGM x WGN waves, each on a (BM / WGM) x (BN / WGN) block of the tile.  (__launch_bounds__' second argument counts waves per SIMD.)
// A32 (F16 only): A is fp32 and is activated and split while it is staged (x3_affine_split8); its K (scale, shift) pairs sit in the pad columns of the two A
// plane images of LDS stage 0 -- four floats behind each of the BM rows, which no staging store and no fragment read touches -- so K <= 4 BM and the form costs
// no LDS.  GMAX: the epilogue keeps the max over every `group` rows and stores that instead of C.  Both default to off: the other instances are unchanged.
template <int BM, int BN, int WGM, int WGN, int ACT, bool PLANES, bool F16, bool A32 = false, bool GMAX = false>
__global__ __launch_bounds__(64 * WGM * WGN, x3_wgs_per_cu(WGM * WGN) * WGM * WGN / 4) void sgemm_nt_bf16x3_kernel(const X3Params p) {
    static_assert(F16 || !(A32 || GMAX), "the on-load split and the group max belong to the f16 form");
    static_assert(!GMAX || (BM / WGM == 64 && !PLANES), "a group of 32 or 64 rows lies inside one wave's 64-row block");
    constexpr int NT = 64 * WGM * WGN, RP = NT / 4;           // threads; rows of a plane tile that one staging pass covers
    constexpr int WM = BM / WGM, WN = BN / WGN;               // the wave's block
    constexpr int TM = WM / 16, TN = WN / 16;                 // 16 x 16 tiles per wave
    constexpr int PA = BM * LROW, PB = BN * LROW;             // bf16 per plane image
    constexpr int NA = (BM + RP - 1) / RP, NB = (BN + RP - 1) / RP;   // 16-byte chunks per thread, plane and K tile (the last pass may be partial)
    constexpr int STAGE = 2 * (PA + PB);
    static_assert(WM % 16 == 0 && WN % 16 == 0 && BM % 16 == 0 && BN % 16 == 0, "whole 16 x 16 blocks per wave, whole waves per staging row test");
    __shared__ __attribute__((aligned(16))) unsigned short L[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int tiles_n = p.N / BN, tiles_m = p.M / BM;
    int wg = blockIdx.x;
    {                                                             // XCD-aware remap (workgroup b runs on XCD b % 8) + grouped rasterisation (gemm_common.h)
        const int nwg = tiles_m * tiles_n, q = nwg >> 3, r = nwg & 7, xcd = wg & 7, loc = wg >> 3;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    constexpr int GM = 8;
    const int per_group = GM * tiles_n, group = wg / per_group, first_m = group * GM;
    const int gsz = min(tiles_m - first_m, GM), in_group = wg - group * per_group;
    const int tile_m = first_m + in_group % gsz, tile_n = in_group / gsz;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int K = p.K, ntiles = K / BK, last = ntiles - 1;

    constexpr int X = F16 ? 1 : 0;                            // accumulator set of the cross terms
    f32x4 acc[X + 1][TM][TN];
#pragma unroll
    for (int x = 0; x <= X; ++x)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[x][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int srow = tid >> 2, sch = tid & 3;                 // staging: (row, 16-byte chunk) of a [rows][32 bf16] plane tile
    const int lda = p.lda, ldb = p.ldb;                       // A32: this thread's eight k of a row are two 16-byte fp32 loads (set 0: k .. k+3, set 1: k+4 .. k+7)
    const long long kta = p.kta, ktb = p.ktb;                 // K tile T of an operand starts T * kt elements behind tile 0 (row-major: BK)
    const size_t goa = (size_t)(m0 + srow) * lda + sch * 8, gob = (size_t)(n0 + srow) * ldb + sch * 8;
    const float* gA32[2] = {A32 ? p.A32 + goa : nullptr, A32 ? p.A32 + goa + 4 : nullptr};
    const unsigned short* gA[2] = {A32 ? nullptr : p.Ah + goa, A32 ? nullptr : p.Al + goa};
    const unsigned short* gB[2] = {p.Bh + gob, p.Bl + gob};
    u32x4v ra0[2][NA], rb0[2][NB], ra1[2][NA], rb1[2][NB];      // two staging sets (native vectors: arrays of HIP's uint4 struct would sit in scratch)
    const int s_off = srow * LROW + sch * 8;
    const int r = lane & 15, g = lane >> 4;
    const int a_off = (wm * WM + r) * LROW + g * 8, b_off = (wn * WN + r) * LROW + g * 8;
    // staging pass i covers rows i * RP .. of the plane tile.  A last PARTIAL pass (BM or BN no multiple of RP) loads unconditionally from its row clamped into
    // the tile (ta / tb: that row's offset from this thread's first row) and stores to the LDS only where the row exists -- a test that is uniform per wave
    // (a wave stages 16 consecutive rows; BM, BN and RP are multiples of 16), so there is still no divergent code around the staging registers
    const long long ta = (long long)(min(srow + RP * (NA - 1), BM - 1) - srow) * lda, tb = (long long)(min(srow + RP * (NB - 1), BN - 1) - srow) * ldb;
    // A32: (scale, shift) of k at float (k / 4) * (LROW / 2) + 16 + k % 4 of the first / second A plane image of stage 0 (the pad columns)
    const float* Lf = reinterpret_cast<const float*>(L);
    const int sx_off = sch * 2 * (LROW / 2) + 16;              // + T * 8 * (LROW / 2): this thread's eight k of K tile T
#define X3_WHOLE(I, ROWS) (RP * ((I) + 1) <= (ROWS))
#define X3_LOAD(RA, RB, T)                                                                                                             \
    _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) {                                                                                 \
        _Pragma("unroll") for (int i_ = 0; i_ < NA; ++i_)                                                                              \
            if constexpr (A32)                                                                                                         \
                RA[s_][i_] = *reinterpret_cast<const u32x4v*>(gA32[s_] + (X3_WHOLE(i_, BM) ? (long long)(RP * i_) * lda : ta) + (T) * kta); \
            else                                                                                                                       \
                RA[s_][i_] = *reinterpret_cast<const u32x4v*>(gA[s_] + (X3_WHOLE(i_, BM) ? (long long)(RP * i_) * lda : ta) + (T) * kta); \
        _Pragma("unroll") for (int i_ = 0; i_ < NB; ++i_)                                                                              \
            RB[s_][i_] = *reinterpret_cast<const u32x4v*>(gB[s_] + (X3_WHOLE(i_, BN) ? (long long)(RP * i_) * ldb : tb) + (T) * ktb);   \
    }
    /* T: the K tile the registers hold (read by the A32 form only) */
#define X3_STORE(RA, RB, STG, T)                                                                                                       \
    if constexpr (A32) {                                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < NA; ++i_)                                                                              \
            if (X3_WHOLE(i_, BM) || srow + RP * i_ < BM) {                                                                             \
                u32x4v h1_, h2_;                                                                                                       \
                x3_affine_split8(RA[0][i_], RA[1][i_], Lf + sx_off + (T) * 8 * (LROW / 2), Lf + PA / 2 + sx_off + (T) * 8 * (LROW / 2), h1_, h2_); \
                *reinterpret_cast<u32x4v*>(&L[(STG) * STAGE + s_off + RP * i_ * LROW]) = h1_;                                          \
                *reinterpret_cast<u32x4v*>(&L[(STG) * STAGE + PA + s_off + RP * i_ * LROW]) = h2_;                                     \
            }                                                                                                                          \
    }                                                                                                                                  \
    _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) {                                                                                 \
        _Pragma("unroll") for (int i_ = 0; i_ < NA; ++i_)                                                                              \
            if (!A32 && (X3_WHOLE(i_, BM) || srow + RP * i_ < BM))                                                                     \
                *reinterpret_cast<u32x4v*>(&L[(STG) * STAGE + s_ * PA + s_off + RP * i_ * LROW]) = RA[s_][i_];                         \
        _Pragma("unroll") for (int i_ = 0; i_ < NB; ++i_)                                                                              \
            if (X3_WHOLE(i_, BN) || srow + RP * i_ < BN)                                                                               \
                *reinterpret_cast<u32x4v*>(&L[(STG) * STAGE + 2 * PA + s_ * PB + s_off + RP * i_ * LROW]) = RB[s_][i_];                \
    }
#define X3_COMPUTE(STG)                                                                                                                \
    {                                                                                                                                  \
        const unsigned short* As_ = L + (STG) * STAGE; const unsigned short* Bs_ = As_ + 2 * PA;                                       \
        bf16x8 af[TM][2];                                                                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < TM; ++i_)                                                                              \
            _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) af[i_][s_] = *reinterpret_cast<const bf16x8*>(&As_[s_ * PA + a_off + i_ * 16 * LROW]); \
        _Pragma("unroll") for (int j_ = 0; j_ < TN; ++j_) {                                                                            \
            bf16x8 bf[2];                                                                                                              \
            _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) bf[s_] = *reinterpret_cast<const bf16x8*>(&Bs_[s_ * PB + b_off + j_ * 16 * LROW]); \
            /* smallest terms first: lo.hi, hi.lo, hi.hi.  The B fragment is the MFMA's FIRST operand: the 16 x 16 result block comes out transposed in the   */ \
            /* register layout (lane (r, g) holds row r, columns 4g .. 4g+3), i.e. every lane owns FOUR CONSECUTIVE COLUMNS of one row -> vector epilogue  */ \
            _Pragma("unroll") for (int i_ = 0; i_ < TM; ++i_) acc[X][i_][j_] = x3_mfma<F16>(bf[0], af[i_][1], acc[X][i_][j_]);           \
            _Pragma("unroll") for (int i_ = 0; i_ < TM; ++i_) acc[X][i_][j_] = x3_mfma<F16>(bf[1], af[i_][0], acc[X][i_][j_]);           \
            _Pragma("unroll") for (int i_ = 0; i_ < TM; ++i_) acc[0][i_][j_] = x3_mfma<F16>(bf[0], af[i_][0], acc[0][i_][j_]);           \
        }                                                                                                                              \
    }
    // loads / stores are unconditional: past the end they re-read the last K tile and fill a stage nobody reads (no divergent code around the staging registers)
    X3_LOAD(ra0, rb0, 0)
    X3_LOAD(ra1, rb1, min(1, last))
    if constexpr (A32) {                                          // the K (scale, shift) pairs, times the activation scale (a power of two: exact), into the pads
        float* Lw = reinterpret_cast<float*>(L);
        for (int q = tid; q < K / 4; q += NT) {
            *reinterpret_cast<float4*>(&Lw[q * (LROW / 2) + 16]) = x3_scale4(*reinterpret_cast<const float4*>(p.a_sc + 4 * q), p.a_fold);
            *reinterpret_cast<float4*>(&Lw[PA / 2 + q * (LROW / 2) + 16]) = x3_scale4(*reinterpret_cast<const float4*>(p.a_sh + 4 * q), p.a_fold);
        }
        __syncthreads();
    }
    X3_STORE(ra0, rb0, 0, 0)
    __syncthreads();
    for (int t = 0; t < ntiles; t += 2) {                         // ntiles is even (K % 64 == 0, checked by the launcher)
        X3_LOAD(ra0, rb0, min(t + 2, last))                       // LDS stage 0 = tile t; set 1 = tile t+1 (in flight); request tile t+2
        X3_COMPUTE(0)
        X3_STORE(ra1, rb1, 1, min(t + 1, last))
        __syncthreads();
        X3_LOAD(ra1, rb1, min(t + 3, last))                       // LDS stage 1 = tile t+1; set 0 = tile t+2 (in flight); request tile t+3
        X3_COMPUTE(1)
        X3_STORE(ra0, rb0, 0, min(t + 2, last))
        __syncthreads();
    }
#undef X3_WHOLE
#undef X3_LOAD
#undef X3_STORE
#undef X3_COMPUTE
    // epilogue: lane (r, g) holds row i*16 + r, columns j*16 + 4g .. 4g+3 of its wave's WM x WN block (operands swapped above): one float4 of bias / residual /
    // result and one 8-byte store per plane, per 16 x 16 block; same per-element arithmetic and order as the f32 kernels (epilogue_apply4_act)
    // F16: v = (acc0 + 2^-11 acc1) / s_B[n] / s_A first -- two multiplications by powers of two, exact -- then the same epilogue
    const bool vec = (((uintptr_t)p.C | (uintptr_t)p.epi.bias | (uintptr_t)p.epi.res | (uintptr_t)p.epi.aux) & 15) == 0 &&
                     ((p.ldc | (p.epi.res ? p.epi.ldr : 0) | (p.epi.aux ? p.epi.ldaux : 0)) & 3) == 0;
    auto value = [&](int i, int j, int row, int col) -> float4 {      // the finished 1 x 4 piece of block (i, j)
        float4 v = make_float4(acc[0][i][j][0], acc[0][i][j][1], acc[0][i][j][2], acc[0][i][j][3]);
        if constexpr (F16) {
            const float4 bi = *reinterpret_cast<const float4*>(p.b_inv + col);           // 16-byte aligned (launcher), col % 4 == 0
            constexpr float W = 1.0f / 2048.0f;
            v.x = __builtin_fmaf(acc[1][i][j][0], W, v.x) * bi.x * p.a_inv; v.y = __builtin_fmaf(acc[1][i][j][1], W, v.y) * bi.y * p.a_inv;
            v.z = __builtin_fmaf(acc[1][i][j][2], W, v.z) * bi.z * p.a_inv; v.w = __builtin_fmaf(acc[1][i][j][3], W, v.w) * bi.w * p.a_inv;
        }
        if (vec) v = epilogue_apply4_act<ACT>(p.epi, v, row, col);
        else {
            v.x = epilogue_apply<ACT>(p.epi, v.x, row, col); v.y = epilogue_apply<ACT>(p.epi, v.y, row, col + 1);
            v.z = epilogue_apply<ACT>(p.epi, v.z, row, col + 2); v.w = epilogue_apply<ACT>(p.epi, v.w, row, col + 3);
        }
        return v;
    };
    if constexpr (GMAX) {
        // max over every `group` (32 or 64) consecutive rows instead of C: the wave's 64 rows are two half blocks (i = 0, 1 | 2, 3), each reduced over i in
        // the lane and over the 16 lanes that share g; lane r == 0 stores one float4 per group.  From -inf: a biased output may be all negative.  (max is
        // associative and commutative: the order of the reduction, hence the tile form, does not change a bit.)
        constexpr float NINF = -__builtin_huge_valf();
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * WN + j * 16 + g * 4;
            float4 m[2] = {make_float4(NINF, NINF, NINF, NINF), make_float4(NINF, NINF, NINF, NINF)};
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const float4 v = value(i, j, m0 + wm * WM + i * 16 + r, col);
                float4& d = m[i / (TM / 2)];
                d.x = fmaxf(d.x, v.x); d.y = fmaxf(d.y, v.y); d.z = fmaxf(d.z, v.z); d.w = fmaxf(d.w, v.w);
            }
            if (p.group == 64) { m[0].x = fmaxf(m[0].x, m[1].x); m[0].y = fmaxf(m[0].y, m[1].y); m[0].z = fmaxf(m[0].z, m[1].z); m[0].w = fmaxf(m[0].w, m[1].w); }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && p.group == 64) break;
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    m[h].x = fmaxf(m[h].x, __shfl_xor(m[h].x, off)); m[h].y = fmaxf(m[h].y, __shfl_xor(m[h].y, off));
                    m[h].z = fmaxf(m[h].z, __shfl_xor(m[h].z, off)); m[h].w = fmaxf(m[h].w, __shfl_xor(m[h].w, off));
                }
                if (r == 0) {
                    float* cp = p.C + (size_t)((m0 + wm * WM + h * 32) / p.group) * p.ldc + col;
                    if (vec) *reinterpret_cast<float4*>(cp) = m[h]; else { cp[0] = m[h].x; cp[1] = m[h].y; cp[2] = m[h].z; cp[3] = m[h].w; }
                }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int row = m0 + wm * WM + i * 16 + r;
            const int col = n0 + wn * WN + j * 16 + g * 4;
            const float4 v = value(i, j, row, col);
            if (!PLANES || p.C) {
                float* cp = p.C + (size_t)row * p.ldc + col;
                if (vec) *reinterpret_cast<float4*>(cp) = v; else { cp[0] = v.x; cp[1] = v.y; cp[2] = v.z; cp[3] = v.w; }
            }
            // N % 128 == 0, col % 4 == 0: 8-byte aligned in either layout (o_kt: x3_kt_index of a [M][N] plane)
            if constexpr (PLANES)
                store_planes4<F16>(p.Oh, p.Ol, (p.o_kt ? ((size_t)(col >> 5) * p.M + row) * BK + (col & 31) : (size_t)row * p.N + col) >> 2, v, p.o_scale);
        }
}

template <int BM, int BN, int WGM, int WGN, bool F16>
int launch_x3(const X3Params& p, hipStream_t s) {
    const dim3 grid((p.M / BM) * (p.N / BN)), block(64 * WGM * WGN);
    const bool planes = p.Oh != nullptr;
    switch (p.epi.act) {
        case ACT_EPI_NONE:
            if (planes) hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_NONE, true, F16>), grid, block, 0, s, p);
            else        hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_NONE, false, F16>), grid, block, 0, s, p);
            break;
        case ACT_EPI_GELU:
            if (planes) hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_GELU, true, F16>), grid, block, 0, s, p);
            else        hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_GELU, false, F16>), grid, block, 0, s, p);
            break;
        case ACT_EPI_MUL_GELU_GRAD:                                  // (the MLP's backward through GELU: aux = the saved pre-activation)
            if (planes) hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_MUL_GELU_GRAD, true, F16>), grid, block, 0, s, p);
            else        hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_MUL_GELU_GRAD, false, F16>), grid, block, 0, s, p);
            break;
        default: return ACT_E_BADARG;
    }
    ACT_LAUNCH_CHECK();
    return 0;
}

// the group-max product (F16, bias only): A as planes, or (a32) as fp32 activated and split on load
template <int BM, int BN, int WGM, int WGN>
int launch_x3_gmax(const X3Params& p, bool a32, hipStream_t s) {
    const dim3 grid((p.M / BM) * (p.N / BN)), block(64 * WGM * WGN);
    if (a32) hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_NONE, false, true, true, true>), grid, block, 0, s, p);
    else     hipLaunchKernelGGL((sgemm_nt_bf16x3_kernel<BM, BN, WGM, WGN, ACT_EPI_NONE, false, true, false, true>), grid, block, 0, s, p);
    ACT_LAUNCH_CHECK();
    return 0;
}

// the argument-checked split pass of both formats (the bf16 form reads neither scale)
template <bool F16>
int split_planes(const float* x, int R, int K, int ldx, float scale, const float* row_scale, uint16_t* p1, uint16_t* p2, int ldp, act_stream_t stream) {
    if (!x || !p1 || !p2) return ACT_E_NULLPTR;
    if (R < 0 || K <= 0 || (K & 3) || ldx < K || (ldx & 3) || (F16 && !(scale > 0.f)) || (((uintptr_t)x | (uintptr_t)p1 | (uintptr_t)p2) & 15)) return ACT_E_BADARG;
    if (ldp < K || (ldp != K && (ldp & 7))) return ACT_E_BADARG;      // strided rows keep every row of a plane 16-byte aligned
    const long long n4 = (long long)R * K / 4; if (n4 == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, 8.0 * R * (double)K);
    long long g = (n4 + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(split_planes_kernel<F16>, dim3((unsigned)g), dim3(256), 0, s, x, K / 4, ldx, ldp / 4, n4, scale, row_scale, p1, p2);
    ACT_LAUNCH_CHECK(); return 0;
}

}  // namespace

extern "C" int act_split_bf16x2_f32(const float* x, int R, int K, int ldx, uint16_t* hi, uint16_t* lo, act_stream_t stream) {
    return split_planes<false>(x, R, K, ldx, 0.f, nullptr, hi, lo, K, stream);
}
extern "C" int act_split_f16x2_f32(const float* x, int R, int K, int ldx, float scale, const float* row_scale, uint16_t* h1, uint16_t* h2,
                                   act_stream_t stream) {
    return split_planes<true>(x, R, K, ldx, scale, row_scale, h1, h2, K, stream);
}
// the same planes (bit for bit) with rows ldp elements apart: a column slice of a wider plane buffer (ldp >= K, ldp % 8 == 0)
extern "C" int act_split_f16x2_ld_f32(const float* x, int R, int K, int ldx, float scale, uint16_t* h1, uint16_t* h2, int ldp, act_stream_t stream) {
    if (ldp & 7) return ACT_E_BADARG;
    return split_planes<true>(x, R, K, ldx, scale, nullptr, h1, h2, ldp, stream);
}

extern "C" int act_sgemm_nt_bf16x3_supported(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && M % 128 == 0 && N % 128 == 0 && K % 64 == 0; }
extern "C" int act_sgemm_nt_f16x3_supported(int M, int N, int K) { return act_sgemm_nt_bf16x3_supported(M, N, K); }

// Tile by shape alone.  The kernel's time follows how its grid fills the CUs, not the arithmetic; count it in the time one 128 x 128 workgroup takes on a CU
// of its own.  Two 128 x 128 workgroups that share a CU take 2 units, so a full round of 2 * cus workgroups costs 2, and a last round costs 1 if it leaves every
// CU at most one workgroup, else 2.  A CU holds one 128 x 192 workgroup, 1.5 units, so every round of cus workgroups costs 1.5, full or not.  Costs are kept
// in half units.  128 x 192 is taken where it is cheaper by an eighth or more: the count is good to about 10 % (23 shapes, profiles/x3_tiles_micro.txt: grids
// of up to cus workgroups, 1 against 1.5: 128 x 128 faster by 8 - 17 %; 288 and 384 workgroups, 2 against 1.5: 128 x 192 faster by 21 - 26 %; equal counts:
// within 6 % either way), and the teacher's qkv product, 1,152 workgroups at 5 against 4.5, was 5 % faster alone and 2 % slower inside the step
// (profiles/x3_tiles_trace_by_grid_qkv192.txt).  N % 384: 192-wide column tiles within the N % 128 contract.  (K does not enter: both tiles walk the same K loop.)
extern "C" int act_sgemm_nt_f16x3_pick_tile(int M, int N, int K, int cus) {
    if (!act_sgemm_nt_f16x3_supported(M, N, K) || cus <= 0) return 0;
    if (N % 384) return 128;
    const long long t128 = (long long)(M / 128) * (N / 128), t192 = (long long)(M / 128) * (N / 192);
    const long long tail = t128 % (2 * cus);
    const long long c128 = t128 / (2 * cus) * 4 + (tail == 0 ? 0 : tail <= cus ? 2 : 4), c192 = (t192 + cus - 1) / cus * 3;
    return 8 * c192 <= 7 * c128 ? 192 : 128;
}

namespace {
int x3_cu_count() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    return n;
}
bool x3_only_128() {                                               // ACT_X3_TILE=128: every launch on the 128 x 128 tile (A/B runs); read once
    static const bool v = [] { const char* e = getenv("ACT_X3_TILE"); return e && atoi(e) == 128; }();
    return v;
}
// the argument-checked product of both formats.  The scales and the tile belong to the F16 form (a_scale = s_A, b_inv = 1 / s_B per row of B, out_scale = the
// scale the planes-out are split at; tile: 0 = the rule above, 128 / 192 forced); the bf16 form reads none of them and runs the 128 x 128 tile
// Where an operand's planes lie (ACT_X3_ROWMAJOR | ACT_X3_KTILE).  Row-major: rows ld elements apart (0 = dense, K).  K-tile-major: the planes are those of a
// [rows_total][K'] matrix of which the operand is rows r0 .. of K tiles c0 / 32 .., the pointers at x3_kt_index(r0, c0, rows_total) -- ld is not read.
struct X3Layout { int layout = ACT_X3_ROWMAJOR, ld = 0, rows_total = 0; };
// -> false: a layout the kernel cannot walk (rows: the operand's rows; p1, p2: its planes).  KT bases lie on a 128-byte line: that is what the layout is for
bool x3_strides(const X3Layout& l, int rows, int K, const uint16_t* p1, const uint16_t* p2, int& ld, int& kt) {
    if (l.layout == ACT_X3_KTILE) {
        if (l.rows_total < rows || (long long)l.rows_total * BK > 0x7fffffffLL || (((uintptr_t)p1 | (uintptr_t)p2) & 127)) return false;
        ld = BK; kt = l.rows_total * BK; return true;
    }
    if (l.layout != ACT_X3_ROWMAJOR) return false;
    ld = l.ld ? l.ld : K; kt = BK;
    return ld >= K && !(ld & 7);                                    // (K % 64 == 0: the dense stride passes) every row of a plane 16-byte aligned
}

template <bool F16>
int multiply_planes(int M, int N, int K, const uint16_t* a1, const uint16_t* a2, float a_scale, const uint16_t* b1, const uint16_t* b2, const float* b_inv,
                    float* C, int ldc, uint16_t* o1, uint16_t* o2, float out_scale, const act_gemm_epilogue_t* epilogue, act_stream_t stream, int tile,
                    const X3Layout& la = X3Layout{}, const X3Layout& lb = X3Layout{}, int out_layout = ACT_X3_ROWMAJOR) {
    int lda, ldb, kta, ktb;
    if (!x3_strides(la, M, K, a1, a2, lda, kta) || !x3_strides(lb, N, K, b1, b2, ldb, ktb)) return ACT_E_BADARG;
    if (out_layout != ACT_X3_ROWMAJOR && (out_layout != ACT_X3_KTILE || !F16 || (((uintptr_t)o1 | (uintptr_t)o2) & 127))) return ACT_E_BADARG;
    if (!a1 || !a2 || !b1 || !b2 || (F16 && !b_inv) || (!C && !o1) || ((o1 == nullptr) != (o2 == nullptr))) return ACT_E_NULLPTR;
    if (!act_sgemm_nt_bf16x3_supported(M, N, K) || (C && ldc < N) || (F16 && (!(a_scale > 0.f) || (o1 && !(out_scale > 0.f))))) return ACT_E_BADARG;
    if ((((uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)o1 | (uintptr_t)o2 | (uintptr_t)b_inv) & 15)) return ACT_E_BADARG;
    if (F16 && tile != 0 && tile != 128 && !(tile == 192 && N % 192 == 0)) return ACT_E_BADARG;       // a forced tile that the shape does not take
    if (F16 && tile == 0) tile = x3_only_128() ? 128 : act_sgemm_nt_f16x3_pick_tile(M, N, K, x3_cu_count());
    X3Params p{};
    p.Ah = a1; p.Al = a2; p.Bh = b1; p.Bl = b2; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.Oh = o1; p.Ol = o2;
    p.lda = lda; p.ldb = ldb; p.kta = kta; p.ktb = ktb; p.o_kt = out_layout == ACT_X3_KTILE;
    if (F16) { p.b_inv = b_inv; p.a_inv = 1.0f / a_scale; p.o_scale = out_scale; }
    if (epilogue) p.epi = *epilogue; else { p.epi = act_gemm_epilogue_t{}; p.epi.alpha = 1.0f; }
    if (p.epi.accumulate || (p.epi.act != ACT_EPI_NONE && p.epi.act != ACT_EPI_GELU && p.epi.act != ACT_EPI_MUL_GELU_GRAD)) return ACT_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GEMM_BF16X3, s, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
    if constexpr (F16) return tile == 192 ? launch_x3<128, 192, 2, 4, true>(p, s) : launch_x3<128, 128, 2, 2, true>(p, s);
    else return launch_x3<128, 128, 2, 2, false>(p, s);
}
}  // namespace

// ---- the group-max product of the frozen tokenizer's mini-PointNet (composite.hip, act_pointnet_fwd_x3_f32) -------------------------------------------------
extern "C" int act_split_f16x2_affine_relu_f32(const float* x, int R, int K, int ldx, const float* col_scale, const float* col_shift, float scale, uint16_t* h1,
                                               uint16_t* h2, act_stream_t stream) {
    if (!x || !col_scale || !col_shift || !h1 || !h2) return ACT_E_NULLPTR;
    if (R < 0 || K <= 0 || (K & 3) || ldx < K || (ldx & 3) || !(scale > 0.f)) return ACT_E_BADARG;
    if (((uintptr_t)x | (uintptr_t)h1 | (uintptr_t)h2 | (uintptr_t)col_scale | (uintptr_t)col_shift) & 15) return ACT_E_BADARG;
    const long long n4 = (long long)R * K / 4; if (n4 == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, 8.0 * R * (double)K);
    long long g = (n4 + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL((split_planes_kernel<true, true>), dim3((unsigned)g), dim3(256), 0, s, x, K / 4, ldx, K / 4, n4, scale, nullptr, h1, h2, col_scale, col_shift);
    ACT_LAUNCH_CHECK(); return 0;
}
extern "C" int act_sgemm_nt_f16x3_gmax_supported(int M, int N, int K, int group) {
    return act_sgemm_nt_f16x3_supported(M, N, K) && K <= 512 && (group == 32 || group == 64);
}
// Tile of the group-max product by shape alone: the rule of the storing product (notebook/pn_f16x3.md has both tiles measured at the tokenizer's shape)
extern "C" int act_sgemm_nt_f16x3_gmax_pick_tile(int M, int N, int K, int cus) { return act_sgemm_nt_f16x3_pick_tile(M, N, K, cus); }
// b_layout / b_rows_total: where the planes of B lie (X3Layout above)
extern "C" int act_sgemm_nt_f16x3_gmax_layout_f32(int M, int N, int K, const float* A, int lda, const float* a_col_scale, const float* a_col_shift,
                                                  const uint16_t* a_h1, const uint16_t* a_h2, float a_scale, const uint16_t* b_h1, const uint16_t* b_h2,
                                                  int b_layout, int b_rows_total, const float* b_inv_scale, const float* bias, int group, float* out, int ldo,
                                                  int tile, act_stream_t stream) {
    const bool a32 = A != nullptr;
    int ldb, ktb;
    if (!x3_strides(X3Layout{b_layout, 0, b_rows_total}, N, K, b_h1, b_h2, ldb, ktb)) return ACT_E_BADARG;
    if (!b_h1 || !b_h2 || !b_inv_scale || !out || (a32 ? (!a_col_scale || !a_col_shift) : (!a_h1 || !a_h2))) return ACT_E_NULLPTR;
    if (!act_sgemm_nt_f16x3_gmax_supported(M, N, K, group) || ldo < N || !(a_scale > 0.f) || (a32 && (lda < K || (lda & 3)))) return ACT_E_BADARG;
    if (((uintptr_t)A | (uintptr_t)a_col_scale | (uintptr_t)a_col_shift | (uintptr_t)a_h1 | (uintptr_t)a_h2 | (uintptr_t)b_h1 | (uintptr_t)b_h2 |
         (uintptr_t)b_inv_scale) & 15) return ACT_E_BADARG;
    if (tile != 0 && tile != 128 && !(tile == 192 && N % 192 == 0)) return ACT_E_BADARG;
    if (tile == 0) tile = x3_only_128() ? 128 : act_sgemm_nt_f16x3_gmax_pick_tile(M, N, K, x3_cu_count());
    X3Params p{};
    p.ldb = ldb; p.kta = BK; p.ktb = ktb;
    p.A32 = A; p.lda = a32 ? lda : K; p.a_sc = a_col_scale; p.a_sh = a_col_shift; p.a_fold = a_scale; p.Ah = a_h1; p.Al = a_h2; p.Bh = b_h1; p.Bl = b_h2;
    p.C = out; p.ldc = ldo; p.M = M; p.N = N; p.K = K; p.group = group; p.b_inv = b_inv_scale; p.a_inv = 1.0f / a_scale;
    p.epi = act_gemm_epilogue_t{}; p.epi.alpha = 1.0f; p.epi.bias = bias;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_GEMM_BF16X3, s, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)(M / group) * N));
    return tile == 192 ? launch_x3_gmax<128, 192, 2, 4>(p, a32, s) : launch_x3_gmax<128, 128, 2, 2>(p, a32, s);
}

extern "C" int act_sgemm_nt_f16x3_gmax_f32(int M, int N, int K, const float* A, int lda, const float* a_col_scale, const float* a_col_shift,
                                           const uint16_t* a_h1, const uint16_t* a_h2, float a_scale, const uint16_t* b_h1, const uint16_t* b_h2,
                                           const float* b_inv_scale, const float* bias, int group, float* out, int ldo, int tile, act_stream_t stream) {
    return act_sgemm_nt_f16x3_gmax_layout_f32(M, N, K, A, lda, a_col_scale, a_col_shift, a_h1, a_h2, a_scale, b_h1, b_h2, ACT_X3_ROWMAJOR, 0, b_inv_scale, bias,
                                              group, out, ldo, tile, stream);
}

extern "C" int act_sgemm_nt_bf16x3_f32(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_lo, const uint16_t* b_hi, const uint16_t* b_lo,
                                       float* C, int ldc, const act_gemm_epilogue_t* epilogue, act_stream_t stream) {
    return multiply_planes<false>(M, N, K, a_hi, a_lo, 0.f, b_hi, b_lo, nullptr, C, ldc, nullptr, nullptr, 0.f, epilogue, stream, 128);
}
extern "C" int act_sgemm_nt_bf16x3_planes_f32(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_lo, const uint16_t* b_hi, const uint16_t* b_lo,
                                              float* C, int ldc, uint16_t* out_hi, uint16_t* out_lo, const act_gemm_epilogue_t* epilogue,
                                              act_stream_t stream) {
    return multiply_planes<false>(M, N, K, a_hi, a_lo, 0.f, b_hi, b_lo, nullptr, C, ldc, out_hi, out_lo, 0.f, epilogue, stream, 128);
}
// ---- the f16 form (default teacher path) --------------------------------------------------------------------------------------------------------------------
extern "C" int act_sgemm_nt_f16x3_planes_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, float a_scale, const uint16_t* b_h1,
                                             const uint16_t* b_h2, const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2,
                                             float out_scale, const act_gemm_epilogue_t* epilogue, act_stream_t stream) {
    return multiply_planes<true>(M, N, K, a_h1, a_h2, a_scale, b_h1, b_h2, b_inv_scale, C, ldc, out_h1, out_h2, out_scale, epilogue, stream, 0);
}
extern "C" int act_sgemm_nt_f16x3_planes_tile_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, float a_scale, const uint16_t* b_h1,
                                                  const uint16_t* b_h2, const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2,
                                                  float out_scale, const act_gemm_epilogue_t* epilogue, act_stream_t stream, int tile) {
    return multiply_planes<true>(M, N, K, a_h1, a_h2, a_scale, b_h1, b_h2, b_inv_scale, C, ldc, out_h1, out_h2, out_scale, epilogue, stream, tile);
}
// A planes as a column slice of a wider plane buffer: rows lda elements apart (lda >= K, lda % 8 == 0, a_h1 / a_h2 16-byte aligned); otherwise the entry above
extern "C" int act_sgemm_nt_f16x3_planes_lda_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, int lda, float a_scale, const uint16_t* b_h1,
                                                 const uint16_t* b_h2, const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2,
                                                 float out_scale, const act_gemm_epilogue_t* epilogue, act_stream_t stream, int tile) {
    if (lda <= 0) return ACT_E_BADARG;
    return multiply_planes<true>(M, N, K, a_h1, a_h2, a_scale, b_h1, b_h2, b_inv_scale, C, ldc, out_h1, out_h2, out_scale, epilogue, stream, tile,
                                 X3Layout{ACT_X3_ROWMAJOR, lda, 0});
}
// the general entry: each operand, and the planes-out, row-major or K-tile-major (X3Layout above; a row-major B is dense)
extern "C" int act_sgemm_nt_f16x3_planes_layout_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, int a_layout, int lda, int a_rows_total,
                                                    float a_scale, const uint16_t* b_h1, const uint16_t* b_h2, int b_layout, int b_rows_total,
                                                    const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2, float out_scale,
                                                    int out_layout, const act_gemm_epilogue_t* epilogue, act_stream_t stream, int tile) {
    if (lda < 0) return ACT_E_BADARG;
    return multiply_planes<true>(M, N, K, a_h1, a_h2, a_scale, b_h1, b_h2, b_inv_scale, C, ldc, out_h1, out_h2, out_scale, epilogue, stream, tile,
                                 X3Layout{a_layout, lda, a_rows_total}, X3Layout{b_layout, 0, b_rows_total}, out_layout);
}

// ---- K-tile-major planes ------------------------------------------------------------------------------------------------------------------------------------
// a pure copy of one 16-bit plane [R][K] (dense) into the K-tile-major layout; K % 32 == 0, both 16-byte aligned, src != dst
extern "C" int act_repack_ktile_u16(const uint16_t* src, uint16_t* dst, int R, int K, act_stream_t stream) {
    if (!src || !dst) return ACT_E_NULLPTR;
    if (R < 0 || K <= 0 || (K % BK) || src == dst || (((uintptr_t)src | (uintptr_t)dst) & 15)) return ACT_E_BADARG;
    const long long n8 = (long long)R * K / 8; if (n8 == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, 4.0 * R * (double)K);
    long long g = (n8 + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(repack_ktile_kernel, dim3((unsigned)g), dim3(256), 0, s, reinterpret_cast<const u32x4v*>(src), reinterpret_cast<u32x4v*>(dst), R, K / 8, n8);
    ACT_LAUNCH_CHECK(); return 0;
}
// act_split_f16x2_f32 (no row scales) whose planes leave K-tile-major, as rows 0 .. R of a [rows_total][K] plane; K % 32 == 0, planes 128-byte aligned
extern "C" int act_split_f16x2_kt_f32(const float* x, int R, int K, int ldx, float scale, uint16_t* h1, uint16_t* h2, int rows_total, act_stream_t stream) {
    if (!x || !h1 || !h2) return ACT_E_NULLPTR;
    if (R < 0 || K <= 0 || (K % BK) || ldx < K || (ldx & 3) || !(scale > 0.f) || rows_total < R || (long long)rows_total * BK > 0x7fffffffLL ||
        ((uintptr_t)x & 15) || (((uintptr_t)h1 | (uintptr_t)h2) & 127))
        return ACT_E_BADARG;
    const long long n4 = (long long)R * K / 4; if (n4 == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ELTWISE, s, 0.0, 8.0 * R * (double)K);
    long long g = (n4 + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(split_planes_kernel<true>, dim3((unsigned)g), dim3(256), 0, s, x, K / 4, ldx, K / 4, n4, scale, nullptr, h1, h2, nullptr, nullptr, rows_total);
    ACT_LAUNCH_CHECK(); return 0;
}
