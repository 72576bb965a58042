// attention.hip -- fused multi-head self-attention for the short sequences of ACT (S = 14 / 64 / 128 tokens, up to a few hundred in the
// stress shapes; head_dim 64 or 32; models/act.py:57-69 == utils/transformer_layers.py:170-182):  softmax(q k^T * hd^-1/2) v, fp32 throughout.
// The packed projection output qkv [B,S,3,H,hd] is consumed in place and the result is written in the [B,S,H*hd] layout the output projection
// GEMM reads -- no permutes, no S x S matrix in memory.  Keys / values may come from two row segments (S0 prompt-prefix rows of kv0 [B,S0,2,H,hd],
// then the Sq rows of the packed qkv); packed self-attention is the S0 = 0 case.  No atomics anywhere: results are bit-identical from run to run.
//
// Five kernel families, picked by (Sq, S0, head_dim) alone (attn_forward / attn_backward at the end of the file):
//   attn_small_fwd_kernel<HD>      packed qkv, S <= 16            one wave per (cloud, head), 16x16x4 MFMAs, registers only
//   attn_small_bwd_kernel<HD>      packed qkv, S <= 16            the same for the backward
//   attn_fwd_kernel<HD,JT,QT>      every other forward            K / V chunks staged in LDS, one wave per 32 queries, online softmax
//   attn_bwd_one_kernel<HD,KW>     backward, Sq >= 32 and         single pass: S and dP once per 32x32 tile pair, dK / dV in registers,
//                                  S0 % 32 == 0 (attn_reg_ok)     dQ partials summed through LDS
//   attn_bwd_mfma_kernel<HD>       every other backward           one workgroup per (cloud, head), 64x64 tiles through LDS
//
// Forward (attn_fwd_kernel): one wave owns 32 query rows of one (cloud, head).  It computes the TRANSPOSED score tile S^T = K Q^T with
// v_mfma_f32_32x32x2_f32 so that, in the MFMA C/D layout, every lane ends up holding all scores of ONE query
// (its lane&31) for 16 keys per 32-key tile: softmax is then a pure in-register reduction plus a single
// lane^32 exchange, and the probabilities are already in the B-operand layout of the second product
// O^T = V^T P^T.  K and V are staged once per (cloud, head) in LDS ([key][hd+4]: conflict-free b128 A-operand
// reads for K, conflict-free b32 reads for V); Q rows are loaded straight into registers.
// All backward kernels recompute P from the saved log-sum-exp and write dqkv (and dkv0) in the layout of their inputs.
#include "attn_frag.h"
#include "split_planes.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

// General operand description: queries come from `q` (Sq rows per cloud), keys/values from up to two row segments
// (segment 0: S0 rows, e.g. the prompt tokens of the teacher; segment 1: S1 rows).  Packed qkv is the special case
// S0 = 0, k1 = qkv + H*hd, v1 = qkv + 2*H*hd.  All pointers address head 0; head h adds h*HD.
struct AttnFwdArgs {
    const float* q; const float* k0; const float* v0; const float* k1; const float* v1;
    long long q_bs, kv0_bs, kv1_bs;      // per-cloud strides (floats)
    int ldq, ld0, ld1;                   // row strides (floats)
    int B, H, Sq, S0, S1;
    float scale;
    float* out; float* lse;              // out [B, Sq, H*HD]; lse [B, H, Sq] or null
    unsigned short* out_hi; unsigned short* out_lo;   // optional: out ALSO / ONLY (out == null) as planes of the same layout, the A operand of a split-operand projection
    PlaneFmt fmt;                        // ... in this format (split_planes.h): bf16 for the opt-in teacher, f16 at a scale for the default one
};

// JT = 32-key tiles per LDS-resident key chunk.  A sequence longer than one chunk runs an online softmax over the chunks -- running
// max m and sum l per query; the rescale of the output accumulators is a per-lane scalar because every accumulator register of a lane
// belongs to the same query.  QT = 32-query tiles per (cloud, head) handled by a workgroup of four waves, which holds 4 / QT (cloud, head)
// pairs (at least one).  attn_forward picks both from (Sq, S0).
template <int HD, int JT, int QT>
__global__ __launch_bounds__(256, (JT == 1 ? 3 : 2)) void attn_fwd_kernel(const AttnFwdArgs a) {
    constexpr int NTHR = 256;
    constexpr int LDK = HD + 4;
    constexpr int PAIRS = 4 / QT;                                   // (cloud, head) pairs per workgroup: 4 / 2 / 1 / 1 for QT = 1 .. 4
    static_assert(PAIRS >= 1, "a workgroup holds at least the query tiles of one pair");
    constexpr int ROWS = JT * 32;
    constexpr int KSZ = ROWS * LDK, PSZ = 2 * KSZ;                  // floats per pair: K image, V image
    static_assert((ROWS * (HD / 4)) % NTHR == 0, "staging: whole iterations per pair");
    extern __shared__ __attribute__((aligned(16))) float smem[];    // [PAIRS][K image | V image]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, Sk = a.S0 + a.S1;
    const long long npairs = (long long)a.B * H;
    const long long pair0 = (long long)blockIdx.x * PAIRS;
    const int qblock = blockIdx.y * (QT * 32);                       // first query row of this workgroup

    const int pl = wave / QT, qt = wave % QT;
    const long long pr = pair0 + pl;
    const bool active = pl < PAIRS && pr < npairs && qblock + qt * 32 < a.Sq;
    const int b = active ? (int)(pr / H) : 0, h = active ? (int)(pr % H) : 0;
    const float* Ks = smem + (size_t)pl * PSZ;
    const float* Vs = smem + (size_t)pl * PSZ + KSZ;
    const int ql = lane & 31, half = lane >> 5;
    const int q = qblock + qt * 32 + ql;
    const float scale = a.scale;
    const float sc2 = scale * ATT_LOG2E;             // scale * log2(e)

    // ---- Q operand: lane (q, half) holds Q[q][half*HD/2 + s], s = 0..HD/2-1
    float qreg[HD / 2];
    if (active) {
        const float* qp = a.q + (size_t)b * a.q_bs + (size_t)min(q, a.Sq - 1) * a.ldq + h * HD + half * (HD / 2);
#pragma unroll
        for (int s4 = 0; s4 < HD / 8; ++s4) {
            float4 t = *reinterpret_cast<const float4*>(qp + s4 * 4);
            if (q >= a.Sq) t = make_float4(0.f, 0.f, 0.f, 0.f);
            qreg[s4 * 4 + 0] = t.x; qreg[s4 * 4 + 1] = t.y; qreg[s4 * 4 + 2] = t.z; qreg[s4 * 4 + 3] = t.w;
        }
    }
    f32x16 o[HD / 32];
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -3.0e38f, l = 0.f;

    // Staging is software-pipelined across key chunks: the float4 of chunk c+1 are requested right after chunk c went to LDS and stay in flight in
    // registers while chunk c is multiplied -- with one 32-key chunk resident per step (JT = 1: the teacher's 64 x 128 prefix shape, 4 chunks) the loop was
    // load-latency bound: every chunk paid a full L2 / fabric round trip between its two barriers (MfmaUtil 36 %).  ROWS * HD / 4 is a multiple of 256, so all
    // threads of an iteration work on the same pair: the (cloud, head) split is wave-uniform 32-bit arithmetic done once per pair, not a 64-bit division per float4.
    // Only for JT <= 2 and QT >= 2 (8 float4 per thread at JT = 1; the larger resident chunks would need 64-128 staging registers -- 256 at JT = 4, QT = 1 -- and
    // lose a wave per SIMD or spill: they stage straight from global memory to LDS in the chunk loop).
    constexpr int ITS = ROWS * (HD / 4) / NTHR;
    constexpr bool PF = (JT <= 2 && QT >= 2);
    float4 kreg[PAIRS][ITS], vreg[PAIRS][ITS];
    // where staging item idx of a pair goes inside the pair's V image.  (Kept as a helper evaluated per item: spelling it through the caller's rl / c4, as for
    // K, is the same address but moves the register allocation of most instantiations by a few VGPRs.)
    auto v_lds_offset = [&](int idx) -> int { return (idx / (HD / 4)) * LDK + (idx % (HD / 4)) * 4; };
    // (cloud, head) of every pair of the workgroup: wave-uniform, divided ONCE (a 32-bit division is ~25 VALU instructions, and it sat inside the chunk loop)
    int pb[PAIRS], ph[PAIRS];
#pragma unroll
    for (int p2 = 0; p2 < PAIRS; ++p2) {
        const unsigned pr2 = (unsigned)pair0 + p2;
        const bool live = (long long)pr2 < npairs;
        const unsigned b2 = live ? pr2 / (unsigned)H : 0u;
        pb[p2] = __builtin_amdgcn_readfirstlane((int)b2);
        ph[p2] = __builtin_amdgcn_readfirstlane((int)(live ? pr2 - b2 * (unsigned)H : 0u));
    }
    const bool all_live = pair0 + PAIRS <= npairs;
    auto load_chunk = [&](int kc) {
        // fast path: a FULL chunk inside ONE key segment, every pair of the workgroup live -- all rows valid, base pointer and row pitch are
        // wave-uniform: an SGPR base plus one 32-bit lane offset per item instead of per-item compares, 64-bit address arithmetic and exec-masked
        // branches (the PMC pass showed 6.5 VALU instructions per MFMA at the teacher shape, 110 of the 290 per chunk in this staging code)
        const bool in0 = kc + ROWS <= a.S0, in1 = kc >= a.S0 && kc + ROWS <= Sk;
        if (all_live && (in0 || in1)) {
            const unsigned ld = in0 ? a.ld0 : a.ld1;
            const int r0 = in0 ? kc : kc - a.S0;
#pragma unroll
            for (int p2 = 0; p2 < PAIRS; ++p2) {
                const size_t po = (in0 ? (size_t)pb[p2] * a.kv0_bs : (size_t)pb[p2] * a.kv1_bs) + (size_t)ph[p2] * HD + (size_t)r0 * ld;
                const float* kb = (in0 ? a.k0 : a.k1) + po; const float* vb = (in0 ? a.v0 : a.v1) + po;
#pragma unroll
                for (int it = 0; it < ITS; ++it) {
                    const int idx = tid + NTHR * it;
                    const unsigned of = (unsigned)(idx / (HD / 4)) * ld + (idx % (HD / 4)) * 4;
                    kreg[p2][it] = *reinterpret_cast<const float4*>(kb + of);
                    vreg[p2][it] = *reinterpret_cast<const float4*>(vb + of);
                }
            }
            return;
        }
#pragma unroll
        for (int p2 = 0; p2 < PAIRS; ++p2) {
            const unsigned pr2 = (unsigned)pair0 + p2;
            const bool live = (long long)pr2 < npairs;
            const unsigned b2 = (unsigned)pb[p2], h2 = (unsigned)ph[p2];
            const float* k0p = a.k0 + (size_t)b2 * a.kv0_bs + h2 * HD; const float* v0p = a.v0 + (size_t)b2 * a.kv0_bs + h2 * HD;
            const float* k1p = a.k1 + (size_t)b2 * a.kv1_bs + h2 * HD; const float* v1p = a.v1 + (size_t)b2 * a.kv1_bs + h2 * HD;
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                const int idx = tid + NTHR * it;
                const int c4 = idx % (HD / 4), rl = idx / (HD / 4), row = kc + rl;
                float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx;
                if (live && row < Sk) {
                    if (row < a.S0) {
                        const unsigned of = (unsigned)row * a.ld0 + c4 * 4;
                        kx = *reinterpret_cast<const float4*>(k0p + of); vx = *reinterpret_cast<const float4*>(v0p + of);
                    } else {
                        const unsigned of = (unsigned)(row - a.S0) * a.ld1 + c4 * 4;
                        kx = *reinterpret_cast<const float4*>(k1p + of); vx = *reinterpret_cast<const float4*>(v1p + of);
                    }
                }
                kreg[p2][it] = kx; vreg[p2][it] = vx;
            }
        }
    };
    if constexpr (PF) load_chunk(0);
    for (int kc = 0; kc < Sk; kc += ROWS) {
        if (kc > 0) __syncthreads();                                 // previous chunk fully consumed
        if constexpr (PF) {
            // ---- this chunk of K and V (zero rows beyond Sk) for every pair of the workgroup: registers -> LDS, then request the next chunk
#pragma unroll
            for (int p2 = 0; p2 < PAIRS; ++p2) {
                float* kd = smem + (size_t)p2 * PSZ; float* vd = kd + KSZ;
#pragma unroll
                for (int it = 0; it < ITS; ++it) {
                    const int idx = tid + NTHR * it;
                    const int c4 = idx % (HD / 4), rl = idx / (HD / 4);
                    *reinterpret_cast<float4*>(kd + rl * LDK + c4 * 4) = kreg[p2][it];
                    *reinterpret_cast<float4*>(vd + v_lds_offset(idx)) = vreg[p2][it];
                }
            }
            if (kc + ROWS < Sk) load_chunk(kc + ROWS);
        } else {
            // ---- stage this chunk of K and V for every pair of the workgroup (zero rows beyond Sk), global memory -> LDS without the register form of
            // load_chunk (see PF above).  ROWS * HD / 4 is a multiple of 256, so all threads of an iteration work on the same pair: the (cloud, head)
            // split is wave-uniform 32-bit arithmetic done once per pair, not a 64-bit division per staged float4
#pragma unroll
            for (int p2 = 0; p2 < PAIRS; ++p2) {
                const unsigned pr2 = (unsigned)pair0 + p2;
                const bool live = (long long)pr2 < npairs;
                const unsigned b2 = live ? pr2 / (unsigned)H : 0u, h2 = live ? pr2 - b2 * (unsigned)H : 0u;
                const float* k0p = a.k0 + (size_t)b2 * a.kv0_bs + h2 * HD; const float* v0p = a.v0 + (size_t)b2 * a.kv0_bs + h2 * HD;
                const float* k1p = a.k1 + (size_t)b2 * a.kv1_bs + h2 * HD; const float* v1p = a.v1 + (size_t)b2 * a.kv1_bs + h2 * HD;
                float* kd = smem + (size_t)p2 * PSZ; float* vd = kd + KSZ;
#pragma unroll
                for (int it = 0; it < ROWS * (HD / 4) / NTHR; ++it) {
                    const int idx = tid + NTHR * it;
                    const int c4 = idx % (HD / 4), rl = idx / (HD / 4), row = kc + rl;
                    float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx;
                    if (live && row < Sk) {
                        if (row < a.S0) {
                            const unsigned of = (unsigned)row * a.ld0 + c4 * 4;
                            kx = *reinterpret_cast<const float4*>(k0p + of); vx = *reinterpret_cast<const float4*>(v0p + of);
                        } else {
                            const unsigned of = (unsigned)(row - a.S0) * a.ld1 + c4 * 4;
                            kx = *reinterpret_cast<const float4*>(k1p + of); vx = *reinterpret_cast<const float4*>(v1p + of);
                        }
                    }
                    *reinterpret_cast<float4*>(kd + rl * LDK + c4 * 4) = kx;
                    *reinterpret_cast<float4*>(vd + v_lds_offset(idx)) = vx;
                }
            }
        }
        __syncthreads();
        if (!active) continue;                                       // idle waves only help staging
        // ---- S^T tiles: acc[jt][r] = score(key = kc + jt*32 + (r&3) + 8*(r>>2) + 4*half, query = ql)
        f32x16 acc[JT];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[jt][r] = 0.f;
            const float* kp = Ks + (size_t)(jt * 32 + ql) * LDK + half * (HD / 2);
#pragma unroll
            for (int s4 = 0; s4 < HD / 8; ++s4) {
                const float4 kk = *reinterpret_cast<const float4*>(kp + s4 * 4);
                acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.x, qreg[s4 * 4 + 0], acc[jt], 0, 0, 0);
                acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.y, qreg[s4 * 4 + 1], acc[jt], 0, 0, 0);
                acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.z, qreg[s4 * 4 + 2], acc[jt], 0, 0, 0);
                acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk.w, qreg[s4 * 4 + 3], acc[jt], 0, 0, 0);
            }
        }
        // ---- online softmax over keys (registers + one lane^32 exchange)
        float mc = -3.0e38f;
        if (kc + ROWS <= Sk) {                                       // (wave-uniform) a full chunk has no key to mask: 3 VALU instructions per score less
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) mc = fmaxf(mc, acc[jt][r]);
        } else {
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kc + jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const float v = key < Sk ? acc[jt][r] : -3.0e38f;
                    acc[jt][r] = v;
                    mc = fmaxf(mc, v);
                }
        }
        mc = fmaxf(mc, __shfl_xor(mc, 32));
        const float mn = fmaxf(m, mc);
        // exp(scale (s - m)) = exp2(s c - m c), c = scale log2(e): ONE packed FMA per two scores in front of v_exp_f32 instead of sub + mul + mul per score, and the
        // row sum as packed adds.  On gfx950 no VALU instruction overlaps an f32 MFMA of the same SIMD (profiles/r06_mfma_valu_kinds.txt): every instruction removed
        // here is matrix-pipe time.  (m c is rounded once: a score equal to the maximum gives exp2(+-1 ulp of m c) instead of exactly 1 -- 1e-7.)
        const float mcn = mn * sc2;
        const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(m, sc2, -mcn));       // 0 on the first chunk (m = -huge)
        m = mn;
        f32x2 lc2 = f32x2{0.f, 0.f};
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 t = __builtin_elementwise_fma(f32x2{acc[jt][r], acc[jt][r + 1]}, f32x2{sc2, sc2}, f32x2{-mcn, -mcn});
                const f32x2 p = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};     // masked keys: exp2(-huge) == 0
                acc[jt][r] = p[0]; acc[jt][r + 1] = p[1];
                lc2 += p;
            }
        float lc = lc2[0] + lc2[1];
        lc += __shfl_xor(lc, 32);
        l = l * alpha + lc;
        if (kc > 0) {
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
        // ---- O^T += V^T P^T : o[dt][r] = out(d = dt*32 + (r&3) + 8*(r>>2) + 4*half, query = ql)
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;   // this half-wave's k index for step r
                const float* vp = Vs + (size_t)key * LDK + ql;
#pragma unroll
                for (int dt = 0; dt < HD / 32; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[dt * 32], acc[jt][r], o[dt], 0, 0, 0);
            }
    }
    if (active && q < a.Sq) {
        const float inv_l = 1.0f / l;
        const size_t obase = ((size_t)b * a.Sq + q) * (H * HD) + h * HD;
        float* op = a.out ? a.out + obase : nullptr;
#pragma unroll
        for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 t;
                t.x = o[dt][g * 4 + 0] * inv_l; t.y = o[dt][g * 4 + 1] * inv_l;
                t.z = o[dt][g * 4 + 2] * inv_l; t.w = o[dt][g * 4 + 3] * inv_l;
                if (op) *reinterpret_cast<float4*>(op + dt * 32 + 8 * g + 4 * half) = t;
                if (a.out_hi) store_planes4(a.fmt, a.out_hi, a.out_lo, (obase + dt * 32 + 8 * g + 4 * half) >> 2, t);   // the projection's A operand
            }
        if (a.lse && half == 0) a.lse[((size_t)b * H + h) * a.Sq + q] = scale * m + __logf(l);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Attention backward on the matrix cores (fp32-input v_mfma_f32_32x32x2).  One workgroup (4 waves) per (cloud, head); keys come
// from two sources (S0 "prefix" rows of kv0, then the Sq rows of qkv1), so the same kernel serves plain self-attention (S0 = 0)
// and the prompt-prefix attention of the prompt-tuned Transformer (models/dvae.py:536-576).  Per (64-key, 64-query) tile pair:
//   S = Q K^T -> P = exp(scale S - lse) ; dP = dO V^T ; dS = P (dP - D) scale            (wave = one 32x32 quadrant, in regs)
//   dV += P^T dO ; dK += dS^T Q   (accumulated in registers over the query tiles, one [32 keys x 32 dims] quadrant per wave)
//   dQ (+)= dS K                  (accumulated over key tiles through global memory: the workgroup owns its dQ rows)
// Operands of the two head-dimension reductions (S, dP) never touch LDS: the MFMA k-index is free to be any permutation as
// long as A and B agree, so lane half 0 reduces d in [0,HD/2) and half 1 d in [HD/2,HD) and each lane keeps HD/2 CONTIGUOUS
// floats of its Q / dO / K / V row in registers (float4 global loads, K/V fragments live across the query loop).
// The three row reductions take their B operand from row-major LDS tiles Q, dO, K [64][HD] (two consecutive rows land in
// opposite bank halves through an XOR-32 column swizzle) and their A operand from one P/dS tile [64][65].
// Invalid rows are zero-filled and masked out of P; quadrants and reduction ranges made of padding only are skipped.
struct AttnBwdArgs {
    const float* kv0; const float* qkv1; const float* out; const float* dout; const float* lse;
    float* dkv0; float* dqkv1;
    int B, S0, Sq, H; float scale;
};

template <int HD>
__global__ __launch_bounds__(256, 2) void attn_bwd_mfma_kernel(const AttnBwdArgs a) {
    constexpr int LDP = 65, DQ = HD / 4, T = 64, FR = HD / 8;      // FR float4 per lane fragment (HD/2 floats)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem; float* Os = Qs + T * HD; float* Ks = Os + T * HD;
    float* Ps = Ks + T * HD; float* Dl = Ps + T * LDP; float* Ll = Dl + T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, khalf = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;               // quadrant of a 64x64 (or 64xHD) tile owned by this wave
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const int D = a.H * HD, rs1 = 3 * D, rs0 = 2 * D;
    const int Skv = a.S0 + a.Sq;
    const float* q_base = a.qkv1 + (size_t)b * a.Sq * rs1 + h * HD;
    float* dq_base = a.dqkv1 + (size_t)b * a.Sq * rs1 + h * HD;
    const bool colq = wc * 32 < HD;                         // HD = 32: only the wc = 0 waves own an output quadrant
    // column of this lane inside a row-major [row][HD] tile for the B-operand fetches of rows (2j + khalf)
    const int bcol = HD == 64 ? ((wc * 32 + l32) ^ (32 * khalf)) : l32;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int k0 = 0; k0 < Skv; k0 += T) {
        const int kn = min(T, Skv - k0);
        __syncthreads();                                    // previous key tile fully consumed
        for (int idx = tid; idx < T * DQ; idx += 256) {     // K tile -> LDS (B operand of dQ)
            const int c4 = idx % DQ, row = idx / DQ, kr = k0 + row;
            float4 kx = z4;
            if (row < kn)
                kx = kr < a.S0 ? *reinterpret_cast<const float4*>(a.kv0 + ((size_t)b * a.S0 + kr) * rs0 + h * HD + c4 * 4)
                               : *reinterpret_cast<const float4*>(q_base + (size_t)(kr - a.S0) * rs1 + D + c4 * 4);
            const int col = HD == 64 ? ((c4 * 4) ^ (32 * (row & 1))) : c4 * 4;
            *reinterpret_cast<float4*>(Ks + row * HD + col) = kx;
        }
        // K / V register fragments of this wave's key rows (wc) for the S and dP products
        float4 kf[FR], vf[FR];
        {
            const int row = wc * 32 + l32, kr = k0 + row;
#pragma unroll
            for (int i = 0; i < FR; ++i) { kf[i] = z4; vf[i] = z4; }
            if (row < kn) {
                const float* kb = kr < a.S0 ? a.kv0 + ((size_t)b * a.S0 + kr) * rs0 + h * HD : q_base + (size_t)(kr - a.S0) * rs1 + D;
                const float* vb = kb + D;
#pragma unroll
                for (int i = 0; i < FR; ++i) {
                    kf[i] = *reinterpret_cast<const float4*>(kb + khalf * (HD / 2) + 4 * i);
                    vf[i] = *reinterpret_cast<const float4*>(vb + khalf * (HD / 2) + 4 * i);
                }
            }
        }
        f32x16 dk_acc, dv_acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk_acc[r] = 0.f; dv_acc[r] = 0.f; }

        for (int q0 = 0; q0 < a.Sq; q0 += T) {
            const int qn = min(T, a.Sq - q0);
            __syncthreads();                                // previous query tile fully consumed (and K staged)
            for (int idx = tid; idx < T * DQ; idx += 256) {             // DQ consecutive lanes own one row
                const int c4 = idx % DQ, row = idx / DQ;
                float4 qx = z4, ox = z4, tx = z4;
                if (row < qn) {
                    const size_t o = ((size_t)b * a.Sq + q0 + row) * D + h * HD + c4 * 4;
                    qx = *reinterpret_cast<const float4*>(q_base + (size_t)(q0 + row) * rs1 + c4 * 4);
                    ox = *reinterpret_cast<const float4*>(a.dout + o);
                    tx = *reinterpret_cast<const float4*>(a.out + o);
                }
                const int col = HD == 64 ? ((c4 * 4) ^ (32 * (row & 1))) : c4 * 4;
                *reinterpret_cast<float4*>(Qs + row * HD + col) = qx;
                *reinterpret_cast<float4*>(Os + row * HD + col) = ox;
                // D[q] = sum_d dO[q][d] * O[q][d]: reduce the DQ per-lane partials inside the 16-lane DPP row
                float part = ox.x * tx.x + ox.y * tx.y + ox.z * tx.z + ox.w * tx.w;
                part += dpp_mov_f<0x111, 0xf>(0.f, part);
                part += dpp_mov_f<0x112, 0xf>(0.f, part);
                part += dpp_mov_f<0x114, 0xf>(0.f, part);
                if (DQ == 16) part += dpp_mov_f<0x118, 0xf>(0.f, part);
                if (c4 == DQ - 1) Dl[row] = part;
                if (c4 == 0) Ll[row] = row < qn ? a.lse[((size_t)b * a.H + h) * a.Sq + q0 + row] : 0.f;
            }
            // ---- S and dP quadrants [32 queries (wr) x 32 keys (wc)], reduction over the head dimension from registers
            f32x16 s_acc, p_acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s_acc[r] = 0.f; p_acc[r] = 0.f; }
            if (wr * 32 < qn && wc * 32 < kn) {             // quadrants made of padding only stay zero
                const int row = wr * 32 + l32;
                float4 qf[FR], of[FR];
#pragma unroll
                for (int i = 0; i < FR; ++i) { qf[i] = z4; of[i] = z4; }
                if (row < qn) {
                    const float* qb = q_base + (size_t)(q0 + row) * rs1 + khalf * (HD / 2);
                    const float* ob = a.dout + ((size_t)b * a.Sq + q0 + row) * D + h * HD + khalf * (HD / 2);
#pragma unroll
                    for (int i = 0; i < FR; ++i) {
                        qf[i] = *reinterpret_cast<const float4*>(qb + 4 * i);
                        of[i] = *reinterpret_cast<const float4*>(ob + 4 * i);
                    }
                }
#pragma unroll
                for (int i = 0; i < FR; ++i) {
                    s_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i].x, kf[i].x, s_acc, 0, 0, 0);
                    p_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(of[i].x, vf[i].x, p_acc, 0, 0, 0);
                    s_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i].y, kf[i].y, s_acc, 0, 0, 0);
                    p_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(of[i].y, vf[i].y, p_acc, 0, 0, 0);
                    s_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i].z, kf[i].z, s_acc, 0, 0, 0);
                    p_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(of[i].z, vf[i].z, p_acc, 0, 0, 0);
                    s_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[i].w, kf[i].w, s_acc, 0, 0, 0);
                    p_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(of[i].w, vf[i].w, p_acc, 0, 0, 0);
                }
            }
            __syncthreads();                                // Q / dO tiles, D and lse visible
            const int kk = wc * 32 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                const float p = (qq < qn && kk < kn) ? __expf(a.scale * s_acc[r] - Ll[qq]) : 0.f;
                Ps[qq * LDP + kk] = p;
                s_acc[r] = p * (p_acc[r] - Dl[qq]) * a.scale;          // dS, kept in registers until P has been consumed
            }
            __syncthreads();
            const int qn2 = (qn + 7) & ~7, kn2 = (kn + 7) & ~7;       // reductions stop at the valid rows (zero padding beyond)
            // ---- dV[k][d] += sum_q P[q][k] dO[q][d]     quadrant: keys wr, dims wc
            if (colq && wr * 32 < kn) {
                const float* pa = Ps + khalf * LDP + wr * 32 + l32;
                const float* ob = Os + khalf * HD + bcol;
#pragma unroll 4
                for (int q = 0; q < qn2; q += 2)
                    dv_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[q * LDP], ob[q * HD], dv_acc, 0, 0, 0);
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                Ps[qq * LDP + kk] = s_acc[r];
            }
            __syncthreads();
            if (colq && wr * 32 < kn) {
                // ---- dK[k][d] += sum_q dS[q][k] Q[q][d]
                const float* pa = Ps + khalf * LDP + wr * 32 + l32;
                const float* qb = Qs + khalf * HD + bcol;
#pragma unroll 4
                for (int q = 0; q < qn2; q += 2)
                    dk_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[q * LDP], qb[q * HD], dk_acc, 0, 0, 0);
            }
            if (colq && wr * 32 < qn) {
                // ---- dQ[q][d] (+)= sum_k dS[q][k] K[k][d]   quadrant: queries wr, dims wc
                f32x16 dq_acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) dq_acc[r] = 0.f;
                const float* sa = Ps + (wr * 32 + l32) * LDP + khalf;
                const float* kb2 = Ks + khalf * HD + bcol;
#pragma unroll 4
                for (int k = 0; k < kn2; k += 2)
                    dq_acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[k], kb2[k * HD], dq_acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qq = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                    if (qq < qn) {
                        float* dst = dq_base + (size_t)(q0 + qq) * rs1 + wc * 32 + l32;
                        *dst = k0 == 0 ? dq_acc[r] : *dst + dq_acc[r];
                    }
                }
            }
        }
        if (colq) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kq = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf, kr = k0 + kq;
                if (kq < kn) {
                    if (kr < a.S0) {
                        float* dst = a.dkv0 + ((size_t)b * a.S0 + kr) * rs0 + h * HD + wc * 32 + l32;
                        dst[0] = dk_acc[r]; dst[D] = dv_acc[r];
                    } else {
                        float* dst = dq_base + (size_t)(kr - a.S0) * rs1 + wc * 32 + l32;
                        dst[D] = dk_acc[r]; dst[2 * D] = dv_acc[r];
                    }
                }
            }
        }
    }
}


// =================================================================================== S <= 16: one wave per (cloud, head), registers only
// The student encoder of Stage II runs on 13 visible tokens + cls = 14 (models/act.py:255): a 32- or 64-wide tile is 80-95 % padding and
// the LDS-staged kernels above are pure latency (7 % MFMA utilisation in the backward).  Here one wave owns one (cloud, head) pair; every
// product is a handful of v_mfma_f32_16x16x4_f32 whose operands come straight from global memory into registers -- no LDS, no barrier:
//   operand "form R" : lane (r = lane&15, g = lane>>4) holds X[r][E*g .. E*g+E-1]  (E = HD/4 contiguous floats, MFMA k-step i uses element i:
//                      the reduction over the head dimension is order-free, so both operands simply use the same permutation)
//   operand "form C" : lane (c, g) holds X[4g + s][16*blk + c] for s = 0..3 (k-step s reduces over rows 4g+s: again a free permutation)
//   MFMA C/D layout  : lane (c, g) holds D[4g + reg][c]
// forward : St = K Q^t (D: key = 4g+reg, query = c) -> softmax over keys = in-lane + two lane^16/32 exchanges -> Pt is directly the
//           B operand of Ot = Vt Pt (key = 4g+s at k-step s) with V in form C; each lane stores 4 consecutive output floats.
// backward: S = Q K^t and St = K Q^t (P and Pt), dP = dO V^t and dPt = V dO^t, dS = P (dP - delta) (both orientations) and then
//           dVt = dOt P, dKt = Qt dS, dQt = Kt dSt with P / dS / dSt as B operands straight from their D registers.
template <int HD>
__device__ __forceinline__ void load_form_r(const float* __restrict__ base, int ld, int r, int g, int S, float* x) {
    constexpr int E = HD / 4;
    if (r < S) {
        const float4* p = reinterpret_cast<const float4*>(base + (size_t)r * ld + E * g);
#pragma unroll
        for (int i = 0; i < E / 4; ++i) { const float4 t = p[i]; x[4 * i] = t.x; x[4 * i + 1] = t.y; x[4 * i + 2] = t.z; x[4 * i + 3] = t.w; }
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) x[i] = 0.f;
    }
}
template <int HD>
__device__ __forceinline__ void load_form_c(const float* __restrict__ base, int ld, int c, int g, int S, float (*x)[HD / 16]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int row = 4 * g + s;
#pragma unroll
        for (int blk = 0; blk < HD / 16; ++blk) x[s][blk] = row < S ? base[(size_t)row * ld + 16 * blk + c] : 0.f;
    }
}
typedef float f32x4s __attribute__((ext_vector_type(4)));

template <int HD>
__global__ __launch_bounds__(256) void attn_small_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                             int B, int S, int H, float scale) {
    constexpr int E = HD / 4, NB = HD / 16;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (long long)B * H) return;
    const int b = (int)(pair / H), h = (int)(pair % H);
    const int D = H * HD, ld = 3 * D;
    const float* q0 = qkv + (size_t)b * S * ld + h * HD;
    float qr[E], kr[E], vc[4][NB];
    load_form_r<HD>(q0, ld, c, g, S, qr);
    load_form_r<HD>(q0 + D, ld, c, g, S, kr);
    load_form_c<HD>(q0 + 2 * D, ld, c, g, S, vc);
    f32x4s st = {0.f, 0.f, 0.f, 0.f};                                  // St[key = 4g+reg][query = c]
#pragma unroll
    for (int i = 0; i < E; ++i) st = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[i], qr[i], st, 0, 0, 0);
    float m = -3.0e38f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { if (4 * g + r >= S) st[r] = -3.0e38f; m = fmaxf(m, st[r]); }
    m = fmaxf(m, __shfl_xor(m, 16)); m = fmaxf(m, __shfl_xor(m, 32));
    float l = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { st[r] = __expf(scale * (st[r] - m)); l += st[r]; }
    l += __shfl_xor(l, 16); l += __shfl_xor(l, 32);
    const float inv_l = 1.0f / l;
    float* op = out + ((size_t)b * S + min(c, S - 1)) * D + h * HD;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {                               // Ot[d = 16 blk + 4g + reg][query = c]; MFMAs outside divergent control flow
        f32x4s o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) o = __builtin_amdgcn_mfma_f32_16x16x4f32(vc[s2][blk], st[s2], o, 0, 0, 0);
        if (c < S) *reinterpret_cast<float4*>(op + 16 * blk + 4 * g) = make_float4(o[0] * inv_l, o[1] * inv_l, o[2] * inv_l, o[3] * inv_l);
    }
    if (lse && g == 0 && c < S) lse[((size_t)b * H + h) * S + c] = scale * m + __logf(l);
}

template <int HD>
__global__ __launch_bounds__(256) void attn_small_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ out, const float* __restrict__ dout,
                                                             const float* __restrict__ lse, float* __restrict__ dqkv, int B, int S, int H, float scale) {
    constexpr int E = HD / 4, NB = HD / 16;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (long long)B * H) return;
    const int b = (int)(pair / H), h = (int)(pair % H);
    const int D = H * HD, ld = 3 * D;
    const float* q0 = qkv + (size_t)b * S * ld + h * HD;
    const float* o0 = out + (size_t)b * S * D + h * HD;
    const float* do0 = dout + (size_t)b * S * D + h * HD;
    float* dq0 = dqkv + (size_t)b * S * ld + h * HD;
    float qr[E], kr[E], vr[E], dor[E], orr[E];
    load_form_r<HD>(q0, ld, c, g, S, qr);
    load_form_r<HD>(q0 + D, ld, c, g, S, kr);
    load_form_r<HD>(q0 + 2 * D, ld, c, g, S, vr);
    load_form_r<HD>(do0, D, c, g, S, dor);
    load_form_r<HD>(o0, D, c, g, S, orr);
    // delta[row c] = sum_d dO[c][d] O[c][d]; log-sum-exp of row c
    float delta = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) delta += dor[i] * orr[i];
    delta += __shfl_xor(delta, 16); delta += __shfl_xor(delta, 32);
    const float lse_c = c < S ? lse[((size_t)b * H + h) * S + c] : 0.f;
    // S / St and dP / dPt
    f32x4s s_qk = {0.f, 0.f, 0.f, 0.f}, s_kq = s_qk, dp = s_qk, dpt = s_qk;
#pragma unroll
    for (int i = 0; i < E; ++i) {
        s_qk = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[i], kr[i], s_qk, 0, 0, 0);      // S [query = 4g+reg][key = c]
        s_kq = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[i], qr[i], s_kq, 0, 0, 0);      // St[key = 4g+reg][query = c]
        dp   = __builtin_amdgcn_mfma_f32_16x16x4f32(dor[i], vr[i], dp, 0, 0, 0);       // dP [query = 4g+reg][key = c]
        dpt  = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[i], dor[i], dpt, 0, 0, 0);      // dPt[key = 4g+reg][query = c]
    }
    f32x4s p, ds, dst;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        // orientation 1: query = row, key = c   (needs lse / delta of the ROW query: fetched from the lane that owns it)
        const float lse_r = __shfl(lse_c, row), del_r = __shfl(delta, row);
        const bool v1 = row < S && c < S;
        p[r] = v1 ? __expf(scale * s_qk[r] - lse_r) : 0.f;
        ds[r] = p[r] * (dp[r] - del_r) * scale;
        // orientation 2: key = row, query = c
        const bool v2 = row < S && c < S;
        const float pt = v2 ? __expf(scale * s_kq[r] - lse_c) : 0.f;
        dst[r] = pt * (dpt[r] - delta) * scale;
    }
    float xc[4][NB];
    // dVt[d][key = c] = sum_q dOt[d][q] P[q][key]      (A: dO form C, B: P)
    load_form_c<HD>(do0, D, c, g, S, xc);
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
        f32x4s a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) a = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[s2][blk], p[s2], a, 0, 0, 0);
        if (c < S) *reinterpret_cast<float4*>(dq0 + 2 * D + (size_t)c * ld + 16 * blk + 4 * g) = make_float4(a[0], a[1], a[2], a[3]);
    }
    // dKt[d][key = c] = sum_q Qt[d][q] dS[q][key]
    load_form_c<HD>(q0, ld, c, g, S, xc);
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
        f32x4s a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) a = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[s2][blk], ds[s2], a, 0, 0, 0);
        if (c < S) *reinterpret_cast<float4*>(dq0 + D + (size_t)c * ld + 16 * blk + 4 * g) = make_float4(a[0], a[1], a[2], a[3]);
    }
    // dQt[d][query = c] = sum_key Kt[d][key] dSt[key][query]
    load_form_c<HD>(q0 + D, ld, c, g, S, xc);
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
        f32x4s a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) a = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[s2][blk], dst[s2], a, 0, 0, 0);
        if (c < S) *reinterpret_cast<float4*>(dq0 + (size_t)c * ld + 16 * blk + 4 * g) = make_float4(a[0], a[1], a[2], a[3]);
    }
}


// =================================================================================== operands of the single-pass backward (fragment forms: attn_frag.h)
// Keys come from two row segments (S0 prefix rows of kv0, then the S1 rows of the packed qkv1), as in the kernels above.
struct AttnRegArgs {
    const float* q;  const float* k0; const float* v0; const float* k1; const float* v1;      // head 0 of row 0 of each operand
    const float* out; const float* dout; const float* lse;
    float* dq; float* dk0; float* dv0; float* dk1; float* dv1;                                // outputs (same strides as the inputs)
    long long q_bs, kv0_bs, kv1_bs;      // per-cloud strides (floats)
    int ldq, ld0, ld1;                   // row strides (floats)
    int B, H, Sq, S0, S1;
    float scale;
};

// Tails without clamps: the LAST 32-row tile of a side is shifted back to end exactly at the last row (rows S-32 .. S-1, all valid) and the
// rows it shares with the previous tile are masked out of P (keys) or simply not stored (owned rows).  So every tile is a full tile inside ONE
// segment (host-side condition: S0 % 32 == 0, S1 >= 32, Sq >= 32), every row address is a wave-uniform base + a 32-bit lane offset, and a
// col-form fetch is a plain run of global_load_dword with SGPR bases.
struct AttSeg { const float* base; int ld; };                           // rows t0 .. t0+31 of a two-segment operand (wave-uniform)
__device__ __forceinline__ AttSeg att_seg_tile(const float* __restrict__ p0, int ld0, const float* __restrict__ p1, int ld1, int S0, int t0) {
    AttSeg g;
    if (t0 >= S0) { g.base = p1 + (size_t)(t0 - S0) * ld1; g.ld = ld1; } else { g.base = p0 + (size_t)t0 * ld0; g.ld = ld0; }
    return g;
}
template <int HD>
__device__ __forceinline__ void att_load_row_form(const AttSeg g, int row, int half, float* x) {              // lane's own row of the tile
    const unsigned off = (unsigned)(row * g.ld + half * (HD / 2));
#pragma unroll
    for (int i = 0; i < HD / 8; ++i) {
        const float4 t = *reinterpret_cast<const float4*>(g.base + off + 4 * i);
        x[4 * i] = t.x; x[4 * i + 1] = t.y; x[4 * i + 2] = t.z; x[4 * i + 3] = t.w;
    }
}
template <int HD>
__device__ __forceinline__ void att_load_col_form(const AttSeg g, int c, int half, float (*x)[HD / 32]) {
    // The m index of the products that consume a col form (the head dimension d of O^t, dQ^t, dK^t, dV^t) is free to be any permutation as long as
    // the store agrees: lane c holds d = (HD/32) * c + dt, so its HD/32 values per row are CONTIGUOUS -- one dwordx2 load per row and lane pair of
    // accumulators instead of two dword loads 128 bytes apart (global-load instructions per tile are what these kernels are short of).
    constexpr int NDT = HD / 32;
    const unsigned lane_off = (unsigned)(4 * half * g.ld + NDT * c);     // per-lane part; the row part below is wave-uniform
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float* rb = g.base + (size_t)ATT_F(r, 0) * g.ld;
        if constexpr (NDT == 2) {
            const float2 v = *reinterpret_cast<const float2*>(rb + lane_off);
            x[r][0] = v.x; x[r][1] = v.y;
        } else {
            x[r][0] = rb[lane_off];
        }
    }
}
// =================================================================================== single-pass backward
// S and dP are computed ONCE per 32x32 tile pair (160 MFMAs), and only one fragment per tile pair comes from global memory:
//   * a workgroup = KW waves owns ONE (cloud, head) pair; wave kw owns 32 keys of the current block of KW key tiles: K, V rows stay in
//     registers (row form) and dK^t, dV^t accumulate in registers over all query tiles;
//   * the 32-query tile of Q and dO is staged ONCE per pair in LDS ([32][HD + 4]; both fragment forms are conflict-free reads of it: row form = b128,
//     col form = b64) together with lse and D = rowsum(dO * O) of its queries, instead of 40 global loads per wave and tile pair;
//   * dS goes through a wave-private [32][36] LDS tile to come back transposed (4 x ds_write_b128 + 16 x ds_read_b32, no barrier: the wave's own LDS
//     queue is in order), which makes dS^t the B operand of the wave's partial dQ^t = K^t dS^t over ITS 32 keys (K in col form: the only global fragment);
//   * the KW partial dQ tiles of a pair meet in LDS and are summed in wave order by the pair's threads (deterministic, no atomics); with more than one
//     key block the sum continues through global memory (the workgroup owns its rows).
// Two workgroup barriers per query tile (stage -> compute -> reduce); two workgroups per CU cover each other's staging.  Tails as above: the last
// tile of a side is shifted back to end at the last row, the rows it shares with its neighbour are masked out of P / not stored.
// KW = 2 for up to 64 keys (128-thread workgroups: the 768 pairs of the student decoder spread over three workgroups per CU), else 4.
template <int HD, int KW>
__global__ __launch_bounds__(64 * KW, 2) void attn_bwd_one_kernel(const AttnRegArgs a) {
    constexpr int NDT = HD / 32, LDQ = HD + 4, LDT = 36, C4 = HD / 4;
    constexpr int PSZ = 2 * 32 * LDQ + 64;                             // floats of the pair: Q tile | dO tile | lse[32] | D[32]
    constexpr int XSZ = 32 * LDQ;                                      // floats per wave: dS^t [32][LDT] first, then the partial dQ [32][LDQ]
    constexpr int NT = 64 * KW;                                        // threads of the workgroup
    constexpr int ITS = 32 * C4 / NT;                                  // float4 per thread and staged operand
    static_assert(32 * LDT <= XSZ && (32 * C4) % NT == 0, "layout");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ql = lane & 31, half = lane >> 5;
    // pair slot (always 0: the workgroup has KW waves), key tile inside the block, thread inside the pair group.  The compiler cannot see wave < KW behind the
    // readfirstlane; folding pl = 0 by hand changes the register allocation (HD = 64, KW = 2: 256 VGPRs + 52 bytes of scratch become 250 + 0), i.e. the
    // schedule of a shipped kernel, which wants a measurement of its own.
    const int pl = wave / KW, kw = wave % KW, tp = tid - pl * NT;
    const int Sk = a.S0 + a.S1, D = a.H * HD;
    const int nqt = (a.Sq + 31) >> 5, nkt = (Sk + 31) >> 5, nkb = (nkt + KW - 1) / KW;
    const float scale = a.scale;
    const unsigned pr = blockIdx.x + (unsigned)pl;
    const bool pair_ok = pr < (unsigned)(a.B * a.H);
    const int b = __builtin_amdgcn_readfirstlane(pair_ok ? (int)(pr / (unsigned)a.H) : 0);
    const int h = __builtin_amdgcn_readfirstlane(pair_ok ? (int)(pr % (unsigned)a.H) : 0);
    float* Qs = smem + (size_t)pl * PSZ; float* Gs = Qs + 32 * LDQ; float* Ls = Gs + 32 * LDQ; float* Ds = Ls + 32;
    float* Xp = smem + PSZ + (size_t)pl * KW * XSZ;                    // the KW partial tiles of the pair
    float* X = Xp + (size_t)kw * XSZ;                                  // this wave's
    const float* qb = a.q + (size_t)b * a.q_bs + h * HD;
    const float* ob = a.out + (size_t)b * a.Sq * D + h * HD;
    const float* gb = a.dout + (size_t)b * a.Sq * D + h * HD;
    const float* lb = a.lse + ((size_t)b * a.H + h) * a.Sq;
    float* dqb = a.dq + (size_t)b * a.q_bs + h * HD;
    const float* k0 = a.k0 + (size_t)b * a.kv0_bs + h * HD; const float* v0 = a.v0 + (size_t)b * a.kv0_bs + h * HD;
    const float* k1 = a.k1 + (size_t)b * a.kv1_bs + h * HD; const float* v1 = a.v1 + (size_t)b * a.kv1_bs + h * HD;

    for (int kb = 0; kb < nkb; ++kb) {
        const int kt = kb * KW + kw;
        const bool work = pair_ok && kt < nkt;                         // wave-uniform
        const int nact = min(KW, nkt - kb * KW);                       // partial tiles to sum
        const int k0n = kt * 32, k0s = min(k0n, Sk - 32);
        const AttSeg kg = att_seg_tile(k0, a.ld0, k1, a.ld1, a.S0, work ? k0s : 0);
        float kreg[HD / 2], vreg[HD / 2];
        f32x16 dk[NDT], dv[NDT];
        if (work) {
            att_load_row_form<HD>(kg, ql, half, kreg);
            att_load_row_form<HD>(att_seg_tile(v0, a.ld0, v1, a.ld1, a.S0, k0s), ql, half, vreg);
        }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }
        const bool keyok = k0s + ql >= k0n;                            // keys shared with the previous tile belong to that tile
        for (int u = 0; u < nqt; ++u) {
            const int u0n = u * 32, u0 = min(u0n, a.Sq - 32);
            // ---- stage Q, dO (LDS) and lse, D = rowsum(dO * O) of the 32 queries: C4 consecutive lanes own one row
            if (pair_ok) {
#pragma unroll
                for (int it = 0; it < ITS; ++it) {
                    if (it > 0 && (it & 1) == 0) __builtin_amdgcn_sched_barrier(0);       // at most two rows' worth of staging registers in flight
                    const int idx = tp + NT * it, row = idx / C4, c4 = idx % C4;
                    const float4 qv = *reinterpret_cast<const float4*>(qb + (size_t)(u0 + row) * a.ldq + 4 * c4);
                    const float4 gv = *reinterpret_cast<const float4*>(gb + (size_t)(u0 + row) * D + 4 * c4);
                    const float4 ov = *reinterpret_cast<const float4*>(ob + (size_t)(u0 + row) * D + 4 * c4);
                    *reinterpret_cast<float4*>(Qs + row * LDQ + 4 * c4) = qv;
                    *reinterpret_cast<float4*>(Gs + row * LDQ + 4 * c4) = gv;
                    float part = (gv.x * ov.x + gv.y * ov.y) + (gv.z * ov.z + gv.w * ov.w);
#pragma unroll
                    for (int m = C4 / 2; m >= 1; m >>= 1) part += __shfl_xor(part, m);
                    if (c4 == 0) { Ds[row] = part; Ls[row] = lb[u0 + row]; }
                }
            }
            __syncthreads();
            if (work) {
                f32x16 sa, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { sa[r] = 0.f; dp[r] = 0.f; }
                {
                    float fr[HD / 2];
                    const float* gp = Gs + ql * LDQ + half * (HD / 2);
#pragma unroll
                    for (int i = 0; i < HD / 8; ++i) { const float4 t = *reinterpret_cast<const float4*>(gp + 4 * i); fr[4 * i] = t.x; fr[4 * i + 1] = t.y; fr[4 * i + 2] = t.z; fr[4 * i + 3] = t.w; }
#pragma unroll
                    for (int s2 = 0; s2 < HD / 2; ++s2) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[s2], vreg[s2], dp, 0, 0, 0);
                    const float* qp = Qs + ql * LDQ + half * (HD / 2);
#pragma unroll
                    for (int i = 0; i < HD / 8; ++i) { const float4 t = *reinterpret_cast<const float4*>(qp + 4 * i); fr[4 * i] = t.x; fr[4 * i + 1] = t.y; fr[4 * i + 2] = t.z; fr[4 * i + 3] = t.w; }
#pragma unroll
                    for (int s2 = 0; s2 < HD / 2; ++s2) sa = __builtin_amdgcn_mfma_f32_32x32x2f32(fr[s2], kreg[s2], sa, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // P and dS: register r <-> query u0 + f(r, half), lane <-> key k0s + ql
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 l4 = *reinterpret_cast<const float4*>(Ls + 8 * g + 4 * half);
                    const float4 d4 = *reinterpret_cast<const float4*>(Ds + 8 * g + 4 * half);
                    const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, dr[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = 4 * g + j;
                        const float pv = (keyok && u0 + 8 * g + 4 * half + j >= u0n) ? __expf(scale * sa[r] - lr[j]) : 0.f;
                        sa[r] = pv;
                        dp[r] = pv * (dp[r] - dr[j]) * scale;
                    }
                    // dS^t: T[key = ql][query = 8g + 4 half + 0..3]
                    *reinterpret_cast<float4*>(X + ql * LDT + 8 * g + 4 * half) = make_float4(dp[4 * g], dp[4 * g + 1], dp[4 * g + 2], dp[4 * g + 3]);
                }
                {   // dV^t += dO^t P
                    float fc[16][NDT];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float* rp = Gs + ATT_F(r, half) * LDQ + NDT * ql;
                        if constexpr (NDT == 2) { const float2 t = *reinterpret_cast<const float2*>(rp); fc[r][0] = t.x; fc[r][1] = t.y; } else fc[r][0] = rp[0];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r)
#pragma unroll
                        for (int dt = 0; dt < NDT; ++dt) dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fc[r][dt], sa[r], dv[dt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // dK^t += Q^t dS
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float* rp = Qs + ATT_F(r, half) * LDQ + NDT * ql;
                        if constexpr (NDT == 2) { const float2 t = *reinterpret_cast<const float2*>(rp); fc[r][0] = t.x; fc[r][1] = t.y; } else fc[r][0] = rp[0];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r)
#pragma unroll
                        for (int dt = 0; dt < NDT; ++dt) dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fc[r][dt], dp[r], dk[dt], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // K of this wave's keys in col form (the A operand of the partial dQ; the only fragment that still comes from global memory: L2 hits, the
                // other wave of the SIMD owns the matrix pipe meanwhile)
                float kc[16][NDT];
                att_load_col_form<HD>(kg, ql, half, kc);
                // partial dQ^t = K^t dS^t over this wave's keys: dS^t[key = f(r, half)][query = ql] back from the wave's own tile
                float dst[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) dst[r] = X[ATT_F(r, half) * LDT + ql];
                f32x16 dq[NDT];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r)
#pragma unroll
                    for (int dt = 0; dt < NDT; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[r][dt], dst[r], dq[dt], 0, 0, 0);
                att_store_o<HD>(X + ql * LDQ, half, dq, 1.0f);         // (every dS^t value of this wave is in registers by now: same region)
            }
            __syncthreads();
            // ---- dQ rows of this query tile: sum of the pair's partial tiles in wave order (+ what earlier key blocks left in global memory)
            if (pair_ok) {
#pragma unroll
                for (int it = 0; it < ITS; ++it) {
                    const int idx = tp + NT * it, row = idx / C4, c4 = idx % C4;
                    float4 acc = *reinterpret_cast<const float4*>(Xp + row * LDQ + 4 * c4);
                    for (int w = 1; w < nact; ++w) {
                        const float4 t = *reinterpret_cast<const float4*>(Xp + (size_t)w * XSZ + row * LDQ + 4 * c4);
                        acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
                    }
                    if (u0 + row >= u0n) {
                        float* dst4 = dqb + (size_t)(u0 + row) * a.ldq + 4 * c4;
                        if (kb > 0) {
                            const float4 t = *reinterpret_cast<const float4*>(dst4);
                            acc.x = t.x + acc.x; acc.y = t.y + acc.y; acc.z = t.z + acc.z; acc.w = t.w + acc.w;
                        }
                        *reinterpret_cast<float4*>(dst4) = acc;
                    }
                }
            }
            // (no barrier here: the next tile's staging writes the Q / dO region, which every wave finished reading before the barrier above; the
            //  partial region is written again only after the next staging barrier, by when every thread has left this reduction)
        }
        if (work) {
            const int key = k0s + ql;
            if (key >= k0n) {
                float* dkp = key < a.S0 ? a.dk0 + (size_t)b * a.kv0_bs + (size_t)key * a.ld0 + h * HD : a.dk1 + (size_t)b * a.kv1_bs + (size_t)(key - a.S0) * a.ld1 + h * HD;
                float* dvp = key < a.S0 ? a.dv0 + (size_t)b * a.kv0_bs + (size_t)key * a.ld0 + h * HD : a.dv1 + (size_t)b * a.kv1_bs + (size_t)(key - a.S0) * a.ld1 + h * HD;
                att_store_o<HD>(dkp, half, dk, 1.0f);
                att_store_o<HD>(dvp, half, dv, 1.0f);
            }
        }
    }
}

// ================================================================================================ dispatch: by (Sq, S0, head_dim) alone
// the single-pass backward wants full 32-row tiles inside one key segment (see the tail rule above)
static inline bool attn_reg_ok(int Sq, int S0) { return Sq >= 32 && (S0 % 32) == 0; }

template <int HD, int KW>
static int launch_attn_bwd_one_t(const AttnRegArgs& a, hipStream_t s) {
    const size_t smem = ((size_t)(2 * 32 * (HD + 4) + 64) + (size_t)KW * 32 * (HD + 4)) * sizeof(float);
    auto k = attn_bwd_one_kernel<HD, KW>;
    if (smem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)(a.B * a.H)), dim3(64 * KW), smem, s, a);
    ACT_LAUNCH_CHECK();
    return 0;
}
// one pair per workgroup also at KW = 2: 128-thread workgroups spread the 768 pairs of the student decoder over three workgroups per CU
// (two pairs per 256-thread workgroup: 50.3 us against 48.0 us, profiles/r06_attn_bwd_np_ab.txt)
static int launch_attn_bwd_one(const AttnRegArgs& a, int head_dim, hipStream_t s) {
    const int nkt = (a.S0 + a.S1 + 31) / 32;
    if (head_dim == 64) return nkt <= 2 ? launch_attn_bwd_one_t<64, 2>(a, s) : launch_attn_bwd_one_t<64, 4>(a, s);
    return nkt <= 2 ? launch_attn_bwd_one_t<32, 2>(a, s) : launch_attn_bwd_one_t<32, 4>(a, s);
}

template <int HD>
static int launch_attn_bwd_mfma_t(const AttnBwdArgs& a, hipStream_t s) {
    const size_t smem = ((size_t)3 * 64 * HD + 64 * 65 + 128) * sizeof(float);
    auto k = attn_bwd_mfma_kernel<HD>;
    if (smem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)(a.B * a.H)), dim3(256), smem, s, a);
    ACT_LAUNCH_CHECK();
    return 0;
}

template <int HD, int JT, int QT>
static int launch_attn_fwd_t(const AttnFwdArgs& a, hipStream_t s) {
    constexpr int pairs = 4 / QT;
    const size_t smem = (size_t)pairs * 2 * JT * 32 * (HD + 4) * sizeof(float);
    const long long np = (long long)a.B * a.H;
    const unsigned gx = (unsigned)((np + pairs - 1) / pairs), gy = (unsigned)((a.Sq + QT * 32 - 1) / (QT * 32));
    auto k = attn_fwd_kernel<HD, JT, QT>;
    if (smem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3(gx, gy), dim3(256), smem, s, a);
    ACT_LAUNCH_CHECK();
    return 0;
}
template <int HD>
static int launch_attn_fwd(const AttnFwdArgs& a, hipStream_t s) {
    const int Sk = a.S0 + a.S1;
    int JT = Sk > 128 ? 4 : (Sk + 31) / 32;                          // key tiles per LDS chunk
    const int QT = a.Sq > 128 ? 4 : (a.Sq + 31) / 32;                // query tiles per workgroup
    // K / V of all pairs of a workgroup live in LDS: beyond ~80 KB only one workgroup fits a CU and the kernel turns into pure latency.
    // 64-key chunks with the online softmax halve the footprint.
    const int pairs = QT == 1 ? 4 : (QT == 2 ? 2 : 1);
    const size_t lds = (size_t)pairs * 2 * JT * 32 * (HD + 4) * sizeof(float);
    if (JT == 4 && QT <= 2 && lds > 80 * 1024) JT = 2;
    // four pairs of 96 keys at head_dim 64 are 204 KB, more than the 160 KB of a CU: that launch cannot succeed -> 64-key chunks (136 KB) as for 97..127 keys
    else if (lds > 160 * 1024) JT = 2;
    // from 128 keys on, ONE 32-key tile per LDS chunk -- 35 KB instead of 70 KB per workgroup = four instead of two workgroups per CU, whose
    // staging / softmax / MFMA phases then overlap (Stage-I prefix shape 56.9 -> 51.8 us, S = 128 83 -> 76 us, stress teacher 64 + 512 320 -> 283 us;
    // shorter sequences keep the single chunk: 64 keys 20.6 vs 21.9 us)
    if (Sk >= 128) JT = 1;
    // Only the (JT, QT) this rule can produce are instantiated.  Every entry point has S1 = Sq, so Sk >= Sq and JT >= QT unless Sk >= 128 made JT = 1;
    // JT = 4 survives only for 97 <= Sk <= 127, where the 80 KB rule turns (4, 1) into (2, 1) and, at head_dim 64, (4, 2) into (2, 2) -- at head_dim 32
    // two pairs of 128 keys are 72 KB and (4, 2) stays; (3, 1) exists at head_dim 32 only (160 KB rule).  Checked by enumerating Sq = 1..700 x S0 = 0..700
    // through this rule for both head dimensions: exactly these ten pairs appear at head_dim 64, and (3, 1) and (4, 2) in addition at head_dim 32.
#define C3(J, Q) if (JT == J && QT == Q) return launch_attn_fwd_t<HD, J, Q>(a, s)
    C3(1, 1); C3(1, 2); C3(1, 3); C3(1, 4); C3(2, 1); C3(2, 2); C3(3, 2); C3(3, 3); C3(4, 3); C3(4, 4);
    if constexpr (HD == 32) { C3(3, 1); C3(4, 2); }
#undef C3
    return ACT_E_BADARG;
}

// forward of every entry point; packed qkv is kv0 = null, S0 = 0.  S <= 16 of the packed entry is handled there (attn_small_fwd_kernel).
static int attn_forward(const float* kv0, int S0, const float* qkv1, int Sq, float* out, uint16_t* out_hi, uint16_t* out_lo, float* lse,
                        int B, int H, int head_dim, float scale, hipStream_t s, PlaneFmt fmt = PlaneFmt::bf16()) {
    const int D = H * head_dim;
    AttnFwdArgs a{};
    a.q = qkv1; a.k0 = kv0; a.v0 = kv0 ? kv0 + D : nullptr; a.k1 = qkv1 + D; a.v1 = qkv1 + 2 * D;
    a.q_bs = (long long)Sq * 3 * D; a.kv0_bs = (long long)S0 * 2 * D; a.kv1_bs = a.q_bs; a.ldq = 3 * D; a.ld0 = 2 * D; a.ld1 = 3 * D;
    a.B = B; a.H = H; a.Sq = Sq; a.S0 = S0; a.S1 = Sq; a.scale = scale; a.out = out; a.lse = lse; a.out_hi = out_hi; a.out_lo = out_lo; a.fmt = fmt;
    return head_dim == 64 ? launch_attn_fwd<64>(a, s) : launch_attn_fwd<32>(a, s);
}

// backward of both entry points; packed qkv is kv0 = dkv0 = null, S0 = 0.  S <= 16 of the packed entry is handled there (attn_small_bwd_kernel).
static int attn_backward(const float* kv0, int S0, const float* qkv1, int Sq, const float* out, const float* dout, const float* lse,
                         float* dkv0, float* dqkv1, int B, int H, int head_dim, float scale, hipStream_t s) {
    if (attn_reg_ok(Sq, S0)) {
        const int D = H * head_dim;
        AttnRegArgs r{};                                               // (segment 0 is never dereferenced at S0 = 0: any valid pointer)
        r.q = qkv1; r.k0 = S0 > 0 ? kv0 : qkv1; r.v0 = S0 > 0 ? kv0 + D : qkv1; r.k1 = qkv1 + D; r.v1 = qkv1 + 2 * D;
        r.out = out; r.dout = dout; r.lse = lse;
        r.dq = dqkv1; r.dk0 = S0 > 0 ? dkv0 : dqkv1; r.dv0 = S0 > 0 ? dkv0 + D : dqkv1; r.dk1 = dqkv1 + D; r.dv1 = dqkv1 + 2 * D;
        r.q_bs = (long long)Sq * 3 * D; r.kv0_bs = (long long)S0 * 2 * D; r.kv1_bs = r.q_bs; r.ldq = 3 * D; r.ld0 = 2 * D; r.ld1 = 3 * D;
        r.B = B; r.H = H; r.Sq = Sq; r.S0 = S0; r.S1 = Sq; r.scale = scale;
        return launch_attn_bwd_one(r, head_dim, s);
    }
    AttnBwdArgs a;
    a.kv0 = kv0; a.qkv1 = qkv1; a.out = out; a.dout = dout; a.lse = lse; a.dkv0 = dkv0; a.dqkv1 = dqkv1;
    a.B = B; a.S0 = S0; a.Sq = Sq; a.H = H; a.scale = scale;
    return head_dim == 64 ? launch_attn_bwd_mfma_t<64>(a, s) : launch_attn_bwd_mfma_t<32>(a, s);
}

extern "C" int act_attention_fwd_f32(const float* qkv, float* out, float* lse, int B, int S, int H, int head_dim, float scale,
                                     act_stream_t stream) {
    if (!qkv || !out) return ACT_E_NULLPTR;
    if (B < 0 || S <= 0 || H <= 0 || (head_dim != 64 && head_dim != 32)) return ACT_E_BADARG;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ATTN_FWD, s, 4.0 * B * H * (double)S * S * head_dim, 16.0 * B * S * (double)H * head_dim);
    if (S <= 16) {                                                     // register-resident kernel: one wave per (cloud, head)
        const unsigned grid = (unsigned)(((long long)B * H + 3) / 4);
        if (head_dim == 64) hipLaunchKernelGGL(attn_small_fwd_kernel<64>, dim3(grid), dim3(256), 0, s, qkv, out, lse, B, S, H, scale);
        else                hipLaunchKernelGGL(attn_small_fwd_kernel<32>, dim3(grid), dim3(256), 0, s, qkv, out, lse, B, S, H, scale);
        ACT_LAUNCH_CHECK();
        return 0;
    }
    return attn_forward(nullptr, 0, qkv, S, out, nullptr, nullptr, lse, B, H, head_dim, scale, s);
}

// queries: the Sq rows of qkv1 [B,Sq,3,H,hd]; keys/values: S0 rows of kv0 [B,S0,2,H,hd] followed by the Sq rows of qkv1.
// (teacher ViT of models/dvae.py:536-576: prompt tokens only ever act as keys/values -- their outputs are replaced by the
//  next layer's prompts -- so queries, projection and MLP are evaluated for the patch tokens only.)
extern "C" int act_attention_fwd_prefix_f32(const float* kv0, int S0, const float* qkv1, int Sq, float* out, float* lse, int B,
                                            int H, int head_dim, float scale, act_stream_t stream) {
    if (!kv0 || !qkv1 || !out) return ACT_E_NULLPTR;
    if (B < 0 || Sq <= 0 || S0 < 0 || H <= 0 || (head_dim != 64 && head_dim != 32)) return ACT_E_BADARG;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ATTN_FWD, s, 4.0 * B * H * (double)Sq * (S0 + Sq) * head_dim, 4.0 * B * (double)H * head_dim * (4.0 * Sq + 2.0 * S0));
    return attn_forward(kv0, S0, qkv1, Sq, out, nullptr, nullptr, lse, B, H, head_dim, scale, s);
}

// the same forward with the output ALSO (out != NULL) or ONLY (out == NULL) as (hi, lo) bf16 planes [B*Sq][H*hd]: the A operand of a split-bf16 projection
// (opt-in teacher path, gemm_bf16x3.hip).
extern "C" int act_attention_fwd_prefix_planes_f32(const float* kv0, int S0, const float* qkv1, int Sq, float* out, uint16_t* out_hi, uint16_t* out_lo,
                                                   float* lse, int B, int H, int head_dim, float scale, act_stream_t stream) {
    if (!kv0 || !qkv1 || !out_hi || !out_lo) return ACT_E_NULLPTR;
    if (B < 0 || Sq <= 0 || S0 < 0 || H <= 0 || (head_dim != 64 && head_dim != 32) || (((uintptr_t)out_hi | (uintptr_t)out_lo) & 7)) return ACT_E_BADARG;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ATTN_FWD, s, 4.0 * B * H * (double)Sq * (S0 + Sq) * head_dim, 4.0 * B * (double)H * head_dim * (4.0 * Sq + 2.0 * S0));
    return attn_forward(kv0, S0, qkv1, Sq, out, out_hi, out_lo, lse, B, H, head_dim, scale, s);
}
// ... as the (h1, h2) f16 planes of out * plane_scale (a power of two that keeps |out * plane_scale| <= 2^15: gemm_bf16x3.hip, F16 form)
extern "C" int act_attention_fwd_prefix_f16_planes_f32(const float* kv0, int S0, const float* qkv1, int Sq, float* out, uint16_t* out_h1, uint16_t* out_h2,
                                                       float plane_scale, float* lse, int B, int H, int head_dim, float scale, act_stream_t stream) {
    if (!kv0 || !qkv1 || !out_h1 || !out_h2) return ACT_E_NULLPTR;
    if (B < 0 || Sq <= 0 || S0 < 0 || H <= 0 || (head_dim != 64 && head_dim != 32) || !(plane_scale > 0.f) || (((uintptr_t)out_h1 | (uintptr_t)out_h2) & 7))
        return ACT_E_BADARG;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ATTN_FWD, s, 4.0 * B * H * (double)Sq * (S0 + Sq) * head_dim, 4.0 * B * (double)H * head_dim * (4.0 * Sq + 2.0 * S0));
    return attn_forward(kv0, S0, qkv1, Sq, out, out_h1, out_h2, lse, B, H, head_dim, scale, s, PlaneFmt::f16(plane_scale));
}

extern "C" int act_attention_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                     int B, int S, int H, int head_dim, float scale, act_stream_t stream) {
    if (!qkv || !out || !dout || !lse || !dqkv) return ACT_E_NULLPTR;
    if (B < 0 || S <= 0 || H <= 0 || (head_dim != 64 && head_dim != 32)) return ACT_E_BADARG;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ATTN_BWD, s, 10.0 * B * H * (double)S * S * head_dim, 28.0 * B * S * (double)H * head_dim);
    if (S <= 16) {
        const unsigned grid = (unsigned)(((long long)B * H + 3) / 4);
        if (head_dim == 64) hipLaunchKernelGGL(attn_small_bwd_kernel<64>, dim3(grid), dim3(256), 0, s, qkv, out, dout, lse, dqkv, B, S, H, scale);
        else                hipLaunchKernelGGL(attn_small_bwd_kernel<32>, dim3(grid), dim3(256), 0, s, qkv, out, dout, lse, dqkv, B, S, H, scale);
        ACT_LAUNCH_CHECK();
        return 0;
    }
    return attn_backward(nullptr, 0, qkv, S, out, dout, lse, nullptr, dqkv, B, H, head_dim, scale, s);
}

// backward of act_attention_fwd_prefix_f32: dqkv1 [B,Sq,3,H,hd] (dQ, and dK/dV of the Sq own rows), dkv0 [B,S0,2,H,hd].
extern "C" int act_attention_bwd_prefix_f32(const float* kv0, int S0, const float* qkv1, int Sq, const float* out, const float* dout,
                                            const float* lse, float* dkv0, float* dqkv1, int B, int H, int head_dim, float scale,
                                            act_stream_t stream) {
    if (!qkv1 || !out || !dout || !lse || !dqkv1 || (S0 > 0 && (!kv0 || !dkv0))) return ACT_E_NULLPTR;
    if (B < 0 || Sq <= 0 || S0 < 0 || H <= 0 || (head_dim != 64 && head_dim != 32)) return ACT_E_BADARG;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_ATTN_BWD, s, 10.0 * B * H * (double)Sq * (S0 + Sq) * head_dim,
                    4.0 * B * (double)H * head_dim * (8.0 * Sq + 4.0 * S0));
    return attn_backward(kv0, S0, qkv1, Sq, out, dout, lse, dkv0, dqkv1, B, H, head_dim, scale, s);
}
