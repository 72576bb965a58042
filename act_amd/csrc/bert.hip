// bert.hip -- the two kernels a frozen post-LayerNorm (BERT) layer needs beyond the GEMMs, both with inverted dropout whose keep mask is either a
// given tensor (parity tests inject the reference's draws) or Philox4x32-10 regenerated wherever it is needed (nothing is stored for the backward):
//   (a) y = LN(keep o t / (1-p) + res) * gamma + beta, rows of width D, and its backward (dt, dres; the language model is frozen: no dgamma / dbeta)
//       mask: dropout.h, domain 1 (dense rows)
//   (b) attention with dropout on the probabilities: out = (softmax(q k^t scale) o keep / (1-p)) v on the packed qkv [B,S,3,H,hd] of
//       act_attention_fwd_f32, any S >= 1, hd 32 or 64.  mask: dropout.h, domain 2 (four keeps per Philox call).
// (b) runs on v_mfma_f32_32x32x2_f32 in the fragment forms of attn_frag.h (the clamped loaders): one wave owns 32 rows of one (cloud, head) and
// meets the other side in 32-row tiles straight from global memory (no LDS, no barrier); rows past S are clamped on the way in and masked out of P.
// At p = 0 the layer calls act_attention_fwd_f32 / act_attention_bwd_f32: these kernels are the dropout path only.
#include "attn_frag.h"
#include "dropout.h"
#include "ln_row.h"

namespace {

// ------------------------------------------------------------------------------------------------ (a) dropout + residual + LayerNorm
// keep / (1-p) of the four channels 4c .. 4c+3 of a row: the given mask, Philox, or 1 (p = 0)
__device__ __forceinline__ float4 bln_keep4(const float4* __restrict__ mask4, float4 mv, float drop_p, const DropoutKey& key, uint32_t row, uint32_t c) {
    float4 k = make_float4(1.f, 1.f, 1.f, 1.f);
    if (drop_p > 0.f) {
        if (mask4) {
            k.x = mv.x * key.inv_keep; k.y = mv.y * key.inv_keep; k.z = mv.z * key.inv_keep; k.w = mv.w * key.inv_keep;
        } else k = dropout_keep4(key, row, c);
    }
    return k;
}

// one wave per row; every load of the row is issued up front (lanes beyond the row read its last float4 and are masked in the arithmetic), as
// layernorm_bwd_kernel does
template <int MAXV>
__global__ __launch_bounds__(256) void bert_dropout_ln_fwd_kernel(const float* __restrict__ t, const float* __restrict__ res,
                                                                  const float* __restrict__ mask, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ rstd_out,
                                                                  int T, int D, float eps, float drop_p, uint64_t seed,
                                                                  const uint64_t* __restrict__ seed_dev) {
    const DropoutKey key = dropout_key(drop_p, seed, seed_dev);
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int nv = D >> 2;
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(t) + (size_t)row * nv;
    const float4* __restrict__ r4 = reinterpret_cast<const float4*>(res) + (size_t)row * nv;
    const float4* __restrict__ m4 = (mask && drop_p > 0.f) ? reinterpret_cast<const float4*>(mask) + (size_t)row * nv : nullptr;
    int cc[MAXV]; float4 tv[MAXV], rv[MAXV], mv[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) { cc[i] = min(lane + 64 * i, nv - 1); tv[i] = t4[cc[i]]; rv[i] = r4[cc[i]]; }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) mv[i] = m4 ? m4[cc[i]] : make_float4(1.f, 1.f, 1.f, 1.f);
    float4 v[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const float4 k = bln_keep4(m4, mv[i], drop_p, key, (uint32_t)row, (uint32_t)c);
            float4 a;
            a.x = fmaf(tv[i].x, k.x, rv[i].x); a.y = fmaf(tv[i].y, k.y, rv[i].y); a.z = fmaf(tv[i].z, k.z, rv[i].z); a.w = fmaf(tv[i].w, k.w, rv[i].w);
            v[i] = a;
        } else v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float mean = ln_row_mean<MAXV>(v, lane, nv, D);
    const float rstd = ln_row_rstd<MAXV>(v, mean, lane, nv, D, eps);
    float4* __restrict__ yr = reinterpret_cast<float4*>(y) + (size_t)row * nv;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(gamma);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) yr[c] = ln_row_norm4(v[i], mean, rstd, g4[c], b4[c]);
    }
    if (lane == 0 && rstd_out) rstd_out[row] = rstd;
}

// dres = rstd * (dy g - mean(dy g) - xhat mean(dy g xhat)), dt = dres o keep / (1-p).  xhat comes back from the forward's OUTPUT, xhat = (y - beta) / gamma
// (gamma != 0: the pre-norm row is never stored), so the backward reads two tensors and writes two.
template <int MAXV>
__global__ __launch_bounds__(256) void bert_dropout_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                  const float* __restrict__ mask, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, const float* __restrict__ rstd,
                                                                  float* __restrict__ dt, float* __restrict__ dres, int T, int D, float drop_p,
                                                                  uint64_t seed, const uint64_t* __restrict__ seed_dev) {
    const DropoutKey key = dropout_key(drop_p, seed, seed_dev);
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int nv = D >> 2;
    const float4* __restrict__ d4 = reinterpret_cast<const float4*>(dy) + (size_t)row * nv;
    const float4* __restrict__ y4 = reinterpret_cast<const float4*>(y) + (size_t)row * nv;
    const float4* __restrict__ m4 = (mask && drop_p > 0.f) ? reinterpret_cast<const float4*>(mask) + (size_t)row * nv : nullptr;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(gamma);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(beta);
    int cc[MAXV]; float4 dv[MAXV], yv[MAXV], mv[MAXV], gv[MAXV], bv[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) { cc[i] = min(lane + 64 * i, nv - 1); dv[i] = d4[cc[i]]; yv[i] = y4[cc[i]]; gv[i] = g4[cc[i]]; bv[i] = b4[cc[i]]; }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) mv[i] = m4 ? m4[cc[i]] : make_float4(1.f, 1.f, 1.f, 1.f);
    const float rs = rstd[row];
    float4 h[MAXV], w[MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const float4 d = dv[i], g = gv[i], b = bv[i], o = yv[i];
            float4 xh; xh.x = (o.x - b.x) / g.x; xh.y = (o.y - b.y) / g.y; xh.z = (o.z - b.z) / g.z; xh.w = (o.w - b.w) / g.w;
            float4 dg; dg.x = d.x * g.x; dg.y = d.y * g.y; dg.z = d.z * g.z; dg.w = d.w * g.w;
            h[i] = xh; w[i] = dg;
            s1 += (dg.x + dg.y) + (dg.z + dg.w);
            s2 += (dg.x * xh.x + dg.y * xh.y) + (dg.z * xh.z + dg.w * xh.w);
        }
    }
    const float m1 = wave_sum_f32(s1) / (float)D, m2 = wave_sum_f32(s2) / (float)D;
    float4* __restrict__ dtr = reinterpret_cast<float4*>(dt) + (size_t)row * nv;
    float4* __restrict__ drr = reinterpret_cast<float4*>(dres) + (size_t)row * nv;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            float4 o;
            o.x = rs * (w[i].x - m1 - h[i].x * m2); o.y = rs * (w[i].y - m1 - h[i].y * m2);
            o.z = rs * (w[i].z - m1 - h[i].z * m2); o.w = rs * (w[i].w - m1 - h[i].w * m2);
            drr[c] = o;
            const float4 k = bln_keep4(m4, mv[i], drop_p, key, (uint32_t)row, (uint32_t)c);
            dtr[c] = make_float4(o.x * k.x, o.y * k.y, o.z * k.z, o.w * k.w);
        }
    }
}

// ------------------------------------------------------------------------------------------------ (b) attention with dropout on the probabilities
struct BertAttnArgs {
    const float* qkv; const uint8_t* mask; const float* out; const float* dout; const float* lse; const float* delta;
    float* o; float* lse_out; float* dqkv;
    int B, S, H;
    float scale, inv_keep; uint32_t thr;
    uint64_t seed; const uint64_t* seed_dev;
};
__device__ __forceinline__ DropoutKey attn_key(const BertAttnArgs& a) { return DropoutKey{philox_fold_seed(a.seed, a.seed_dev), a.thr, a.inv_keep}; }

// forward: grid (ceil(S/128), B*H), a wave = 32 queries.  S^t = K Q^t puts all scores of ONE query into one lane pair (c, c+32), so the online softmax
// is 16 registers + one cross-half exchange, and P^t is the B operand of O^t = V^t P^t straight from its registers.
template <int HD>
__global__ __launch_bounds__(256) void bert_attn_fwd_kernel(const BertAttnArgs a) {
    constexpr int NDT = HD / 32, HH = HD / 2;
    const DropoutKey key = attn_key(a);
    const int lane = threadIdx.x & 63, c = lane & 31, half = lane >> 5;
    const int S = a.S, q0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (q0 >= S) return;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int ld = 3 * a.H * HD;
    const float* __restrict__ qb = a.qkv + (size_t)b * S * ld + h * HD;
    const float* __restrict__ kb = qb + a.H * HD;
    const float* __restrict__ vb = kb + a.H * HD;
    const int qrow = min(q0 + c, S - 1);
    const uint32_t rowid = (uint32_t)bh * (uint32_t)S + (uint32_t)qrow;
    float qreg[HH];
    bert_load_row_form<HD>(qb + (size_t)qrow * ld, half, a.scale * ATT_LOG2E, qreg);
    f32x16 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < S; k0 += 32) {
        float kreg[HH];
        bert_load_row_form<HD>(kb + (size_t)min(k0 + c, S - 1) * ld, half, 1.0f, kreg);
        float vc[16][NDT];
        bert_load_col_form<HD>(vb, ld, k0, S, c, half, vc);
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int i = 0; i < HH; ++i) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[i], qreg[i], st, 0, 0, 0);
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (k0 + ATT_F(r, half) >= S) st[r] = -INFINITY;
            mx = fmaxf(mx, st[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);                                   // finite: key k0 < S is in every tile
        const float alpha = exp2f(m - mn);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = exp2f(st[r] - mn); sum += st[r]; }
        sum += __shfl_xor(sum, 32);
        l = l * alpha + sum;                                             // the normaliser is over the UNDROPPED probabilities
        m = mn;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float kf[4];
            dropout_attn_keep4(a.mask, a.S, key, rowid, k0 + 8 * g + 4 * half, kf);
#pragma unroll
            for (int k = 0; k < 4; ++k) st[4 * g + k] *= kf[k];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[r][dt], st[r], o[dt], 0, 0, 0);
    }
    if (q0 + c < S) {
        att_store_o<HD>(a.o + ((size_t)b * S + q0 + c) * (a.H * HD) + h * HD, half, o, 1.0f / l);
        if (half == 0 && a.lse_out) a.lse_out[(size_t)bh * S + q0 + c] = (m + log2f(l)) * ATT_LN2;
    }
}

// delta[b,h,s] = sum_d dout o out (= rowsum(dP o P) with the dropped dP), one thread per (row, head)
__global__ __launch_bounds__(256) void bert_attn_delta_kernel(const float* __restrict__ out, const float* __restrict__ dout, float* __restrict__ delta,
                                                              int B, int S, int H, int HD) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * S * H) return;
    const int h = (int)(i % H); const long long row = i / H; const int s = (int)(row % S); const int b = (int)(row / S);
    const float4* __restrict__ o4 = reinterpret_cast<const float4*>(out + (size_t)i * HD);
    const float4* __restrict__ d4 = reinterpret_cast<const float4*>(dout + (size_t)i * HD);
    float acc = 0.f;
    for (int j = 0; j < HD / 4; ++j) { const float4 x = o4[j], y = d4[j]; acc += (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w); }
    delta[((size_t)b * H + h) * S + s] = acc;
}

// dQ: a wave = 32 queries, walks the key tiles.  S^t and dP^t in the forward's layout (lane pair = one query), dS^t is the B operand of dQ^t = K^t dS^t.
template <int HD>
__global__ __launch_bounds__(256) void bert_attn_bwd_dq_kernel(const BertAttnArgs a) {
    constexpr int NDT = HD / 32, HH = HD / 2;
    const DropoutKey key = attn_key(a);
    const int lane = threadIdx.x & 63, c = lane & 31, half = lane >> 5;
    const int S = a.S, q0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (q0 >= S) return;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int ld = 3 * a.H * HD, ldo = a.H * HD;
    const float* __restrict__ qb = a.qkv + (size_t)b * S * ld + h * HD;
    const float* __restrict__ kb = qb + a.H * HD;
    const float* __restrict__ vb = kb + a.H * HD;
    const int qrow = min(q0 + c, S - 1);
    const uint32_t rowid = (uint32_t)bh * (uint32_t)S + (uint32_t)qrow;
    float qreg[HH], doreg[HH];
    bert_load_row_form<HD>(qb + (size_t)qrow * ld, half, a.scale * ATT_LOG2E, qreg);
    bert_load_row_form<HD>(a.dout + ((size_t)b * S + qrow) * ldo + h * HD, half, 1.0f, doreg);
    const float lse2 = a.lse[(size_t)bh * S + qrow] * ATT_LOG2E, dl = a.delta[(size_t)bh * S + qrow];
    f32x16 dq[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
    for (int k0 = 0; k0 < S; k0 += 32) {
        const int krow = min(k0 + c, S - 1);
        float kreg[HH], vreg[HH];
        bert_load_row_form<HD>(kb + (size_t)krow * ld, half, 1.0f, kreg);
        bert_load_row_form<HD>(vb + (size_t)krow * ld, half, 1.0f, vreg);
        float kc[16][NDT];
        bert_load_col_form<HD>(kb, ld, k0, S, c, half, kc);
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int i = 0; i < HH; ++i) {
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[i], qreg[i], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vreg[i], doreg[i], dp, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float kf[4];
            dropout_attn_keep4(a.mask, a.S, key, rowid, k0 + 8 * g + 4 * half, kf);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = 4 * g + k;
                const float p = (k0 + ATT_F(r, half) < S) ? exp2f(st[r] - lse2) : 0.f;
                st[r] = p * (dp[r] * kf[k] - dl) * a.scale;              // dS^t
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[r][dt], st[r], dq[dt], 0, 0, 0);
    }
    if (q0 + c < S) att_store_o<HD>(a.dqkv + ((size_t)b * S + q0 + c) * ld + h * HD, half, dq, 1.0f);
}

// dK, dV: a wave = 32 keys (a lane pair = one key column), walks the query tiles: S and dP as [query f(r, half)][key c], so P o keep and dS are the
// B operands of dV^t = dO^t (P o keep) and dK^t = Q^t dS.  The lane's key is fixed, so a Philox call serves one element here (four in the other kernels).
template <int HD>
__global__ __launch_bounds__(256) void bert_attn_bwd_dkv_kernel(const BertAttnArgs a) {
    constexpr int NDT = HD / 32, HH = HD / 2;
    const DropoutKey dkey = attn_key(a);
    const int lane = threadIdx.x & 63, c = lane & 31, half = lane >> 5;
    const int S = a.S, k0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (k0 >= S) return;
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int ld = 3 * a.H * HD, ldo = a.H * HD;
    const float* __restrict__ qb = a.qkv + (size_t)b * S * ld + h * HD;
    const float* __restrict__ kb = qb + a.H * HD;
    const float* __restrict__ vb = kb + a.H * HD;
    const float* __restrict__ dob = a.dout + (size_t)b * S * ldo + h * HD;
    const int key = k0 + c, krow = min(key, S - 1);
    const bool kvalid = key < S;
    float kreg[HH], vreg[HH];
    bert_load_row_form<HD>(kb + (size_t)krow * ld, half, 1.0f, kreg);
    bert_load_row_form<HD>(vb + (size_t)krow * ld, half, 1.0f, vreg);
    f32x16 dk[NDT], dv[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }
    for (int q0 = 0; q0 < S; q0 += 32) {
        const int qrow = min(q0 + c, S - 1);
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
        {
            float qreg[HH], doreg[HH];
            bert_load_row_form<HD>(qb + (size_t)qrow * ld, half, a.scale * ATT_LOG2E, qreg);
            bert_load_row_form<HD>(dob + (size_t)qrow * ldo, half, 1.0f, doreg);
#pragma unroll
            for (int i = 0; i < HH; ++i) {
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(qreg[i], kreg[i], st, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(doreg[i], vreg[i], dp, 0, 0, 0);
            }
        }
        float qc[16][NDT], doc[16][NDT];
        bert_load_col_form<HD>(qb, ld, q0, S, c, half, qc);
        bert_load_col_form<HD>(dob, ldo, q0, S, c, half, doc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = q0 + ATT_F(r, half), qic = min(qi, S - 1);
            const size_t li = (size_t)bh * S + qic;
            const float kf = dropout_attn_keep1(a.mask, a.S, dkey, (uint32_t)li, key);
            const float p = (qi < S && kvalid) ? exp2f(st[r] - a.lse[li] * ATT_LOG2E) : 0.f;
            st[r] = p * (dp[r] * kf - a.delta[li]) * a.scale;            // dS
            dp[r] = p * kf;                                              // P o keep / (1-p)
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(doc[r][dt], dp[r], dv[dt], 0, 0, 0);
                dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[r][dt], st[r], dk[dt], 0, 0, 0);
            }
    }
    if (kvalid) {
        float* __restrict__ rowp = a.dqkv + ((size_t)b * S + key) * ld + h * HD;
        att_store_o<HD>(rowp + a.H * HD, half, dk, 1.0f);
        att_store_o<HD>(rowp + 2 * a.H * HD, half, dv, 1.0f);
    }
}

bool attn_args_ok(int B, int S, int H, int hd, float p) {
    return B >= 0 && S >= 0 && H > 0 && (hd == 32 || hd == 64) && p >= 0.f && p < 1.f && (long long)B * H * S < (1ll << 32) && (long long)B * H <= 65535;
}

}  // namespace

extern "C" int act_dropout_add_layernorm_fwd_f32(const float* t, const float* res, const float* mask, int T, int D, float drop_p, uint64_t seed,
                                                 const uint64_t* seed_dev, const float* gamma, const float* beta, float eps, float* y, float* rstd,
                                                 act_stream_t stream) {
    if (T < 0 || D <= 0 || (D & 3) || D > 64 * 4 * LN_ROW_MAXV || drop_p < 0.f || drop_p >= 1.f) return ACT_E_BADARG;
    if (T == 0) return 0;                                               // before the pointers: an empty tensor has none
    if (!t || !res || !gamma || !beta || !y) return ACT_E_NULLPTR;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_LAYERNORM_FWD, s, 0.0, 4.0 * T * (double)D * (3 + (mask && drop_p > 0.f ? 1 : 0)));
#define BLF(MV_) hipLaunchKernelGGL((bert_dropout_ln_fwd_kernel<MV_>), dim3((T + 3) / 4), dim3(256), 0, s, t, res, mask, gamma, beta, y, rstd, T, D, eps, drop_p, seed, seed_dev)
    if (D <= 512) BLF(2); else if (D <= 1024) BLF(4); else BLF(8);
#undef BLF
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_dropout_add_layernorm_bwd_f32(const float* dy, const float* y, const float* mask, int T, int D, float drop_p, uint64_t seed,
                                                 const uint64_t* seed_dev, const float* gamma, const float* beta, const float* rstd, float* dt,
                                                 float* dres, act_stream_t stream) {
    if (T < 0 || D <= 0 || (D & 3) || D > 64 * 4 * LN_ROW_MAXV || drop_p < 0.f || drop_p >= 1.f) return ACT_E_BADARG;
    if (T == 0) return 0;
    if (!dy || !y || !gamma || !beta || !rstd || !dt || !dres) return ACT_E_NULLPTR;
    hipStream_t s = (hipStream_t)stream;
    ActProfScope ps(KID_LAYERNORM_BWD, s, 0.0, 4.0 * T * (double)D * (4 + (mask && drop_p > 0.f ? 1 : 0)));
#define BLB(MV_) hipLaunchKernelGGL((bert_dropout_ln_bwd_kernel<MV_>), dim3((T + 3) / 4), dim3(256), 0, s, dy, y, mask, gamma, beta, rstd, dt, dres, T, D, drop_p, seed, seed_dev)
    if (D <= 512) BLB(2); else if (D <= 1024) BLB(4); else BLB(8);
#undef BLB
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_attention_dropout_fwd_f32(const float* qkv, const uint8_t* mask, float* out, float* lse, int B, int S, int H, int head_dim,
                                             float scale, float drop_p, uint64_t seed, const uint64_t* seed_dev, act_stream_t stream) {
    if (!attn_args_ok(B, S, H, head_dim, drop_p)) return ACT_E_BADARG;
    if (B == 0 || S == 0) return 0;                                     // before the pointers: an empty tensor has none
    if (!qkv || !out) return ACT_E_NULLPTR;
    hipStream_t s = (hipStream_t)stream;
    BertAttnArgs a{};
    a.qkv = qkv; a.mask = mask; a.o = out; a.lse_out = lse; a.B = B; a.S = S; a.H = H; a.scale = scale;
    a.inv_keep = dropout_inv_keep(drop_p); a.thr = dropout_thr(drop_p); a.seed = seed; a.seed_dev = seed_dev;
    ActProfScope ps(KID_ATTN_FWD, s, 4.0 * B * H * (double)S * S * head_dim, 4.0 * 4.0 * B * S * (double)H * head_dim);
    const dim3 grid((S + 127) / 128, B * H);
    if (head_dim == 64) hipLaunchKernelGGL(bert_attn_fwd_kernel<64>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(bert_attn_fwd_kernel<32>, grid, dim3(256), 0, s, a);
    ACT_LAUNCH_CHECK(); return 0;
}

extern "C" int act_attention_dropout_bwd_f32(const float* qkv, const uint8_t* mask, const float* out, const float* dout, const float* lse,
                                             float* delta, float* dqkv, int B, int S, int H, int head_dim, float scale, float drop_p, uint64_t seed,
                                             const uint64_t* seed_dev, act_stream_t stream) {
    if (!attn_args_ok(B, S, H, head_dim, drop_p)) return ACT_E_BADARG;
    if (B == 0 || S == 0) return 0;
    if (!qkv || !out || !dout || !lse || !delta || !dqkv) return ACT_E_NULLPTR;
    hipStream_t s = (hipStream_t)stream;
    BertAttnArgs a{};
    a.qkv = qkv; a.mask = mask; a.out = out; a.dout = dout; a.lse = lse; a.delta = delta; a.dqkv = dqkv; a.B = B; a.S = S; a.H = H; a.scale = scale;
    a.inv_keep = dropout_inv_keep(drop_p); a.thr = dropout_thr(drop_p); a.seed = seed; a.seed_dev = seed_dev;
    ActProfScope ps(KID_ATTN_BWD, s, 14.0 * B * H * (double)S * S * head_dim, 4.0 * 8.0 * B * S * (double)H * head_dim);
    const long long n = (long long)B * S * H;
    hipLaunchKernelGGL(bert_attn_delta_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, dout, delta, B, S, H, head_dim);
    ACT_LAUNCH_CHECK();
    const dim3 grid((S + 127) / 128, B * H);
    if (head_dim == 64) {
        hipLaunchKernelGGL(bert_attn_bwd_dq_kernel<64>, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(bert_attn_bwd_dkv_kernel<64>, grid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(bert_attn_bwd_dq_kernel<32>, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(bert_attn_bwd_dkv_kernel<32>, grid, dim3(256), 0, s, a);
    }
    ACT_LAUNCH_CHECK(); return 0;
}
