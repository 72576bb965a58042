// augment.hip -- an ordered chain of up to 8 point-cloud augmentations (reference: datasets/data_transforms.py) in ONE launch, in place.
//
// One workgroup owns one cloud.  For N <= 8192 the cloud is staged once into LDS (96 KB at N = 8192), every op of the chain runs there and the
// cloud is written back once; for larger N (or ACT_AUGMENT_GLOBAL) the same op code runs in place on global memory.  The two forms are template
// instances, so neither pays flat addressing.  Ops are separated by a workgroup barrier: the flip's maximum and the dropout's point 0 are taken
// from the cloud as the EARLIER ops of the chain left it.
// Draws: a per-op device pointer (parity tests inject the reference's draws) or Philox4x32-10 in the kernel; the counter layout is documented in
// include/act_hip.h and restated by tests/augment_ref.py.
// Built with -ffp-contract=off (act_amd/build.py): every product and sum below rounds once, so a fp32 host restatement reproduces the affine ops
// bit for bit.
#include "dropout.h"

#define AUG_LDS_MAX_N 8192
#define AUG_RED 64                    // floats of reduction scratch ahead of the cloud image: [2][16 waves] partial maxima

namespace {

struct AugArgs {                      // the op table, passed to the kernel BY VALUE (no allocation, no H2D copy, capturable)
    int nops;
    int kind[ACT_AUGMENT_MAX_OPS];
    float p0[ACT_AUGMENT_MAX_OPS], p1[ACT_AUGMENT_MAX_OPS], p2[ACT_AUGMENT_MAX_OPS];
    const float* d0[ACT_AUGMENT_MAX_OPS];
    const float* d1[ACT_AUGMENT_MAX_OPS];
};

__device__ __forceinline__ float aug_u01(uint32_t bits) { return (float)(bits >> 8) * 5.9604644775390625e-08f; }              // [0, 1)
__device__ __forceinline__ float aug_u01_open(uint32_t bits) { return (float)((bits >> 8) + 1u) * 5.9604644775390625e-08f; }   // (0, 1]

// the words of one counter: (slot, cloud, PHILOX_DOMAIN_AUGMENT = 3, position + 8 * sub); sub 0 = the op's per-cloud draws, sub 1 = its per-point draws
__device__ __forceinline__ void aug_philox(uint64_t seed, uint32_t slot, uint32_t cloud, uint32_t pos, uint32_t sub, uint32_t r[4]) {
    philox_draw(seed, slot, cloud, PHILOX_DOMAIN_AUGMENT, pos + 8u * sub, r);
}

// three per-cloud uniforms of an op: injected [B,3] or the first three words of per-cloud counter `slot`
__device__ __forceinline__ void aug_cloud3(const float* __restrict__ inj, uint64_t seed, uint32_t slot, uint32_t b, uint32_t pos, float u[3]) {
    if (inj) { u[0] = inj[3 * b]; u[1] = inj[3 * b + 1]; u[2] = inj[3 * b + 2]; return; }
    uint32_t r[4];
    aug_philox(seed, slot, b, pos, 0u, r);
    u[0] = aug_u01(r[0]); u[1] = aug_u01(r[1]); u[2] = aug_u01(r[2]);
}

template <bool LDS>
__global__ __launch_bounds__(1024) void augment_kernel(float* pc, int N, AugArgs a, uint64_t seed,
                                                       const uint64_t* __restrict__ seed_dev) {
    extern __shared__ __attribute__((aligned(16))) float aug_smem[];
    seed = philox_fold_seed(seed, seed_dev);
    const uint32_t b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = nt >> 6;
    const int n3 = 3 * N;
    float* gcloud = pc + (size_t)b * n3;
    float* s_red = aug_smem;
    float* p = LDS ? aug_smem + AUG_RED : gcloud;
    if (LDS) {
        for (int i = tid; i < n3; i += nt) p[i] = gcloud[i];
        __syncthreads();
    }
    for (int pos = 0; pos < a.nops; ++pos) {
        const int kind = a.kind[pos];
        const float q0 = a.p0[pos], q1 = a.p1[pos], q2 = a.p2[pos];
        const float* __restrict__ d0 = a.d0[pos];
        const float* __restrict__ d1 = a.d1[pos];
        if (kind == ACT_AUG_SCALE || kind == ACT_AUG_TRANSLATE || kind == ACT_AUG_SCALE_TRANSLATE) {
            float u[3], sc[3] = {1.f, 1.f, 1.f}, sh[3] = {0.f, 0.f, 0.f};
            if (kind != ACT_AUG_TRANSLATE) {                                   // s = lo + (hi - lo) u
                aug_cloud3(d0, seed, 0u, b, pos, u);
                for (int c = 0; c < 3; ++c) sc[c] = d0 ? u[c] : q0 + (q1 - q0) * u[c];
            }
            if (kind != ACT_AUG_SCALE) {                                       // t = -r + (2 r) u
                const float* inj = kind == ACT_AUG_TRANSLATE ? d0 : d1;
                const float r = kind == ACT_AUG_TRANSLATE ? q0 : q2;
                aug_cloud3(inj, seed, kind == ACT_AUG_TRANSLATE ? 0u : 1u, b, pos, u);
                for (int c = 0; c < 3; ++c) sh[c] = inj ? u[c] : -r + (2.f * r) * u[c];
            }
            if (kind == ACT_AUG_SCALE) {
                for (int i = tid; i < n3; i += nt) { const int c = i % 3; p[i] = p[i] * (c == 0 ? sc[0] : c == 1 ? sc[1] : sc[2]); }
            } else if (kind == ACT_AUG_TRANSLATE) {
                for (int i = tid; i < n3; i += nt) { const int c = i % 3; p[i] = p[i] + (c == 0 ? sh[0] : c == 1 ? sh[1] : sh[2]); }
            } else {
                for (int i = tid; i < n3; i += nt) {
                    const int c = i % 3;
                    p[i] = __fadd_rn(__fmul_rn(p[i], c == 0 ? sc[0] : c == 1 ? sc[1] : sc[2]), c == 0 ? sh[0] : c == 1 ? sh[1] : sh[2]);
                }
            }
        } else if (kind == ACT_AUG_ROTATE_Y) {
            float u;
            if (d0) u = d0[b];
            else { uint32_t r[4]; aug_philox(seed, 0u, b, pos, 0u, r); u = aug_u01(r[0]); }
            float sn, cs;
            sincospif(2.f * u, &sn, &cs);                                      // angle 2 pi u: 2u is exact, no rounding of the angle itself
            const float nsn = -sn;
            for (int n = tid; n < N; n += nt) {                               // R = [[c,0,s],[0,1,0],[-s,0,c]], out_j = (x R0j + y R1j) + z R2j
                const float x = p[3 * n], y = p[3 * n + 1], z = p[3 * n + 2];
                p[3 * n]     = (x * cs + y * 0.f) + z * nsn;
                p[3 * n + 1] = (x * 0.f + y * 1.f) + z * 0.f;
                p[3 * n + 2] = (x * sn + y * 0.f) + z * cs;
            }
        } else if (kind == ACT_AUG_JITTER) {
            const float sd = q0, clip = q1;
            if (d0) {
                const float* __restrict__ z = d0 + (size_t)b * n3;
                for (int i = tid; i < n3; i += nt) p[i] = p[i] + fminf(fmaxf(sd * z[i], -clip), clip);
            } else {
                for (int n = tid; n < N; n += nt) {                           // Box-Muller: (w0, w1) -> z0, z1; (w2, w3) -> z2
                    uint32_t r[4];
                    aug_philox(seed, (uint32_t)n, b, pos, 1u, r);
                    const float ra = sqrtf(-2.f * logf(aug_u01_open(r[0]))), rb = sqrtf(-2.f * logf(aug_u01_open(r[2])));
                    float sa, ca, sb, cb;
                    sincospif(2.f * aug_u01(r[1]), &sa, &ca);
                    sincospif(2.f * aug_u01(r[3]), &sb, &cb);
                    (void)sb;
                    p[3 * n]     = p[3 * n]     + fminf(fmaxf(sd * (ra * ca), -clip), clip);
                    p[3 * n + 1] = p[3 * n + 1] + fminf(fmaxf(sd * (ra * sa), -clip), clip);
                    p[3 * n + 2] = p[3 * n + 2] + fminf(fmaxf(sd * (rb * cb), -clip), clip);
                }
            }
        } else if (kind == ACT_AUG_DROPOUT) {
            float ub;
            if (d0) ub = d0[b];
            else { uint32_t r[4]; aug_philox(seed, 0u, b, pos, 0u, r); ub = aug_u01(r[0]); }
            const float ratio = ub * q0;
            const float x0 = p[0], y0 = p[1], z0 = p[2];                      // point 0 as the earlier ops left it (it may itself be dropped: same bits)
            __syncthreads();
            for (int n = tid; n < N; n += nt) {
                float un;
                if (d1) un = d1[(size_t)b * N + n];
                else { uint32_t r[4]; aug_philox(seed, (uint32_t)n, b, pos, 1u, r); un = aug_u01(r[0]); }
                if (un <= ratio) { p[3 * n] = x0; p[3 * n + 1] = y0; p[3 * n + 2] = z0; }
            }
        } else if (kind == ACT_AUG_FLIP) {
            float u[3];
            aug_cloud3(d0, seed, 0u, b, pos, u);
            const int up = (int)q0;
            const int ax0 = up == 0 ? 1 : 0, ax1 = up == 2 ? 1 : 2;           // the horizontal axes, ascending
            const bool gate = u[0] < 0.95f;
            const bool f0 = gate && u[1] < 0.5f, f1 = gate && u[2] < 0.5f;
            if (f0 || f1) {                                                  // uniform over the workgroup
                float m0 = -INFINITY, m1 = -INFINITY;
                for (int n = tid; n < N; n += nt) { m0 = fmaxf(m0, p[3 * n + ax0]); m1 = fmaxf(m1, p[3 * n + ax1]); }
                m0 = wave_max_f32(m0, -INFINITY); m1 = wave_max_f32(m1, -INFINITY);
                if (lane == 0) { s_red[wave] = m0; s_red[16 + wave] = m1; }
                __syncthreads();
                m0 = s_red[0]; m1 = s_red[16];
                for (int w = 1; w < nwaves; ++w) { m0 = fmaxf(m0, s_red[w]); m1 = fmaxf(m1, s_red[16 + w]); }
                for (int i = tid; i < n3; i += nt) {
                    const int c = i % 3;
                    if (f0 && c == ax0) p[i] = m0 - p[i];
                    else if (f1 && c == ax1) p[i] = m1 - p[i];
                }
            }
        }
        __syncthreads();
    }
    if (LDS)
        for (int i = tid; i < n3; i += nt) gcloud[i] = p[i];
}

}  // namespace

extern "C" int act_augment_f32(float* pc, int B, int N, const act_augment_op_t* ops, int nops, uint64_t seed, const uint64_t* seed_dev,
                               int flags, act_stream_t stream) {
    if (B < 0 || N < 0 || (long long)N * 3 > 0x7FFFFFFFLL || nops < 1 || nops > ACT_AUGMENT_MAX_OPS || (flags & ~ACT_AUGMENT_GLOBAL)) return ACT_E_BADARG;
    if (!ops) return ACT_E_NULLPTR;                                          // (the table is a host array: read before anything can be checked)
    AugArgs a;
    a.nops = nops;
    for (int i = 0; i < ACT_AUGMENT_MAX_OPS; ++i) {
        const bool live = i < nops;
        a.kind[i] = live ? ops[i].kind : 0;
        a.p0[i] = live ? ops[i].p0 : 0.f; a.p1[i] = live ? ops[i].p1 : 0.f; a.p2[i] = live ? ops[i].p2 : 0.f;
        a.d0[i] = live ? ops[i].draws : nullptr; a.d1[i] = live ? ops[i].draws2 : nullptr;
        if (!live) continue;
        const float p0 = a.p0[i], p1 = a.p1[i], p2 = a.p2[i];
        switch (a.kind[i]) {                                                 // (negated comparisons: a NaN parameter is refused too)
            case ACT_AUG_SCALE:           if (!(p0 <= p1)) return ACT_E_BADARG; break;
            case ACT_AUG_TRANSLATE:       if (!(p0 >= 0.f)) return ACT_E_BADARG; break;
            case ACT_AUG_SCALE_TRANSLATE: if (!(p0 <= p1) || !(p2 >= 0.f)) return ACT_E_BADARG; break;
            case ACT_AUG_ROTATE_Y:        break;
            case ACT_AUG_JITTER:          if (!(p0 >= 0.f) || !(p1 >= 0.f)) return ACT_E_BADARG; break;
            case ACT_AUG_DROPOUT:         if (!(p0 >= 0.f) || !(p0 < 1.f)) return ACT_E_BADARG; break;
            case ACT_AUG_FLIP:            if (!(p0 == 0.f || p0 == 1.f || p0 == 2.f)) return ACT_E_BADARG; break;
            default: return ACT_E_BADARG;
        }
    }
    if (B == 0 || N == 0) return 0;                                          // before the cloud pointer: an empty tensor has none
    if (!pc) return ACT_E_NULLPTR;
    hipStream_t s = (hipStream_t)stream;
    const bool lds = N <= AUG_LDS_MAX_N && !(flags & ACT_AUGMENT_GLOBAL);
    const int threads = N <= 256 ? 256 : N <= 2048 ? 512 : 1024;
    ActProfScope ps(KID_AUGMENT_CHAIN, s, 0.0, 24.0 * (double)B * N);
    if (lds) {
        const size_t smem = ((size_t)AUG_RED + (size_t)3 * N) * sizeof(float);
        auto k = augment_kernel<true>;
        if (smem > 48 * 1024) {                                              // raised once per device, to the largest staged cloud: the hot path is the launch alone
            static bool raised[64] = {false};
            int d = 0;
            if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return ACT_E_BADARG;
            if (!raised[d]) {
                const int most = (int)(((size_t)AUG_RED + (size_t)3 * AUG_LDS_MAX_N) * sizeof(float));
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, most);
                if (e != hipSuccess) return (int)e;
                raised[d] = true;
            }
        }
        hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(threads), smem, s, pc, N, a, seed, seed_dev);
    } else {
        hipLaunchKernelGGL(augment_kernel<false>, dim3((unsigned)B), dim3(threads), AUG_RED * sizeof(float), s, pc, N, a, seed, seed_dev);
    }
    ACT_LAUNCH_CHECK(); return 0;
}
