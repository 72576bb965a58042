// gemm_q_asm.hip -- launchers (= instantiations) of the NN / TN kernels with the hand-scheduled main loop (gemm_q_asm_kernel.h)
#include "gemm_q_asm_kernel.h"

// NN: 128x128, 64x128, 64x64, 128x64; TN: 128x128 with M % 128 == 0.  N % BN == 0, every K range % 32 == 0, 16-byte aligned operands,
// 32-bit lane offsets inside a tile (host-checked).  false: no such kernel.
bool launch_sgemm_q_asm(const GemmParams& p, int bm, int bn, int a_kmajor, dim3 grid, hipStream_t s) {
#define QA_ACT(BM_, BN_, AK_) \
    switch (p.epi.act) { \
        case ACT_EPI_NONE:          hipLaunchKernelGGL((sgemm_q_asm_kernel<BM_, BN_, AK_, false, false, ACT_EPI_NONE>), grid, dim3(256), 0, s, p); break; \
        case ACT_EPI_MUL_GELU_GRAD: hipLaunchKernelGGL((sgemm_q_asm_kernel<BM_, BN_, AK_, false, false, ACT_EPI_MUL_GELU_GRAD>), grid, dim3(256), 0, s, p); break; \
        case ACT_EPI_MUL_RELU_MASK: hipLaunchKernelGGL((sgemm_q_asm_kernel<BM_, BN_, AK_, false, false, ACT_EPI_MUL_RELU_MASK>), grid, dim3(256), 0, s, p); break; \
        default:                    hipLaunchKernelGGL((sgemm_q_asm_kernel<BM_, BN_, AK_>), grid, dim3(256), 0, s, p); break; \
    }
#define QA_NN_MTAIL(BM_, BN_) hipLaunchKernelGGL((sgemm_q_asm_kernel<BM_, BN_, true, true>), grid, dim3(256), 0, s, p);
#define QA_NN_ACT(BM_, BN_) QA_ACT(BM_, BN_, true)
#define QA_NN_TILE(X) \
    if (bm == 128 && bn == 128)     { X(128, 128) } \
    else if (bm == 64 && bn == 128) { X(64, 128) } \
    else if (bm == 64 && bn == 64)  { X(64, 64) } \
    else if (bm == 128 && bn == 64) { X(128, 64) } \
    else return false;
    if (!a_kmajor) {
        if (bm != 128 || bn != 128 || p.M % 128 != 0) return false;
        QA_ACT(128, 128, false)
    }
    else if (p.M % bm != 0) { QA_NN_TILE(QA_NN_MTAIL) }
    else                    { QA_NN_TILE(QA_NN_ACT) }
    return true;
#undef QA_NN_TILE
#undef QA_NN_ACT
#undef QA_NN_MTAIL
#undef QA_ACT
}

// fused max-pool backward: only the epilogue-side term (FX_SCATTER_EPI) exists on the hand-scheduled loop -- the on-load terms (FX_SCATTER_A, FX_AFFINE_B)
// stay on sgemm_q16_kernel.  Same contract as launch_sgemm_q16_fx plus K % 32 == 0; bit-identical.  false = no such kernel.
bool launch_sgemm_q_asm_fx(const GemmParams& p, int a_kmajor, int fx_mask, dim3 grid, hipStream_t s) {
    if (p.epi.act != ACT_EPI_NONE || !a_kmajor || fx_mask != FX_SCATTER_EPI || (p.K & 31) || p.k_per_split != p.K) return false;
    if ((long long)128 * p.lda * 4 >= (1ll << 31) || (long long)32 * p.ldb * 4 >= (1ll << 31)) return false;
    hipLaunchKernelGGL((sgemm_q_asm_kernel<128, 128, true, false, true, ACT_EPI_NONE>), grid, dim3(256), 0, s, p);
    return true;
}
