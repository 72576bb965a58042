// gemm_q16.hip -- launchers (= instantiations) of the plain quad-fragment NN / TN kernels
#include "gemm_q16_kernel.h"

// NN: 128x128, 64x128, 64x64, 128x64 (M tail allowed); TN: 128x128.  false: no such kernel.
bool launch_sgemm_q16(const GemmParams& p, int bm, int bn, int a_kmajor, int b_kmajor, dim3 grid, hipStream_t s) {
    // kernels instantiated per activation (see epilogue_apply): none (dW, plain dX), gelu' (dX through fc2 -> GELU), relu mask (MLP heads)
#define Q16_ACT(BM_, BN_, AK_) \
    switch (p.epi.act) { \
        case ACT_EPI_NONE:          hipLaunchKernelGGL((sgemm_q16_kernel<BM_, BN_, AK_, false, false, false, false, false, ACT_EPI_NONE>), grid, dim3(256), 0, s, p); break; \
        case ACT_EPI_MUL_GELU_GRAD: hipLaunchKernelGGL((sgemm_q16_kernel<BM_, BN_, AK_, false, false, false, false, false, ACT_EPI_MUL_GELU_GRAD>), grid, dim3(256), 0, s, p); break; \
        case ACT_EPI_MUL_RELU_MASK: hipLaunchKernelGGL((sgemm_q16_kernel<BM_, BN_, AK_, false, false, false, false, false, ACT_EPI_MUL_RELU_MASK>), grid, dim3(256), 0, s, p); break; \
        default:                    hipLaunchKernelGGL((sgemm_q16_kernel<BM_, BN_, AK_, false>), grid, dim3(256), 0, s, p); break; \
    }
#define Q16_NN_MTAIL(BM_, BN_) hipLaunchKernelGGL((sgemm_q16_kernel<BM_, BN_, true, false, true>), grid, dim3(256), 0, s, p);
#define Q16_NN_ACT(BM_, BN_) Q16_ACT(BM_, BN_, true)
#define Q16_NN_TILE(X) \
    if (bm == 128 && bn == 128)     { X(128, 128) } \
    else if (bm == 64 && bn == 128) { X(64, 128) } \
    else if (bm == 64 && bn == 64)  { X(64, 64) } \
    else if (bm == 128 && bn == 64) { X(128, 64) } \
    else return false;
    if (b_kmajor) return false;                                       // NT has its own families; (A [K][M], B [N][K]) never occurs on this path
    if (!a_kmajor) {                                                  // TN: dW = dY^T . X
        if (bm != 128 || bn != 128) return false;
        Q16_ACT(128, 128, false)
    }
    else if (p.M % bm != 0) { Q16_NN_TILE(Q16_NN_MTAIL) }             // NN: dX = dY . W
    else                    { Q16_NN_TILE(Q16_NN_ACT) }
    return true;
#undef Q16_NN_TILE
#undef Q16_NN_ACT
#undef Q16_NN_MTAIL
#undef Q16_ACT
}
