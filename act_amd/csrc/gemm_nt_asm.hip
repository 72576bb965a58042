// gemm_nt_asm.hip -- launchers (= instantiations) of the NT kernels with the hand-scheduled main loop (gemm_nt_asm_kernel.h)
#include "gemm_nt_asm_kernel.h"

// N % BN == 0, every K range % 32 == 0, 16-byte aligned operands, 32-bit lane offsets inside a tile (host-checked); an M tail is clamped on load
// and guarded on store.  The activation is a template parameter of the hot instantiations (see epilogue_rows).
bool launch_sgemm_nt_asm(const GemmParams& p, int bm, int bn, dim3 grid, hipStream_t s) {
#define NTA_TILE(X) \
    if (bm == 128 && bn == 128)     { X(128, 128) } \
    else if (bm == 128 && bn == 64) { X(128, 64) } \
    else if (bm == 64 && bn == 64)  { X(64, 64) } \
    else return false;
#define NTA_MTAIL(BM_, BN_) hipLaunchKernelGGL((sgemm_nt_asm_kernel<BM_, BN_, true>), grid, dim3(256), 0, s, p);
#define NTA_ACT(BM_, BN_) \
    switch (p.epi.act) { \
        case ACT_EPI_NONE: hipLaunchKernelGGL((sgemm_nt_asm_kernel<BM_, BN_, false, 0, ACT_EPI_NONE>), grid, dim3(256), 0, s, p); break; \
        case ACT_EPI_GELU: hipLaunchKernelGGL((sgemm_nt_asm_kernel<BM_, BN_, false, 0, ACT_EPI_GELU>), grid, dim3(256), 0, s, p); break; \
        case ACT_EPI_RELU: hipLaunchKernelGGL((sgemm_nt_asm_kernel<BM_, BN_, false, 0, ACT_EPI_RELU>), grid, dim3(256), 0, s, p); break; \
        default:           hipLaunchKernelGGL((sgemm_nt_asm_kernel<BM_, BN_>), grid, dim3(256), 0, s, p); break; \
    }
    if (p.M % bm != 0) { NTA_TILE(NTA_MTAIL) }
    else               { NTA_TILE(NTA_ACT) }
    return true;
#undef NTA_ACT
#undef NTA_MTAIL
#undef NTA_TILE
}
