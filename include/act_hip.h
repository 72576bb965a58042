/* act_hip.h -- C ABI of libact_hip.so: the MI355X (gfx950) kernels behind ACT's
 * masked-point-modeling hot path.
 *
 * Every entry point takes plain device pointers + sizes + a hipStream_t (as void*),
 * allocates nothing, never synchronises, and returns 0 or a hipError_t / negative
 * ACT_E* code.  All tensors are dense row-major fp32 unless stated; indices are
 * int32 (FPS, Chamfer) or int64 (kNN), exactly as the reference operator returns them.
 * Citations are file:line in the reference tree (RunpeiDong/ACT @ 2024_08_07).
 */
#ifndef ACT_HIP_H
#define ACT_HIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* act_stream_t;            /* hipStream_t */

#define ACT_E_BADARG   (-1)            /* shape / size outside what the kernel supports */
#define ACT_E_NULLPTR  (-2)
#define ACT_E_UNSUPPORTED (-3)         /* the entry does not take this shape (or is switched off): run the dense sequence instead */

/* ---- library ------------------------------------------------------------------------------ */
int         act_version(void);
const char* act_arch(void);             /* "gfx950" */

/* ---- live per-kernel timing (hipEvents on the launch stream; used by bench.py roofline) ---- */
int         act_prof_enable(int on);    /* returns previous state */
int         act_prof_reset(void);
int         act_prof_num_kernels(void);
const char* act_prof_kernel_name(int id);
/* synchronises the recorded events; totals since the last reset */
int         act_prof_read(int id, double* total_ms, long long* launches, double* flops, double* bytes);

/* ---- point operators ---------------------------------------------------------------------- */
/* pointnet2_ops.furthest_point_sample + gather_operation as used by misc.fps
 * (utils/misc.py:39-46; call site models/dvae.py:170).  xyz [B,N,3] -> idx int32 [B,G]
 * (idx[:,0]==0, lowest-index tie-break) and, if centers_out != NULL, centers [B,G,3]. */
size_t act_fps_scratch_floats(int B, int N);   /* 0 for N <= 16384 (the cloud lives in registers / LDS), else B*N running distances */
int act_fps_f32(const float* xyz, int B, int N, int G, int32_t* idx_out, float* centers_out,
                int skip_near_origin, float* scratch /* act_fps_scratch_floats floats, NULL when that is 0 */, act_stream_t stream);
/* Measurement infrastructure (bench.py: group_fps_knn.fps_chain), not a product entry point: latency in microseconds per iteration of the four dependent
   phases of one FPS step -- {distance evaluations, wave arg-max, cross-wave arg-max (LDS + barrier), winner's coordinates} -- and of the whole step, each
   timed as `iters` dependent repetitions in ONE workgroup of the launch configuration act_fps_f32 uses for clouds of N points (N <= 8192).  Synchronises. */
int act_fps_chain_probe(int N, int iters, double* us_per_iteration /* [5] */, int* waves_out, int* points_per_lane_out, act_stream_t stream);

/* knn_cuda.KNN(k).forward fused with Group's gather + centre subtraction
 * (models/dvae.py:159,172-182; DGCNN graph k=4 models/dvae.py:23,68).
 * ref [B,N,3], query [B,Q,3], any K <= N (K <= 64 and N <= 8192: register-resident fast path) -> idx int64 ([B,Q,K], or [B,K,Q] when idx_kq != 0:
 * transpose_mode=False layout), ascending (distance, index).
 * nbr_out  (nullable) [B,Q,K,3] = ref[idx] - query      dist_out (nullable) sqrt distance, idx layout. */
int act_knn_group_f32(const float* ref, const float* query, int B, int N, int Q, int K,
                      int64_t* idx_out, int idx_kq, float* nbr_out, float* dist_out, act_stream_t stream);

/* pointnet2_ops.gather_operation (utils/misc.py:45): feat [B,C,N], idx int32 [B,S] -> out [B,C,S];
 * backward scatter-add: grad_out [B,C,S] -> grad_feat [B,C,N] (zero-filled here, deterministic). */
int act_gather_points_f32(const float* feat, const int32_t* idx, int B, int C, int N, int S, float* out, act_stream_t stream);
int act_gather_points_bwd_f32(const float* grad_out, const int32_t* idx, int B, int C, int N, int S, float* grad_feat,
                              act_stream_t stream);

/* PointcloudScaleAndTranslate (datasets/data_transforms.py:20-34), in place:
 * pc[b,n,:] = pc[b,n,:] * scale[b,:] + shift[b,:]   (mul then add, no FMA). */
int act_scale_translate_f32(float* pc, const float* scale, const float* shift, int B, int N, act_stream_t stream);

/* PointcloudRotate (datasets/data_transforms.py:6-18), in place: pc[b,n,:] = pc[b,n,:] @ R[b] with R[b] row-major [3,3]
 * (the reference builds R = [[c,0,s],[0,1,0],[-s,0,c]] per sample on the host; any per-sample 3x3 is accepted here). */
int act_rotate_points_f32(float* pc, const float* rot, int B, int N, act_stream_t stream);

/* ---- fused augmentation chain (csrc/augment.hip; datasets/data_transforms.py, all seven transforms) ------------------------------
 * An ordered chain of 1 .. ACT_AUGMENT_MAX_OPS ops applied in place to pc [B,N,3] by ONE launch: one workgroup per cloud; for N <= 8192 the
 * cloud is staged once into LDS, every op runs there and it is written back once; for larger N, or with ACT_AUGMENT_GLOBAL in flags, the same op
 * code runs in place on global memory.  Every op sees the cloud as the earlier ops of the chain left it.  The table `ops` is a HOST array; it
 * reaches the kernel as an argument by value (nothing is allocated or copied, the entry can be captured in a hipGraph).
 * Draws are per cloud unless stated.  u denotes a uniform in [0,1).
 *   kind             p0, p1, p2      effect
 *   SCALE            lo, hi, -       s[3] = lo + (hi - lo) u;  p[:,c] *= s[c]
 *   TRANSLATE        r, -, -         t[3] = -r + (2 r) u;      p[:,c] += t[c]
 *   SCALE_TRANSLATE  lo, hi, r       p[:,c] = p[:,c] * s[c] + t[c], multiply then add (the bits of act_scale_translate_f32 for the same s, t)
 *   ROTATE_Y         -               angle 2 pi u; R = [[c,0,s],[0,1,0],[-s,0,c]]; out_j = (p0 R0j + p1 R1j) + p2 R2j
 *   JITTER           std, clip, -    per point and axis z ~ N(0,1): p += clamp(std z, -clip, clip)
 *   DROPOUT          max_ratio, -, - ratio = u_b max_ratio (fp32); per point u_n; every point with u_n <= ratio becomes a copy of point 0
 *   FLIP             upright axis    three draws (gate, first horizontal axis, second; the horizontal axes ascending); if gate < 0.95, every
 *                    (0, 1 or 2)     horizontal axis whose draw is < 0.5 becomes max_n(x) - x
 * Injected draws (device pointers, NULL: Philox): draws = scale [B,3] (SCALE, SCALE_TRANSLATE: the scale itself, not its uniform), shift [B,3]
 * (TRANSLATE), u [B] (ROTATE_Y), z [B,N,3] (JITTER), u_b [B] (DROPOUT), [B,3] (FLIP); draws2 = shift [B,3] (SCALE_TRANSLATE), u_n [B,N] (DROPOUT).
 * Philox4x32-10 draws: key = seed ^ (seed_dev[0] * 0x9E3779B97F4A7C15) (seed_dev nullable: the device-resident step counter of the bert.hip
 * kernels), counter words (c0, c1, c2, c3) = (slot, cloud, 3, position + 8 sub) with `position` the index of the op in the chain; a uniform is
 * (word >> 8) * 2^-24.  sub = 0, the per-cloud draws: slot 0 words 0..2 = the three scale / shift / flip uniforms, word 0 = the rotation's u or
 * the dropout's u_b; SCALE_TRANSLATE takes its shift uniforms from slot 1 words 0..2.  sub = 1, the per-point draws, slot = point index n:
 * DROPOUT u_n = word 0; JITTER is Box-Muller, z0 = r01 cos(2 pi u1), z1 = r01 sin(2 pi u1), z2 = r23 cos(2 pi u3) with
 * r01 = sqrt(-2 ln(((w0 >> 8) + 1) 2^-24)), u1 = (w1 >> 8) 2^-24, r23 and u3 likewise from w2 and w3 (|z| <= 5.77).
 * Returns ACT_E_BADARG for nops outside 1..8, an unknown kind or flag, lo > hi, a negative std, clip, r or max_ratio, max_ratio >= 1, an upright
 * axis other than 0, 1, 2; B == 0 or N == 0 is a success without a launch. */
#define ACT_AUGMENT_MAX_OPS 8
#define ACT_AUGMENT_GLOBAL  1          /* flags: run in place on global memory at any N (tests compare the two paths) */
#define ACT_AUG_SCALE           1
#define ACT_AUG_TRANSLATE       2
#define ACT_AUG_SCALE_TRANSLATE 3
#define ACT_AUG_ROTATE_Y        4
#define ACT_AUG_JITTER          5
#define ACT_AUG_DROPOUT         6
#define ACT_AUG_FLIP            7
typedef struct {
    int kind;
    float p0, p1, p2;
    const float *draws, *draws2;
} act_augment_op_t;
int act_augment_f32(float* pc, int B, int N, const act_augment_op_t* ops, int nops, uint64_t seed, const uint64_t* seed_dev, int flags,
                    act_stream_t stream);

/* ---- Chamfer distance (extensions/chamfer_dist: chamfer_cuda.cpp:12-39, chamfer.cu:15-229) --- */
/* forward: xyz1 [B,n,3], xyz2 [B,m,3] -> dist1 [B,n], dist2 [B,m] (squared), idx1 int32 [B,n], idx2 int32 [B,m] */
int act_chamfer_fwd_f32(const float* xyz1, const float* xyz2, int B, int n, int m,
                        float* dist1, float* dist2, int32_t* idx1, int32_t* idx2, act_stream_t stream);
/* same with the rounding of the distance selectable: fma_contract = 0 rounds every product and sum (act_chamfer_fwd_f32, the oracle
 * convention); fma_contract = 1 evaluates chamfer.cu:43-57's x2*x2 + y2*y2 + z2*z2 as fma(z2, z2, fma(x2, x2, y2*y2)), the form an
 * FMA-contracting build (nvcc's default) of the reference makes of it -- for comparing against outputs of a real CUDA build: distances agree
 * to 2 ulps, the arg-min index may differ on (near) ties. */
int act_chamfer_fwd_ex_f32(const float* xyz1, const float* xyz2, int B, int n, int m,
                           float* dist1, float* dist2, int32_t* idx1, int32_t* idx2, int fma_contract, act_stream_t stream);
/* backward: deterministic gather formulation of the reference's atomicAdd scatter */
int act_chamfer_bwd_f32(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2,
                        const float* grad_dist1, const float* grad_dist2, int B, int n, int m,
                        float* grad_xyz1, float* grad_xyz2, act_stream_t stream);


/* ---- dense fp32 GEMM on the matrix cores with fused epilogue -------------------------------- */
/* C[M,N] (+)= epilogue( alpha * opA(A)[M,K] . opB(B)[K,N] )
 *   a_kmajor=1: A stored [M][K] (lda>=K)   a_kmajor=0: A stored [K][M] (lda>=M)
 *   b_kmajor=1: B stored [N][K] (ldb>=K)   b_kmajor=0: B stored [K][N] (ldb>=N)
 * nn.Linear / Conv1d(k=1) forward = (1,1) with B = weight [out,in] (models/act.py:25-69, models/dvae.py:185-215);
 * input gradient = (1,0); weight gradient = (0,0) with K = number of rows (split-K through `workspace`).
 * epilogue order: v = alpha*acc; v += bias[col]; activation; v *= rowscale[row / rows_per_scale]; v += res[row / res_row_div, col];
 * if accumulate: v += C[row,col].   (rowscale = DropPath gate/keep per sample, res = residual stream.)
 *   ACT_EPI_GELU          : if aux != NULL the pre-activation is stored to aux[row,col]; v = gelu_erf(v)
 *   ACT_EPI_MUL_GELU_GRAD : v *= gelu'(aux[row,col])        ACT_EPI_MUL_RELU_MASK: v = aux[row,col] > 0 ? v : 0
 * workspace (nullable): scratch for split-K partials, workspace_bytes long; never allocated here. */
enum { ACT_EPI_NONE = 0, ACT_EPI_GELU = 1, ACT_EPI_RELU = 2, ACT_EPI_MUL_GELU_GRAD = 3, ACT_EPI_MUL_RELU_MASK = 4 };
typedef struct {
    float        alpha;            /* 1.0f */
    int          act;              /* ACT_EPI_* */
    int          accumulate;       /* C += result */
    int          rows_per_scale;   /* rows sharing one rowscale entry (tokens per sample) */
    int          ldr, ldaux;       /* leading dimensions of res / aux */
    int          res_row_div;      /* res row = row / res_row_div (0/1: per row; n: one res row per group of n rows) */
    const float* bias;             /* [N] or NULL */
    const float* rowscale;         /* [ceil(M / rows_per_scale)] or NULL */
    const float* res;              /* [M, ldr] or NULL */
    float*       aux;              /* [M, ldaux] or NULL */
} act_gemm_epilogue_t;
int act_sgemm_f32(int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                  float* C, int ldc, const act_gemm_epilogue_t* epilogue, float* workspace, size_t workspace_bytes,
                  act_stream_t stream);
/* same, with an explicit launch configuration (used by the host-side autotuner, act_amd/kernels.py): `tile` names a workgroup tile (BM x BN) of one
 * kernel family, splits >= 1 = split-K factor (deterministic two-pass; needs the workspace).  The ids, from the tile table in csrc/gemm.hip
 * (act_gemm_tile_info reads it); "full" = 16-byte aligned operands, M % BM == N % BN == 0, K and every K range % 32 == 0; "M tail" = full but for
 * M % BM, with A K-major:
 *    0            built-in cost model: picks the tile of 1..3 and its own split-K (`splits` is ignored); skinny TN products stream instead
 *    1,  2,  3    128x128, 128x64, 64x64 on v_mfma_f32_32x32x2_f32: all layouts, any shape
 *    4,  5,  6    the same tiles, software-pipelined (3-stage LDS, mid-tile barrier) when the shape is full, else exactly the kernels of 1..3
 *    7,  8,  9    the same tiles on v_mfma_f32_16x16x4_f32: all layouts; full or M tail
 *   10, 11, 12    the same tiles, NT only, ds_read_b128 operand fragments: full or M tail
 *   13 .. 16      128x128, 64x128, 64x64, 128x64 quad-fragment kernels: 13 NN and TN, 14..16 NN only; full or M tail
 *   17, 18        128x128, 128x64, NT, software-pipelined: full only; bit-identical to 10, 11
 *   20, 21        128x128, 128x64, NT, 32-deep K tiles: full only; bit-identical to 10, 11
 *   30, 31, 32    as 10..12 with the hand-scheduled main loop (bit-identical); additionally the byte offsets inside one K tile must fit 32 bits
 *   33 .. 36      as 13..16 with the hand-scheduled main loop (bit-identical); same offset bound
 * ACT_E_BADARG for an id that is not listed, a layout or shape the id does not take, or splits > 1 without room for the partial sums.  Between
 * families results are identical up to the fp32 summation order (and that of split-K). */
int act_sgemm_ex_f32(int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                     float* C, int ldc, const act_gemm_epilogue_t* epilogue, float* workspace, size_t workspace_bytes,
                     int tile, int splits, act_stream_t stream);

/* Several weight-gradient GEMMs of one module in ONE launch (csrc/gemm_grouped.hip): C_p[M_p,N_p] = A_p^T . B_p with A_p stored [K][M_p] (the
 * output gradient dY of a Linear, lda >= M_p), B_p stored [K][N_p] (the Linear's input X), the same K (token rows) for every problem -- the
 * dW = dY^T . X of models/act.py:25-69 for all Linears of a Transformer block -- plus, where bias_out != NULL, db_p[M_p] = column sums of A_p
 * (the bias gradient), accumulated by the workgroups that stage A_p anyway.  M_p, N_p multiples of 128, K a multiple of 16, operands 16-byte
 * aligned, at most 8 problems.  splits = number of K ranges (0: about two workgroups per CU, act_sgemm_tn_grouped_splits); for splits > 1 the
 * partials go through `workspace` (act_sgemm_tn_grouped_workspace bytes) and ONE reduction launch folds them in ascending K order
 * (deterministic).  With the same split factor C_p is bit-identical to act_sgemm_ex_f32(0, 0, ..., tile 13, splits). */
typedef struct {
    const float* A; int lda;
    const float* B; int ldb;
    float* C; int ldc;
    int M, N;
    float* bias_out;               /* [M] or NULL */
} act_gemm_tn_problem_t;
size_t act_sgemm_tn_grouped_workspace(const act_gemm_tn_problem_t* probs, int nprob, int K, int splits);
int act_sgemm_tn_grouped_splits(const act_gemm_tn_problem_t* probs, int nprob, int K);
int act_sgemm_tn_grouped_f32(const act_gemm_tn_problem_t* probs, int nprob, int K, int splits, float* workspace, size_t workspace_bytes,
                             act_stream_t stream);

/* GEMM with the producer / consumer passes of the mini-PointNet fused in (models/dvae.py:201-215: Conv1d -> BatchNorm1d -> ReLU -> Conv1d -> max):
 *  (1,1) forward conv:  a_scale/a_shift [K] (nullable, K <= 1024): A'[r,k] = max(0, A[r,k]*a_scale[k] + a_shift[k]) applied while A is staged --
 *        the BatchNorm + ReLU of the producing layer, whose output tensor then never exists;  tile_stats (nullable): per 128-row tile the
 *        column mean and sum of squared deviations of the stored values, [M/128][2][N] (act_sgemm_fx_tile_stats_floats), input of
 *        act_bn_tiles_finalize_f32 -- no statistics pass over the output;  gmax (nullable) [M/group][N] (+ garg int32, first arg-max): max over
 *        every `group` (32 | 64) consecutive rows, the max-pool over the points of a group;  store_c = 0: C itself is not written.
 *        Needs M % 128 == 0, N % 64 == 0, K % 16 == 0, 16-byte aligned operands.
 *  (0,0) weight gradient: b_scale/b_shift [N]: B'[k,n] = max(0, B[k,n]*b_scale[n] + b_shift[n]) applied while B is staged (M, N % 128 == 0, K % 32 == 0,
 *        deterministic split-K through `workspace`).
 *  backward of the max-pool (torch.max(feature, dim=2), models/dvae.py:211,214: the gradient goes to the arg-max row of every group only):
 *        sa_src [R/group][C] + sa_arg int32 (nullable pair): the A operand is VIRTUAL, A[r][c] = sa_arg[r/group][c] == r % group ? sa_src[r/group][c] : 0,
 *        generated while it is staged (A may be NULL, lda = C) -- for the input gradient (1,0: rows r = M, c = K) and the weight gradient
 *        (0,0: r = K, c = M) of the conv in front of the pool, so the scattered [R][C] gradient tensor never exists;  ep_src / ep_arg
 *        [M/group][N] (nullable pair, (1,0) only): C[r][c] += ep_arg[r/group][c] == r % group ? ep_src[r/group][c] : 0 in the epilogue (the
 *        second path into the tensor in front of the first pool).  group 32 | 64, M % 128 == 0, N % 128 == 0, C % 4 == 0.
 * The epilogue of a fused launch takes alpha / bias / rowscale / res (incl. res_row_div) / accumulate but NO activation (epi->act must be
 * ACT_EPI_NONE, else ACT_E_BADARG): the mini-PointNet applies BatchNorm + ReLU while the NEXT layer stages its operand. */
typedef struct {
    const float *a_scale, *a_shift, *b_scale, *b_shift;
    float*   tile_stats;
    float*   gmax;
    int32_t* garg;
    int      group, store_c;
    const float*   sa_src;
    const int32_t* sa_arg;
    const float*   ep_src;
    const int32_t* ep_arg;
    const int32_t* row_groups;   /* (1,1) with gmax and store_c = 0 only, nullable: the M / group row groups of A are the LISTED groups of a larger
                                  * tensor -- virtual row m is row row_groups[m / group] * group + m % group of A, and the pooled row m / group is
                                  * written to row row_groups[m / group] of gmax / garg (Stage II: the patch embedding is only needed for the
                                  * visible patches, models/act.py:269-275).  A group may be listed twice (padding M to a multiple of 128). */
} act_gemm_fx_t;
size_t act_sgemm_fx_tile_stats_floats(int M, int N);
/* Which fused launches run on the hand-scheduled main loops (csrc/gemm_nt_asm_kernel.h, gemm_q_asm_kernel.h) instead of the compiler-scheduled kernels;
 * bit-identical either way.  Bit 0: the (1,1) launches with K % 32 == 0 (default off: not faster at K <= 512); bit 1: the (1,0) launch with the
 * epilogue-side ep_src / ep_arg term only (default off: 574 -> 598 us at K = 512).  on >= 0 sets the mask (returns the previous one), on < 0 queries; initial value: env
 * ACT_GEMM_FX_ASM (default 0). */
int act_gemm_fx_asm(int on);
int act_sgemm_fx_f32(int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                     const act_gemm_epilogue_t* epilogue, const act_gemm_fx_t* fx, float* workspace, size_t workspace_bytes, act_stream_t stream);
/* BatchNorm (train mode) statistics from those tile partials: mean, rstd, scale = gamma*rstd, shift = beta - mean*scale, running stats updated
 * in place when non-NULL (what act_bn_stats_f32 produces from a pass over the tensor). */
int act_bn_tiles_finalize_f32(const float* tile_stats, int tiles, int rows_per_tile, int C, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                              act_stream_t stream);

/* ---- row-wise fused kernels of a Transformer block ------------------------------------------- */
/* xin = x + pos (pos nullable); y = LayerNorm(xin) * gamma + beta  (models/act.py:87-90 with the
 * `x = blk(x + pos)` of :109-112,140-143 fused in).  xin_out / mean / rstd are nullable. D % 4 == 0, D <= 2048. */
int act_layernorm_fwd_f32(const float* x, const float* pos, const float* gamma, const float* beta, float* xin_out,
                          float* y, float* mean, float* rstd, int T, int D, float eps, act_stream_t stream);
/* Frozen-teacher prompt rows (models/dvae.py:485-498,556-566): y[b*P+p,:] = LN(dropout(tok[p,:]) + ppos[p,:]) * gamma + beta,
 * inverted dropout with rate drop_p, keep mask from Philox4x32-10 keyed by (seed, row, column/4); tok, ppos [P,D]; y [B*P,D].
 * seed_dev (nullable): device-resident 64-bit step counter mixed into the key, so a captured hipGraph draws fresh noise per replay. */
int act_prompt_layernorm_fwd_f32(const float* tok, const float* ppos, int B, int P, int D, float drop_p, uint64_t seed,
                                 const uint64_t* seed_dev, const float* gamma, const float* beta, float eps, float* y,
                                 act_stream_t stream);
/* Prompt rows of a trained prompt layer (Stage I): y[b*P+p,:] = dropout(tok[p,:]) + ppos[p,:]; keep mask = `mask` (0/1 floats [B*P, D], nullable)
 * or Philox keyed by (seed, row, column/4) as above; backward: dppos[p,:] = sum_b dy, dtok[p,:] = sum_b dy * keep / (1 - drop_p), fixed order. */
int act_prompt_rows_fwd_f32(const float* tok, const float* ppos, const float* mask, int B, int P, int D, float drop_p, uint64_t seed,
                            float* y, act_stream_t stream);
int act_prompt_rows_bwd_f32(const float* dy, const float* mask, int B, int P, int D, float drop_p, uint64_t seed, float* dtok, float* dppos,
                            act_stream_t stream);
/* dx = dres (nullable, residual-stream gradient) + LayerNorm backward of dy; dgamma/dbeta (nullable) summed over
 * rows in a fixed order through `workspace` (act_layernorm_bwd_workspace bytes). */
size_t act_layernorm_bwd_workspace(int T, int D);
int act_layernorm_bwd_f32(const float* dy, const float* xin, const float* gamma, const float* mean, const float* rstd,
                          const float* dres, float* dx, float* dgamma, float* dbeta, int accumulate_params,
                          float* workspace, size_t workspace_bytes, int T, int D, act_stream_t stream);
/* out[c] (+)= sum_r in[r, c]  (bias gradients); deterministic two-stage. */
size_t act_colsum_workspace(int R, int C);
int act_colsum_f32(const float* in, int R, int C, int ld, float* out, int accumulate, float* workspace,
                   size_t workspace_bytes, act_stream_t stream);

/* Fused multi-head self-attention (models/act.py:57-69): qkv [B,S,3,H,hd] packed as the qkv Linear writes it,
 * out [B,S,H*hd] as the proj Linear reads it, lse [B,H,S] (nullable) = log-sum-exp of the scaled scores.
 * forward: any S (keys streamed through LDS in chunks of 128 with an online softmax), hd in {32,64}.  backward (recomputes P from lse; 128-key x 64-query LDS chunks): any S. */
int act_attention_fwd_f32(const float* qkv, float* out, float* lse, int B, int S, int H, int head_dim, float scale,
                          act_stream_t stream);
/* prefix variant: keys/values = S0 rows of kv0 [B,S0,2,H,hd] followed by the Sq rows of qkv1 [B,Sq,3,H,hd]; queries = qkv1.
 * Used for the prompt-tuned teacher (models/dvae.py:536-576): prompt tokens are keys/values only. */
int act_attention_fwd_prefix_f32(const float* kv0, int S0, const float* qkv1, int Sq, float* out, float* lse, int B,
                                 int H, int head_dim, float scale, act_stream_t stream);
int act_attention_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                          int B, int S, int H, int head_dim, float scale, act_stream_t stream);
/* backward of the prefix variant: dqkv1 [B,Sq,3,H,hd] receives dQ and the dK/dV of the Sq own rows, dkv0 [B,S0,2,H,hd] the
 * dK/dV of the prefix rows (gradients of the learnable prompts of Stage I, models/dvae.py:420-437). */
int act_attention_bwd_prefix_f32(const float* kv0, int S0, const float* qkv1, int Sq, const float* out, const float* dout,
                                 const float* lse, float* dkv0, float* dqkv1, int B, int H, int head_dim, float scale,
                                 act_stream_t stream);

/* Cosine distillation loss (models/act.py:1243-1254; lightly NegativeCosineSimilarity(dim=1, eps=1e-8)):
 * loss = mean over rows of 1 - cos(student_r, teacher_r), cos = s.t / (max(|s|, eps) max(|t|, eps)) as F.cosine_similarity has it: every
 * norm clamped on its own; backward is autograd's gradient of that.  row_loss [R], stats [R,3] are scratch kept for backward. */
int act_cosine_loss_fwd_f32(const float* student, const float* teacher, int R, int D, float eps, float* loss_out,
                            float* row_loss, float* stats, act_stream_t stream);
int act_cosine_loss_bwd_f32(const float* student, const float* teacher, const float* stats, const float* grad_loss,
                            int R, int D, float eps, float* grad_student, act_stream_t stream);

/* Alternative distillation losses (models/act.py:1186-1191,1255): kind 0 = 'l2' (nn.MSELoss, mean), kind 1 = 'smoothl1'
 * (nn.SmoothL1Loss, mean, beta 1) over [R,D]; row_loss [R] scratch. */
int act_regression_loss_fwd_f32(const float* student, const float* teacher, int R, int D, int kind, float* loss_out,
                                float* row_loss, act_stream_t stream);
int act_regression_loss_bwd_f32(const float* student, const float* teacher, const float* grad_loss, int R, int D, int kind,
                                float* grad_student, act_stream_t stream);

/* Classification loss of the finetune path (models/act.py:823-830: nn.CrossEntropyLoss(), mean over rows):
 * logits [R,C], labels int64 [R] -> loss_out[0] = mean_r (logsumexp(logits_r) - logits_r[label_r]); row_buf [3,R] =
 * {row maximum, row loss, log sum exp(logits_r - maximum) with the sign bit set where arg-max==label} (rows 0 and 2 are kept
 * for backward: maximum and log-sum are never added, so logits of any size keep their probabilities); acc_out (nullable) [1] =
 * fraction of rows whose arg-max (lowest index on ties) equals the label.
 * backward: grad_logits = grad_loss * (softmax(logits) - onehot(label)) / R. */
int act_softmax_xent_fwd_f32(const float* logits, const int64_t* labels, int R, int C, float* loss_out, float* row_buf,
                             float* acc_out, act_stream_t stream);
int act_softmax_xent_bwd_f32(const float* logits, const int64_t* labels, const float* row_buf, const float* grad_loss,
                             int R, int C, float* grad_logits, act_stream_t stream);

/* ---- mini-PointNet / FoldingNet row kernels (models/dvae.py:185-275), rows = points, columns = channels ------ */
/* train-mode BatchNorm1d statistics over all R rows: mean, rstd, scale = gamma*rstd, shift = beta - mean*scale;
 * running stats updated in place when non-NULL (momentum, unbiased variance).  The statistics do not depend on the order of the rows beyond
 * rounding: sums pivoted on row 0 where that row is a typical sample, per-part (mean, M2) combined by Chan's rule where it is not.
 * workspace: act_colstats_workspace bytes (four rows of C floats per stage-1 part), for every entry below that takes one. */
size_t act_colstats_workspace(int R, int C);
int act_bn_stats_f32(const float* x, int R, int C, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                     float* workspace, size_t workspace_bytes, act_stream_t stream);
/* y = relu?(x * scale[c] + shift[c])    (BatchNorm apply, eval or train) */
int act_affine_act_f32(const float* x, const float* scale, const float* shift, int relu, int R, int C, float* y,
                       act_stream_t stream);
/* BatchNorm(+ReLU) backward in train mode: dy w.r.t. the activation output, x = BN input -> dx, dgamma, dbeta */
int act_bn_bwd_f32(const float* x, const float* dy, const float* scale, const float* shift, const float* mean,
                   const float* rstd, int relu, int R, int C, float* dx, float* dgamma, float* dbeta,
                   float* workspace, size_t workspace_bytes, act_stream_t stream);
/* the same backward when dy is known to be zero on whole groups of n consecutive rows: rows r with live[r / n] == 0 are treated as dy = 0 and dy is not
 * read for them (bit-identical to act_bn_bwd_f32 on a dy that holds zeros there: the skipped terms are exact zeros).  live == NULL: act_bn_bwd_f32. */
int act_bn_bwd_groups_f32(const float* x, const float* dy, const float* scale, const float* shift, const float* mean, const float* rstd, int relu,
                          int R, int C, const int32_t* live, int n, float* dx, float* dgamma, float* dbeta, float* workspace,
                          size_t workspace_bytes, act_stream_t stream);
/* SyncBatchNorm building blocks (the statistics are all-reduced across ranks by the host between the calls, tools/runner_pretrain.py:86-88):
 * per-column mean / biased variance of this rank's rows; backward sums of this rank's rows; dx from the global sums over `count` rows. */
int act_col_mean_var_f32(const float* x, int R, int C, float* mean, float* var, float* workspace, size_t workspace_bytes, act_stream_t stream);
int act_bn_bwd_sums_f32(const float* x, const float* dy, const float* scale, const float* shift, const float* mean, const float* rstd,
                        int relu, int R, int C, float* sum_dy, float* sum_dy_xhat, float* workspace, size_t workspace_bytes,
                        act_stream_t stream);
int act_bn_bwd_apply_f32(const float* x, const float* dy, const float* scale, const float* shift, const float* mean, const float* rstd,
                         const float* sum_dy, const float* sum_dy_xhat, float count, int relu, int R, int C, float* dx, act_stream_t stream);
/* torch.max over the n points of each group: in [G*n, C] -> out [G,C], arg int32 [G,C] (first maximum; nullable) */
int act_group_max_f32(const float* in, int G, int n, int C, float* out, int32_t* arg, act_stream_t stream);
int act_group_max_bwd_f32(const float* dout, const int32_t* arg, int G, int n, int C, int accumulate, float* din,
                          act_stream_t stream);
/* The two products of Encoder.backward whose left operand is the gradient of that max (models/dvae.py:209-216, :262-275: the conv in front of
 * torch.max(feature, dim=2)).  dh[g*n + j][c] = (arg[g][c] == j ? dout[g][c] : 0) has one non-zero per (group, channel); these walk the live
 * entries instead of running a dense [G*n, C] GEMM operand (csrc/pool_bwd.hip):
 *   matmul: dx[g*n + j][0:N] = sum over {c : arg[g][c] == j} dout[g][c] * w[c][0:N]        (w [C, N] row-major; N in {128 (n % 8 == 0), 256, 512, 1024})
 *   wgrad:  dw[c][0:N]       = sum over g of dout[g][c] * act(x[g*n + arg[g][c]][0:N])     (x [G*n, N]; act = relu(x * scale + shift) per
 *           column when scale/shift are given, identity when both are NULL; N % 64 == 0, C % 128 == 0)
 * n <= 64 and 256 % n == 0; 16-byte aligned operands, leading dimensions multiples of 4.  The wgrad splits the groups over workgroups and folds
 * the partial sums in order (workspace bytes from act_group_max_bwd_wgrad_workspace; a smaller workspace only lowers the split count). */
int act_group_max_bwd_matmul_f32(const float* dout, const int32_t* arg, int G, int n, int C, const float* w, int ldw, int N, float* dx, int lddx,
                                 act_stream_t stream);
/* live[g] = (d[g][0:C] has a non-zero entry).  In Stage II the patch embedding runs on all B*G patches but only the visible ones feed the loss, so
 * 80 % of the rows of its output gradient are exactly zero (models/act.py:269-275); the kernels below skip those groups (the wgrad builds its own list).
 * matmul_live: the n rows of a group with live[g] == 0 are NOT written -- for a consumer that takes the same list (act_bn_bwd_groups_f32). */
int act_group_live_i32(const float* d, int G, int C, int32_t* live, act_stream_t stream);
int act_group_max_bwd_matmul_live_f32(const float* dout, const int32_t* arg, int G, int n, int C, const float* w, int ldw, int N, float* dx, int lddx,
                                      const int32_t* live, act_stream_t stream);
size_t act_group_max_bwd_wgrad_workspace(int G, int n, int C, int N);
int act_group_max_bwd_wgrad_f32(const float* dout, const int32_t* arg, int G, int n, int C, const float* x, int ldx, int N, const float* scale,
                                const float* shift, float* dw, int lddw, float* workspace, size_t workspace_bytes, act_stream_t stream);
/* out[g,c] = sum over the n rows of group g (gradient of a per-group broadcast add) */
int act_group_sum_f32(const float* in, int G, int n, int C, float* out, act_stream_t stream);

/* ---- DGCNN token mixer + dVAE tokenizer glue (models/dvae.py:26-117, 587-588) -------------------------------- */
/* Edge-conv tail.  yz [B*G, ldy] holds Y = Wa.x at column 0 and (zoff >= 0) Z = (Wb-Wa).x at column zoff; idx int64
 * [B,k,G] (KNN transpose_mode=False layout; NULL: no gather, k must be 1).  out[b*G+g, ooff + c] =
 * max_j LeakyReLU(GroupNorm_groups(Y[b, idx[b,j,g], c] + Z[b,g,c])).  stats: scratch [18*B*groups]. */
int act_edge_gn_lrelu_max_f32(const float* yz, int ldy, int zoff, const int64_t* idx, int B, int G, int k, int C,
                              int groups, const float* gamma, const float* beta, float eps, float slope, float* stats,
                              float* out, int ldo, int ooff, act_stream_t stream);
/* backward of act_edge_gn_lrelu_max_f32 (DGCNN backward of Stage I): stats = the mean/rstd the forward left in its
 * stats buffer; dout [B*G, ldd]; dyz [B*G, ldy] receives dY (columns 0..C) and dZ (columns zoff..zoff+C; idx == NULL: k = 1 head,
 * dY only); part [2][B][C] receives the per-sample partial sums of dgamma / dbeta (column-sum them for the parameter
 * gradients); mstat [2][B*groups] scratch.  Deterministic (no atomics). */
int act_edge_gn_lrelu_max_bwd_f32(const float* yz, int ldy, int zoff, const int64_t* idx, int B, int G, int k, int C, int groups,
                                  const float* gamma, const float* beta, const float* stats, float slope,
                                  const float* dout, int ldd, float* dyz, float* part, float* mstat, act_stream_t stream);
/* runtime switch of the graph-layer passes of that backward (A/B and identity tests): 1 (default) = LDS-resident slabs + gather over an inverse
 * adjacency where G <= 128 (round 6), 0 = the global-gather / scatter-image kernels; on < 0 only reads.  Returns the previous value. */
int act_edge_bwd_lds(int on);
/* Tokenizer head: logits = LeakyReLU(GroupNorm(h [B*G, C])); index = argmax_c((logits + gumbel) / tau);
 * out [B*G, D] = codebook[index]  (F.gumbel_softmax(hard=True) + einsum with the codebook, models/dvae.py:587-588).
 * noise [B*G, C] (nullable: Philox4x32-10 keyed by seed); index_out / logits_out nullable. */
int act_gn_gumbel_argmax_gather_f32(const float* h, int B, int G, int C, int groups, const float* gamma, const float* beta,
                                    float eps, float slope, const float* noise, uint64_t seed, const uint64_t* seed_dev, float tau,
                                    const float* codebook, int D, float* stats, int64_t* index_out, float* out,
                                    float* logits_out, act_stream_t stream);
/* Stage-I tokenizer (models/dvae.py:600, 470-476).  Soft gumbel-softmax over rows: y = softmax((logits + G)/tau), G = noise
 * (parity tests) or Philox keyed by (seed,row,c/4) when noise == NULL; C % 4 == 0, C <= 16384.  backward: dlogits = y (dy - <y,dy>)/tau. */
int act_gumbel_softmax_fwd_f32(const float* logits, int R, int C, const float* noise, uint64_t seed, float tau, float* y,
                               act_stream_t stream);
int act_gumbel_softmax_bwd_f32(const float* y, const float* dy, int R, int C, float tau, float* dlogits, act_stream_t stream);
/* klv = KL(mean_g softmax(logits[b,g,:]) || uniform), reduction 'batchmean'; lse [B*G] and qbar [B,C] are kept for backward. */
int act_kl_uniform_fwd_f32(const float* logits, int B, int G, int C, float* lse, float* qbar, float* klv_out, act_stream_t stream);
int act_kl_uniform_bwd_f32(const float* logits, const float* lse, const float* qbar, const float* grad_klv, int B, int G, int C,
                           float* dlogits, act_stream_t stream);

/* ---- OPT-IN: NT GEMM on the bf16 matrix cores with split operands ("bf16x3"), frozen teacher only (csrc/gemm_bf16x3.hip) -------------------------
 * x ~ hi + lo with hi = bf16(x), lo = bf16(x - hi) (round to nearest even): C = epilogue(A_hi.B_hi^T + A_hi.B_lo^T + A_lo.B_hi^T), fp32 accumulation.
 * 16 significand bits per operand: 4e-6 relative per product; NOT used by default (ACT_TEACHER_BF16X3=1 routes the teacher's ViT GEMMs here).
 * act_split_bf16x2_f32: fp32 [R, K] (row stride ldx, K % 4 == 0, 16-byte aligned) -> planes hi / lo [R][K] (uint16 bf16 bit patterns).
 * act_sgemm_nt_bf16x3_f32: planes of A [M][K] and B [N][K] (contiguous rows) -> C [M, ldc] fp32; M, N % 128 == 0, K % 64 == 0
 * (act_sgemm_nt_bf16x3_supported); epilogue: alpha, bias, ACT_EPI_NONE | ACT_EPI_GELU (+ aux), rowscale, res -- no accumulate. */
int act_split_bf16x2_f32(const float* x, int R, int K, int ldx, uint16_t* hi, uint16_t* lo, act_stream_t stream);
int act_sgemm_nt_bf16x3_supported(int M, int N, int K);
int act_sgemm_nt_bf16x3_f32(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_lo, const uint16_t* b_hi, const uint16_t* b_lo,
                            float* C, int ldc, const act_gemm_epilogue_t* epilogue, act_stream_t stream);
/* producers that hand their result on as planes (y nullable: planes only): LayerNorm of x + pos, and the prompt rows' dropout + position + LayerNorm;
 * bit-identical to producing fp32 and splitting it with act_split_bf16x2_f32 */
int act_layernorm_fwd_planes_f32(const float* x, const float* pos, const float* gamma, const float* beta, float* xin_out, float* y,
                                 uint16_t* y_hi, uint16_t* y_lo, float* mean /* nullable */, float* rstd /* nullable */, int T, int D, float eps,
                                 act_stream_t stream);
int act_prompt_layernorm_fwd_planes_f32(const float* tok, const float* ppos, int B, int P, int D, float drop_p, uint64_t seed,
                                        const uint64_t* seed_dev, const float* gamma, const float* beta, float eps, uint16_t* y_hi, uint16_t* y_lo,
                                        act_stream_t stream);
int act_attention_fwd_prefix_planes_f32(const float* kv0, int S0, const float* qkv1, int Sq, float* out, uint16_t* out_hi, uint16_t* out_lo, float* lse,
                                        int B, int H, int head_dim, float scale, act_stream_t stream);
/* the same product with the result ALSO (C != NULL) or ONLY (C == NULL) written as (hi, lo) bf16 planes [M][N]: the A operand of the next split-bf16
 * product comes straight out of this epilogue (teacher MLP: fc1 + GELU -> planes -> fc2) */
int act_sgemm_nt_bf16x3_planes_f32(int M, int N, int K, const uint16_t* a_hi, const uint16_t* a_lo, const uint16_t* b_hi, const uint16_t* b_lo,
                                   float* C, int ldc, uint16_t* out_hi, uint16_t* out_lo, const act_gemm_epilogue_t* epilogue, act_stream_t stream);

/* ---- DEFAULT teacher arithmetic: the same kernel on f16 planes with a scaled low plane ("f16x3", csrc/gemm_bf16x3.hip F16 form, csrc/split_planes.h) ----
 * x s = h1 + 2^-11 h2 with h1 = f16(x s), h2 = f16((x s - h1) 2^11) (round to nearest even; a plane element below 2^-14 is written as +0 before the
 * residual is taken), s a power of two that keeps |x s| <= 2^15: 22 significand bits + the residual's sign per operand, fp32-grade products.
 * C = epilogue( (A_h1.B_h1^T + 2^-11 (A_h1.B_h2^T + A_h2.B_h1^T)) * b_inv_scale[n] / a_scale ), two fp32 accumulators, lo.lo term (2^-22) dropped.
 * act_split_f16x2_f32: planes of x * scale * row_scale[row] (row_scale nullable).  b_inv_scale [N] = 1 / (B's row scales), 16-byte aligned.
 * out_h1 / out_h2 (nullable pair): the result also (C != NULL) or only as planes [M][N] of result * out_scale.  Shapes as act_sgemm_nt_bf16x3_supported. */
int act_split_f16x2_f32(const float* x, int R, int K, int ldx, float scale, const float* row_scale, uint16_t* h1, uint16_t* h2, act_stream_t stream);
/* the same planes, bit for bit, written with rows ldp elements apart (ldp >= K, ldp % 8 == 0, h1 / h2 16-byte aligned): a column slice of a wider plane buffer */
int act_split_f16x2_ld_f32(const float* x, int R, int K, int ldx, float scale, uint16_t* h1, uint16_t* h2, int ldp, act_stream_t stream);
int act_sgemm_nt_f16x3_supported(int M, int N, int K);
int act_sgemm_nt_f16x3_planes_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, float a_scale, const uint16_t* b_h1,
                                  const uint16_t* b_h2, const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2, float out_scale,
                                  const act_gemm_epilogue_t* epilogue, act_stream_t stream);
/* The product picks its tile from the shape alone: 128 x 128 (4 waves, two workgroups per CU) or, where N % 384 == 0 and the grid then fills the CUs in fewer
 * tile units, 128 x 192 (8 waves, one workgroup per CU).  Every tile gives the same bits.  act_sgemm_nt_f16x3_pick_tile: that rule as a pure host function of
 * the shape and the CU count -> 128 or 192 (0: unsupported shape).  ..._planes_tile_f32: the same product with the tile given -- 0: the rule (what the entry
 * above does), 128, or 192 (N % 192 == 0); any other tile, or one the shape does not take, is ACT_E_BADARG.  ACT_X3_TILE=128 in the environment (read once)
 * makes the rule answer 128 everywhere. */
int act_sgemm_nt_f16x3_pick_tile(int M, int N, int K, int cus);
int act_sgemm_nt_f16x3_planes_tile_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, float a_scale, const uint16_t* b_h1,
                                       const uint16_t* b_h2, const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2,
                                       float out_scale, const act_gemm_epilogue_t* epilogue, act_stream_t stream, int tile);
/* ..._planes_lda_f32: the same product with the rows of the A planes lda elements apart -- a column slice of a wider plane buffer (lda >= K, lda % 8 == 0, a_h1 and
 * a_h2 16-byte aligned; anything else is ACT_E_BADARG and launches nothing).  lda == K is the entry above, bit for bit. */
int act_sgemm_nt_f16x3_planes_lda_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, int lda, float a_scale, const uint16_t* b_h1,
                                      const uint16_t* b_h2, const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2,
                                      float out_scale, const act_gemm_epilogue_t* epilogue, act_stream_t stream, int tile);
/* K-TILE-MAJOR PLANES (notebook/x3_ktile.md).  Element (r, k) of a plane [R][K] at ((k / 32) * R + r) * 32 + k % 32: the 64-byte pieces
 * of the rows of one K tile lie side by side, and the product stages an operand tile in whole 128-byte lines.  Same values, same bits.
 * act_repack_ktile_u16: a pure copy of one dense plane into that layout (K % 32 == 0, 16-byte aligned, src != dst, else ACT_E_BADARG).
 * act_split_f16x2_kt_f32: act_split_f16x2_f32 without row scales whose planes leave K-tile-major, as rows 0 .. R of a [rows_total][K] plane.
 * ..._planes_layout_f32: the product with the layout of each operand and of the planes-out given.  ACT_X3_ROWMAJOR: as the entries above (lda: 0 = K; a
 * row-major B is dense; *_rows_total not read).  ACT_X3_KTILE: the pointers are at element (r0, c0) of the planes of a
 * [rows_total][..] matrix -- the operand is its rows r0 .. and columns c0 .. c0 + K, c0 % 32 == 0 -- and lie on a 128-byte line; rows_total >= the operand's
 * rows (M or N).  out_layout ACT_X3_KTILE: the planes-out [M][N] leave K-tile-major (128-byte aligned).  Any other layout value, rows_total too small or a
 * misaligned K-tile-major plane is ACT_E_BADARG and launches nothing. */
enum { ACT_X3_ROWMAJOR = 0, ACT_X3_KTILE = 1 };
int act_repack_ktile_u16(const uint16_t* src, uint16_t* dst, int R, int K, act_stream_t stream);
int act_split_f16x2_kt_f32(const float* x, int R, int K, int ldx, float scale, uint16_t* h1, uint16_t* h2, int rows_total, act_stream_t stream);
int act_sgemm_nt_f16x3_planes_layout_f32(int M, int N, int K, const uint16_t* a_h1, const uint16_t* a_h2, int a_layout, int lda, int a_rows_total,
                                         float a_scale, const uint16_t* b_h1, const uint16_t* b_h2, int b_layout, int b_rows_total,
                                         const float* b_inv_scale, float* C, int ldc, uint16_t* out_h1, uint16_t* out_h2, float out_scale,
                                         int out_layout, const act_gemm_epilogue_t* epilogue, act_stream_t stream, int tile);
/* ACT_X3_KT (environment, read once; default 1) / act_x3_kt: whether the callers that build the planes of frozen weights (act_amd/composite.py) keep them
 * K-tile-major, and the composites hand activations on that way; 0 is the row-major step. */
int act_x3_kt(int on /* < 0: query */);                 /* -> previous setting */
/* the plane producers in this format: bit-identical to producing fp32 and splitting it with act_split_f16x2_f32 at plane_scale */
int act_layernorm_fwd_f16_planes_f32(const float* x, const float* pos, const float* gamma, const float* beta, float* xin_out, float* y,
                                     uint16_t* y_h1, uint16_t* y_h2, float plane_scale, float* mean /* nullable */, float* rstd /* nullable */, int T, int D,
                                     float eps, act_stream_t stream);
int act_attention_fwd_prefix_f16_planes_f32(const float* kv0, int S0, const float* qkv1, int Sq, float* out, uint16_t* out_h1, uint16_t* out_h2,
                                            float plane_scale, float* lse, int B, int H, int head_dim, float scale, act_stream_t stream);
/* the prompt rows of act_prompt_layernorm_fwd_f32 (same Philox mask, bit for bit) as f16 planes at plane_scale (> 0, else ACT_E_BADARG; planes 8-byte aligned) */
int act_prompt_layernorm_fwd_f16_planes_f32(const float* tok, const float* ppos, int B, int P, int D, float drop_p, uint64_t seed,
                                            const uint64_t* seed_dev, const float* gamma, const float* beta, float eps, uint16_t* y_h1, uint16_t* y_h2,
                                            float plane_scale, act_stream_t stream);
/* The group-max product of the frozen tokenizer's mini-PointNet on this kernel:  out[g, :] = max over the `group` (32 or 64) rows of group g of
 * (a . B^T + bias), a [M, K] = relu(A * a_col_scale[k] + a_col_shift[k]) -- nothing else is stored.  A != NULL: a is formed, scaled by a_scale and split
 * while the kernel stages A (fp32, row stride lda; a_h1 / a_h2 unused); A == NULL: a_h1 / a_h2 are the planes of a * a_scale, as the pass
 * act_split_f16x2_affine_relu_f32 writes them.  The two forms give the same bits, as do the two tiles (tile: 0 = act_sgemm_nt_f16x3_gmax_pick_tile, 128, 192).
 * ..._supported: the shapes of act_sgemm_nt_f16x3_supported with K <= 512 and group in {32, 64}.  bias nullable; out [M / group, N], row stride ldo. */
int act_split_f16x2_affine_relu_f32(const float* x, int R, int K, int ldx, const float* col_scale, const float* col_shift, float scale, uint16_t* h1,
                                    uint16_t* h2, act_stream_t stream);
int act_sgemm_nt_f16x3_gmax_supported(int M, int N, int K, int group);
int act_sgemm_nt_f16x3_gmax_pick_tile(int M, int N, int K, int cus);
int act_sgemm_nt_f16x3_gmax_f32(int M, int N, int K, const float* A, int lda, const float* a_col_scale, const float* a_col_shift, const uint16_t* a_h1,
                                const uint16_t* a_h2, float a_scale, const uint16_t* b_h1, const uint16_t* b_h2, const float* b_inv_scale,
                                const float* bias, int group, float* out, int ldo, int tile, act_stream_t stream);
/* the same with the layout of B's planes given (ACT_X3_ROWMAJOR: the entry above; ACT_X3_KTILE and b_rows_total as in act_sgemm_nt_f16x3_planes_layout_f32) */
int act_sgemm_nt_f16x3_gmax_layout_f32(int M, int N, int K, const float* A, int lda, const float* a_col_scale, const float* a_col_shift, const uint16_t* a_h1,
                                       const uint16_t* a_h2, float a_scale, const uint16_t* b_h1, const uint16_t* b_h2, int b_layout, int b_rows_total,
                                       const float* b_inv_scale, const float* bias, int group, float* out, int ldo, int tile, act_stream_t stream);

/* ---- GEMM launch-configuration table (host side) ------------------------------------------------------------------------
 * act_sgemm_f32 (no explicit configuration) first consults this table keyed by (a_kmajor, b_kmajor, M, N, K), then its built-in
 * cost model.  The Python host fills it from the shipped tune file and from first-use timing (act_amd/kernels.py); the composite
 * entry points below therefore launch exactly the configurations the single-GEMM path uses. */
int act_gemm_tune_set(int a_kmajor, int b_kmajor, int M, int N, int K, int tile, int splits);   /* ACT_E_BADARG: tile not 0 and in no row, splits < 0 */
int act_gemm_tune_get(int a_kmajor, int b_kmajor, int M, int N, int K, int* tile, int* splits);   /* 0 = found, 1 = absent */
int act_gemm_tune_clear(void);
/* One row of the tile table behind act_sgemm_ex_f32: 0 = found, 1 = `tile` names no kernel (0, the cost model, is no row).  Out-pointers nullable.
 * layouts: ACT_GEMM_LAYOUT_* bits, bit 2 * a_kmajor + b_kmajor;  need: ACT_GEMM_NEED_ANY / _FULL_OR_MTAIL / _FULL, possibly | ACT_GEMM_NEED_OFFSET32. */
#define ACT_GEMM_LAYOUT_TN 1           /* a_kmajor = 0, b_kmajor = 0 */
#define ACT_GEMM_LAYOUT_TT 2           /* 0, 1 */
#define ACT_GEMM_LAYOUT_NN 4           /* 1, 0 */
#define ACT_GEMM_LAYOUT_NT 8           /* 1, 1 */
#define ACT_GEMM_NEED_ANY           0
#define ACT_GEMM_NEED_FULL_OR_MTAIL 1
#define ACT_GEMM_NEED_FULL          2
#define ACT_GEMM_NEED_OFFSET32      4
int act_gemm_tile_info(int tile, int* bm, int* bn, int* layouts, int* need);

/* x[r,:] * gate[r / rows_per_scale] -> y   (DropPath gate applied to a gradient, utils/transformer_layers.py:105-120) */
int act_scale_rows_f32(const float* x, const float* gate, int T, int D, int rows_per_scale, float* y, act_stream_t stream);
/* eval-mode BatchNorm folded to an affine map: scale = gamma * rsqrt(running_var + eps), shift = beta - running_mean * scale */
int act_bn_eval_affine_f32(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                           int C, float* scale, float* shift, act_stream_t stream);

/* ---- composite entry points: one host call enqueues every kernel of a module -------------------------------------------
 * A Stage-II step is ~500 kernel launches; issued one ctypes call at a time the host needs ~16 ms per step, which is what
 * bounds an 8-rank node sharing one host.  These functions run the launch sequence of a whole module in C: same kernels, same
 * order, same results (bit-identical to calling the single-kernel entry points above one by one).  All buffers are caller-owned;
 * `saved` / `scratch` are single slabs whose sizes the *_floats helpers return; nothing is allocated, nothing synchronises.
 * `side_stream` (nullable): weight-gradient GEMMs and bias column sums are enqueued there (forked after the producing kernel on
 * `stream`, joined back before the function returns) so they share the chip with the latency-bound dX chain. */
/* GEMM-shape collection (host-side autotuning of composites): between begin and end, on the same host thread, the composite
 * entry points launch nothing and record the (a_kmajor, b_kmajor, M, N, K) of each GEMM they would launch.
 * end -> number recorded (the first `max` written to shapes [max][5]). */
int act_composite_collect_begin(void);
int act_composite_collect_end(int* shapes, int max);
/* The only state the library keeps: up to 32 fork / join events (hipEventDisableTiming) per stream that ever produced work for another stream
 * inside a composite call.  act_composite_shutdown destroys them; call it when no composite call is in flight on any host thread and the
 * streams involved are idle (e.g. before hipDeviceReset / at interpreter exit).  Later composite calls simply create new events.  Returns
 * the number of events destroyed. */
int act_composite_shutdown(void);

typedef struct {                     /* parameters of one pre-LN Transformer block (models/act.py:72-90; timm ViT block) */
    const float *norm1_w, *norm1_b, *qkv_w, *qkv_b /* nullable */, *proj_w, *proj_b, *norm2_w, *norm2_b,
                *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} act_block_params_t;
typedef struct {                     /* where the gradients go; NULL struct pointer = frozen block (dX only) */
    float *norm1_w, *norm1_b, *qkv_w, *qkv_b /* nullable */, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} act_block_grads_t;
typedef struct { int B, S, D, heads, hidden; float eps; } act_block_dims_t;

/* forward of blk(x + pos) (models/act.py:87-90 called as :109-112): 7 launches.  x, pos (nullable), out: [B*S, D];
 * gate1 / gate2 (nullable) [B] = DropPath floor(keep+U)/keep of the two residual branches; keep_for_backward = 0 skips the
 * statistics / pre-activation stores.  saved: act_block_saved_floats(dims) floats (activations kept for the backward). */
size_t act_block_saved_floats(const act_block_dims_t* d);
int act_block_fwd_f32(const act_block_dims_t* d, const act_block_params_t* w, const float* x, const float* pos,
                      const float* gate1, const float* gate2, int keep_for_backward, float* saved, float* out,
                      float* workspace, size_t workspace_bytes, act_stream_t stream);
/* backward: dout [B*S, D] -> dx [B*S, D] (gradient of x and of pos) + parameter gradients.  scratch: act_block_bwd_scratch_floats. */
size_t act_block_bwd_scratch_floats(const act_block_dims_t* d);
int act_block_bwd_f32(const act_block_dims_t* d, const act_block_params_t* w, const float* gate1, const float* gate2,
                      const float* saved, const float* dout, float* dx, const act_block_grads_t* grads, float* scratch,
                      float* workspace, size_t workspace_bytes, float* side_workspace, size_t side_workspace_bytes,
                      act_stream_t stream, act_stream_t side_stream);

/* A STACK of `depth` such blocks in one host call -- x = blk_l(x + pos) for l = 0 .. depth-1, the loop of TransformerEncoder.forward /
 * TransformerDecoder.forward (models/act.py:109-112,140-143) -- and its backward.  Pure launch sequencing: the forward is depth calls of
 * act_block_fwd_f32, the backward depth calls of act_block_bwd_f32 in reverse order plus, when dpos != NULL, depth-1 element-wise additions that
 * accumulate the gradient of the shared `pos` input as ((dx_{depth-1} + dx_{depth-2}) + ...) + dx_0, the order in which an autograd engine
 * folds the per-block gradients: results are bit-identical to the per-block calls (tests/test_gpu_composite.py).
 * gate1 / gate2: arrays of depth pointers (entries nullable; a NULL array = no DropPath anywhere).
 * saved: act_block_stack_saved_floats(d, depth, keep_for_backward) floats; scratch: act_block_stack_bwd_scratch_floats(d, depth).
 * grads: array of depth structs (NULL = frozen stack, dX only).  dx = gradient of x; dpos (nullable) = gradient of pos, a separate buffer
 * when depth > 1 (with depth == 1 it is not written: the gradient of pos IS dx). */
typedef struct {
    int depth;
    const act_block_params_t* blocks;          /* [depth] */
    const float* const* gate1;                 /* [depth] or NULL */
    const float* const* gate2;                 /* [depth] or NULL */
} act_block_stack_t;
size_t act_block_stack_saved_floats(const act_block_dims_t* d, int depth, int keep_for_backward);
size_t act_block_stack_bwd_scratch_floats(const act_block_dims_t* d, int depth);
int act_block_stack_fwd_f32(const act_block_dims_t* d, const act_block_stack_t* st, const float* x, const float* pos, int keep_for_backward,
                            float* saved, float* out, float* workspace, size_t workspace_bytes, act_stream_t stream);
/* dpos (nullable): gradient of the shared pos, folded in the order the blocks finish; with depth 1 and no dpos_in nothing is written (it IS dx).
   dpos_in (nullable, needs dpos): the fold of the deeper chunks of the same stack -- the chain continues through it, so a stack differentiated in
   chunks associates exactly like the unchunked call */
int act_block_stack_bwd_f32(const act_block_dims_t* d, const act_block_stack_t* st, const float* saved, const float* dout, float* dx, float* dpos,
                            const float* dpos_in, const act_block_grads_t* grads, float* scratch, float* workspace, size_t workspace_bytes, float* side_workspace,
                            size_t side_workspace_bytes, act_stream_t stream, act_stream_t side_stream);
/* out[i] = a[i] + b[i] (one rounding; out may alias a or b), n % 4 == 0, 16-byte aligned */
int act_add_f32(const float* a, const float* b, float* out, long long n, act_stream_t stream);

/* Block on G patch tokens per cloud with P prompt tokens acting as keys / values only (prompt-tuned frozen Transformer,
 * models/dvae.py:536-576: every layer replaces the prompt rows of its input and the output drops them).  dims: S = G.
 * x, pos [B*G, D]; prompt rows either prm [B*P, D] (= dropout(prompt) + prompt_pos, differentiable path) or n1p [B*P, D]
 * (their LayerNorm, already computed by act_prompt_layernorm_fwd_f32).  Weights are frozen: the backward produces dx (= dpos) and
 * dprm only.  saved: act_prefix_block_saved_floats; scratch: act_prefix_block_bwd_scratch_floats. */
size_t act_prefix_block_saved_floats(const act_block_dims_t* d, int P);
int act_prefix_block_fwd_f32(const act_block_dims_t* d, int P, const act_block_params_t* w, const float* x, const float* pos,
                             const float* prm, const float* n1p, int keep_for_backward, float* saved, float* out,
                             float* workspace, size_t workspace_bytes, act_stream_t stream);
/* The same block, inference only, with the prompts' keys / values kvp [B*P, 2D] given (act_prompt_kv_fwd_f32) instead of prm / n1p. */
int act_prefix_block_fwd_kv_f32(const act_block_dims_t* d, int P, const act_block_params_t* w, const float* x, const float* pos,
                                const float* kvp, float* saved, float* out, float* workspace, size_t workspace_bytes, act_stream_t stream);
/* Keys / values of the frozen teacher's prompt rows without the dense product: kvp [B*P, N] = LN(dropout(tok[p]) + ppos[p]) . W^T + bias with the
 * rows, the Philox keying and the mask of act_prompt_layernorm_fwd_f32; W [N, D] (16-byte aligned), bias [N] nullable.  The cloud-independent part
 * (undropped rows, centred on their mean) is ONE (P+2) x N x D product per call; the dropped channels of every row are then walked against a weight
 * tile held in LDS, in increasing channel order (no atomics: bit-identical runs).  scratch: act_prompt_kv_workspace bytes, 16-byte aligned;
 * workspace: the GEMM's.  ACT_E_UNSUPPORTED (nothing launched) for D % 4 != 0, a D whose tile does not fit LDS (D > 1240), or when switched off
 * (ACT_PROMPT_KV_SPARSE=0 / act_prompt_kv_sparse(0)): the caller runs act_prompt_layernorm_fwd_f32 + the dense product. */
int act_prompt_kv_sparse(int on /* < 0: query */);      /* -> previous setting */
size_t act_prompt_kv_workspace(int B, int P, int D, int N);      /* bytes; 0 for an unsupported shape */
int act_prompt_kv_fwd_f32(const float* tok, const float* ppos, int B, int P, int D, int N, float drop_p, uint64_t seed,
                          const uint64_t* seed_dev, const float* gamma, const float* beta, float eps, const float* W, const float* bias,
                          float* kvp, float* scratch, size_t scratch_bytes, float* workspace, size_t workspace_bytes, act_stream_t stream);
/* The same keys / values as ONE dense product on the split-f16 kernel (the default teacher's form): act_prompt_layernorm_fwd_f16_planes_f32 into `planes`
 * (second plane B P D elements further; planes_elems >= 2 B P D, 16-byte aligned) at a_scale, then act_sgemm_nt_f16x3_planes_tile_f32 with the bias epilogue
 * -> kv [B P, N] fp32.  w_h1 / w_h2 / w_inv: the planes and inverse row scales of W [N, D]; a_scale: the static activation scale of the LayerNorm rows; tile: 0 =
 * the library's rule, 128, 192.  ACT_E_UNSUPPORTED (nothing launched) when switched off (ACT_PROMPT_KV_F16X3=0 / act_prompt_kv_f16x3(0)), for a_scale <= 0,
 * a null plane or scale pointer, planes_elems too small, or a shape act_sgemm_nt_f16x3_supported(B P, N, D) refuses: the caller runs act_prompt_kv_fwd_f32. */
int act_prompt_kv_f16x3(int on /* < 0: query */);       /* -> previous setting */
int act_prompt_kv_fwd_f16x3_f32(const float* tok, const float* ppos, int B, int P, int D, int N, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                                const float* gamma, const float* beta, float eps, const uint16_t* w_h1, const uint16_t* w_h2, const float* w_inv,
                                float a_scale, const float* bias, float* kv, uint16_t* planes, size_t planes_elems, int tile, act_stream_t stream);
/* the same with the layout of the weight planes given: ACT_X3_KTILE, w_rows_total as the B operand of act_sgemm_nt_f16x3_planes_layout_f32 (the K,V rows of
 * a K-tile-major qkv weight: pointers 32 D elements behind the planes, w_rows_total = 3 D) */
int act_prompt_kv_fwd_f16x3_layout_f32(const float* tok, const float* ppos, int B, int P, int D, int N, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                                       const float* gamma, const float* beta, float eps, const uint16_t* w_h1, const uint16_t* w_h2, int w_layout,
                                       int w_rows_total, const float* w_inv, float a_scale, const float* bias, float* kv, uint16_t* planes,
                                       size_t planes_elems, int tile, act_stream_t stream);
size_t act_prefix_block_bwd_scratch_floats(const act_block_dims_t* d, int P);
int act_prefix_block_bwd_f32(const act_block_dims_t* d, int P, const act_block_params_t* w, const float* prm, const float* saved,
                             const float* dout, float* dx, float* dprm, float* scratch, float* workspace, size_t workspace_bytes,
                             act_stream_t stream);

/* Whole frozen prompt-tuned Transformer of the Stage-II teacher in ONE call (visual_embedding_deep_prompt, models/dvae.py:536-576,
 * inference form): pos = visual_pos_embed(center); x = proj_pre(tokens); depth x { LN(dropout(prompt_i) + prompt_pos_i) (in-kernel
 * Philox keyed by seed_base + 7919 (i+1) and the device-resident step counter), prefix block }; LN; proj_post.  ~125 launches. */
typedef struct {
    int B, P, G, D, heads, hidden, depth, tokens_dims, pos_hidden;
    float eps, drop_p;
    uint64_t seed_base;
    const uint64_t* seed_dev;
    const float *pos_w0, *pos_b0, *pos_w1, *pos_b1, *pre_w, *pre_b, *post_w, *post_b, *norm_w, *norm_b;
    const float* const* prompt_tok;           /* [depth] -> [P, D] */
    const float* const* prompt_pos;           /* [depth] -> [P, D] */
    const act_block_params_t* blocks;         /* [depth] */
} act_prefix_vit_t;
size_t act_prefix_vit_scratch_floats(const act_prefix_vit_t* m);
/* OPT-IN variant (never the default; ACT_TEACHER_BF16X3=1 on the host side): the five Linear products of every block on the split-bf16 kernel
 * (act_sgemm_nt_bf16x3_f32) wherever it takes the shape, everything else as act_prefix_vit_fwd_f32.  w_planes[4 i + {0,1,2,3}] = hi plane of block i's
 * qkv_w [3D][D], proj_w [D][D], fc1_w [hidden][D], fc2_w [D][hidden] (the lo plane follows the hi plane: rows * cols elements further);
 * a_planes: scratch for activation planes, a_planes_elems >= 2 * B*G * hidden + 2 * max(B*G, B*P) * D (the MLP's hidden activation leaves fc1's epilogue
 * as planes and never exists in fp32; the other activations are split by a pass).  Teacher features move by ~7e-6 of their range. */
typedef struct {
    const uint16_t* const* w_planes;          /* [4 * depth] */
    uint16_t* a_planes;
    size_t a_planes_elems;
} act_vit_bf16x3_t;
int act_prefix_vit_fwd_bf16x3_f32(const act_prefix_vit_t* m, const act_vit_bf16x3_t* x3, const float* tokens, const float* center, float* out,
                                  float* scratch, float* workspace, size_t workspace_bytes, act_stream_t stream);
/* ... and the differentiable forward of ONE prefix block (Stage-I prompt tuning) the same way: x3->w_planes[0..3] = this block's four weights; the backward
 * (act_prefix_block_bwd_f32) is unchanged, everything it reads is still written. */
int act_prefix_block_fwd_bf16x3_f32(const act_block_dims_t* d, int P, const act_block_params_t* w, const act_vit_bf16x3_t* x3, const float* x, const float* pos,
                                    const float* prm, int keep_for_backward, float* saved, float* out, float* workspace, size_t workspace_bytes,
                                    act_stream_t stream);
/* ... and its backward: x3->w_planes[0..4] = planes of the TRANSPOSED weights fc2_w^T [hidden][D], fc1_w^T [D][hidden], proj_w^T [D][D], qkv_w^T [D][3D],
 * (qkv_w rows D..3D)^T [D][2D]; the five input-gradient products run on the split-bf16 kernel, LayerNorm / attention backward stay f32. */
int act_prefix_block_bwd_bf16x3_f32(const act_block_dims_t* d, int P, const act_block_params_t* w, const act_vit_bf16x3_t* x3, const float* prm,
                                    const float* saved, const float* dout, float* dx, float* dprm, float* scratch, float* workspace,
                                    size_t workspace_bytes, act_stream_t stream);
int act_prefix_vit_fwd_f32(const act_prefix_vit_t* m, const float* tokens, const float* center, float* out, float* scratch,
                           float* workspace, size_t workspace_bytes, act_stream_t stream);
/* DEFAULT on the host side (ACT_TEACHER_F16X3, 0 restores act_prefix_vit_fwd_f32): the FOUR Linear products of every block (qkv, proj, fc1, fc2 on the patch
 * tokens) on the split-f16 kernel, and the prompts' keys / values through act_prompt_kv_fwd_f16x3_f32 at the qkv Linear's scale (act_prompt_kv_fwd_f32 where
 * that entry answers ACT_E_UNSUPPORTED).  w_planes[4 i + j] = h1 plane of block i's j-th weight, split
 * with one power of two per output row (h2 plane rows * cols elements further); w_inv_scale[4 i + j] = the N inverse row scales (device); a_scale[4 i + j]
 * (HOST) = the static activation scale s_A of that Linear, from a weight-only bound on its operand (bound * s_A <= 2^15: overflow impossible by
 * construction), or 0: that Linear stays on the f32 kernel, as does any shape the kernel does not take.  a_planes as in act_vit_bf16x3_t. */
typedef struct {
    const uint16_t* const* w_planes;          /* [4 * depth] */
    const float* const* w_inv_scale;          /* [4 * depth] */
    const float* a_scale;                     /* [4 * depth], host memory */
    uint16_t* a_planes;
    size_t a_planes_elems;
    int w_layout;                             /* bit j (0..3: qkv, proj, fc1, fc2) set: the planes of that weight, in every block, are K-tile-major
                                               * (act_repack_ktile_u16 of each plane); 0: all row-major.  Any other bit is ACT_E_BADARG */
} act_vit_f16x3_t;
int act_prefix_vit_fwd_f16x3_f32(const act_prefix_vit_t* m, const act_vit_f16x3_t* x3, const float* tokens, const float* center, float* out,
                                 float* scratch, float* workspace, size_t workspace_bytes, act_stream_t stream);

/* mini-PointNet patch embedding (Encoder, models/dvae.py:185-215) on rows = points: x [BG*n, 3] -> tokens [BG, C].
 * conv 3->128, BN, ReLU, conv 128->256, max over the n points of a group, conv 512->512 on cat(global, local) (the global half
 * evaluated once per group), BN, ReLU, conv 512->C, max.  training: batch statistics + running-stat update, else running stats. */
typedef struct {
    const float *c1_w, *c1_b, *bn1_w, *bn1_b, *c2_w, *c2_b, *c3_w, *c3_b, *bn2_w, *bn2_b, *c4_w, *c4_b;
    float *bn1_mean, *bn1_var, *bn2_mean, *bn2_var;      /* running statistics (updated in place when training) */
} act_pointnet_params_t;
typedef struct { float *c1_w, *c1_b, *bn1_w, *bn1_b, *c2_w, *c2_b, *c3_w, *c3_b, *bn2_w, *bn2_b, *c4_w, *c4_b; } act_pointnet_grads_t;
typedef struct { int BG, n, C; float eps1, eps2, momentum1, momentum2; } act_pointnet_dims_t;
size_t act_pointnet_saved_floats(const act_pointnet_dims_t* d);
int act_pointnet_fwd_f32(const act_pointnet_dims_t* d, const act_pointnet_params_t* w, const float* x, int training,
                         int keep_for_backward, float* saved, float* out, float* workspace, size_t workspace_bytes,
                         act_stream_t stream);
/* The same forward when only some groups' tokens are wanted (Stage II: MaskTransformer keeps the visible patches, models/act.py:269-275): everything in
 * front of the last conv still runs on all groups (its BatchNorm statistics are over all of them), the last conv + max-pool only on the n_groups listed
 * groups (int32 ids, device memory; n_groups * n a multiple of 128 -- repeat an id to pad).  out / the saved arg-max rows of unlisted groups are set to
 * zero; the backward then expects a zero gradient row for them.  groups == NULL: act_pointnet_fwd_f32. */
int act_pointnet_fwd_groups_f32(const act_pointnet_dims_t* d, const act_pointnet_params_t* w, const float* x, int training, int keep_for_backward,
                                float* saved, float* out, const int32_t* groups, int n_groups, float* workspace, size_t workspace_bytes,
                                act_stream_t stream);
/* The same entry for a FROZEN encoder under no-grad (the Stage-II tokenizer): the last product -- R = BG * n rows, C columns, K = 512, the group max as its
 * epilogue -- on the split-f16 kernel (act_sgemm_nt_f16x3_gmax_f32, A activated and split on load).  c4_planes = the h1 plane of c4_w split with one power of
 * two per output row (act_split_f16x2_f32; the h2 plane C * 512 elements behind it), c4_inv_scale [C] the inverse row scales, a_scale a power of two with
 * a_scale * max|relu(bn2(h3))| <= 2^15 (training-mode statistics bound that by sqrt(R) max|gamma| + max|beta|; the caller derives it).  Everything up to and
 * including h3 and the BatchNorm-2 affine is act_pointnet_fwd_groups_f32's, bit for bit.  The split path is taken only with a usable x3 (not NULL, no NULL
 * pointer in it, a_scale > 0), keep_for_backward == 0, groups == NULL, the fused schedule, and R % 128 == 0, C % 128 == 0; every other call runs the f32
 * product and equals act_pointnet_fwd_groups_f32 bit for bit. */
typedef struct {
    const uint16_t* c4_planes;
    const float* c4_inv_scale;
    float a_scale;
    int w_layout;                             /* ACT_X3_ROWMAJOR (0) | ACT_X3_KTILE: both planes of c4_w K-tile-major */
} act_pointnet_f16x3_t;
int act_pointnet_fwd_groups_f16x3_f32(const act_pointnet_dims_t* d, const act_pointnet_params_t* w, const act_pointnet_f16x3_t* x3, const float* x,
                                      int training, int keep_for_backward, float* saved, float* out, const int32_t* groups, int n_groups,
                                      float* workspace, size_t workspace_bytes, act_stream_t stream);
size_t act_pointnet_bwd_scratch_floats(const act_pointnet_dims_t* d);
int act_pointnet_bwd_f32(const act_pointnet_dims_t* d, const act_pointnet_params_t* w, const float* x, const float* saved,
                         const float* dout, const act_pointnet_grads_t* grads, float* scratch, float* workspace,
                         size_t workspace_bytes, act_stream_t stream);

/* DGCNN (models/dvae.py:26-117), inference form, everything up to (not including) layer5's GroupNorm: f [B*G, Cin], graph idx
 * int64 [B,k,G] -> h [B*G, Cout].  w_in/b_in = input_trans; stacked[l] = [Wa ; Wb - Wa] of edge-conv layer l ([2*cout_l, cin_l]);
 * gn_w/gn_b[l] = its GroupNorm(4) affine; w5 = layer5 conv [Cout, 2304]. */
typedef struct {
    int B, G, k, Cin, Cout, groups;
    float eps, slope;
    const float *w_in, *b_in, *w5;
    const float* stacked[4];
    const float* gn_w[4];
    const float* gn_b[4];
} act_dgcnn_t;
size_t act_dgcnn_scratch_floats(const act_dgcnn_t* m);
int act_dgcnn_features_f32(const act_dgcnn_t* m, const float* f, const int64_t* idx, float* h, float* scratch, float* workspace,
                           size_t workspace_bytes, act_stream_t stream);
/* the same with the head product (T = B*G rows, Cout columns, K = 2304, the frozen w5) on the split-f16 kernel (act_sgemm_nt_f16x3_planes_f32): cat is split
 * at the static scale a_scale (a power of two with a_scale * max|cat| <= 2^15; the caller derives the bound from the four GroupNorm affines) and multiplied
 * with the planes of w5 (act_split_f16x2_f32 with the row scales whose inverses are w5_inv_scale [Cout]).  w5_planes = the h1 plane, the h2 plane Cout * 2304
 * elements behind it; a_planes = scratch for the planes of cat, >= 2 * T * 2304 elements.  Everything up to cat is act_dgcnn_features_f32's, bit for bit.
 * x3 unusable -- NULL, a NULL pointer in it, a_scale <= 0, a_planes_elems too small, or !act_sgemm_nt_f16x3_supported(T, Cout, 2304) -- runs the f32 head
 * product: the result then equals act_dgcnn_features_f32 bit for bit.
 * layers != 0: the stacked edge-conv products of layers 2-4 (T x 2 cout x cin against the frozen [Wa ; Wb - Wa]) run on the same kernel as well.  st_planes[i] /
 * st_inv_scale[i] (i = 0..2: layers 2, 3, 4) are the planes (h2 plane 2 cout cin elements behind h1) and inverse row scales of stacked[i + 1].  Each tail's
 * fp32 slice of cat is split into a_planes at its column, at the same a_scale (the bound covers all four tails), row stride 2304; the next layer reads its A
 * operand there (act_sgemm_nt_f16x3_planes_lda_f32) and the head multiplies the planes that are then already complete -- the same bytes the whole-cat pass
 * writes.  With layers != 0, w5_planes may be NULL (or the head's shape refused): the head alone then stays on the f32 kernel.  With layers != 0 a NULL layer
 * pointer, a_scale <= 0, a short or NULL a_planes or T % 128 != 0 run the whole f32 sequence: act_dgcnn_features_f32 bit for bit. */
typedef struct {
    const uint16_t* w5_planes;
    const float* w5_inv_scale;
    float a_scale;
    uint16_t* a_planes;
    size_t a_planes_elems;
    int layers;
    const uint16_t* st_planes[3];
    const float* st_inv_scale[3];
    int w_layout;                             /* ACT_X3_ROWMAJOR (0) | ACT_X3_KTILE: the planes of w5 and of every stacked matrix K-tile-major */
} act_dgcnn_f16x3_t;
int act_dgcnn_features_f16x3_f32(const act_dgcnn_t* m, const act_dgcnn_f16x3_t* x3, const float* f, const int64_t* idx, float* h, float* scratch,
                                 float* workspace, size_t workspace_bytes, act_stream_t stream);

/* ---- dense per-point prediction (semantic segmentation head; csrc/seg.hip; models/pt.py log_softmax, nll_loss) -----------------
 * row log-softmax [R,C] (C <= 64) and its backward dz = dout - exp(logp) * rowsum(dout) */
int act_log_softmax_fwd_f32(const float* z, long long R, int C, float* out, act_stream_t stream);
int act_log_softmax_bwd_f32(const float* logp, const float* dout, long long R, int C, float* dz, act_stream_t stream);
/* F.nll_loss(logp, target, weight) (weighted mean; weight NULL = ones): loss[0], wsum[0] = sum of w[t], correct[0] (int64, may be NULL) = rows whose
 * arg-max (lowest index on ties) equals the target.  Deterministic: per-block partials, one ordered pass.  Targets outside [0,C) are skipped. */
size_t act_nll_weighted_workspace(long long R);
int act_nll_weighted_fwd_f32(const float* logp, const int64_t* target, const float* weight, long long R, int C, float* loss, float* wsum,
                             int64_t* correct, float* workspace, size_t workspace_bytes, act_stream_t stream);
int act_nll_weighted_bwd_f32(const int64_t* target, const float* weight, const float* wsum, const float* gloss, long long R, int C, float* dlogp,
                             act_stream_t stream);
/* cm int64 [C,C] += counts of (target, arg-max of pred row) (lowest index on ties); rows with a target outside [0,C) are skipped */
int act_confusion_i64(const float* pred, const int64_t* target, long long R, int C, int64_t* cm, act_stream_t stream);

/* ---- part segmentation (ShapeNetPart; csrc/partseg.hip) -------------------------------------------------------------------------
 * part_segmentation/models/pt.py label_conv_cls = Conv1d(16, 64, bias=False) + BatchNorm1d(64) + LeakyReLU(slope) on the category rows
 * cls [B,16] (any values, not only one-hot), W [64,16] -> y [B,64].  training: batch statistics over the B rows (B >= 2), running_mean /
 * running_var updated in place (momentum, unbiased variance with count B); eval: running statistics.  One launch each, float64 inside,
 * one rounding per output; every reduction over B runs in a fixed order (bit-identical run to run, no float atomics). */
int act_label_branch_fwd_f32(const float* cls, const float* W, const float* gamma, const float* beta, int B, int training, float eps, float momentum,
                             float slope, float* running_mean, float* running_var, float* y, act_stream_t stream);
/* backward of the train-mode branch from dy [B,64] (batch statistics recomputed from cls and W): dW [64,16], dgamma [64], dbeta [64]
 * (no gradient for cls) */
int act_label_branch_bwd_f32(const float* cls, const float* W, const float* gamma, const float* beta, const float* dy, int B, float eps, float slope,
                             float* dW, float* dgamma, float* dbeta, act_stream_t stream);
/* category-masked evaluation (main.py:235-299), one workgroup per shape: logp [B*N,P] (P <= 64), target int64 [B*N]; the shape's category is
 * part2cat[target[first point]] (int32 [P]) and its parts are [cat_first[c], cat_first[c+1]) (int32 [ncat+1], at most 6 parts).
 * pred (int32 [B*N], may be NULL) = arg-max over that range (ties: first index).  counts int32 [num_shapes,16]: row shape_offset + i gets
 * [0,6) intersections and [6,12) unions of the local parts, [12] the category (-1 when the first target is not a valid part), [13] the
 * number of parts, [14,16) zero.  seen / correct int64 [P] += per-part counts of target == l and pred == target == l (integer atomics). */
int act_part_eval_f32(const float* logp, const int64_t* target, int B, int N, int P, const int32_t* part2cat, const int32_t* cat_first, int ncat,
                      int32_t* pred, int32_t* counts, int shape_offset, int num_shapes, int64_t* seen, int64_t* correct, act_stream_t stream);

/* ---- whole-room sliding-window testing (S3DIS; csrc/wholescene.hip) ---------------------------------------------------------------
 * semantic_segmentation/main_test.py with dataset.py ScannetDatasetWholeScene.  xyz float64 [P,3] (the room, promoted exactly from a float32
 * file); table float64 [gy*gx, 6] = lo_x, hi_x, lo_y, hi_y, cx, cy of block iy*gx + ix, computed on the host in the file's dtype.
 * Membership: point p is in block b iff lo_x <= x <= hi_x && lo_y <= y <= hi_y (the reference's np.where), lists in increasing point order.
 * member_count: counts int32 [gx*gy], offsets int32 [gx*gy + 1] (exclusive scan); ws of act_scene_member_workspace bytes, kept for
 * member_fill, which writes members int32 [offsets[gx*gy]] (block b at [offsets[b], offsets[b+1])).  P <= 2^27, gx*gy <= 2^20. */
size_t act_scene_member_workspace(long long P, int gx, int gy);
int act_scene_member_count(const double* xyz, long long P, const double* table, int gx, int gy, int32_t* counts, int32_t* offsets, void* ws,
                           size_t ws_bytes, act_stream_t stream);
int act_scene_member_fill(const double* xyz, long long P, const double* table, int gx, int gy, const int32_t* offsets, int32_t* members, void* ws,
                          size_t ws_bytes, act_stream_t stream);
/* keyed row-index build of one vote: rows int32 [R]; nb non-empty blocks block_ids[s] (grid index, count > 0), block s at rows
 * [row_off[s], row_off[s+1]) (point_size = ceil(count / block_points) * block_points).  Fill (point_size - count draws from the members,
 * without replacement when that is <= count) and shuffle are counter-based functions of (seed, room, vote, block) (csrc/wholescene.hip). */
int act_scene_rows(const int32_t* members, const int32_t* member_off, const int32_t* block_ids, const int32_t* row_off, int nb, long long R,
                   int block_points, unsigned seed, unsigned room, unsigned vote, int32_t* rows, act_stream_t stream);
/* out float32 [R,3] = (x - cx, y - cy, z) of point rows[r] with its block's centre, in float64 and rounded once (rows outside [0,P): NaN) */
int act_scene_gather(const double* xyz, long long P, const double* table, const int32_t* rows, const int32_t* block_ids, const int32_t* row_off,
                     int nb, long long R, float* out, act_stream_t stream);
/* votes int32 [P,C] += 1 at (rows[r], arg-max of logp[r, :]) for r < n (ties: the first maximum; a NaN wins) when labelweights[label[point]]
 * is non-zero and not infinite (main_test.py add_vote); rows outside [0,P) and labels outside [0,C) do not vote.  C <= 64. */
int act_scene_vote(const float* logp, const int32_t* rows, long long n, long long P, int C, const int32_t* label, const float* labelweights,
                   int32_t* votes, act_stream_t stream);
/* pred int32 [P] = arg-max of votes[p, :] (ties: lowest class; no votes: 0); cm int64 [C,C] (may be NULL) += (label, pred) counts, labels
 * outside [0,C) skipped.  C <= 64. */
int act_scene_finish(const int32_t* votes, const int32_t* label, long long P, int C, int32_t* pred, int64_t* cm, act_stream_t stream);

/* ---- S3DIS training blocks from resident rooms (csrc/s3dis_sample.hip) -----------------------------------------------------------------
 * semantic_segmentation/dataset.py:119-147, one launch per batch, one workgroup per item.  Rooms back to back: xyz float64 [P_total,3], labels
 * int32 [P_total], room_off int64 [R+1].  Grid of room r: origin grid_origin[r] = (min x, min y), square cells of side `cell`, grid_dims[r] =
 * (gx, gy, first cell of the room in cell_off); cell iy*gx + ix; cell_off int64 [cells + 1] offsets into cell_pts int32 [P_total] (point index
 * within the room, ascending inside a cell).  Item b: room room_ids[b], draws keyed by (seed, epoch, item_ids[b], attempt).  Attempt t takes a
 * point of the room as centre; members: cx - block_size/2 <= x <= cx + block_size/2, the same in y (float64, inclusive).  The first attempt with
 * count > min_points is taken; after max_tries (<= 65536) the largest count (earliest on ties) and info = -max_tries, else info = attempts used.
 * center_in (may be NULL) fixes the centre point of every item: one attempt, accepted whatever its count.  count >= num_point: num_point distinct
 * members in random order (keyed bijection); else with replacement.  out_xyz float32 [B,num_point,3] = (x - cx, y - cy, z) in float64 rounded
 * once, out_labels int64 [B,num_point], rows int32 [B,num_point] (point index within the room), count / center_idx / info int32 [B].  ws:
 * act_s3dis_sample_workspace(B, max_window) bytes, max_window >= the points of any window of overlapped cells.  An item whose room id or
 * injected centre is out of range reads nothing: rows -1, labels -1, xyz NaN, count 0, info 0. */
size_t act_s3dis_sample_workspace(int B, long long max_window);
int act_s3dis_sample_f32(const double* xyz, const int32_t* labels, const long long* room_off, int R, const double* grid_origin,
                         const long long* grid_dims, const long long* cell_off, const int32_t* cell_pts, double block_size, double cell,
                         int min_points, int max_tries, long long max_window, const int32_t* room_ids, const int32_t* item_ids,
                         const int32_t* center_in, int B, int num_point, unsigned seed, unsigned epoch, float* out_xyz, int64_t* out_labels,
                         int32_t* rows, int32_t* count, int32_t* center_idx, int32_t* info, void* ws, size_t ws_bytes, act_stream_t stream);

/* ---- Object-dataset batches from a resident split (csrc/cloud_sample.hip) ---------------------------------------------------------------
 * datasets/ShapeNet55Dataset.py:35-51, datasets/ModelNetDataset.py:120-140, one launch per batch, one workgroup per item.  clouds float32
 * [M,N,C], C = 3 or 6, xyz first.  Item b reads cloud item_ids[b]; its draws are keyed by (seed, epoch, draw_ids[b]) alone.  With
 * ACT_CLOUD_PERMUTE position j < n takes source row ws_feistel(j, N, key): n distinct rows in random order (a full permutation at n == N);
 * without it row j.  With ACT_CLOUD_NORMALIZE xyz gets numpy's pc_norm in numpy's order: per coordinate the fp32 sum over j ascending, divided
 * by (float)n and subtracted; m = max_j sqrtf((x*x + y*y) + z*z); every coordinate / m (m == 0: NaN, as numpy).  Channels 3..5 are copied.
 * out float32 [B,n,C]; src_rows int32 [B,n] (may be NULL) receives the source rows.  ACT_E_BADARG for B < 1, M < 1, n < 1, n > N,
 * n > act_cloud_sample_max_points(), C not 3 or 6, an unknown flag.  An item id outside [0,M) reads nothing: out NaN, src_rows -1. */
#define ACT_CLOUD_PERMUTE   1
#define ACT_CLOUD_NORMALIZE 2
int act_cloud_sample_max_points(void);
int act_cloud_sample_f32(const float* clouds, long long M, int N, int C, const int32_t* item_ids, const int32_t* draw_ids, int B, int n,
                         unsigned seed, unsigned epoch, int flags, float* out, int32_t* src_rows, act_stream_t stream);

/* ---- Stage-I reconstruction evaluation (csrc/recon_eval.hip) ------------------------------------------------------------------------
 * tools/runner_autoencoder.py:219-323 (validate) with utils/metrics.py, one launch per batch, one workgroup per cloud: coarse [B,nc,3],
 * dense [B,nd,3], gt [B,N,3] -> row row0 + b of out (float64 [num_rows, ACT_RECON_FIELDS]):
 *   [0] sparse L1  [1] sparse L2   ChamferDistanceL1 / L2 (coarse, gt) of that one cloud: L1 = (mean sqrt d1 + mean sqrt d2) / 2, L2 = mean d1 + mean d2
 *   [2] dense L1   [3] dense L2    the same for dense
 *   [4] CDL1       [5] CDL2        (dense, gt) with ignore_zeros at batch size 1: points whose fp32 (x + y) + z == 0 are neither queries nor
 *                                  candidates, the means divide by the counts that remain; NaN when either cloud has no point left
 *   [6] precision hits  [7] recall hits   dense points whose nearest gt point / gt points whose nearest dense point is closer than th (all points)
 *   [8] F-Score = 2 r p / (r + p), 0 when r + p == 0     [9] non-zero dense points  [10] non-zero gt points  [11] 0
 * Values are NOT scaled by 1000.  Squared distances are fp32 with every product and sum rounded (the per-point minima are those of
 * act_chamfer_fwd_f32, lowest index on ties); sums are float64 in a fixed order (bit-identical run to run, no atomics); the threshold is
 * applied to the float64 distance between the query and the selected neighbour.  Clouds that fit in LDS are staged once; larger ones are
 * tiled.  B == 0 is a no-op; rows outside [row0, row0 + B) are not touched. */
#define ACT_RECON_FIELDS 12
int act_recon_eval_f32(const float* coarse, const float* dense, const float* gt, int B, int nc, int nd, int N, float th, double* out, int row0,
                       int num_rows, act_stream_t stream);

/* ---- linear-SVM validation of pretrained features (csrc/svm.hip) ---------------------------------------------------------------------
 * tools/runner_pretrain.py:47-51, 228-287: sklearn.svm.LinearSVC() on extracted features, i.e. liblinear's L2-regularised L2-loss SVC,
 * one-vs-rest, with the bias regularised (its appended constant feature) but kept as a separate scalar per class:
 *   f_c(w, b) = 1/2 (|w|^2 + b^2) + C sum_i max(0, 1 - y_ic (x_i . w + b))^2,   y_ic = +1 if labels[i] == classes[c] else -1.
 * X fp32 [N,D], labels int64 [N], classes int64 [K], K <= 64.  Every reduction has a fixed order (float64 where it runs over the N rows) and
 * there are no atomics: all outputs are bit-identical run to run.  X is read with 16-byte loads when D % 4 == 0 and X is 16-byte aligned.
 *
 * scores: out [N,K] = X . W^T + b (b [K], may be NULL); mask ([N,K], may be NULL): out = 0 where mask == 0. */
int act_svm_scores_f32(const float* X, const float* W, const float* b, const float* mask, int N, int D, int K, float* out, act_stream_t stream);
/* hinge: from scores M [N,K], R [N,K] = y max(0, 1 - y m) (its non-zero pattern is the active set) and sums float64 [K] = sum_i h^2 */
size_t act_svm_hinge_workspace(int N, int K);
int act_svm_hinge_f32(const float* M, const int64_t* labels, const int64_t* classes, int N, int K, float* R, double* sums, void* workspace,
                      size_t workspace_bytes, act_stream_t stream);
/* transposed product: out [K,D] = P[N,K]^T . X[N,D], colsum [K] (may be NULL) = column sums of P; fp32 partial products over 256 rows, summed
 * in float64 and rounded once */
size_t act_svm_tprod_workspace(int N, int D, int K);
int act_svm_tprod_f32(const float* P, const float* X, int N, int D, int K, float* out, float* colsum, void* workspace, size_t workspace_bytes,
                      act_stream_t stream);
/* ONE Newton iteration of all K classes, in place on W [K,D], b [K]: gradient, up to max_cg conjugate-gradient iterations on the generalised
 * Hessian I + 2C X_A^T X_A (per class, until |r| <= 0.05 |g|), then the largest step 2^-t (t < 16) that passes the Armijo test on the true
 * objective.  istate int32 [3,K]: row 0 = 0 running / 1 converged (|grad f_c| <= tol) / 2 no progress (no step accepted, or an accepted
 * decrease below fp32 epsilon times the objective: the resolution of an objective built on fp32 scores), row 1 Newton steps taken, row 2 CG
 * iterations.  dstate float64 [2,K]: row 0 objective and row 1 gradient norm at the iteration's START.  Start from istate = 0; a class whose
 * row-0 flag is set is frozen.  The caller repeats the call until every flag is set;
 * nothing is read back or synchronised here. */
size_t act_svm_newton_workspace(int N, int D, int K);
int act_svm_newton_f32(const float* X, const int64_t* labels, const int64_t* classes, int N, int D, int K, float C, float tol, int max_cg,
                       float* W, float* b, int32_t* istate, double* dstate, void* workspace, size_t workspace_bytes, act_stream_t stream);

/* ---- exact t-SNE of classifier features (csrc/tsne.hip) ------------------------------------------------------------------------------
 * tools/runner_tsne.py: openTSNE's TSNE(perplexity=25, metric="cosine") on the concat_f features.  Here: the exact objective (no Barnes-Hut,
 * no interpolation), every stage on the device.  Every reduction has a fixed order (float64 wherever many terms meet); the only atomics are
 * integer counters whose order a sort removes: all outputs are bit-identical run to run.  Workspaces are 16-byte aligned.
 *
 * kNN graph under the cosine distance 1 - x^_i . x^_j (x^ = x / |x|; a row of zero norm has x^ = 0, i.e. distance 1 to every row): for every
 * row of X fp32 [N,D] its k nearest OTHER rows, idx int32 [N,k] and dist fp32 [N,k] in ascending distance, ties towards the lower index.
 * 1 <= k <= min(N - 1, 1024).  Distances are formed in slabs of 512 rows: no N x N matrix exists. */
size_t act_tsne_knn_workspace(int N, int D);
int act_tsne_knn_cosine_f32(const float* X, int N, int D, int k, int32_t* idx, float* dist, void* workspace, size_t workspace_bytes,
                            act_stream_t stream);
/* conditional p fp32 [N,k] from dist fp32 [N,k]: per row the beta at which the entropy of p_j ~ exp(-beta (d_j - d_min)) equals
 * log(perplexity), by bisection in float64 (beta doubles while the upper bound is open, halves while the lower one is), until
 * |H - log perplexity| < 1e-5 or 100 steps; every row sums to 1.  beta fp32 [N] may be NULL. */
int act_tsne_conditional_p_f32(const float* dist, int N, int k, float perplexity, float* p, float* beta, act_stream_t stream);
/* P = (P_cond + P_cond^T) / 2N as CSR: indptr int32 [N + 1], indices (ascending within a row) and values with room for `capacity` >= 2 N k
 * entries; indptr[N] entries are written.  count -> scan -> fill through the sorted inverse adjacency. */
size_t act_tsne_symmetrize_workspace(int N, int k);
int act_tsne_symmetrize_f32(const int32_t* idx, const float* p, int N, int k, int32_t* indptr, int32_t* indices, float* values,
                            long long capacity, void* workspace, size_t workspace_bytes, act_stream_t stream);
/* one optimisation step, in place on Y, update and gains (fp32 [N,2] each), nothing read back:
 *   w_ij = 1 / (1 + |y_i - y_j|^2),  Z = sum_{i != j} w_ij,  g_i = exaggeration sum_j P_ij w_ij (y_i - y_j) - (1/Z) sum_j w_ij^2 (y_i - y_j)
 *   gain += 0.2 where sign(g) != sign(update) else gain *= 0.8, floor 0.01;  update = momentum update - lr gain g;  Y += update;  Y -= mean(Y).
 * The repulsive term and Z are the exact sweep over all pairs.  act_tsne_steps_f32 runs n_steps such steps in one call (the same launches:
 * bit-identical to n_steps single calls). */
size_t act_tsne_step_workspace(int N);
int act_tsne_step_f32(const int32_t* indptr, const int32_t* indices, const float* values, int N, float exaggeration, float momentum, float lr,
                      float* Y, float* update, float* gains, void* workspace, size_t workspace_bytes, act_stream_t stream);
int act_tsne_steps_f32(const int32_t* indptr, const int32_t* indices, const float* values, int N, int n_steps, float exaggeration,
                       float momentum, float lr, float* Y, float* update, float* gains, void* workspace, size_t workspace_bytes,
                       act_stream_t stream);
/* out[0] (one device double) = KL(P || Q) = sum_ij P_ij log(P_ij / (w_ij / Z)), accumulated in float64; workspace: act_tsne_step_workspace */
int act_tsne_kl_f32(const int32_t* indptr, const int32_t* indices, const float* values, const float* Y, int N, double* out, void* workspace,
                    size_t workspace_bytes, act_stream_t stream);
/* PCA initialisation Y fp32 [N,2]: centred features, covariance by the TN GEMM, its two leading eigenvectors by orthogonal iteration in float64
 * (one workgroup; until the subspace moves by less than 1e-10 or 500 sweeps) and a Rayleigh-Ritz rotation, each signed so that its
 * largest-magnitude entry is positive; the projection is scaled so that column 0 has standard deviation 1e-4.  2 <= D <= 1024.
 * info float64 [4]: the two eigenvalues of X_c^T X_c, the sweeps run, the last subspace change. */
size_t act_tsne_pca_workspace(int N, int D);
int act_tsne_pca_init_f32(const float* X, int N, int D, float* Y, double* info, void* workspace, size_t workspace_bytes, act_stream_t stream);

/* ---- frozen post-LayerNorm language teacher (csrc/bert.hip; reference models/dvae.py:617-857) ------------------------------------ */
/* y = LayerNorm(keep o t / (1 - drop_p) + res) * gamma + beta on rows [T, D] (D % 4 == 0, D <= 2048); rstd [T] (nullable) for the backward.
 * keep: `mask` (0/1 floats [T, D], nullable) or Philox4x32-10 keyed by (seed, row, column/4) and the device-resident counter seed_dev (nullable),
 * the convention of act_prompt_layernorm_fwd_f32; drop_p == 0 reads neither.
 * backward: dres = LayerNorm backward of dy, dt = dres o keep / (1 - drop_p) with the mask regenerated; the normalised row comes back from the
 * forward's output, (y - beta) / gamma, so gamma must have no zero entry.  No dgamma / dbeta: the language model is frozen. */
int act_dropout_add_layernorm_fwd_f32(const float* t, const float* res, const float* mask, int T, int D, float drop_p, uint64_t seed,
                                      const uint64_t* seed_dev, const float* gamma, const float* beta, float eps, float* y, float* rstd,
                                      act_stream_t stream);
int act_dropout_add_layernorm_bwd_f32(const float* dy, const float* y, const float* mask, int T, int D, float drop_p, uint64_t seed,
                                      const uint64_t* seed_dev, const float* gamma, const float* beta, const float* rstd, float* dt,
                                      float* dres, act_stream_t stream);
/* Self-attention with dropout on the probabilities: out = (softmax(q k^t scale) o keep / (1 - drop_p)) v, the normaliser over the undropped
 * probabilities; qkv / out / lse / dqkv as act_attention_fwd_f32, any S >= 1, hd in {32,64}, B*H <= 65535.
 * keep: `mask` (uint8 [B,H,S,S], nullable) or Philox4x32-10 keyed by (seed, (b H + h) S + query, key/4) and seed_dev (nullable).
 * backward: recomputes P from lse and the mask from its key; delta [B,H,S] is scratch (rowsum(dout o out)). */
int act_attention_dropout_fwd_f32(const float* qkv, const uint8_t* mask, float* out, float* lse, int B, int S, int H, int head_dim,
                                  float scale, float drop_p, uint64_t seed, const uint64_t* seed_dev, act_stream_t stream);
int act_attention_dropout_bwd_f32(const float* qkv, const uint8_t* mask, const float* out, const float* dout, const float* lse,
                                  float* delta, float* dqkv, int B, int S, int H, int head_dim, float scale, float drop_p, uint64_t seed,
                                  const uint64_t* seed_dev, act_stream_t stream);

/* ---- CLIP image teacher (csrc/clip.hip; reference models/dvae.py:394-403, :500-511) ------------------------------------------------ */
/* QuickGELU of CLIP's residual blocks on rows [rows, cols] (dense; any rows * cols, any 4-byte aligned pointers, 16-byte accesses where the
 * pointers agree modulo 16 bytes):  out = pre * sigmoid(1.702 pre);  dx = dy * s * (1 + 1.702 pre (1 - s)),  s = sigmoid(1.702 pre).
 * Finite for every finite input: s and 1 - s come from exp(-|1.702 pre|).  out may alias pre, dx may alias dy. */
int act_quickgelu_fwd_f32(const float* pre, float* out, int rows, int cols, act_stream_t stream);
int act_quickgelu_bwd_f32(const float* pre, const float* dy, float* dx, int rows, int cols, act_stream_t stream);

/* ---- weighted k-NN validation of frozen features (csrc/knn_probe.hip) ----------------------------------------------------------------
 * The protocol of Wu et al. 2018 (instance discrimination) that DINO's eval_knn uses: for every query the kmax most similar bank rows under
 * the dot product of (optionally L2-normalised) fp32 features, then per k a class vote weighted by exp(sim / T).  No solver, no tolerance.
 * Order is total: larger similarity first, then lower bank index.  Every similarity is one k-ordered fp32 fmaf chain (v_mfma_f32_16x16x4_f32),
 * so all outputs are bit-identical run to run and do not depend on `splits`.  1 <= kmax <= 256; the Nq x Nb similarities never reach memory.
 *
 * normalize: out [N,D] = x / max(|x|, 1e-12), the norm summed in a fixed order; a zero row stays zero. */
int act_knn_probe_normalize_f32(const float* X, int N, int D, float* out, act_stream_t stream);
/* search: Q fp32 [Nq,D], bank fp32 [Nb,D] -> idx int32 [Nq,kmax], sim fp32 [Nq,kmax] (either may be NULL), best first.  normalize != 0: both
 * sides are normalised as above (into the workspace) first.  exclude_self != 0: query i never selects bank row i (by index: leave-one-out of
 * the bank on itself; an exact duplicate elsewhere is still returned).  kmax <= Nb - (exclude_self != 0).
 * splits: number of bank ranges searched by separate workgroups and merged (0 = chosen from the shape; at most 16 and at most ceil(Nb / 128));
 * act_knn_probe_splits returns the number used.  The workspace (16-byte aligned) holds the padded copies of both sides and kmax 64-bit keys
 * per query and split. */
int act_knn_probe_splits(int Nq, int Nb, int kmax, int splits);
size_t act_knn_probe_workspace(int Nq, int Nb, int D, int kmax, int splits);
int act_knn_probe_search_f32(const float* Q, int Nq, const float* bank, int Nb, int D, int kmax, int normalize, int exclude_self, int splits,
                             int32_t* idx, float* sim, void* workspace, size_t workspace_bytes, act_stream_t stream);
/* vote: sim / idx [Nq,kmax] of a search, bank_cls int32 [Nb] and q_cls int32 [Nq] (may be NULL) class indices in 0 .. C-1 (C <= 1024; a q_cls
 * outside that range never counts as a hit), ks: nk <= 16 ascending values in 1 .. kmax, read on the HOST.  For every query and ks[j]:
 *   scores [Nq,nk,C] (may be NULL): s_c = sum over ranks r < ks[j] with bank_cls[idx_r] == c of exp(sim_r / T), added in rank order in fp32;
 *   pred int64 [Nq,nk] (may be NULL): the class index of the largest score, ties to the lowest class;
 *   counts int64 [nk,2] (may be NULL): += 1 per query whose q_cls is the prediction (column 0) / among the five best scores under the same tie
 *   rule (column 1).  Integer atomics: the caller zeroes counts, may accumulate several calls into it, and reads it once. */
int act_knn_probe_vote_f32(const float* sim, const int32_t* idx, int Nq, int kmax, const int32_t* bank_cls, int Nb, const int32_t* q_cls, int C,
                           const int* ks, int nk, float T, float* scores, long long* pred, long long* counts, act_stream_t stream);

/* ---- Earth Mover's Distance between equal-sized clouds (csrc/emd.hip) ------------------------------------------------------------------
 * xyz1, xyz2 fp32 [B,N,3], 1 <= N <= act_emd_max_points(): the bijection a that minimises sum_i |xyz1[i] - xyz2[a(i)]|^2, by a forward
 * auction with eps-scaling (Bertsekas), one workgroup per pair for the whole solve, all state in LDS.  xyz1 are the bidders, xyz2 the objects;
 * cost d_ij = (dx*dx + dy*dy) + dz*dz in fp32, every product and sum rounded.  One round (Jacobi): every unassigned bidder takes its best and
 * second-best value -(d_ij + price_j) (ties: lower j) and bids price_j1 + (v1 - v2) + eps on j1 (N == 1: price + eps; never less than the next
 * float above the price); every object that got bids takes the highest (ties: lower bidder), raises its price to it and evicts its owner.
 * A phase ends when nobody is unassigned; the next one drops all assignments, keeps the prices and runs with eps / 4.  The ladder is
 * eps_final * 4^k, k descending from the smallest k with eps_final * 4^k >= max_ij d_ij / 4 (so every eps is eps_final times a power of two
 * and lattice inputs stay exact), and the solve ends after the phase at eps_final.  Then, in exact arithmetic,
 *     sum_i dist[i] <= optimum + N * eps_final;
 * in fp32 every comparison carries at most 3 ulp of the largest d_ij + price_j on top of eps_final.
 * The rounds of all phases together are capped by max_rounds (>= 1): when the cap is hit the bidders still unassigned get the objects still
 * free, both in ascending index order, so `assignment` is ALWAYS a bijection.  Bids are resolved by a 64-bit LDS atomic max whose result does
 * not depend on arrival order: all outputs are bit-identical run to run and a pair's result does not depend on its batch.
 * dist fp32 [B,N] = d_{i,a(i)}; assignment int32 [B,N] = a(i); info int32 [B] = rounds used, NEGATED when the cap was hit;
 * evals uint64 [B] (may be NULL) = bids made, i.e. the sum over rounds of the unassigned bidders (x N = distance evaluations).
 * eps_final must be positive and finite.  B == 0 is a no-op. */
int act_emd_max_points(void);
int act_emd_fwd_f32(const float* xyz1, const float* xyz2, int B, int N, float eps_final, int max_rounds, float* dist, int32_t* assignment,
                    int32_t* info, act_stream_t stream);
int act_emd_fwd_ex_f32(const float* xyz1, const float* xyz2, int B, int N, float eps_final, int max_rounds, float* dist, int32_t* assignment,
                       int32_t* info, uint64_t* evals, act_stream_t stream);
/* The same problem for MANY SMALL pairs (the Stage-I loss: B*G group patches of group_size points), 1 <= N <= act_emd_wave_max_points() = 64:
 * one wavefront per pair, object j and bidder i in lane j / i, the whole auction in registers (no LDS, no barrier, no atomic), four pairs per
 * workgroup.  Costs and values are rounded as above.  Gauss-Seidel instead of Jacobi: ONE bid at a time, by the lowest-index unassigned
 * bidder, on its best object (ties: lower j) at price + (v1 - v2) + eps (N == 1: price + eps; never less than the next float above the
 * price); the object's owner, if any, becomes unassigned.  The final eps is relative to the pair's scale:
 *     eps_used = max(eps_final, eps_rel * max_ij d_ij)      (eps_final > 0 and finite, eps_rel >= 0 and finite),
 * the ladder is eps_used * 4^k entered and descended as above, and sum_i dist[i] <= optimum + N * eps_used in exact arithmetic.
 * max_bids (>= 1) caps the bids of all phases together; at the cap the unassigned bidders get the free objects, both ascending, so
 * `assignment` is ALWAYS a bijection.  info int32 [B] = bids made, NEGATED when the cap was hit; eps_used fp32 [B] (may be NULL).
 * A pair's result depends only on its own inputs and the arguments.  B == 0 is a no-op.  The backward is act_emd_bwd_f32. */
int act_emd_wave_max_points(void);
int act_emd_wave_fwd_f32(const float* xyz1, const float* xyz2, int B, int N, float eps_final, float eps_rel, int max_bids, float* dist,
                         int32_t* assignment, int32_t* info, float* eps_used, act_stream_t stream);
/* gx1[i] = (2 * (xyz1[i] - xyz2[a(i)])) * grad_dist[i], gx2[a(i)] = -gx1[i] (fp32 [B,N,3] each, the operations in this order, no atomics).
 * Rows of gx2 that `assignment` does not name are zero; an entry outside [0,N) is skipped. */
int act_emd_bwd_f32(const float* xyz1, const float* xyz2, const int32_t* assignment, const float* grad_dist, int B, int N, float* gx1,
                    float* gx2, act_stream_t stream);

/* ---- PointNet++ set abstraction (csrc/sa.hip; reference models/pointnet2_utils.py:84-155, upstream pointnet2_ops ball_query / group_points) ----
 * Ball query: xyz [B,N,3], new_xyz [B,S,3] -> idx int32 [B,S,nsample]: for every query the lowest nsample point indices whose squared
 * distance passes the radius test, in ascending index order; the remaining slots repeat the first hit; a query with no hit gets a row of
 * zeros.  cnt int32 [B,S] (may be NULL) = min(hits, nsample).  The distance is the DIFFERENCE form (dx*dx + dy*dy) + dz*dz in fp32, every
 * product and sum rounded; the threshold is the fp32 product radius * radius.  inclusive == 0: d2 < radius^2 (upstream pointnet2_ops);
 * inclusive != 0: d2 <= radius^2 (the reference's torch form, which drops sqrdists > radius ** 2).  Any N >= 1, nsample >= 1; B <= 65535. */
int act_ball_query_f32(const float* xyz, const float* new_xyz, int B, int N, int S, float radius, int nsample, int inclusive, int32_t* idx,
                       int32_t* cnt, act_stream_t stream);
/* rows [B*S*nsample, (use_xyz ? 3 : 0) + D]: row (b,s,j) = xyz[b,i] - new_xyz[b,s] (if use_xyz) followed by feat[b,i,:] (feat [B,N,D]; NULL
 * when D == 0), i = idx[b,s,j]: sample_and_group's output in the row layout of the row GEMMs.  An index outside [0,N) gives a row of zeros. */
int act_group_rows_fwd_f32(const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx, int B, int N, int S, int nsample, int D,
                           int use_xyz, float* rows, act_stream_t stream);
/* dfeat [B,N,D] = for every point the sum of the feature columns of the rows that gathered it, in ascending (s, j) order over an inverse
 * adjacency built in the workspace (count, exclusive scan, fill; no atomics): bit-identical run to run.  The xyz columns carry no gradient. */
size_t act_group_rows_bwd_workspace(int B, int N, int S, int nsample);
int act_group_rows_bwd_f32(const float* drows, const int32_t* idx, int B, int N, int S, int nsample, int D, int use_xyz, float* dfeat,
                           void* workspace, size_t workspace_bytes, act_stream_t stream);
/* upstream's channel-first grouping: features [B,C,N], idx [B,S,nsample] -> out [B,C,S,nsample] (index outside [0,N): 0), and its backward
 * dfeatures [B,C,N] over the same adjacency (workspace: act_group_rows_bwd_workspace).  B, C <= 65535. */
int act_group_gather_f32(const float* features, const int32_t* idx, int B, int C, int N, int S, int nsample, float* out, act_stream_t stream);
int act_group_gather_bwd_f32(const float* dout, const int32_t* idx, int B, int C, int N, int S, int nsample, float* dfeatures, void* workspace,
                             size_t workspace_bytes, act_stream_t stream);

/* ---- three-NN feature propagation (csrc/sa.hip; reference models/pointnet2_utils.py:262-312, upstream three_nn / three_interpolate; the
 * PointNet++ networks and the Transformer segmentation head) ----
 * unknown [B,n,3], known [B,m,3], n >= 1, m >= 1, B <= 65535 -> idx int32 [B,n,3], weight fp32 [B,n,3], d2 fp32 [B,n,3] (may be NULL): the three
 * nearest known points in ascending (distance, index) order, equal distances to the lower index, and the weights r_k / ((r0 + r1) + r2),
 * r_k = 1 / (d2_k + 1e-8).  d2 is the DIFFERENCE form (dx*dx+dy*dy)+dz*dz in fp32 without FMA (the reference uses the expansion form).
 * Slots past m (m < 3) get idx 0, d2 +inf and weight exactly 0.  adj_off int32 [B,m+1] / adj_ent int32 [B,3n] (both or neither): per known point
 * g the entries e = 3 * unknown + slot that name it, ascending, at adj_ent[off[g] .. off[g+1]) -- the inverse adjacency of the interpolation
 * backward, a counting sort without atomics (one launch at m <= 256, the grouping backward's three-launch builder above that: same lists). */
int act_three_nn_f32(const float* unknown, const float* known, int B, int n, int m, int32_t* idx, float* weight, float* d2, int32_t* adj_off,
                     int32_t* adj_ent, act_stream_t stream);
/* the same adjacency of caller-supplied indices idx int32 [B,n,3]; an index outside [0,m) is in no list */
int act_three_adj_i32(const int32_t* idx, int B, int n, int m, int32_t* adj_off, int32_t* adj_ent, act_stream_t stream);
/* Y [B*N,C] = sum_k weight[.,k] * P[b*G + idx[.,k], :] over the slots with weight != 0 and idx in [0,G): a skipped slot is not read;
 * then + xyz[n] . wxyz[c,:] if wxyz (xyz [B*N,3], wxyz [C,3]) and + bias[c] if bias.  Any C >= 1 (float4 lanes when C % 4 == 0 and P, Y and bias
 * are 16-byte aligned).  B*N <= 2^27 rows (a one-dimensional grid of row blocks). */
int act_interp_rows_fwd_f32(const float* P, const int32_t* idx, const float* weight, const float* xyz, const float* wxyz, const float* bias,
                            int B, int N, int G, int C, float* Y, act_stream_t stream);
/* dP [B*G,C] = sum over the adjacency of known point g (increasing e) of weight[e] * dY[b*N + e/3, :], skipping entries of weight 0: a gather,
 * bit-identical run to run.  B*G <= 2^27 rows and row blocks (of 4) x channel blocks (of 64 lanes) <= 2^31 - 1. */
int act_interp_rows_bwd_f32(const float* dY, const int32_t* adj_off, const int32_t* adj_ent, const float* weight, int B, int N, int G, int C,
                            float* dP, act_stream_t stream);
/* dwxyz [C,3] = dY^T xyz, dbias [C] = column sums of dY (either may be NULL); dY [R,C], xyz [R,3]; per-block partials + one ordered pass. */
size_t act_interp_xyz_grad_workspace(long long R, int C);
int act_interp_xyz_grad_f32(const float* dY, const float* xyz, long long R, int C, float* dwxyz, float* dbias, float* workspace,
                            size_t workspace_bytes, act_stream_t stream);

/* ---- DGCNN classifier (csrc/edgeconv.hip; Wang et al. 2019) ----------------------------------------------------------------------------
 * Batched Euclidean kNN in feature space: x fp32 [B,N,C] -> idx int32 [B,N,k], d2 fp32 [B,N,k] (may be NULL): for every point of a cloud
 * the k points of the same cloud in ascending (d2, index) order, the point itself a candidate.  d2(i,j) = sum_c (x_ic - x_jc)^2 in the
 * difference form, channels ascending, every subtraction, product and sum rounded, no FMA: d2(i,i) == 0 and d2 is symmetric.  A NaN
 * distance orders after every other one (ties by index), so a row is always k distinct indices in [0,N).  No atomics; a cloud's result does
 * not depend on B.  N >= 1, 1 <= C <= 512, 1 <= k <= min(N, 64), B <= 65535, else ACT_E_BADARG. */
int act_knn_feat_f32(const float* x, int B, int N, int C, int k, int32_t* idx, float* d2, act_stream_t stream);
/* Fused EdgeConv tail with BatchNorm.  pq fp32 [B*N, ld] holds P at column 0 and Q at column qoff; idx int32 [B,N,k], any values (an
 * index outside [0,N) is clamped into range, duplicates allowed); C % 4 == 0, k <= 65535, B <= 65535.
 *   v[b,i,j,c] = P[b, idx[b,i,j], c] + Q[b,i,c]          (one rounded add, never stored)
 *   training != 0: mean_c and the biased var_c over the B*N*k values of v[..,c] (float64 moments around a value of v), and running_mean /
 *                  running_var (both or neither NULL) move by momentum, the variance unbiased; training == 0: the running statistics
 *   scale_c = gamma_c * rstd_c, shift_c = beta_c - mean_c * scale_c, out[b*N+i, ooff + c] = max_j LeakyReLU_slope(scale_c * v + shift_c),
 * evaluated on the largest v (scale_c >= 0) or the smallest (scale_c < 0), which is exact because the map is monotone, and in the centred form
 * scale_c * ((v - mean_c) - mean_lo_c) + beta_c so that a common offset of v does not cancel.  Also written: arg int32 [B*N,C] the selected j
 * (the lowest on ties), vsum [B*N,C] = sum_j v in ascending j, mean, mean_lo (the float64 mean minus its float32 rounding; 0 in eval mode)
 * and rstd [C].  Fixed order, no atomics. */
size_t act_edge_bn_workspace(int B, int N, int k, int C);
int act_edge_bn_lrelu_max_fwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C, const float* gamma,
                                  const float* beta, float* running_mean, float* running_var, int training, float momentum, float eps,
                                  float slope, float* out, int ldo, int ooff, int32_t* arg, float* vsum, float* mean, float* mean_lo,
                                  float* rstd, void* workspace, size_t workspace_bytes, act_stream_t stream);
/* its backward in train mode, from the forward's arg, vsum, mean, mean_lo and rstd and dout [B*N, ldd]: dpq [B*N, ld] receives dP at column 0 and dQ
 * at column qoff (qoff >= C; other columns are not written), dgamma and dbeta [C].  The BatchNorm backward of the materialised form,
 * gathered per point over the inverse adjacency of the clamped idx (built in the workspace: count, exclusive scan, fill) in ascending
 * (i, j): no atomics, bit-identical run to run. */
int act_edge_bn_lrelu_max_bwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C, const float* gamma,
                                  const float* beta, const float* mean, const float* mean_lo, const float* rstd, float slope,
                                  const int32_t* arg, const float* vsum, const float* dout, int ldd, float* dpq, float* dgamma,
                                  float* dbeta, void* workspace, size_t workspace_bytes, act_stream_t stream);
/* LeakyReLU forms of act_affine_act_f32 and act_bn_bwd_f32 on rows [R,C]: y = LeakyReLU_slope(x * scale + shift) (product and sum rounded),
 * and with g = dy * (z > 0 ? 1 : slope): dbeta = sum g, dgamma = sum g xhat (float64 sums in a fixed order), dx = scale * (g - dbeta / R -
 * xhat * dgamma / R). */
int act_affine_lrelu_f32(const float* x, const float* scale, const float* shift, float slope, int R, int C, float* y, act_stream_t stream);
size_t act_bn_lrelu_bwd_workspace(int R, int C);
int act_bn_lrelu_bwd_f32(const float* x, const float* dy, const float* scale, const float* shift, const float* mean, const float* rstd,
                         float slope, int R, int C, float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                         act_stream_t stream);

/* ---- DGCNN segmentation networks (csrc/edge_mlp2.hip) ------------------------------------------------------------------------------- */
/* Two-layer EdgeConv tail.  pq, idx as for act_edge_bn_lrelu_max_fwd_f32 (P [.., C1] at column 0, Q at column qoff), w2 fp32 [C2, C1].
 *   v = P[b, idx[b,i,j], :] + Q[b,i,:]    h = LeakyReLU(BN1(v))    y = w2 . h    out[b*N+i, :] = max_j LeakyReLU(BN2(y))
 * both BatchNorms over the M = B*N*k edges, with the statistics, running-statistics update and centred evaluation of the one-layer tail.  y is
 * formed tile by tile on the f32 matrix cores and never stored: per (point, channel) the largest and smallest y with their first j are kept, and
 * the one the sign of BN2's scale selects is evaluated.  Written: out [B*N, C2], arg int32 [B*N, C2] (the selected j), ysel [B*N, C2] (the
 * selected y), stats1 [3, C1] and stats2 [3, C2] (mean | mean_lo | rstd).  Fixed order, no atomics, a cloud's y does not depend on B.
 * 1 <= k <= 64, 4 <= C1, C2 <= 128 and multiples of 4, B <= 65535, slope >= 0, else ACT_E_BADARG with nothing written. */
size_t act_edge_mlp2_workspace(int B, int N, int k, int C1, int C2);
int act_edge_mlp2_fwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C1, int C2, const float* gamma1,
                          const float* beta1, float* running_mean1, float* running_var1, const float* w2, const float* gamma2,
                          const float* beta2, float* running_mean2, float* running_var2, int training, float momentum1, float eps1,
                          float momentum2, float eps2, float slope, float* out, int32_t* arg, float* ysel, float* stats1, float* stats2,
                          void* workspace, size_t workspace_bytes, act_stream_t stream);
/* its backward in train mode from the forward's arg, ysel, stats1, stats2 and dout [B*N, ldd]: dpq [B*N, ld] (dP at column 0, dQ at column
 * qoff >= C1; other columns are not written), dgamma1, dbeta1 [C1], dw2 [C2, C1], dgamma2, dbeta2 [C2].  h and y are recomputed per tile with
 * the forward's instruction sequence; one fp32 [B*N*k, C1] tensor (the gradient ahead of BN1) goes through the workspace.  No atomics,
 * bit-identical run to run. */
int act_edge_mlp2_bwd_f32(const float* pq, int ld, int qoff, const int32_t* idx, int B, int N, int k, int C1, int C2, const float* gamma1,
                          const float* beta1, const float* w2, const float* gamma2, const float* beta2, const float* stats1,
                          const float* stats2, float slope, const int32_t* arg, const float* ysel, const float* dout, int ldd, float* dpq,
                          float* dgamma1, float* dbeta1, float* dw2, float* dgamma2, float* dbeta2, void* workspace, size_t workspace_bytes,
                          act_stream_t stream);
/* y[b,n,:] = x[b,n,:] . T[b] for x [B,N,3], T [B,3,3] (products and sums rounded, i ascending), and its backward: dx = dy . T[b]^T,
 * dT[b] = sum_n x_n^T dy_n in float64, in a fixed order. */
int act_cloud_transform3_fwd_f32(const float* x, const float* T, int B, int N, float* y, act_stream_t stream);
int act_cloud_transform3_bwd_f32(const float* x, const float* T, const float* dy, int B, int N, float* dx, float* dT, act_stream_t stream);

/* ---- PointMLP (csrc/pointmlp.hip; Ma et al., ICLR 2022) --------------------------------------------------------------------------------- */
#define ACT_E_INDEX    (-4)            /* an index operand holds a value outside its range (only where an entry is asked to check) */
/* The geometric affine module of LocalGrouper, normalize="anchor".  feat fp32 [B,N,D], fps_idx int32 [B,S] (the anchors' rows), idx int32 [B,S,k]:
 *   e = feat[b, idx[b,i,j], c] - feat[b, fps_idx[b,i], c]     sigma_b = sqrt(sum (e - mean e)^2 / (n - 1)), n = S*k*D (over the whole cloud)
 *   r_b = 1 / (sigma_b + eps)                                 out[(b,i,j), c] = alpha[c] * (e * r_b) + beta[c]
 * every operation rounded once, no FMA; the moments of e in float64 around a value of e, in a fixed order, so that a common offset of the
 * features does not reach sigma and a cloud's result does not depend on B.  out is [B*S*k, D], or with cat != 0 [B*S*k, 2D] with the anchor's row in
 * the columns [D, 2D).  Also written: sigma [B] and mean [B] (the mean of e), which the backward takes.  validate != 0: idx and fps_idx are
 * range-checked on the device first (one host synchronisation) and ACT_E_INDEX is returned with nothing written if a value lies outside [0,N);
 * validate == 0: such a value is clamped into range.  Any D >= 1 (float4 lanes when D % 4 == 0 and the operands are 16-byte aligned),
 * 1 <= k <= N, S*k*D >= 2, B <= 65535, else ACT_E_BADARG with nothing written.  No atomics. */
size_t act_geo_affine_fwd_workspace(int B, int N, int S, int k, int D);
int act_geo_affine_group_fwd_f32(const float* feat, const int32_t* fps_idx, const int32_t* idx, const float* alpha, const float* beta, float eps,
                                 int B, int N, int S, int k, int D, int cat, int validate, float* out, float* sigma, float* mean,
                                 void* workspace, size_t workspace_bytes, act_stream_t stream);
/* its backward from the forward's sigma and mean and dout [B*S*k, D or 2D]: dfeat [B,N,D], dalpha [D], dbeta [D].
 *   dalpha = sum g e r, dbeta = sum g, dsigma_b = -r^2 sum g alpha e, de = alpha g r + dsigma_b (e - mean) / ((n - 1) sigma_b)
 * (the second term is 0 where sigma_b == 0), g the cotangent of the normalised columns.  Every point gathers de over the inverse adjacency of idx
 * (built in the workspace: count, exclusive scan, fill) in ascending (i, j); an anchor adds the cotangent of its k copies minus the sum of its own
 * k rows of de.  The column sums are float64 in two fixed-order stages.  No [B*S*k, D] tensor, no atomics, bit-identical run to run.  Indices are
 * clamped into [0,N). */
size_t act_geo_affine_bwd_workspace(int B, int N, int S, int k, int D);
int act_geo_affine_group_bwd_f32(const float* feat, const int32_t* fps_idx, const int32_t* idx, const float* alpha, const float* sigma,
                                 const float* mean, float eps, const float* dout, int B, int N, int S, int k, int D, int cat, float* dfeat,
                                 float* dalpha, float* dbeta, void* workspace, size_t workspace_bytes, act_stream_t stream);
/* The residual block tail on rows [R,C], any C: out = max((y * scale + shift) + res, 0), product and sums rounded; and its train-mode backward
 * with the mask taken from the saved output: g = dout where out > 0, dres = g, dbeta = sum g, dgamma = sum g xhat (float64 column sums in a fixed
 * order), dy = gamma rstd (g - dbeta / R - xhat * dgamma / R).  dy and dres are written in one pass.  The backward takes the forward's mean [C] as a
 * pivot only: it forms the moments of y around it again in float64, in the pass of the column sums, and takes xhat and rstd from those. */
int act_affine_add_relu_f32(const float* y, const float* res, const float* scale, const float* shift, int R, int C, float* out,
                            act_stream_t stream);
size_t act_bn_add_relu_bwd_workspace(int R, int C);
int act_bn_add_relu_bwd_f32(const float* y, const float* out, const float* dout, const float* gamma, const float* mean, float eps, int R, int C,
                            float* dy, float* dres, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, act_stream_t stream);

/* ---- PCT offset attention (csrc/offset_attn.hip; Guo et al., CVM 2021) ------------------------------------------------------------------------ */
/* Per cloud, rows q [N,Dq], k [N,Dq], v [N,C] and, optionally, x [N,C] (all fp32, clouds stacked: [B*N, .]):
 *   E[i,j] = q_i . k_j (no scale)     P[i,j] = exp(E[i,j] - lse_i), lse_i = max_j E[i,j] + log sum_j exp(E[i,j] - max)     (softmax over the keys)
 *   c_j = sum_i P[i,j]                s_j = 1 / (1e-9f + c_j)                                                               (L1 over the queries)
 *   x_r[j] = s_j sum_i P[i,j] v_i     out[j] = x_r[j], or x[j] - x_r[j] when x != NULL
 * Written: out [B*N,C], lse [B*N], colsum [B*N] (c_j) and, when xr != NULL, x_r [B*N,C].  Both products run on v_mfma_f32_16x16x4_f32; no [N,N]
 * tensor reaches memory.  Fixed summation order, no atomics: a cloud's result does not depend on B and is bit-identical run to run.
 * 1 <= N <= 1024 (any N), 4 <= Dq <= 64 and Dq % 4 == 0, 4 <= C <= 256 and C % 4 == 0, 1 <= B <= 65535, else ACT_E_BADARG with nothing written.
 * The workspace (16-byte aligned) is shared by both directions. */
size_t act_offset_attn_workspace(int B, int N, int Dq, int C);
int act_offset_attn_fwd_f32(const float* q, const float* k, const float* v, const float* x, int B, int N, int Dq, int C, float* out, float* lse,
                            float* colsum, float* xr, void* workspace, size_t workspace_bytes, act_stream_t stream);
/* its backward from colsum and x_r; the row statistics behind lse are formed again (one Dq-deep sweep), because lse rounded to fp32 is a common
 * factor of up to 1 +- 4e-8 |lse| on a whole row of P.  g_j is the cotangent of x_r[j]: dout_j, or -dout_j with negate != 0 (the fused x, whose own gradient is
 * dout).  D_j = g_j . x_r[j], dP[i,j] = s_j (v_i . g_j - D_j), R_i = sum_j P dP, dE = P (dP - R_i); dq_i = sum_j dE k_j, dk_j = sum_i dE q_i,
 * dv_i = sum_j P[i,j] s_j g_j.  dq and dk are written separately (dq == dk is ACT_E_BADARG); q and k may be one tensor.  P and dP are recomputed
 * tile by tile in three sweeps (R and dv; dq; dk), all products on the matrix cores. */
int act_offset_attn_bwd_f32(const float* q, const float* k, const float* v, const float* colsum, const float* xr, const float* dout, int negate,
                            int B, int N, int Dq, int C, float* dq, float* dk, float* dv, void* workspace, size_t workspace_bytes,
                            act_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ACT_HIP_H */
