"""The C ABI of libact_hip.so as ctypes sees it: the one mirror of include/act_hip.h.

Every struct and every function of the header is declared HERE and nowhere else; _C applies SIGNATURES to the library once, when it is
loaded.  A new entry point gets one line in the table below (and a Structure above it if it takes a new struct);
tests/test_cabi.py parses the header and checks every return type, every parameter and every struct field against this file.

Pure ctypes: importing this module needs neither the library nor a GPU.
"""
import ctypes

_vp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_u, _u64, _ll, _str = ctypes.c_uint, ctypes.c_uint64, ctypes.c_longlong, ctypes.c_char_p
_d = ctypes.c_double
_P = ctypes.POINTER


# ---- structs (field order and types as in the header) -----------------------------------------------------------------------
class GemmEpilogue(ctypes.Structure):                  # act_gemm_epilogue_t
    _fields_ = [("alpha", _f), ("act", _i), ("accumulate", _i), ("rows_per_scale", _i), ("ldr", _i), ("ldaux", _i),
                ("res_row_div", _i), ("bias", _vp), ("rowscale", _vp), ("res", _vp), ("aux", _vp)]


class GemmTnProblem(ctypes.Structure):                 # act_gemm_tn_problem_t
    _fields_ = [("A", _vp), ("lda", _i), ("B", _vp), ("ldb", _i), ("C", _vp), ("ldc", _i), ("M", _i), ("N", _i), ("bias_out", _vp)]


class GemmFx(ctypes.Structure):                        # act_gemm_fx_t
    _fields_ = ([(n, _vp) for n in ("a_scale", "a_shift", "b_scale", "b_shift", "tile_stats", "gmax", "garg")] + [("group", _i), ("store_c", _i)]
                + [(n, _vp) for n in ("sa_src", "sa_arg", "ep_src", "ep_arg", "row_groups")])


class BlockParams(ctypes.Structure):                   # act_block_params_t, act_block_grads_t
    _fields_ = [(n, _vp) for n in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b",
                                   "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class BlockDims(ctypes.Structure):                     # act_block_dims_t
    _fields_ = [("B", _i), ("S", _i), ("D", _i), ("heads", _i), ("hidden", _i), ("eps", _f)]


class BlockStack(ctypes.Structure):                    # act_block_stack_t
    _fields_ = [("depth", _i), ("blocks", _vp), ("gate1", _vp), ("gate2", _vp)]


class PrefixVit(ctypes.Structure):                     # act_prefix_vit_t
    _fields_ = ([(n, _i) for n in ("B", "P", "G", "D", "heads", "hidden", "depth", "tokens_dims", "pos_hidden")] +
                [("eps", _f), ("drop_p", _f), ("seed_base", _u64), ("seed_dev", _vp)] +
                [(n, _vp) for n in ("pos_w0", "pos_b0", "pos_w1", "pos_b1", "pre_w", "pre_b", "post_w", "post_b", "norm_w", "norm_b")] +
                [("prompt_tok", _P(_vp)), ("prompt_pos", _P(_vp)), ("blocks", _P(BlockParams))])


class VitBf16x3(ctypes.Structure):                     # act_vit_bf16x3_t
    _fields_ = [("w_planes", _vp), ("a_planes", _vp), ("a_planes_elems", _sz)]


class VitF16x3(ctypes.Structure):                      # act_vit_f16x3_t
    _fields_ = [("w_planes", _vp), ("w_inv_scale", _vp), ("a_scale", _vp), ("a_planes", _vp), ("a_planes_elems", _sz), ("w_layout", _i)]


class PointnetParams(ctypes.Structure):                # act_pointnet_params_t
    _fields_ = [(n, _vp) for n in ("c1_w", "c1_b", "bn1_w", "bn1_b", "c2_w", "c2_b", "c3_w", "c3_b", "bn2_w", "bn2_b", "c4_w", "c4_b",
                                   "bn1_mean", "bn1_var", "bn2_mean", "bn2_var")]


class PointnetGrads(ctypes.Structure):                 # act_pointnet_grads_t
    _fields_ = [(n, _vp) for n in ("c1_w", "c1_b", "bn1_w", "bn1_b", "c2_w", "c2_b", "c3_w", "c3_b", "bn2_w", "bn2_b", "c4_w", "c4_b")]


class PointnetDims(ctypes.Structure):                  # act_pointnet_dims_t
    _fields_ = [("BG", _i), ("n", _i), ("C", _i), ("eps1", _f), ("eps2", _f), ("momentum1", _f), ("momentum2", _f)]


class Dgcnn(ctypes.Structure):                         # act_dgcnn_t
    _fields_ = ([(n, _i) for n in ("B", "G", "k", "Cin", "Cout", "groups")] + [("eps", _f), ("slope", _f)] +
                [(n, _vp) for n in ("w_in", "b_in", "w5")] + [("stacked", _vp * 4), ("gn_w", _vp * 4), ("gn_b", _vp * 4)])


class DgcnnF16x3(ctypes.Structure):                    # act_dgcnn_f16x3_t
    _fields_ = [("w5_planes", _vp), ("w5_inv_scale", _vp), ("a_scale", _f), ("a_planes", _vp), ("a_planes_elems", _sz), ("layers", _i),
                ("st_planes", _vp * 3), ("st_inv_scale", _vp * 3), ("w_layout", _i)]


class PointnetF16x3(ctypes.Structure):                 # act_pointnet_f16x3_t
    _fields_ = [("c4_planes", _vp), ("c4_inv_scale", _vp), ("a_scale", _f), ("w_layout", _i)]


class AugmentOp(ctypes.Structure):                     # act_augment_op_t
    _fields_ = [("kind", _i), ("p0", _f), ("p1", _f), ("p2", _f), ("draws", _vp), ("draws2", _vp)]


# header typedef -> its mirror (act_block_grads_t has the fields of act_block_params_t and shares its class)
STRUCTS = {
    "act_gemm_epilogue_t": GemmEpilogue, "act_gemm_tn_problem_t": GemmTnProblem, "act_gemm_fx_t": GemmFx,
    "act_block_params_t": BlockParams, "act_block_grads_t": BlockParams, "act_block_dims_t": BlockDims, "act_block_stack_t": BlockStack,
    "act_prefix_vit_t": PrefixVit, "act_vit_bf16x3_t": VitBf16x3, "act_vit_f16x3_t": VitF16x3,
    "act_pointnet_params_t": PointnetParams,
    "act_pointnet_grads_t": PointnetGrads, "act_pointnet_dims_t": PointnetDims, "act_dgcnn_t": Dgcnn, "act_dgcnn_f16x3_t": DgcnnF16x3,
    "act_pointnet_f16x3_t": PointnetF16x3,
    "act_augment_op_t": AugmentOp,
}

_epi, _probs, _fx = _P(GemmEpilogue), _P(GemmTnProblem), _P(GemmFx)
_dims, _blk, _x3 = _P(BlockDims), _P(BlockParams), _P(VitBf16x3)
_pnd, _pnp = _P(PointnetDims), _P(PointnetParams)

# ---- functions, in header order.  name -> argtypes for a function that returns int, name -> (restype, argtypes) for the others ----------
_TABLE = {
    # library
    "act_version": [],
    "act_arch": (_str, []),
    # live per-kernel timing
    "act_prof_enable": [_i],
    "act_prof_reset": [],
    "act_prof_num_kernels": [],
    "act_prof_kernel_name": (_str, [_i]),
    "act_prof_read": [_i, _vp, _vp, _vp, _vp],
    # point operators (csrc/point_ops.hip)
    "act_fps_scratch_floats": (_sz, [_i, _i]),
    "act_fps_f32": [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp],
    "act_fps_chain_probe": [_i, _i, _vp, _vp, _vp, _vp],
    "act_knn_group_f32": [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp],
    "act_gather_points_f32": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "act_gather_points_bwd_f32": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "act_scale_translate_f32": [_vp, _vp, _vp, _i, _i, _vp],
    "act_rotate_points_f32": [_vp, _vp, _i, _i, _vp],
    # fused augmentation chain (csrc/augment.hip)
    "act_augment_f32": [_vp, _i, _i, _P(AugmentOp), _i, _u64, _vp, _i, _vp],
    # Chamfer distance (csrc/chamfer.hip)
    "act_chamfer_fwd_f32": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "act_chamfer_fwd_ex_f32": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp],
    "act_chamfer_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp],
    # dense fp32 GEMM with fused epilogue
    "act_sgemm_f32": [_i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _epi, _vp, _sz, _vp],
    "act_sgemm_ex_f32": [_i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _epi, _vp, _sz, _i, _i, _vp],
    "act_sgemm_tn_grouped_workspace": (_sz, [_probs, _i, _i, _i]),
    "act_sgemm_tn_grouped_splits": [_probs, _i, _i],
    "act_sgemm_tn_grouped_f32": [_probs, _i, _i, _i, _vp, _sz, _vp],
    "act_sgemm_fx_tile_stats_floats": (_sz, [_i, _i]),
    "act_gemm_fx_asm": [_i],
    "act_sgemm_fx_f32": [_i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _epi, _fx, _vp, _sz, _vp],
    "act_bn_tiles_finalize_f32": [_vp, _i, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # row-wise fused kernels of a Transformer block
    "act_layernorm_fwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp],
    "act_prompt_layernorm_fwd_f32": [_vp, _vp, _i, _i, _i, _f, _u64, _vp, _vp, _vp, _f, _vp, _vp],
    "act_prompt_rows_fwd_f32": [_vp, _vp, _vp, _i, _i, _i, _f, _u64, _vp, _vp],
    "act_prompt_rows_bwd_f32": [_vp, _vp, _i, _i, _i, _f, _u64, _vp, _vp, _vp],
    "act_layernorm_bwd_workspace": (_sz, [_i, _i]),
    "act_layernorm_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _i, _i, _vp],
    "act_colsum_workspace": (_sz, [_i, _i]),
    "act_colsum_f32": [_vp, _i, _i, _i, _vp, _i, _vp, _sz, _vp],
    "act_attention_fwd_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp],
    "act_attention_fwd_prefix_f32": [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _f, _vp],
    "act_attention_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp],
    "act_attention_bwd_prefix_f32": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp],
    # losses
    "act_cosine_loss_fwd_f32": [_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp],
    "act_cosine_loss_bwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp],
    "act_regression_loss_fwd_f32": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp],
    "act_regression_loss_bwd_f32": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "act_softmax_xent_fwd_f32": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp],
    "act_softmax_xent_bwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
    # mini-PointNet / FoldingNet row kernels (csrc/pointnet.hip)
    "act_colstats_workspace": (_sz, [_i, _i]),
    "act_bn_stats_f32": [_vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_affine_act_f32": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "act_bn_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_bn_bwd_groups_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_col_mean_var_f32": [_vp, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_bn_bwd_sums_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_bn_bwd_apply_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _vp, _vp],
    "act_group_max_f32": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "act_group_max_bwd_f32": [_vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "act_group_max_bwd_matmul_f32": [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp],
    "act_group_live_i32": [_vp, _i, _i, _vp, _vp],
    "act_group_max_bwd_matmul_live_f32": [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp],
    "act_group_max_bwd_wgrad_workspace": (_sz, [_i, _i, _i, _i]),
    "act_group_max_bwd_wgrad_f32": [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp],
    "act_group_sum_f32": [_vp, _i, _i, _i, _vp, _vp],
    # DGCNN token mixer + dVAE tokenizer glue (csrc/dgcnn.hip)
    "act_edge_gn_lrelu_max_f32": [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _i, _i, _vp],
    "act_edge_gn_lrelu_max_bwd_f32": [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _vp, _i, _vp, _vp, _vp, _vp],
    "act_edge_bwd_lds": [_i],
    "act_gn_gumbel_argmax_gather_f32": [_vp, _i, _i, _i, _i, _vp, _vp, _f, _f, _vp, _u64, _vp, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp],
    "act_gumbel_softmax_fwd_f32": [_vp, _i, _i, _vp, _u64, _f, _vp, _vp],
    "act_gumbel_softmax_bwd_f32": [_vp, _vp, _i, _i, _f, _vp, _vp],
    "act_kl_uniform_fwd_f32": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp],
    "act_kl_uniform_bwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    # opt-in split-bf16 products of the frozen teacher (csrc/gemm_bf16x3.hip)
    "act_split_bf16x2_f32": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "act_sgemm_nt_bf16x3_supported": [_i, _i, _i],
    "act_sgemm_nt_bf16x3_f32": [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _epi, _vp],
    "act_layernorm_fwd_planes_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp],
    "act_prompt_layernorm_fwd_planes_f32": [_vp, _vp, _i, _i, _i, _f, _u64, _vp, _vp, _vp, _f, _vp, _vp, _vp],
    "act_attention_fwd_prefix_planes_f32": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp],
    "act_sgemm_nt_bf16x3_planes_f32": [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _epi, _vp],
    # default split-f16 products of the frozen teacher (same file, F16 form)
    "act_split_f16x2_f32": [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp],
    "act_split_f16x2_ld_f32": [_vp, _i, _i, _i, _f, _vp, _vp, _i, _vp],
    "act_sgemm_nt_f16x3_supported": [_i, _i, _i],
    "act_sgemm_nt_f16x3_planes_f32": [_i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _epi, _vp],
    "act_sgemm_nt_f16x3_pick_tile": [_i, _i, _i, _i],
    "act_sgemm_nt_f16x3_planes_tile_f32": [_i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _epi, _vp, _i],
    "act_sgemm_nt_f16x3_planes_lda_f32": [_i, _i, _i, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _epi, _vp, _i],
    # K-tile-major planes
    "act_repack_ktile_u16": [_vp, _vp, _i, _i, _vp],
    "act_split_f16x2_kt_f32": [_vp, _i, _i, _i, _f, _vp, _vp, _i, _vp],
    "act_sgemm_nt_f16x3_planes_layout_f32": [_i, _i, _i, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _f, _i, _epi, _vp, _i],
    "act_x3_kt": [_i],
    "act_layernorm_fwd_f16_planes_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _f, _vp],
    "act_attention_fwd_prefix_f16_planes_f32": [_vp, _i, _vp, _i, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _f, _vp],
    "act_prompt_layernorm_fwd_f16_planes_f32": [_vp, _vp, _i, _i, _i, _f, _u64, _vp, _vp, _vp, _f, _vp, _vp, _f, _vp],
    "act_split_f16x2_affine_relu_f32": [_vp, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp],
    "act_sgemm_nt_f16x3_gmax_supported": [_i, _i, _i, _i],
    "act_sgemm_nt_f16x3_gmax_pick_tile": [_i, _i, _i, _i],
    "act_sgemm_nt_f16x3_gmax_f32": [_i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp],
    "act_sgemm_nt_f16x3_gmax_layout_f32": [_i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _vp],
    # GEMM launch-configuration table
    "act_gemm_tune_set": [_i] * 7,
    "act_gemm_tune_get": [_i] * 5 + [_P(_i), _P(_i)],
    "act_gemm_tune_clear": [],
    "act_gemm_tile_info": [_i] + [_P(_i)] * 4,
    "act_scale_rows_f32": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "act_bn_eval_affine_f32": [_vp, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp],
    # composite entry points (csrc/composite.hip)
    "act_composite_collect_begin": [],
    "act_composite_collect_end": [_P(_i), _i],
    "act_composite_shutdown": [],
    "act_block_saved_floats": (_sz, [_dims]),
    "act_block_fwd_f32": [_dims, _blk, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp],
    "act_block_bwd_scratch_floats": (_sz, [_dims]),
    "act_block_bwd_f32": [_dims, _blk, _vp, _vp, _vp, _vp, _vp, _blk, _vp, _vp, _sz, _vp, _sz, _vp, _vp],
    "act_block_stack_saved_floats": (_sz, [_dims, _i, _i]),
    "act_block_stack_bwd_scratch_floats": (_sz, [_dims, _i]),
    "act_block_stack_fwd_f32": [_dims, _P(BlockStack), _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp],
    "act_block_stack_bwd_f32": [_dims, _P(BlockStack), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp],
    "act_add_f32": [_vp, _vp, _vp, _ll, _vp],
    "act_prefix_block_saved_floats": (_sz, [_dims, _i]),
    "act_prefix_block_fwd_f32": [_dims, _i, _blk, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp],
    "act_prefix_block_fwd_kv_f32": [_dims, _i, _blk, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_prompt_kv_sparse": [_i],
    "act_prompt_kv_workspace": (_sz, [_i, _i, _i, _i]),
    "act_prompt_kv_fwd_f32": [_vp, _vp, _i, _i, _i, _i, _f, _u64, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp],
    "act_prompt_kv_f16x3": [_i],
    "act_prompt_kv_fwd_f16x3_f32": [_vp, _vp, _i, _i, _i, _i, _f, _u64, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, _sz, _i, _vp],
    "act_prompt_kv_fwd_f16x3_layout_f32": [_vp, _vp, _i, _i, _i, _i, _f, _u64, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _vp, _f, _vp, _vp, _vp, _sz, _i, _vp],
    "act_prefix_block_bwd_scratch_floats": (_sz, [_dims, _i]),
    "act_prefix_block_bwd_f32": [_dims, _i, _blk, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_prefix_vit_scratch_floats": (_sz, [_P(PrefixVit)]),
    "act_prefix_vit_fwd_bf16x3_f32": [_P(PrefixVit), _x3, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_prefix_block_fwd_bf16x3_f32": [_dims, _i, _blk, _x3, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp],
    "act_prefix_block_bwd_bf16x3_f32": [_dims, _i, _blk, _x3, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_prefix_vit_fwd_f32": [_P(PrefixVit), _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_prefix_vit_fwd_f16x3_f32": [_P(PrefixVit), _P(VitF16x3), _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_pointnet_saved_floats": (_sz, [_pnd]),
    "act_pointnet_fwd_f32": [_pnd, _pnp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_pointnet_fwd_groups_f32": [_pnd, _pnp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp],
    "act_pointnet_fwd_groups_f16x3_f32": [_pnd, _pnp, _P(PointnetF16x3), _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp],
    "act_pointnet_bwd_scratch_floats": (_sz, [_pnd]),
    "act_pointnet_bwd_f32": [_pnd, _pnp, _vp, _vp, _vp, _P(PointnetGrads), _vp, _vp, _sz, _vp],
    "act_dgcnn_scratch_floats": (_sz, [_P(Dgcnn)]),
    "act_dgcnn_features_f32": [_P(Dgcnn), _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_dgcnn_features_f16x3_f32": [_P(Dgcnn), _P(DgcnnF16x3), _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    # dense per-point prediction (csrc/seg.hip)
    "act_log_softmax_fwd_f32": [_vp, _ll, _i, _vp, _vp],
    "act_log_softmax_bwd_f32": [_vp, _vp, _ll, _i, _vp, _vp],
    "act_nll_weighted_workspace": (_sz, [_ll]),
    "act_nll_weighted_fwd_f32": [_vp, _vp, _vp, _ll, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_nll_weighted_bwd_f32": [_vp, _vp, _vp, _vp, _ll, _i, _vp, _vp],
    "act_confusion_i64": [_vp, _vp, _ll, _i, _vp, _vp],
    # part segmentation (csrc/partseg.hip)
    "act_label_branch_fwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp],
    "act_label_branch_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _vp],
    "act_part_eval_f32": [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp],
    # whole-room sliding-window testing (csrc/wholescene.hip)
    "act_scene_member_workspace": (_sz, [_ll, _i, _i]),
    "act_scene_member_count": [_vp, _ll, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_scene_member_fill": [_vp, _ll, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_scene_rows": [_vp, _vp, _vp, _vp, _i, _ll, _i, _u, _u, _u, _vp, _vp],
    "act_scene_gather": [_vp, _ll, _vp, _vp, _vp, _vp, _i, _ll, _vp, _vp],
    "act_scene_vote": [_vp, _vp, _ll, _ll, _i, _vp, _vp, _vp, _vp],
    "act_scene_finish": [_vp, _vp, _ll, _i, _vp, _vp, _vp],
    # S3DIS training blocks from resident rooms (csrc/s3dis_sample.hip)
    "act_s3dis_sample_workspace": (_sz, [_i, _ll]),
    "act_s3dis_sample_f32": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _d, _d, _i, _i, _ll, _vp, _vp, _vp, _i, _i, _u, _u, _vp, _vp, _vp, _vp, _vp, _vp,
                             _vp, _sz, _vp],
    # object-dataset batches from a resident split (csrc/cloud_sample.hip)
    "act_cloud_sample_max_points": [],
    "act_cloud_sample_f32": [_vp, _ll, _i, _i, _vp, _vp, _i, _i, _u, _u, _i, _vp, _vp, _vp],
    # Stage-I reconstruction evaluation (csrc/recon_eval.hip)
    "act_recon_eval_f32": [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _i, _vp],
    # linear-SVM validation of pretrained features (csrc/svm.hip)
    "act_svm_scores_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "act_svm_hinge_workspace": (_sz, [_i, _i]),
    "act_svm_hinge_f32": [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_svm_tprod_workspace": (_sz, [_i, _i, _i]),
    "act_svm_tprod_f32": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_svm_newton_workspace": (_sz, [_i, _i, _i]),
    "act_svm_newton_f32": [_vp, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    # exact t-SNE of classifier features (csrc/tsne.hip)
    "act_tsne_knn_workspace": (_sz, [_i, _i]),
    "act_tsne_knn_cosine_f32": [_vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_tsne_conditional_p_f32": [_vp, _i, _i, _f, _vp, _vp, _vp],
    "act_tsne_symmetrize_workspace": (_sz, [_i, _i]),
    "act_tsne_symmetrize_f32": [_vp, _vp, _i, _i, _vp, _vp, _vp, _ll, _vp, _sz, _vp],
    "act_tsne_step_workspace": (_sz, [_i]),
    "act_tsne_step_f32": [_vp, _vp, _vp, _i, _f, _f, _f, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_tsne_steps_f32": [_vp, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_tsne_kl_f32": [_vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp],
    "act_tsne_pca_workspace": (_sz, [_i, _i]),
    "act_tsne_pca_init_f32": [_vp, _i, _i, _vp, _vp, _vp, _sz, _vp],
    # frozen post-LayerNorm language teacher (csrc/bert.hip)
    "act_dropout_add_layernorm_fwd_f32": [_vp, _vp, _vp, _i, _i, _f, _u64, _vp, _vp, _vp, _f, _vp, _vp, _vp],
    "act_dropout_add_layernorm_bwd_f32": [_vp, _vp, _vp, _i, _i, _f, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "act_attention_dropout_fwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _u64, _vp, _vp],
    "act_attention_dropout_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _u64, _vp, _vp],
    # CLIP image teacher (csrc/clip.hip)
    "act_quickgelu_fwd_f32": [_vp, _vp, _i, _i, _vp],
    "act_quickgelu_bwd_f32": [_vp, _vp, _vp, _i, _i, _vp],
    # weighted k-NN validation of frozen features (csrc/knn_probe.hip)
    "act_knn_probe_normalize_f32": [_vp, _i, _i, _vp, _vp],
    "act_knn_probe_splits": [_i, _i, _i, _i],
    "act_knn_probe_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "act_knn_probe_search_f32": [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp],
    "act_knn_probe_vote_f32": [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _P(_i), _i, _f, _vp, _vp, _vp, _vp],
    # Earth Mover's Distance (csrc/emd.hip)
    "act_emd_max_points": [],
    "act_emd_fwd_f32": [_vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp],
    "act_emd_fwd_ex_f32": [_vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp],
    "act_emd_bwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp],
    "act_emd_wave_max_points": [],
    "act_emd_wave_fwd_f32": [_vp, _vp, _i, _i, _f, _f, _i, _vp, _vp, _vp, _vp, _vp],
    # PointNet++ set abstraction (csrc/sa.hip)
    "act_ball_query_f32": [_vp, _vp, _i, _i, _i, _f, _i, _i, _vp, _vp, _vp],
    "act_group_rows_fwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "act_group_rows_bwd_workspace": (_sz, [_i, _i, _i, _i]),
    "act_group_rows_bwd_f32": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp],
    "act_group_gather_f32": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "act_group_gather_bwd_f32": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp],
    # three-NN feature propagation (csrc/sa.hip)
    "act_three_nn_f32": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "act_three_adj_i32": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "act_interp_rows_fwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "act_interp_rows_bwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "act_interp_xyz_grad_workspace": (_sz, [_ll, _i]),
    "act_interp_xyz_grad_f32": [_vp, _vp, _ll, _i, _vp, _vp, _vp, _sz, _vp],
    # DGCNN classifier: feature-space kNN, EdgeConv tail with BatchNorm, LeakyReLU row BatchNorm (csrc/edgeconv.hip)
    "act_knn_feat_f32": [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "act_edge_bn_workspace": (_sz, [_i, _i, _i, _i]),
    "act_edge_bn_lrelu_max_fwd_f32": [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _sz, _vp],
    "act_edge_bn_lrelu_max_bwd_f32": [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    # DGCNN segmentation networks: two-layer EdgeConv tail, 3x3 transform of a cloud (csrc/edge_mlp2.hip)
    "act_edge_mlp2_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "act_edge_mlp2_fwd_f32": [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _f, _f, _vp, _vp,
                              _vp, _vp, _vp, _vp, _sz, _vp],
    "act_edge_mlp2_bwd_f32": [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp, _sz, _vp],
    "act_cloud_transform3_fwd_f32": [_vp, _vp, _i, _i, _vp, _vp],
    "act_cloud_transform3_bwd_f32": [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp],
    "act_affine_lrelu_f32": [_vp, _vp, _vp, _f, _i, _i, _vp, _vp],
    "act_bn_lrelu_bwd_workspace": (_sz, [_i, _i]),
    "act_bn_lrelu_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    # PointMLP: geometric affine grouping, residual BatchNorm tail (csrc/pointmlp.hip)
    "act_geo_affine_fwd_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "act_geo_affine_group_fwd_f32": [_vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_geo_affine_bwd_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "act_geo_affine_group_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_affine_add_relu_f32": [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
    "act_bn_add_relu_bwd_workspace": (_sz, [_i, _i]),
    "act_bn_add_relu_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    # PCT: offset attention (csrc/offset_attn.hip)
    "act_offset_attn_workspace": (_sz, [_i, _i, _i, _i]),
    "act_offset_attn_fwd_f32": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "act_offset_attn_bwd_f32": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp],
}

# name -> (restype, argtypes) for every function of the header
SIGNATURES = {name: sig if isinstance(sig, tuple) else (_i, sig) for name, sig in _TABLE.items()}
