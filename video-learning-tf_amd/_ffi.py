"""ctypes binding of libvltf_hip.so (include/vltf.h).  There is no CPU fallback: if the library is
missing or a call fails this module raises, loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VLTF_HIP_LIB") or os.path.join(_HERE, "libvltf_hip.so")   # override: kernel experiments only

p = C.c_void_p
i32, i64, f32, u32, u64, sz = C.c_int, C.c_int64, C.c_float, C.c_uint32, C.c_uint64, C.c_size_t

# name -> (restype, argtypes); mirrors include/vltf.h one to one
SIGNATURES = {
    "vl_last_error": (C.c_char_p, []),
    "vl_version": (i32, []),
    "vl_device_count": (i32, []),
    "vl_input_prep_u8": (i32, [p, p, i32, i32, i32, i32, i32, p, p, p, p, i32, i32, p]),
    "vl_input_prep_u8_box": (i32, [p, p, i32, i32, i32, i32, i32, p, p, p, i32, i32, p]),
    "vl_nhwc_to_nchw": (i32, [p, p, i32, i32, i32, i32, i32, i32, p]),
    "vl_nchw_to_nhwc": (i32, [p, p, i32, i32, i32, i32, p]),
    "vl_conv_create": (i32, [C.POINTER(p), i32, i32, i32, i32, i32, i32, i32, i32]),
    "vl_conv_destroy": (None, [p]),
    "vl_conv_out_hw": (i32, [p, C.POINTER(i32), C.POINTER(i32)]),
    "vl_conv_set_halo": (i32, [p, i32, i32, i32, i32]),
    "vl_conv_set_x_phase_split": (i32, [p, i32]),
    "vl_conv_x_phase": (i32, [p]),
    "vl_set_conv_math": (i32, [i32]),
    "vl_conv_math": (i32, []),
    "vl_conv_set_row_classes": (i32, [i32]),
    "vl_conv_set_stage_depth": (i32, [i32]),
    "vl_conv_last_launch": (i32, []),
    "vl_gemm_split_ws_bytes": (C.c_size_t, [i32, i32, i32]),
    "vl_conv_fwd": (i32, [p, p, p, p, p, i32, i32, p]),
    "vl_conv_wt_transpose": (i32, [p, p, p, p]),
    "vl_conv_dgrad": (i32, [p, p, p, p, p, i32, p]),
    "vl_conv_wgrad_ws_bytes": (sz, [p, i32]),
    "vl_conv_wgrad_fuses_bias": (i32, [p]),
    "vl_conv_wgrad": (i32, [p, p, p, p, p, p, sz, i32, p]),
    "vl_c8_bytes": (sz, [i32, i32, i32, i32, i32]),
    "vl_pack_c8": (i32, [p, p, i32, i32, i32, i32, i32, i32, p]),
    "vl_conv_c8_w_bytes": (sz, [p, i32]),
    "vl_conv_c8_pack_w": (i32, [p, p, p, i32, p]),
    "vl_conv_c8_fwd": (i32, [p, p, p, p, p, p, i32, i32, p]),
    "vl_conv_c8_dgrad": (i32, [p, p, p, p, p, p, p, i32, p]),
    "vl_pack_kc8": (i32, [p, p, i64, i32, i64, i64, p]),
    "vl_gemm_kc8_ws_bytes": (sz, [i32, i32, i32]),
    "vl_gemm_kc8": (i32, [p, p, p, i32, i32, i32, p, i32, p, sz, p]),
    "vl_s2d_c8_from_x0": (i32, [p, p, p, i32, p]),
    "vl_input_prep_u8_s2d": (i32, [p, p, p, i32, i32, i32, p, p, p, p, p]),
    "vl_input_prep_u8_box_s2d": (i32, [p, p, p, i32, i32, i32, p, p, p, p]),
    "vl_s2d_weights": (i32, [p, p, p, i32, p]),
    "vl_bias_grad_c8": (i32, [p, p, p, i32, i32, i32, i32, i32, p]),
    "vl_conv_c8_wgrad_ws_bytes": (sz, [p, i32]),
    "vl_conv_c8_wgrad": (i32, [p, p, p, p, p, sz, i32, p]),
    "vl_bias_grad_nchw": (i32, [p, p, p, i32, i32, i32, p]),
    "vl_lrn_fwd": (i32, [p, p, i32, i32, i32, i32, f32, f32, f32, p]),
    "vl_lrn_bwd": (i32, [p, p, p, i32, i32, i32, i32, f32, f32, f32, i32, i32, i32, p]),
    "vl_lrn_pool_fwd": (i32, [p, p, p, i32, i32, i32, i32, i32, i32, f32, f32, f32, p]),
    "vl_pool_lrn_bwd": (i32, [p, p, p, p, i32, i32, i32, i32, i32, i32, f32, f32, f32, i32, i32, p]),
    "vl_pool_lrn_bwd_test_ranges": (i32, [i32]),
    "vl_lrn_pool_fwd_c8": (i32, [p, i32, p, p, i32, i32, i32, i32, i32, i32, f32, f32, f32, p]),
    "vl_pool_lrn_bwd_c8": (i32, [p, i32, p, p, p, i32, i32, i32, i32, i32, i32, f32, f32, f32, i32, i32, p]),
    "vl_maxpool_fwd": (i32, [p, p, p, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, p]),
    "vl_maxpool_bwd": (i32, [p, p, p, p, i32, i32, i32, i32, i32, i32, i64, i64, i64, i64, i32, p]),
    "vl_gemm": (i32, [i32, i32, i32, i32, i32, p, i64, p, i64, p, i64, p, i32, p, p, sz, p]),
    "vl_colsum": (i32, [p, i64, p, p, i32, i32, p]),
    "vl_lstm_step_fwd": (i32, [p, p, p, p, p, p, i32, i32, i32, i32, f32, p]),
    "vl_lstm_step_bwd": (i32, [p, p, p, p, p, p, i32, i32, i32, i32, p]),
    "vl_lstm_seq_ws_bytes": (sz, [i32, i32, i32]),
    "vl_lstm_seq_fwd": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, f32, p, sz, p]),
    "vl_lstm_seq_bwd": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, p, sz, p]),
    "vl_lstm_seq_fwd_len": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, f32, p, p, sz, p]),
    "vl_lstm_seq_bwd_len": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, p, p, sz, p]),
    "vl_lstm_seq_tag_span": (sz, [i32, i32, i32]),
    "vl_lstm_seq_fwd_st": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, f32, p, sz, p, u32, p]),
    "vl_lstm_seq_bwd_st": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, p, sz, p, u32, p]),
    "vl_lstm_seq_bi_fwd": (i32, [p] * 14 + [i64, p, p, i32, i32, i32, f32, p, p, sz, p]),
    "vl_lstm_seq_bi_bwd": (i32, [p, p, i64] + [p] * 14 + [i32, i32, i32, p, p, sz, p]),
    "vl_lstm_seq_bi_tag_span": (sz, [i32, i32, i32]),
    "vl_lstm_seq_bi_fwd_st": (i32, [p] * 14 + [i64, p, p, i32, i32, i32, f32, p, sz, p, u32, p]),
    "vl_lstm_seq_bi_bwd_st": (i32, [p, p, i64] + [p] * 14 + [i32, i32, i32, p, sz, p, u32, p]),
    "vl_gru_seq_fwd": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, p, p, sz, p]),
    "vl_gru_seq_bwd": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, p, p, sz, p]),
    "vl_gru_seq_tag_span": (sz, [i32, i32, i32]),
    "vl_gru_seq_fwd_st": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, p, sz, p, u32, p]),
    "vl_gru_seq_bwd_st": (i32, [p, p, p, p, p, p, p, p, i32, i32, i32, p, sz, p, u32, p]),
    "vl_lstm_seq_ws_clear": (i32, [p, sz, p]),
    "vl_lstm_seq_status": (i32, [p, C.POINTER(i32)]),
    "vl_lstm_seq_test_hooks": (i32, [C.c_uint, i32]),
    "vl_transpose": (i32, [p, i64, p, i32, i32, p]),
    "vl_temporal_fusion_fwd": (i32, [p, p, i32, i32, i32, i32, p]),
    "vl_temporal_fusion_bwd": (i32, [p, p, i32, i32, i32, i32, p]),
    "vl_temporal_fusion_fwd_len": (i32, [p, p, i32, i32, i32, i32, p, p]),
    "vl_temporal_fusion_bwd_len": (i32, [p, p, i32, i32, i32, i32, p, p]),
    "vl_attn_pool_fwd": (i32, [p, p, p, p, p, p, p, i32, i32, i32, i32, p]),
    "vl_attn_pool_bwd": (i32, [p, p, p, p, p, p, p, p, p, i32, i32, i32, i32, p]),
    "vl_netvlad_fwd": (i32, [p, p, p, p, p, p, p, i32, i32, i32, i32, p]),
    "vl_netvlad_bwd": (i32, [p, p, p, p, p, p, p, p, p, p, i32, i32, i32, i32, p]),
    "vl_mhsa_fwd": (i32, [p, p, p, p, p, i32, i32, i32, i32, p]),
    "vl_mhsa_bwd": (i32, [p, p, p, p, p, p, i32, i32, i32, i32, p]),
    "vl_live_rows": (i32, [p, p, p, i32, i32, i32, p]),
    "vl_tconv_cols_fwd": (i32, [p, p, p, i32, i32, i32, i32, i32, i32, p]),
    "vl_tconv_cols_bwd": (i32, [p, p, p, p, i32, i32, i32, i32, i32, i32, p]),
    "vl_add_layer_norm_fwd": (i32, [p, p, p, p, p, p, p, i32, i32, i32, f32, p, p]),
    "vl_layer_norm_bwd": (i32, [p, p, p, p, p, p, p, i32, i32, i32, p, p]),
    "vl_gelu_fwd": (i32, [p, p, i64, p]),
    "vl_gelu_bwd": (i32, [p, p, p, i64, p]),
    "vl_mhsa_drop_fwd": (i32, [p, p, p, p, p, i32, i32, i32, i32, f32, u64, u32, i64, p]),
    "vl_mhsa_drop_fwd_st": (i32, [p, p, p, p, p, i32, i32, i32, i32, f32, p, u32, i64, p]),
    "vl_mhsa_drop_bwd": (i32, [p, p, p, p, p, p, i32, i32, i32, i32, f32, u64, u32, i64, p]),
    "vl_mhsa_drop_bwd_st": (i32, [p, p, p, p, p, p, i32, i32, i32, i32, f32, p, u32, i64, p]),
    "vl_add_layer_norm_drop_fwd": (i32, [p, p, p, p, p, p, p, i32, i32, i32, f32, p, f32, f32, u64, u32, u32, i32, i64, p]),
    "vl_add_layer_norm_drop_fwd_st": (i32, [p, p, p, p, p, p, p, i32, i32, i32, f32, p, f32, f32, p, u32, u32, i32, i64, p]),
    "vl_branch_drop_grad": (i32, [p, p, i32, i32, i32, p, f32, f32, u64, u32, u32, i32, i64, p]),
    "vl_branch_drop_grad_st": (i32, [p, p, i32, i32, i32, p, f32, f32, p, u32, u32, i32, i64, p]),
    "vl_dropout_fwd": (i32, [p, p, p, i64, f32, u64, p]),
    "vl_dropout_bwd": (i32, [p, p, p, i64, f32, p]),
    "vl_dropout_fwd_st": (i32, [p, p, p, i64, f32, p, p]),
    "vl_fc_dropout_fwd": (i32, [p, i64, f32, u64, u32, p]),
    "vl_fc_dropout_fwd_st": (i32, [p, i64, f32, p, u32, p]),
    "vl_relu_dropout_grad": (i32, [p, p, i64, f32, p]),
    "vl_softmax_xent": (i32, [p, p, p, p, p, i32, i32, f32, p]),
    "vl_softmax_xent_len": (i32, [p, p, p, p, p, i32, i32, f32, p, i32, p]),
    "vl_softmax_xent_ls": (i32, [p, p, p, p, p, i32, i32, f32, p, i32, f32, i32, p]),
    "vl_mixup_pairs": (i32, [p, i32, i32, i64, f32, p, p]),
    "vl_softmax_xent_mix": (i32, [p, p, p, p, p, i32, i32, f32, i32, f32, i32, f32, p, p]),
    "vl_softmax_xent_wf": (i32, [p, p, p, p, p, i32, i32, f32, p, i32, i32, f32, i32, f32, p, p, f32, p]),
    "vl_sigmoid_xent": (i32, [p, p, p, p, p, i32, i32, f32, p, i32, i32, f32, f32, p, p, f32, p]),
    "vl_cutmix_pairs": (i32, [p, i32, i32, i32, i32, i32, i32, p, p, p]),
    "vl_cutmix_pairs_s2d": (i32, [p, p, i32, i32, p, p, p]),
    "vl_erase_boxes": (i32, [p, i32, i32, i32, i32, i32, i32, p, i32, f32, p]),
    "vl_erase_boxes_s2d": (i32, [p, p, i32, i32, p, i32, f32, p]),
    "vl_sumsq": (i32, [p, i64, p, p, i32, p]),
    "vl_sgd_apply": (i32, [p, p, i64, f32, f32, p, f32, p, p]),
    "vl_adam_apply": (i32, [p, p, p, p, i64, f32, f32, p, f32, i32, p, p]),
    "vl_status_or": (i32, [p, p, i32, p]),
    "vl_step_state_bytes": (sz, []),
    "vl_step_state_set": (i32, [p, i64, f32, u32, p]),
    "vl_step_state_set_micro": (i32, [p, i64, i64, f32, u32, p]),
    "vl_step_state_set_ema": (i32, [p, f32, p]),
    "vl_sgd_apply_st": (i32, [p, p, i64, p, f32, p, f32, p, p]),
    "vl_adam_apply_st": (i32, [p, p, p, p, i64, p, f32, p, f32, p, p]),
    "vl_sgd_apply_tiers": (i32, [p, p, i64, f32, f32, p, f32, p, p, i32, p]),
    "vl_adam_apply_tiers": (i32, [p, p, p, p, i64, f32, f32, p, f32, i32, p, p, i32, p]),
    "vl_sgd_apply_tiers_st": (i32, [p, p, i64, p, f32, p, f32, p, p, i32, p]),
    "vl_adam_apply_tiers_st": (i32, [p, p, p, p, i64, p, f32, p, f32, p, p, i32, p]),
    "vl_sumsq_tiers": (i32, [p, i64, p, i32, p, p, p]),
    "vl_momentum_apply": (i32, [p, p, p, i64, f32, f32, i32, f32, p, f32, p, p, i32, p]),
    "vl_momentum_apply_st": (i32, [p, p, p, i64, p, f32, i32, f32, p, f32, p, p, i32, p]),
    "vl_l2_regularize": (i32, [p, p, i64, p, i32, p, p, p]),
    "vl_grad_accumulate": (i32, [p, p, i64, i32, p, i32, p]),
    "vl_ema_update": (i32, [p, p, i64, f32, p, p, i32, p]),
    "vl_ema_update_st": (i32, [p, p, i64, p, p, p, i32, p]),
    "vl_tensor_stats_ws_bytes": (sz, [p, i32]),
    "vl_tensor_stats": (i32, [p, p, i64, p, i32, p, p, sz, p]),
    "vl_lars_trust": (i32, [p, i32, C.c_double, C.c_double, p, f32, p, f32, p, p]),
    "vl_lars_apply": (i32, [p, p, p, i64, f32, f32, i32, f32, p, f32, p, p, i32, p, i32, p]),
    "vl_lars_apply_st": (i32, [p, p, p, i64, p, f32, i32, f32, p, f32, p, p, i32, p, i32, p]),
    "vl_lamb_moments_ws_bytes": (sz, [p, i32]),
    "vl_lamb_moments": (i32, [p, p, p, p, i64, f32, f32, f32, f32, p, f32, p, p, i32, p, p, i32, p, sz, p]),
    "vl_lamb_moments_st": (i32, [p, p, p, p, i64, p, f32, f32, p, f32, p, p, i32, p, p, i32, p, sz, p]),
    "vl_lamb_apply": (i32, [p, p, p, i64, f32, f32, f32, f32, p, p, i32, p, i32, p]),
    "vl_lamb_apply_st": (i32, [p, p, p, i64, p, f32, p, p, i32, p, i32, p]),
    "vl_step_state_set_lamb": (i32, [p, f32, f32, p]),
    "vl_fill": (i32, [p, i64, f32, p]),
    "vl_resize_create": (i32, [C.POINTER(p), i32, i32, i32, i32, i32]),
    "vl_resize_destroy": (None, [p]),
    "vl_resize_tmp_bytes": (sz, [p, i32]),
    "vl_resize_u8": (i32, [p, p, p, p, i32, p]),
    "vl_copy2d": (i32, [p, i64, p, i64, i32, i32, p]),
    "vl_eltwise2": (i32, [p, p, p, i64, i32, p]),
    "vl_max2_grad": (i32, [p, p, p, p, p, i64, p]),
    "vl_fuse_n": (i32, [p, i32, p, i64, i32, p]),
    "vl_fuse_n_grad": (i32, [p, i32, p, p, i64, i32, p]),
    "vl_relu_grad": (i32, [p, p, i64, p]),
}


class LrTier(C.Structure):
    """vl_lr_tier (include/vltf.h)."""
    _fields_ = [("begin", i64), ("end", i64), ("lr_mult", f32)]


MAX_LR_TIERS = 16         # VL_MAX_LR_TIERS


class StepState(C.Structure):
    """vl_step_state (include/vltf.h): 32 bytes; the host never reads the device block, this is the layout's record."""
    _fields_ = [("step", i64), ("lr", f32), ("tag_origin", u32), ("adam_lr", f32), ("ema_rate", f32), ("reserved", u32 * 2)]


class DecayRange(C.Structure):
    """vl_decay_range (include/vltf.h)."""
    _fields_ = [("begin", i64), ("end", i64), ("decay", f32)]


MAX_DECAY_RANGES = 64     # VL_MAX_DECAY_RANGES


class StatSegment(C.Structure):
    """vl_stat_segment (include/vltf.h)."""
    _fields_ = [("begin", i64), ("end", i64)]


class TensorStat(C.Structure):
    """vl_tensor_stat (include/vltf.h): 64 bytes, one per segment."""
    _fields_ = [("g_sum", C.c_double), ("g_sumsq", C.c_double), ("w_sum", C.c_double), ("w_sumsq", C.c_double),
                ("g_min", f32), ("g_max", f32), ("w_min", f32), ("w_max", f32),
                ("g_nonfinite", u32), ("w_nonfinite", u32), ("g_zero", u32), ("reserved", u32)]


MAX_STAT_SEGMENTS = 64    # VL_MAX_STAT_SEGMENTS
STAT_CHUNK = 16384        # VL_STAT_CHUNK


class LarsRange(C.Structure):
    """vl_lars_range (include/vltf.h)."""
    _fields_ = [("begin", i64), ("end", i64), ("lr_mult", f32), ("trust_index", C.c_int32)]


class LambRange(C.Structure):
    """vl_lamb_range (include/vltf.h): 32 bytes."""
    _fields_ = [("begin", i64), ("end", i64), ("lr_mult", f32), ("decay", f32), ("trust_index", C.c_int32), ("reserved", C.c_int32)]


class LambRow(C.Structure):
    """vl_lamb_row (include/vltf.h): 24 bytes, one per trust index."""
    _fields_ = [("w_sumsq", C.c_double), ("u_sumsq", C.c_double), ("nonfinite", u32), ("reserved", u32)]


# LAMB's bias corrections in vl_step_state: the words reserved[VL_STEP_STATE_LAMB_C1 / _C2], as byte offsets of the block
STEP_STATE_LAMB_C1_OFFSET = 24
STEP_STATE_LAMB_C2_OFFSET = 28


class VltfError(RuntimeError):
    pass


_lib = None


def lib():
    """The loaded library; raises VltfError when it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VltfError("libvltf_hip.so not found at %s -- build it with "
                            "`python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)" % LIB_PATH)
        # ONE HIP runtime per process: torch bundles its own libamdhip64.so (soname libamdhip64.so.7, the
        # same as /opt/rocm's).  Loading torch first makes our NEEDED entry resolve to that copy; the other
        # order would put two runtimes in the process and device pointers would not be shared.
        import torch  # noqa: F401
        tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(tl):
            C.CDLL(tl, mode=C.RTLD_GLOBAL)
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as ex:
            raise VltfError("cannot load %s: %s" % (LIB_PATH, ex))
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                raise VltfError("libvltf_hip.so does not export %s (stale build?)" % name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().vl_last_error()
        raise VltfError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


def call(name, *args):
    """Call an int-returning entry point and raise on failure."""
    check(getattr(lib(), name)(*args), name)
