"""ctypes mirror of include/lwm_hip.h (struct layouts + prototypes).

Pure declarations: no library is loaded here.  `lwm_amd._lib` binds these to
liblwm_hip.so (the product); tests bind the same declarations to the
host-emulated build of the kernels.
"""
import ctypes as C

LWM_OK = 0
LWM_EINVAL = -1
LWM_EUNSUPPORTED = -2
LWM_ELAUNCH = -3


MAX_PIECES = 8     # LWM_MAX_PIECES


def set_pieces(args, side, pieces):
    """pieces = [(first row, position of that row), ...] of LwmAttnArgs' piecewise position map of `side` ("q" / "k");
    None or one piece leaves the single-piece fields alone."""
    if not pieces or len(pieces) < 2:
        return
    if len(pieces) > MAX_PIECES:
        raise ValueError(f"{side}: {len(pieces)} pieces, at most {MAX_PIECES}")
    setattr(args, side + "_pieces", len(pieces))
    rows, poss = getattr(args, side + "_piece_row"), getattr(args, side + "_piece_pos")
    for i, (r, p) in enumerate(pieces):
        rows[i], poss[i] = int(r), int(p)


class LwmTensor4(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("stride_b", C.c_int64), ("stride_s", C.c_int64),
                ("stride_h", C.c_int64)]


class LwmAttnArgs(C.Structure):
    _fields_ = [
        ("q", LwmTensor4), ("k", LwmTensor4), ("v", LwmTensor4),
        ("out", LwmTensor4),
        ("lse", C.c_void_p), ("out_acc", C.c_void_p), ("lse_acc", C.c_void_p),
        ("dout", LwmTensor4), ("dq", LwmTensor4), ("dk", LwmTensor4), ("dv", LwmTensor4),
        ("delta", C.c_void_p), ("dq_acc", C.c_void_p), ("dk_acc", C.c_void_p),
        ("dv_acc", C.c_void_p),
        ("segment_ids_q", C.c_void_p), ("segment_ids_k", C.c_void_p), ("key_valid", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("Sq", C.c_int32), ("Sk", C.c_int32), ("D", C.c_int32),
        ("q_start", C.c_int64), ("k_start", C.c_int64),
        ("scale", C.c_float),
        ("causal", C.c_int32), ("carry_in", C.c_int32), ("final_out", C.c_int32),
        ("dense_mask", C.c_void_p), ("mask_stride_b", C.c_int64), ("mask_stride_q", C.c_int64),
        ("k_splits", C.c_int32),
        ("seg_blocks_q", C.c_void_p), ("seg_blocks_k", C.c_void_p),
        ("dq_acc_head_major", C.c_int32),
        ("q_pieces", C.c_int32), ("k_pieces", C.c_int32),
        ("q_piece_row", C.c_int32 * MAX_PIECES), ("k_piece_row", C.c_int32 * MAX_PIECES),
        ("q_piece_pos", C.c_int64 * MAX_PIECES), ("k_piece_pos", C.c_int64 * MAX_PIECES),
        ("delta_bytes", C.c_int64),
        ("ds_ws", C.c_void_p), ("ds_ws_bytes", C.c_int64),
    ]


class LwmRingArgs(C.Structure):
    _fields_ = [
        ("q", LwmTensor4), ("k", LwmTensor4), ("v", LwmTensor4), ("out", LwmTensor4),
        ("lse", C.c_void_p), ("dout", LwmTensor4), ("dq", LwmTensor4), ("dk", LwmTensor4), ("dv", LwmTensor4),
        ("segment_ids", C.c_void_p), ("key_valid", C.c_void_p),
        ("B", C.c_int32), ("c", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("scale", C.c_float), ("causal", C.c_int32), ("workspace", C.c_void_p),
        ("layout", C.c_int32), ("schedule", C.c_int32),
        ("chunk_owner", C.c_void_p), ("n_chunks", C.c_int32),
        ("kv_keep", C.c_void_p), ("kv_kept", C.c_int32),
    ]


RING_LAYOUT = {"contiguous": 0, "zigzag": 1, "table": 2}
RING_SCHEDULE = {"ring": 0, "direct": 1, "mesh": 1}


class LwmGemvArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int64), ("nmat", C.c_int32), ("rows", C.c_int32), ("K", C.c_int32),
        ("w", C.c_void_p * 3), ("y", C.c_void_p * 3), ("ldy", C.c_int64 * 3), ("y_f32", C.c_void_p * 3), ("N", C.c_int32 * 3),
        ("workspace", C.c_void_p),
        ("norm_weight", C.c_void_p), ("ss_in", C.c_void_p), ("ss_n", C.c_int32), ("eps", C.c_float),
        ("residual", C.c_void_p * 3), ("ldres", C.c_int64 * 3),
        ("ss_out", C.c_void_p),
    ]


class LwmGemvW8Args(C.Structure):
    """LwmGemvArgs with w[i] as e4m3 bytes plus their scale tables"""
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int64), ("nmat", C.c_int32), ("rows", C.c_int32), ("K", C.c_int32),
        ("w", C.c_void_p * 3), ("w_scale", C.c_void_p * 3), ("y", C.c_void_p * 3), ("ldy", C.c_int64 * 3),
        ("y_f32", C.c_void_p * 3), ("N", C.c_int32 * 3),
        ("workspace", C.c_void_p),
        ("norm_weight", C.c_void_p), ("ss_in", C.c_void_p), ("ss_n", C.c_int32), ("eps", C.c_float),
        ("residual", C.c_void_p * 3), ("ldres", C.c_int64 * 3),
        ("ss_out", C.c_void_p),
    ]


class LwmGemvW4Args(C.Structure):
    """LwmGemvArgs with w[i] as e2m1 nibble pairs plus their e8m0 scale-byte tables"""
    _fields_ = LwmGemvW8Args._fields_


class LwmGemvW6Args(C.Structure):
    """LwmGemvArgs with w[i] as 24-byte slots of e2m3 codes plus their e8m0 scale-byte tables"""
    _fields_ = LwmGemvW8Args._fields_


class LwmKv8DecodeArgs(C.Structure):
    _fields_ = [
        ("q", LwmTensor4), ("k", C.c_void_p), ("v", C.c_void_p),
        ("k_stride_b", C.c_int64), ("k_stride_s", C.c_int64), ("k_stride_h", C.c_int64),
        ("v_stride_b", C.c_int64), ("v_stride_s", C.c_int64), ("v_stride_h", C.c_int64),
        ("k_scale", C.c_void_p), ("v_scale", C.c_void_p),
        ("k_scale_stride_b", C.c_int64), ("k_scale_stride_s", C.c_int64),
        ("v_scale_stride_b", C.c_int64), ("v_scale_stride_s", C.c_int64),
        ("dense_mask", C.c_void_p), ("mask_stride_b", C.c_int64),
        ("B", C.c_int32), ("Sk", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("scale", C.c_float), ("k_splits", C.c_int32),
        ("out_acc", C.c_void_p), ("lse_acc", C.c_void_p),
    ]


class LwmKv4DecodeArgs(C.Structure):
    """the field list of LwmKv8DecodeArgs; the scales are e8m0 bytes and their strides are in bytes"""
    _fields_ = list(LwmKv8DecodeArgs._fields_)


class LwmKv8PrefillArgs(C.Structure):
    _fields_ = [
        ("q", LwmTensor4), ("k", C.c_void_p), ("v", C.c_void_p),
        ("k_stride_b", C.c_int64), ("k_stride_s", C.c_int64), ("k_stride_h", C.c_int64),
        ("v_stride_b", C.c_int64), ("v_stride_s", C.c_int64), ("v_stride_h", C.c_int64),
        ("k_scale", C.c_void_p), ("v_scale", C.c_void_p),
        ("k_scale_stride_b", C.c_int64), ("k_scale_stride_s", C.c_int64),
        ("v_scale_stride_b", C.c_int64), ("v_scale_stride_s", C.c_int64),
        ("key_valid", C.c_void_p), ("key_valid_stride_b", C.c_int64),
        ("B", C.c_int32), ("Sq", C.c_int32), ("Sk", C.c_int32), ("H", C.c_int32), ("D", C.c_int32),
        ("q_start", C.c_int64), ("scale", C.c_float), ("k_splits", C.c_int32),
        ("out_acc", C.c_void_p), ("lse_acc", C.c_void_p),
    ]


class LwmKv6DecodeArgs(C.Structure):
    """the field list of LwmKv4DecodeArgs: e8m0 scale bytes, strides in bytes; the cache rows are 96-byte heads of e2m3 blocks"""
    _fields_ = list(LwmKv8DecodeArgs._fields_)


class LwmKv6PrefillArgs(C.Structure):
    """the field list of LwmKv8PrefillArgs; the scales are e8m0 bytes and their strides are in bytes"""
    _fields_ = list(LwmKv8PrefillArgs._fields_)


class LwmSampleArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("rows", C.c_int32), ("V", C.c_int32),
        ("cfg_scale", C.c_void_p), ("temperature", C.c_float), ("top_k", C.c_int32), ("seed", C.c_uint64),
        ("step_dev", C.c_void_p), ("step_base", C.c_int32), ("step", C.c_int32),
        ("force_period", C.c_int32), ("force_token", C.c_int32), ("done", C.c_void_p), ("eos", C.c_int64),
        ("pad", C.c_int64), ("tokens", C.c_void_p), ("copies", C.c_int32), ("seq", C.c_void_p), ("seq_ld", C.c_int64),
        ("seq_cols", C.c_int32), ("top_p", C.c_float),
    ]


class LwmAdamWTensor(C.Structure):
    """one entry of the DEVICE tensor table of the fused AdamW (built on the host, copied over)"""
    _fields_ = [
        ("master", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("copy_bf16", C.c_void_p), ("numel", C.c_int64), ("grad_bf16", C.c_int32), ("decay", C.c_int32),
        ("bias_corr1", C.c_float), ("sqrt_bias_corr2", C.c_float),
    ]


class LwmAdamWArgs(C.Structure):
    _fields_ = [
        ("tensors", C.c_void_p), ("chunks", C.c_void_p), ("n_tensors", C.c_int32), ("n_chunks", C.c_int32),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
        ("max_norm", C.c_double),
        ("grad_partials", C.c_void_p), ("grad_partials_len", C.c_int64),
        ("param_partials", C.c_void_p), ("param_partials_len", C.c_int64),
        ("norms", C.c_void_p),
    ]


class LwmDropoutArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("res", C.c_void_p), ("y", C.c_void_p), ("B", C.c_int32), ("S", C.c_int32), ("C", C.c_int32),
                ("s_offset", C.c_int64), ("site", C.c_uint32), ("key0", C.c_uint32), ("key1", C.c_uint32), ("thr16", C.c_uint32),
                ("inv", C.c_float)]


RING_GROUP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
RING_SEND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)


class LwmRingTransport(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("group_start", RING_GROUP_FN), ("send", RING_SEND_FN), ("recv", RING_SEND_FN),
                ("group_end", RING_GROUP_FN)]


class LwmConvArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p),
                ("y", C.c_void_p)] + [(n, C.c_int32) for n in (
                    "B", "Hin", "Win", "Cin", "Cout", "KH", "KW", "stride", "pad", "up_shift", "Ho",
                    "Wo", "clip")]


class LwmFramesArgs(C.Structure):
    """the tables (h_* / v_* / scale) are HOST pointers; frames, out, workspace are device pointers"""
    _fields_ = [("frames", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("h_bounds", C.c_void_p), ("h_coeffs", C.c_void_p), ("v_bounds", C.c_void_p), ("v_coeffs", C.c_void_p),
                ("scale", C.c_void_p)] + [(n, C.c_int32) for n in (
                    "T", "H", "W", "size", "h_ksize", "v_ksize", "left", "top")]


# name -> (restype, argtypes); every symbol include/lwm_hip.h declares
PROTOTYPES = {
    "lwm_attn_fwd": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_attn_bwd_delta": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_attn_bwd_dq": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_attn_bwd_dkdv": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_attn_bwd_delta_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "lwm_attn_bwd_ds_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64]),
    "lwm_attn_fwd_f32": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_attn_bwd_delta_f32": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_attn_bwd_dq_f32": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_attn_bwd_dkdv_f32": (C.c_int, [C.POINTER(LwmAttnArgs), C.c_void_p]),
    "lwm_rope_f32": (C.c_int, [LwmTensor4, LwmTensor4, C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p]),
    "lwm_rmsnorm_fwd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "lwm_rmsnorm_bwd_f32": (C.c_int, [C.c_void_p] * 7 + [C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_swiglu_fwd_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "lwm_swiglu_bwd_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
    "lwm_softmax_ce_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_sum_f32": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "lwm_ring_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lwm_ring_unique_id": (C.c_int, [C.c_void_p]),
    "lwm_ring_create_from_id": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lwm_ring_create_transport": (C.c_int, [C.POINTER(LwmRingTransport), C.c_int32, C.c_int32, C.c_void_p,
                                            C.POINTER(C.c_void_p)]),
    "lwm_ring_destroy": (C.c_int, [C.c_void_p]),
    "lwm_ring_workspace_bytes": (C.c_int64, [C.c_int32] * 7),
    "lwm_ring_attn_fwd": (C.c_int, [C.c_void_p, C.POINTER(LwmRingArgs), C.c_void_p]),
    "lwm_ring_attn_bwd": (C.c_int, [C.c_void_p, C.POINTER(LwmRingArgs), C.c_void_p]),
    "lwm_ring_bytes_sent": (C.c_int64, [C.c_void_p]),
    "lwm_ring_planned_bytes": (C.c_int64, [C.c_int32] * 10),
    "lwm_ring_planned_bytes_table": (C.c_int64, [C.c_void_p] + [C.c_int32] * 7),
    "lwm_ring_selftest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lwm_ring_set_fetch_groups": (C.c_int, [C.c_void_p, C.c_int32]),
    "lwm_ring_last_form": (C.c_int, [C.c_void_p]),
    "lwm_ring_kv_keep_bytes": (C.c_int64, [C.c_int32] * 5),
    "lwm_ring_fetch_timeline": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32]),
    "lwm_ring_ipc_info_bytes": (C.c_int64, []),
    "lwm_ring_ipc_export": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lwm_ring_ipc_connect": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lwm_ring_create_ipc": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lwm_ring_ipc_destroy": (C.c_int, [C.c_void_p]),
    "lwm_attn_segment_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_attn_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, LwmTensor4, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_kv_cache_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                    C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_kv_cache_write_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_kv8_cache_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_kv8_cache_write_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                         C.c_void_p]),
    "lwm_attn_decode_kv8": (C.c_int, [C.POINTER(LwmKv8DecodeArgs), C.c_void_p]),
    "lwm_attn_prefill_kv8": (C.c_int, [C.POINTER(LwmKv8PrefillArgs), C.c_void_p]),
    "lwm_kv4_cache_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_kv4_cache_write_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                         C.c_void_p]),
    "lwm_attn_decode_kv4": (C.c_int, [C.POINTER(LwmKv4DecodeArgs), C.c_void_p]),
    "lwm_kv6_cache_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_kv6_cache_write_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                         C.c_void_p]),
    "lwm_attn_decode_kv6": (C.c_int, [C.POINTER(LwmKv6DecodeArgs), C.c_void_p]),
    "lwm_attn_prefill_kv6": (C.c_int, [C.POINTER(LwmKv6PrefillArgs), C.c_void_p]),
    "lwm_rope_bf16": (C.c_int, [LwmTensor4, LwmTensor4, C.c_void_p, C.c_void_p] + [C.c_int32] * 6 + [C.c_void_p]),
    "lwm_rmsnorm_fwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                      C.c_float, C.c_void_p]),
    "lwm_rmsnorm_bwd_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "lwm_rmsnorm_bwd_bf16": (C.c_int, [C.c_void_p] * 7 + [C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_rmsnorm_bwd_res_bf16": (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_swiglu_fwd_ld_bf16": (C.c_int, [C.c_void_p, C.c_int64] * 3 + [C.c_int64, C.c_int64, C.c_void_p]),
    "lwm_swiglu_bwd_ld_bf16": (C.c_int, [C.c_void_p, C.c_int64] * 5 + [C.c_int64, C.c_int64, C.c_void_p]),
    "lwm_wgrad_workspace_bytes": (C.c_int64, [C.c_int64] * 3),
    "lwm_wgrad_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int64] * 4 +
                       [C.c_void_p, C.c_int64, C.c_void_p]),
    "lwm_transpose_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "lwm_swiglu_fwd_bf16": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]),
    "lwm_swiglu_bwd_bf16": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
    "lwm_softmax_ce_bf16": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int32, C.c_void_p]),
    "lwm_gemv_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "lwm_gemv_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_gemv_multi_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_void_p,
                                      C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_gemv_fused_bf16": (C.c_int, [C.POINTER(LwmGemvArgs), C.c_void_p]),
    "lwm_w8_quantise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_gemv_fused_w8": (C.c_int, [C.POINTER(LwmGemvW8Args), C.c_void_p]),
    "lwm_w4_quantise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_gemv_fused_w4": (C.c_int, [C.POINTER(LwmGemvW4Args), C.c_void_p]),
    "lwm_w6_quantise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_gemv_fused_w6": (C.c_int, [C.POINTER(LwmGemvW6Args), C.c_void_p]),
    "lwm_gemm_rows_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "lwm_gemm_rows_fused_bf16": (C.c_int, [C.POINTER(LwmGemvArgs), C.c_void_p]),
    "lwm_gemm_rows_fused_w8": (C.c_int, [C.POINTER(LwmGemvW8Args), C.c_void_p]),
    "lwm_gemm_rows_fused_w6": (C.c_int, [C.POINTER(LwmGemvW6Args), C.c_void_p]),
    "lwm_sample_tokens": (C.c_int, [C.POINTER(LwmSampleArgs), C.c_void_p]),
    "lwm_adamw_grad_norm": (C.c_int, [C.POINTER(LwmAdamWArgs), C.c_void_p]),
    "lwm_adamw_step": (C.c_int, [C.POINTER(LwmAdamWArgs), C.c_void_p]),
    "lwm_adamw_chunk": (C.c_int, []),
    "lwm_dropout_add_bf16": (C.c_int, [C.POINTER(LwmDropoutArgs), C.c_void_p]),
    "lwm_dropout_add_f32": (C.c_int, [C.POINTER(LwmDropoutArgs), C.c_void_p]),
    "lwm_dropout_bwd_bf16": (C.c_int, [C.POINTER(LwmDropoutArgs), C.c_void_p]),
    "lwm_dropout_bwd_f32": (C.c_int, [C.POINTER(LwmDropoutArgs), C.c_void_p]),
    "lwm_cast_f32_to_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "lwm_sum_f32_to_bf16": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "lwm_conv2d_nhwc_f32": (C.c_int, [C.POINTER(LwmConvArgs), C.c_void_p]),
    "lwm_conv2d_nhwc_bf16": (C.c_int, [C.POINTER(LwmConvArgs), C.c_void_p]),
    "lwm_groupnorm_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    "lwm_groupnorm_silu_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                                            C.c_float, C.c_int32, C.c_void_p]),
    "lwm_vq_sqnorm_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_vq_argmin_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_vq_gather_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "lwm_frames_preprocess_workspace_bytes": (C.c_int64, [C.c_int32] * 5),
    "lwm_frames_preprocess_u8": (C.c_int, [C.POINTER(LwmFramesArgs), C.c_void_p]),
    "lwm_last_error": (C.c_char_p, []),
    "lwm_version": (C.c_int, []),
    "lwm_sizeof": (C.c_int, [C.c_int]),
}


def bind(lib):
    """Attach restype/argtypes for every declared symbol; raises if one is missing or if
    the struct mirrors above do not have the library's layout."""
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    for which, cls in ((0, LwmAttnArgs), (1, LwmConvArgs), (2, LwmRingArgs), (4, LwmSampleArgs), (5, LwmKv8DecodeArgs),
                       (6, LwmKv8PrefillArgs), (7, LwmAdamWArgs), (8, LwmAdamWTensor), (9, LwmGemvW8Args),
                       (10, LwmKv4DecodeArgs), (11, LwmGemvW4Args), (12, LwmFramesArgs), (13, LwmKv6DecodeArgs),
                       (14, LwmKv6PrefillArgs), (15, LwmGemvW6Args), (16, LwmDropoutArgs)):
        if lib.lwm_sizeof(which) != C.sizeof(cls):
            raise ImportError(f"{cls.__name__}: ctypes mirror is {C.sizeof(cls)} bytes, library has "
                              f"{lib.lwm_sizeof(which)} (include/lwm_hip.h and lwm_amd/_capi.py out of step)")
    return lib


class LwmError(RuntimeError):
    pass


def check(lib, rc, what):
    if rc != LWM_OK:
        msg = lib.lwm_last_error()
        raise LwmError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")
