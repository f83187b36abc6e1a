"""Block attention over the 8-bit (e4m3) KV cache: the torch-tensor front end of lwm_attn_prefill_kv8
(include/lwm_hip.h, csrc/attn_prefill_kv8.h).  As everything in lwm_amd.ops: a hand-written HIP kernel on the current
torch stream, no PyTorch / CPU fallback."""
import ctypes as C
import math

import torch

from . import _capi
from ._lib import lib
from .ops import _stream_ptr, _t4


def attn_prefill_kv8(q, cached_key, key_scale, cached_value, value_scale, *, q_start, k_splits, key_valid=None, scale=None):
    """A block of queries over the 8-bit cache: q bf16 (B,Sq,H,128) at positions q_start + i; cached_key / cached_value
    uint8 (B,Sk,H,128) and key_scale / value_scale f32 (B,Sk,H) as written by ops.kv8_cache_write (views of a longer cache
    are fine: only the innermost stride must be 1); key_valid u8 (B,Sk) or None, rows may be strided.  Key j is visible to
    query i iff j <= q_start + i and key_valid[b, j] != 0.  The bytes are dequantised on their way into LDS; no bf16 copy
    of the cache is made.  Returns normalised partials (o_parts f32 [k_splits,B,Sq,H,D], lse_parts f32 [k_splits,B,H,Sq])
    -- merge with ops.attn_combine."""
    if not torch.is_tensor(q) or q.dim() != 4:
        raise ValueError("attn_prefill_kv8: q: expected a bf16 (B,Sq,H,D) device tensor")
    B, Sq, H, D = q.shape
    if q.dtype != torch.bfloat16:
        raise ValueError("attn_prefill_kv8: expected a bf16 (B,Sq,H,D) query (the 8-bit cache holds quantised bf16 rows; "
                         "there is no float32 flavour)")
    if Sq < 1 or D != 128:
        raise ValueError(f"attn_prefill_kv8: q of shape {tuple(q.shape)}: need Sq >= 1 and head_dim 128")
    a = _capi.LwmKv8PrefillArgs()
    a.q = _t4(q, "q", torch.bfloat16)
    if not torch.is_tensor(cached_key) or cached_key.dim() != 4:
        raise ValueError(f"cached_key: expected a uint8 device tensor of shape ({B},Sk,{H},{D})")
    Sk = cached_key.shape[1]
    if Sk < 1:
        raise ValueError("cached_key: expected at least one cache row")
    for n, c, s in (("key", cached_key, key_scale), ("value", cached_value, value_scale)):
        if not torch.is_tensor(c) or not c.is_cuda or c.device != q.device or c.dtype != torch.uint8 or \
                tuple(c.shape) != (B, Sk, H, D) or c.stride(3) != 1:
            raise ValueError(f"cached_{n}: expected a uint8 tensor of shape {(B, Sk, H, D)} on {q.device} with contiguous D")
        if not torch.is_tensor(s) or not s.is_cuda or s.device != q.device or s.dtype != torch.float32 or \
                tuple(s.shape) != (B, Sk, H) or s.stride(2) != 1:
            raise ValueError(f"{n}_scale: expected an f32 tensor of shape {(B, Sk, H)} on {q.device} with contiguous heads")
    q_start = int(q_start)
    if q_start < 0:
        raise ValueError(f"attn_prefill_kv8: q_start = {q_start} < 0")
    a.k, a.v = cached_key.data_ptr(), cached_value.data_ptr()
    a.k_stride_b, a.k_stride_s, a.k_stride_h = cached_key.stride()[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = cached_value.stride()[:3]
    a.k_scale, a.v_scale = key_scale.data_ptr(), value_scale.data_ptr()
    a.k_scale_stride_b, a.k_scale_stride_s = key_scale.stride()[:2]
    a.v_scale_stride_b, a.v_scale_stride_s = value_scale.stride()[:2]
    if key_valid is not None:
        m = key_valid
        if not torch.is_tensor(m) or not m.is_cuda or m.device != q.device or m.dtype != torch.uint8 or \
                tuple(m.shape) != (B, Sk) or m.stride(1) != 1:
            raise ValueError(f"key_valid: expected a u8 tensor of shape {(B, Sk)} on {q.device} with contiguous keys")
        a.key_valid, a.key_valid_stride_b = m.data_ptr(), m.stride(0)
    a.B, a.Sq, a.Sk, a.H, a.D = B, Sq, Sk, H, D
    a.q_start = q_start
    a.scale = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    k_splits = max(1, int(k_splits))
    if k_splits > 4096:
        raise ValueError(f"attn_prefill_kv8: k_splits = {k_splits} > 4096")
    a.k_splits = k_splits
    o_parts = torch.empty((k_splits, B, Sq, H, D), dtype=torch.float32, device=q.device)
    lse_parts = torch.empty((k_splits, B, H, Sq), dtype=torch.float32, device=q.device)
    a.out_acc, a.lse_acc = o_parts.data_ptr(), lse_parts.data_ptr()
    L = lib()
    _capi.check(L, L.lwm_attn_prefill_kv8(C.byref(a), _stream_ptr()), "lwm_attn_prefill_kv8")
    return o_parts, lse_parts
