"""The 4-bit (MXFP4) KV cache: the torch-tensor front end of lwm_kv4_cache_write / _at and lwm_attn_decode_kv4
(include/lwm_hip.h "4-bit KV cache", csrc/attn_decode_kv4.h).  As everything in lwm_amd.ops: hand-written HIP kernels on
the current torch stream, no PyTorch / CPU fallback.  kv4_dequant alone is a torch expression: the yardstick of the tests."""
import ctypes as C
import math

import torch

from . import _capi
from ._lib import lib
from .ops import _stream_ptr, _t4

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


def _kv4_check(cache, scale, src):
    """(nibble bytes (B,S,H,64) u8, e8m0 bytes (B,S,H,4) u8, bf16 source (B,*,H,128)) with contiguous rows"""
    if not cache.is_cuda or cache.dtype != torch.uint8 or cache.dim() != 4 or not cache[0].is_contiguous():
        raise ValueError("cache: expected a uint8 (B,S,H,64) device tensor of e2m1 nibble pairs with contiguous (S,H,64)")
    B, rows, H, D2 = cache.shape
    if D2 != 64:
        raise ValueError(f"cache: last dimension {D2}; the 4-bit cache holds heads of 128 elements in 64 bytes")
    if not scale.is_cuda or scale.dtype != torch.uint8 or tuple(scale.shape) != (B, rows, H, 4) or not scale[0].is_contiguous():
        raise ValueError(f"scale: expected a uint8 device tensor of e8m0 bytes of shape {(B, rows, H, 4)} with contiguous (S,H,4)")
    if not src.is_cuda or src.dtype != torch.bfloat16 or src.dim() != 4 or not src[0].is_contiguous() or \
            src.shape[0] != B or tuple(src.shape[2:]) != (H, 128):
        raise ValueError(f"src: expected a bf16 device tensor (B,*,H,D) = ({B},*,{H},128) with contiguous (S,H,D) "
                         "(the 4-bit cache quantises bf16 rows; there is no float32 flavour)")
    return B, rows, H, 128


def kv4_cache_write(cache, scale, src, *, dst_row0, src_row0=0, nrows=None):
    """Quantise src[:, src_row0:src_row0+nrows] (bf16) into the 4-bit cache at row dst_row0: `cache` takes the e2m1 nibble
    pairs, `scale` one e8m0 byte per block of 32 elements (lwm_kv4_cache_write; the format: include/lwm_hip.h)."""
    B, rows, H, D = _kv4_check(cache, scale, src)
    if nrows is None:
        nrows = src.shape[1] - src_row0
    if dst_row0 < 0 or dst_row0 + nrows > rows or src_row0 < 0 or src_row0 + nrows > src.shape[1]:
        raise ValueError("kv4_cache_write: row range out of bounds")
    L = lib()
    _capi.check(L, L.lwm_kv4_cache_write(cache.data_ptr(), src.data_ptr(), B, cache.stride(0), src.stride(0), dst_row0,
                                         src_row0, nrows, H * D, scale.data_ptr(), scale.stride(0), H, _stream_ptr()),
                "lwm_kv4_cache_write")
    return cache, scale


def kv4_cache_write_at(cache, scale, src, index_dev, *, row_offset=0, src_row0=0, nrows=None):
    """The same with the destination row `index + row_offset` read from an int32 DEVICE tensor
    (lwm_kv4_cache_write_at); rows that fall outside the cache are skipped."""
    B, rows, H, D = _kv4_check(cache, scale, src)
    if not index_dev.is_cuda or index_dev.dtype != torch.int32 or index_dev.numel() != 1:
        raise ValueError("index_dev: expected a one-element int32 device tensor")
    if nrows is None:
        nrows = src.shape[1] - src_row0
    if src_row0 < 0 or src_row0 + nrows > src.shape[1]:
        raise ValueError("kv4_cache_write_at: source row range out of bounds")
    L = lib()
    _capi.check(L, L.lwm_kv4_cache_write_at(cache.data_ptr(), src.data_ptr(), B, cache.stride(0), src.stride(0),
                                            index_dev.data_ptr(), row_offset, rows, src_row0, nrows, H * D,
                                            scale.data_ptr(), scale.stride(0), H, _stream_ptr()),
                "lwm_kv4_cache_write_at")
    return cache, scale


def kv4_dequant(q, scale):
    """The numbers a 4-bit cache holds, as bf16 (..., 128): e2m1(code) * 2^(scale byte - 127), exactly (2 significant bits
    times a power of two).  q uint8 (..., 64), scale uint8 (..., 4).  A torch table lookup for tests and debugging -- the
    decode kernel never materialises it."""
    if q.dtype != torch.uint8 or scale.dtype != torch.uint8 or q.shape[-1] != 64 or scale.shape[-1] != 4 or \
            q.shape[:-1] != scale.shape[:-1]:
        raise ValueError("kv4_dequant: expected uint8 nibble bytes (..., 64) and uint8 e8m0 bytes (..., 4)")
    table = torch.tensor(E2M1_VALUES, dtype=torch.float64, device=q.device)
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(*q.shape[:-1], 128).long()      # element 2i low, 2i+1 high
    s = torch.exp2(scale.to(torch.float64) - 127.0).repeat_interleave(32, dim=-1)
    return (table[codes] * s).to(torch.bfloat16)


def attn_decode_kv4(q, cached_key, key_scale, cached_value, value_scale, *, k_splits, dense_mask=None, scale=None):
    """One query per batch row over the 4-bit cache (lwm_attn_decode_kv4): q bf16 (B,1,H,128); the cache as written by
    kv4_cache_write; dense_mask u8 (B,1,Sk) or None.  Returns normalised partials (o_parts f32 [k_splits,B,1,H,D],
    lse_parts f32 [k_splits,B,H,1]) -- merge with ops.attn_combine."""
    if not torch.is_tensor(q) or q.dim() != 4:
        raise ValueError("attn_decode_kv4: q: expected a bf16 (B,1,H,D) device tensor")
    B, Sq, H, D = q.shape
    if Sq != 1 or q.dtype != torch.bfloat16:
        raise ValueError("attn_decode_kv4: expected a bf16 (B,1,H,D) query (the 4-bit cache serves one-token decode steps)")
    if D != 128:
        raise ValueError(f"attn_decode_kv4: head_dim {D} (the 4-bit decode kernel is built for 128)")
    a = _capi.LwmKv4DecodeArgs()
    a.q = _t4(q, "q", torch.bfloat16)
    Sk = cached_key.shape[1]
    for n, c, s in (("key", cached_key, key_scale), ("value", cached_value, value_scale)):
        if not c.is_cuda or c.device != q.device or c.dtype != torch.uint8 or tuple(c.shape) != (B, Sk, H, D // 2) or \
                c.stride(3) != 1:
            raise ValueError(f"cached_{n}: expected a uint8 tensor of shape {(B, Sk, H, D // 2)} on {q.device} with contiguous bytes")
        if not s.is_cuda or s.device != q.device or s.dtype != torch.uint8 or tuple(s.shape) != (B, Sk, H, 4) or \
                s.stride(3) != 1 or s.stride(2) != 4:
            raise ValueError(f"{n}_scale: expected a uint8 tensor of shape {(B, Sk, H, 4)} on {q.device} with contiguous heads")
    a.k, a.v = cached_key.data_ptr(), cached_value.data_ptr()
    a.k_stride_b, a.k_stride_s, a.k_stride_h = cached_key.stride()[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = cached_value.stride()[:3]
    a.k_scale, a.v_scale = key_scale.data_ptr(), value_scale.data_ptr()
    a.k_scale_stride_b, a.k_scale_stride_s = key_scale.stride()[:2]
    a.v_scale_stride_b, a.v_scale_stride_s = value_scale.stride()[:2]
    if dense_mask is not None:
        m = dense_mask
        if not m.is_cuda or m.dtype != torch.uint8 or tuple(m.shape) != (B, 1, Sk) or m.stride(2) != 1:
            raise ValueError(f"dense_mask: expected a u8 device tensor of shape {(B, 1, Sk)} with contiguous keys")
        a.dense_mask, a.mask_stride_b = m.data_ptr(), m.stride(0)
    a.B, a.Sk, a.H, a.D = B, Sk, H, D
    a.scale = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    k_splits = max(1, int(k_splits))
    if k_splits > 4096:
        raise ValueError(f"attn_decode_kv4: k_splits = {k_splits} > 4096")
    a.k_splits = k_splits
    o_parts = torch.empty((k_splits, B, 1, H, D), dtype=torch.float32, device=q.device)
    lse_parts = torch.empty((k_splits, B, H, 1), dtype=torch.float32, device=q.device)
    a.out_acc, a.lse_acc = o_parts.data_ptr(), lse_parts.data_ptr()
    L = lib()
    _capi.check(L, L.lwm_attn_decode_kv4(C.byref(a), _stream_ptr()), "lwm_attn_decode_kv4")
    return o_parts, lse_parts
