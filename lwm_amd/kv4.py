"""The 4-bit (MXFP4) KV cache: the torch-tensor front end of lwm_kv4_cache_write / _at and lwm_attn_decode_kv4
(include/lwm_hip.h "4-bit KV cache", csrc/attn_decode_kv4.h).  As everything in lwm_amd.ops: hand-written HIP kernels on
the current torch stream, no PyTorch / CPU fallback.  kv4_dequant alone is a torch expression: the yardstick of the tests."""
import torch

from . import _capi
from .ops import KvFormat, _kvq_attn_decode, _kvq_cache_write, _kvq_cache_write_at

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)

KV4 = KvFormat("kv4", "fp4", "4-bit", "e2m1 nibble pairs", 64, torch.uint8, (4,), 127, ("key_scale_e8m0", "value_scale_e8m0"),
               "lwm_kv4_cache_write", "lwm_kv4_cache_write_at", "lwm_attn_decode_kv4", _capi.LwmKv4DecodeArgs, False)


def kv4_cache_write(cache, scale, src, *, dst_row0, src_row0=0, nrows=None):
    """Quantise src[:, src_row0:src_row0+nrows] (bf16) into the 4-bit cache at row dst_row0: `cache` takes the e2m1 nibble
    pairs, `scale` one e8m0 byte per block of 32 elements (lwm_kv4_cache_write; the format: include/lwm_hip.h)."""
    return _kvq_cache_write(KV4, cache, scale, src, dst_row0=dst_row0, src_row0=src_row0, nrows=nrows)


def kv4_cache_write_at(cache, scale, src, index_dev, *, row_offset=0, src_row0=0, nrows=None):
    """The same with the destination row `index + row_offset` read from an int32 DEVICE tensor
    (lwm_kv4_cache_write_at); rows that fall outside the cache are skipped."""
    return _kvq_cache_write_at(KV4, cache, scale, src, index_dev, row_offset=row_offset, src_row0=src_row0, nrows=nrows)


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
    return _kvq_attn_decode(KV4, q, cached_key, key_scale, cached_value, value_scale, k_splits=k_splits, dense_mask=dense_mask,
                            scale=scale)
