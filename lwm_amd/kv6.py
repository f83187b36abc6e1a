"""The 6-bit (MXFP6 e2m3) KV cache: the torch-tensor front end of lwm_kv6_cache_write / _at, lwm_attn_decode_kv6 and
lwm_attn_prefill_kv6 (include/lwm_hip.h "6-bit KV cache", csrc/attn_decode_kv6.h, csrc/attn_prefill_kv6.h).  As everything
in lwm_amd.ops: hand-written HIP kernels on the current torch stream, no PyTorch / CPU fallback.  kv6_dequant alone is a
torch expression: the yardstick of the tests."""
import torch

from . import _capi
from ._lib import lib  # noqa: F401  (unused here: every call goes through ops.lib.  Kept as an attribute only because
#                                      tests/test_kv6_boundary.py assigns to it; drop it with that assignment)
from .ops import KvFormat, _kvq_attn_decode, _kvq_attn_prefill, _kvq_cache_write, _kvq_cache_write_at

# magnitude code c = 0..31: c / 8 below 8, (1 + (c & 7) / 8) * 2^((c >> 3) - 1) from 8 on; bit 5 is the sign
E2M3_VALUES = tuple(sign * (c / 8.0 if c < 8 else (1.0 + (c & 7) / 8.0) * 2.0 ** ((c >> 3) - 1)) for sign in (1.0, -1.0) for c in range(32))

KV6 = KvFormat("kv6", "fp6", "6-bit", "e2m3 blocks", 96, torch.uint8, (4,), 127, ("key_scale_e8m0", "value_scale_e8m0"),
               "lwm_kv6_cache_write", "lwm_kv6_cache_write_at", "lwm_attn_decode_kv6", _capi.LwmKv6DecodeArgs, True,
               "lwm_amd.kv6:attn_prefill_kv6")


def kv6_cache_write(cache, scale, src, *, dst_row0, src_row0=0, nrows=None):
    """Quantise src[:, src_row0:src_row0+nrows] (bf16) into the 6-bit cache at row dst_row0: `cache` takes the e2m3 blocks
    (24 bytes per 32 elements), `scale` one e8m0 byte per block (lwm_kv6_cache_write; the format: include/lwm_hip.h)."""
    return _kvq_cache_write(KV6, cache, scale, src, dst_row0=dst_row0, src_row0=src_row0, nrows=nrows)


def kv6_cache_write_at(cache, scale, src, index_dev, *, row_offset=0, src_row0=0, nrows=None):
    """The same with the destination row `index + row_offset` read from an int32 DEVICE tensor
    (lwm_kv6_cache_write_at); rows that fall outside the cache are skipped."""
    return _kvq_cache_write_at(KV6, cache, scale, src, index_dev, row_offset=row_offset, src_row0=src_row0, nrows=nrows)


def kv6_codes(q):
    """cache bytes uint8 (..., 96) -> the e2m3 codes (..., 128), element order: element j of a block is bits [6j, 6j + 6)
    of the block's 24 bytes read as one little-endian integer, i.e. four codes per three bytes."""
    b = q.reshape(*q.shape[:-1], 32, 3).to(torch.int32)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack([(w >> (6 * i)) & 63 for i in range(4)], dim=-1).reshape(*q.shape[:-1], 128)


def kv6_dequant(q, scale):
    """The numbers a 6-bit cache holds, as bf16 (..., 128): e2m3(code) * 2^(scale byte - 127), exactly (4 significant bits
    times a power of two).  q uint8 (..., 96), scale uint8 (..., 4).  A torch table lookup for tests and debugging -- the
    kernels never materialise it."""
    if q.dtype != torch.uint8 or scale.dtype != torch.uint8 or q.shape[-1] != 96 or scale.shape[-1] != 4 or \
            q.shape[:-1] != scale.shape[:-1]:
        raise ValueError("kv6_dequant: expected uint8 e2m3 block bytes (..., 96) and uint8 e8m0 bytes (..., 4)")
    table = torch.tensor(E2M3_VALUES, dtype=torch.float64, device=q.device)
    s = torch.exp2(scale.to(torch.float64) - 127.0).repeat_interleave(32, dim=-1)
    return (table[kv6_codes(q).long()] * s).to(torch.bfloat16)


def attn_decode_kv6(q, cached_key, key_scale, cached_value, value_scale, *, k_splits, dense_mask=None, scale=None):
    """One query per batch row over the 6-bit cache (lwm_attn_decode_kv6): q bf16 (B,1,H,128); the cache as written by
    kv6_cache_write; dense_mask u8 (B,1,Sk) or None.  Returns normalised partials (o_parts f32 [k_splits,B,1,H,D],
    lse_parts f32 [k_splits,B,H,1]) -- merge with ops.attn_combine."""
    return _kvq_attn_decode(KV6, q, cached_key, key_scale, cached_value, value_scale, k_splits=k_splits, dense_mask=dense_mask,
                            scale=scale)


def attn_prefill_kv6(q, cached_key, key_scale, cached_value, value_scale, *, q_start, k_splits, key_valid=None, scale=None):
    """A block of queries over the 6-bit cache: q bf16 (B,Sq,H,128) at positions q_start + i; cached_key / cached_value
    uint8 (B,Sk,H,96) and key_scale / value_scale uint8 (B,Sk,H,4) as written by kv6_cache_write (views of a longer cache
    are fine: only the innermost strides must be contiguous); key_valid u8 (B,Sk) or None, rows may be strided.  Key j is
    visible to query i iff j <= q_start + i and key_valid[b, j] != 0.  The blocks are dequantised on their way into LDS; no
    bf16 copy of the cache is made.  Returns normalised partials (o_parts f32 [k_splits,B,Sq,H,D], lse_parts f32
    [k_splits,B,H,Sq]) -- merge with ops.attn_combine."""
    return _kvq_attn_prefill(KV6, "lwm_attn_prefill_kv6", _capi.LwmKv6PrefillArgs, q, cached_key, key_scale, cached_value,
                             value_scale, q_start=q_start, k_splits=k_splits, key_valid=key_valid, scale=scale)
