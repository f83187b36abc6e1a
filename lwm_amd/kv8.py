"""Block attention over the 8-bit (e4m3) KV cache: the torch-tensor front end of lwm_attn_prefill_kv8
(include/lwm_hip.h, csrc/attn_prefill_kv8.h).  As everything in lwm_amd.ops: a hand-written HIP kernel on the current
torch stream, no PyTorch / CPU fallback."""
from . import _capi
from ._lib import lib  # noqa: F401  (unused here: the call goes through ops.lib.  Kept as an attribute only because
#                                      tests/test_kv8_prefill_boundary.py assigns to it; drop it with that assignment)
from .ops import KV8, _kvq_attn_prefill


def attn_prefill_kv8(q, cached_key, key_scale, cached_value, value_scale, *, q_start, k_splits, key_valid=None, scale=None):
    """A block of queries over the 8-bit cache: q bf16 (B,Sq,H,128) at positions q_start + i; cached_key / cached_value
    uint8 (B,Sk,H,128) and key_scale / value_scale f32 (B,Sk,H) as written by ops.kv8_cache_write (views of a longer cache
    are fine: only the innermost stride must be 1); key_valid u8 (B,Sk) or None, rows may be strided.  Key j is visible to
    query i iff j <= q_start + i and key_valid[b, j] != 0.  The bytes are dequantised on their way into LDS; no bf16 copy
    of the cache is made.  Returns normalised partials (o_parts f32 [k_splits,B,Sq,H,D], lse_parts f32 [k_splits,B,H,Sq])
    -- merge with ops.attn_combine."""
    return _kvq_attn_prefill(KV8, "lwm_attn_prefill_kv8", _capi.LwmKv8PrefillArgs, q, cached_key, key_scale, cached_value,
                             value_scale, q_start=q_start, k_splits=k_splits, key_valid=key_valid, scale=scale)
