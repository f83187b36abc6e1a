"""Thin torch-tensor front end of the C ABI (include/lwm_hip.h).

Every function here enqueues hand-written HIP kernels from liblwm_hip.so on the
current torch stream.  There is no PyTorch / CPU fallback: tensors must be
bf16/f32 on a ROCm device and the shared library must be present.
"""
import ctypes as C
import os
import math
import typing

import torch

from . import _capi
from ._lib import lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(stream=None):
    """The HIP stream the launches go to: torch's current stream of the current device (the raw-handle query is
    ~10x cheaper than building a torch.cuda.Stream object -- a decode step asks some 50 times per token)."""
    if stream is not None:
        return C.c_void_p(stream.cuda_stream)
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t4(t, name, dtype=None, shape=None, like=None):
    """(B,S,H,D) bf16 -- or f32, the fp32 flavour of the op -- device tensor -> LwmTensor4; `dtype`: the one it must have;
    `shape`: the one it must have; `like`: a tensor whose device it must share"""
    if t is None:
        return _capi.LwmTensor4(None, 0, 0, 0)
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a ROCm device tensor (lwm_amd has no CPU path)")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name}: expected a tensor on {like.device}, got {t.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype not in ((torch.bfloat16, torch.float32) if dtype is None else (dtype,)) or t.dim() != 4 or t.stride(3) != 1:
        raise ValueError(f"{name}: expected {'bf16 / f32' if dtype is None else dtype} (B,S,H,D) with contiguous D, got "
                         f"{t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return _capi.LwmTensor4(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def _entry(L, name, dtype):
    """The C entry point of an attention launch for operands of `dtype`: bf16 = the headline kernels, f32 = the
    `--dtype=fp32` flavour on the exact-f32 matrix instruction (lwm_attn_*_f32, csrc/attn_f32.h)."""
    return getattr(L, name + "_f32") if dtype == torch.float32 else getattr(L, name)


def _f32(t, name, shape=None, like=None):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or (like is not None and t.device != like.device):
        raise ValueError(f"{name}: expected a contiguous f32 device tensor" + ("" if like is None else f" on {like.device}"))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr()


def _base(q, k, v, *, q_start, k_start, causal, seg_q, seg_k, key_valid, scale, q_piece2=None, k_piece2=None):
    """q_piece2 / k_piece2 = (cut row, position of that row) -- or a list of such cuts, in ascending order: the pieces of
    LwmAttnArgs' piecewise position maps beyond the first (rows before the first cut sit at *_start + row, rows from a cut
    on at its position + (row - cut); cuts are multiples of 256 rows)"""
    a = _capi.LwmAttnArgs()
    a.q = _t4(q, "q")
    B, Sq, H, D = q.shape
    if k.dim() != 4:
        raise ValueError(f"k: expected (B,Sk,H,D), got {tuple(k.shape)}")
    Sk = k.shape[1]
    a.k, a.v = _t4(k, "k", q.dtype, (B, Sk, H, D), q), _t4(v, "v", q.dtype, (B, Sk, H, D), q)
    a.B, a.H, a.Sq, a.Sk, a.D = B, H, Sq, Sk, D
    a.q_start, a.k_start = int(q_start), int(k_start)
    cuts = lambda c: [c] if isinstance(c, tuple) else list(c)
    if q_piece2 is not None:
        _capi.set_pieces(a, "q", [(0, q_start)] + cuts(q_piece2))
    if k_piece2 is not None:
        _capi.set_pieces(a, "k", [(0, k_start)] + cuts(k_piece2))
    a.scale = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    a.causal = int(bool(causal))
    if (seg_q is None) != (seg_k is None):
        raise ValueError("seg_q and seg_k must be given together")
    if seg_q is not None:
        for n, s, L in (("seg_q", seg_q, Sq), ("seg_k", seg_k, Sk)):
            if s.dtype != torch.int32 or not s.is_contiguous() or tuple(s.shape) != (B, L) or s.device != q.device:
                raise ValueError(f"{n}: expected contiguous int32 tensor of shape {(B, L)} on {q.device}")
        a.segment_ids_q, a.segment_ids_k = seg_q.data_ptr(), seg_k.data_ptr()
    if key_valid is not None:
        if key_valid.dtype != torch.uint8 or not key_valid.is_contiguous() or \
                tuple(key_valid.shape) != (B, Sk) or key_valid.device != q.device:
            raise ValueError(f"key_valid: expected contiguous uint8 tensor of shape {(B, Sk)} on {q.device}")
        a.key_valid = key_valid.data_ptr()
    if seg_q is not None and SEGMENT_SKIP and q.dtype == torch.bfloat16:
        a._hint_src = (seg_q, seg_k, key_valid)
    return a


def _set_hints(a):
    """block-sparsity hints: whole documents of a packed batch are skipped in-kernel (the f32 kernels do not read them).
    Computed by a launch of their own, hence LAST: after every operand of the call has passed its checks."""
    src = getattr(a, "_hint_src", None)
    if src is not None:
        seg_q, seg_k, key_valid = src
        bq, bk = _cached_segment_blocks(seg_q, None), _cached_segment_blocks(seg_k, key_valid)
        a.seg_blocks_q, a.seg_blocks_k = bq.data_ptr(), bk.data_ptr()
        a._keep = (bq, bk)


def _cached_segment_blocks(seg, valid):
    """The hint table of a segment-id tensor is computed once and kept ON that tensor object (the ring
    driver hands the same slice objects to the forward, dQ and dK/dV launches of a block pair:
    lwm_amd/ring.py::_MaskSlices); an in-place edit (tensor._version) or another key_valid recomputes."""
    key = (seg._version, None if valid is None else (id(valid), valid._version))
    hit = getattr(seg, "_lwm_seg_blocks", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    blocks = segment_blocks(seg, valid)
    seg._lwm_seg_blocks = (key, blocks, valid)      # `valid` kept alive: its id is part of the key
    return blocks


SEGMENT_SKIP = True   # set False to A/B the in-kernel document skipping


def segment_blocks(seg, valid=None):
    """(min, max) segment id per block of 32 rows -> int32 (B, ceil(S/32), 2) (lwm_attn_segment_blocks)."""
    if not seg.is_cuda or seg.dtype != torch.int32 or seg.dim() != 2 or not seg.is_contiguous():
        raise ValueError("segment_blocks: seg must be a contiguous int32 (B,S) device tensor")
    if valid is not None and (valid.device != seg.device or valid.dtype != torch.uint8 or valid.shape != seg.shape or
                              not valid.is_contiguous()):
        raise ValueError(f"segment_blocks: valid must be a contiguous uint8 tensor of shape {tuple(seg.shape)} on {seg.device}")
    B, S = seg.shape
    out = torch.empty((B, (S + 31) // 32, 2), dtype=torch.int32, device=seg.device)
    L = lib()
    _capi.check(L, L.lwm_attn_segment_blocks(seg.data_ptr(), None if valid is None else valid.data_ptr(),
                                             out.data_ptr(), B, S, _stream_ptr()), "lwm_attn_segment_blocks")
    return out


def attn_fwd_block(q, k, v, *, q_start=0, k_start=0, causal=True, seg_q=None, seg_k=None,
                   key_valid=None, scale=None, out=None, lse=None, out_acc=None, lse_acc=None,
                   carry_in=False, final=True, dense_mask=None, q_piece2=None, k_piece2=None):
    """One ring step of the forward (lwm_attn_fwd).  Returns (out, lse) when
    `final`, else the updated (out_acc, lse_acc).  dense_mask: optional u8
    (B,Sq,Sk) view (last dim contiguous) ANDed with the other masks."""
    B, Sq, H, D = q.shape
    a = _base(q, k, v, q_start=q_start, k_start=k_start, causal=causal, seg_q=seg_q, seg_k=seg_k,
              key_valid=key_valid, scale=scale, q_piece2=q_piece2, k_piece2=k_piece2)
    _set_dense_mask(a, dense_mask, B, Sq, k.shape[1], q)
    if final:
        if out is None:
            out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
        if lse is None:
            lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
        a.out = _t4(out, "out", q.dtype, (B, Sq, H, D), q)
        a.lse = _f32(lse, "lse", (B, H, Sq), q)
    else:
        if out_acc is None:
            out_acc = torch.empty((B, Sq, H, D), dtype=torch.float32, device=q.device)
        if lse_acc is None:
            lse_acc = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    a.out_acc = _f32(out_acc, "out_acc", (B, Sq, H, D), q)
    a.lse_acc = _f32(lse_acc, "lse_acc", (B, H, Sq), q)
    a.carry_in = int(bool(carry_in))
    a.final_out = int(bool(final))
    _set_hints(a)
    L = lib()
    _capi.check(L, _entry(L, "lwm_attn_fwd", q.dtype)(C.byref(a), _stream_ptr()), "lwm_attn_fwd")
    return (out, lse) if final else (out_acc, lse_acc)


def _set_dense_mask(a, dense_mask, B, Sq, Sk, like=None):
    if dense_mask is None:
        return
    m = dense_mask
    if not m.is_cuda or m.dtype != torch.uint8 or tuple(m.shape) != (B, Sq, Sk) or m.stride(2) != 1 or \
            (like is not None and m.device != like.device):
        raise ValueError(f"dense_mask: expected a u8 device tensor of shape {(B, Sq, Sk)} with contiguous keys")
    a.dense_mask, a.mask_stride_b, a.mask_stride_q = m.data_ptr(), m.stride(0), m.stride(1)


def attn_fwd_splitk(q, k, v, *, k_splits, q_start=0, k_start=0, causal=False, seg_q=None, seg_k=None,
                    key_valid=None, dense_mask=None, scale=None):
    """Split-K forward for short query blocks (decode): returns normalised partials
    (o_parts f32 [k_splits,B,Sq,H,D], lse_parts f32 [k_splits,B,H,Sq]) -- merge with
    attn_combine."""
    B, Sq, H, D = q.shape
    if q.dtype != torch.bfloat16:
        raise ValueError("attn_fwd_splitk: the inference kernels take bf16 operands (the f32 flavour serves the training op)")
    a = _base(q, k, v, q_start=q_start, k_start=k_start, causal=causal, seg_q=seg_q, seg_k=seg_k,
              key_valid=key_valid, scale=scale)
    _set_dense_mask(a, dense_mask, B, Sq, k.shape[1], q)
    k_splits = max(1, int(k_splits))
    o_parts = torch.empty((k_splits, B, Sq, H, D), dtype=torch.float32, device=q.device)
    lse_parts = torch.empty((k_splits, B, H, Sq), dtype=torch.float32, device=q.device)
    a.out_acc, a.lse_acc = o_parts.data_ptr(), lse_parts.data_ptr()
    a.carry_in, a.final_out, a.k_splits = 0, 0, k_splits
    _set_hints(a)
    L = lib()
    _capi.check(L, L.lwm_attn_fwd(C.byref(a), _stream_ptr()), "lwm_attn_fwd")
    return o_parts, lse_parts


def attn_combine(o_parts, lse_parts, *, out=None, out_f32=None, lse=None, want_bf16=True):
    """Merge normalised partials (lwm_attn_combine).  Returns (out bf16 or f32, lse)."""
    if not torch.is_tensor(o_parts) or o_parts.dim() != 5:
        raise ValueError("o_parts: expected a contiguous f32 (P,B,Sq,H,D) device tensor")
    P, B, Sq, H, D = o_parts.shape
    if lse is None:
        lse = torch.empty((B, H, Sq), dtype=torch.float32, device=o_parts.device)
    if want_bf16 and out is None:
        out = torch.empty((B, Sq, H, D), dtype=torch.bfloat16, device=o_parts.device)
    if not want_bf16 and out_f32 is None:
        out_f32 = torch.empty((B, Sq, H, D), dtype=torch.float32, device=o_parts.device)
    args = (_f32(o_parts, "o_parts"), _f32(lse_parts, "lse_parts", (P, B, H, Sq), o_parts), P,
            _t4(out, "out", torch.bfloat16, (B, Sq, H, D), o_parts) if want_bf16 else _capi.LwmTensor4(None, 0, 0, 0),
            None if want_bf16 else _f32(out_f32, "out_f32", (B, Sq, H, D), o_parts),
            _f32(lse, "lse", (B, H, Sq), o_parts), B, Sq, H, D)
    L = lib()
    _capi.check(L, L.lwm_attn_combine(*args, _stream_ptr()),
                "lwm_attn_combine")
    return (out if want_bf16 else out_f32), lse


def kv_cache_write(cache, src, *, dst_row0, src_row0=0, nrows=None):
    """cache[:, dst_row0:dst_row0+nrows] = src[:, src_row0:src_row0+nrows] for (B,S,H,D) bf16 -- or f32: the copy moves
    bytes, a float row is two bf16-sized elements per value -- tensors whose (S,H,D) block is contiguous
    (lwm_kv_cache_write)."""
    for n, t in (("cache", cache), ("src", src)):
        if not t.is_cuda or t.dtype not in (torch.bfloat16, torch.float32) or t.dtype != cache.dtype or t.dim() != 4 or \
                not t[0].is_contiguous():
            raise ValueError(f"{n}: expected bf16 / f32 (B,S,H,D) device tensors of one dtype with contiguous (S,H,D)")
    B, _, H, D = cache.shape
    if src.device != cache.device or src.shape[0] != B or tuple(src.shape[2:]) != (H, D):
        raise ValueError(f"src: expected a (B,*,H,D) = ({B},*,{H},{D}) tensor on {cache.device}, got {tuple(src.shape)} on "
                         f"{src.device}")
    if nrows is None:
        nrows = src.shape[1] - src_row0
    if nrows < 0 or dst_row0 < 0 or dst_row0 + nrows > cache.shape[1] or src_row0 < 0 or src_row0 + nrows > src.shape[1]:
        raise ValueError("kv_cache_write: row range out of bounds")
    w = cache.element_size() // 2            # bf16-sized units per element
    L = lib()
    _capi.check(L, L.lwm_kv_cache_write(cache.data_ptr(), src.data_ptr(), B, cache.stride(0) * w, src.stride(0) * w,
                                        dst_row0, src_row0, nrows, H * D * w, _stream_ptr()),
                "lwm_kv_cache_write")
    return cache


def kv_cache_write_at(cache, src, index_dev, *, row_offset=0, src_row0=0, nrows=None):
    """cache[:, index + row_offset + i] = src[:, src_row0 + i] with `index` an int32 DEVICE tensor
    (lwm_kv_cache_write_at); rows that fall outside the cache are skipped."""
    for n, t in (("cache", cache), ("src", src)):
        if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 4 or not t[0].is_contiguous():
            raise ValueError(f"{n}: expected bf16 (B,S,H,D) device tensor with contiguous (S,H,D)")
    if index_dev.device != cache.device or index_dev.dtype != torch.int32 or index_dev.numel() != 1:
        raise ValueError("index_dev: expected a one-element int32 device tensor")
    B, rows, H, D = cache.shape
    if src.device != cache.device or src.shape[0] != B or tuple(src.shape[2:]) != (H, D):
        raise ValueError(f"src: expected a (B,*,H,D) = ({B},*,{H},{D}) tensor on {cache.device}, got {tuple(src.shape)} on "
                         f"{src.device}")
    if nrows is None:
        nrows = src.shape[1] - src_row0
    if nrows < 0 or src_row0 < 0 or src_row0 + nrows > src.shape[1]:
        raise ValueError("kv_cache_write_at: source row range out of bounds")
    L = lib()
    _capi.check(L, L.lwm_kv_cache_write_at(cache.data_ptr(), src.data_ptr(), B, cache.stride(0), src.stride(0),
                                           index_dev.data_ptr(), row_offset, rows, src_row0, nrows, H * D,
                                           _stream_ptr()), "lwm_kv_cache_write_at")
    return cache


class KvFormat(typing.NamedTuple):
    """What the front end knows of a quantised KV cache format (csrc/attn_decode_kvq.h; the formats themselves:
    include/lwm_hip.h).  KV8 below, lwm_amd.kv4.KV4, lwm_amd.kv6.KV6."""
    name: str                   # "kv8": the prefix of the public names and of the error messages
    kv_dtype: str               # "fp8": what init_cache / generate call it
    bits: str                   # "8-bit"
    codes: str                  # what the cache bytes are, in words
    head_bytes: int             # bytes of one head (128 elements) of one cache row
    scale_dtype: torch.dtype
    scale_tail: tuple           # the scale tensors are (B, S, H) + scale_tail
    scale_one: float            # the scale element that stands for 1 (an empty cache)
    scale_keys: tuple           # the names of the two scale tensors in a model's cache dict
    write: str                  # the three entry points
    write_at: str
    decode: str
    decode_args: type
    block_kernel: bool          # a block of queries over the cache?
    block: str = "lwm_amd.kv8:attn_prefill_kv8"      # ... then "module:function" of its front end (_kvq_block_fn below)


def _kvq_block_fn(f):
    """The front end of format f's block kernel: f(q, cached_key, key_scale, cached_value, value_scale, *, q_start,
    k_splits, key_valid) -> partials.  Imported on use (the module of a format imports this one)."""
    import importlib
    if not f.block_kernel:
        raise NotImplementedError(f"a block kernel over the {f.bits} cache is not built")
    mod, name = f.block.split(":")
    return getattr(importlib.import_module(mod), name)


KV8 = KvFormat("kv8", "fp8", "8-bit", "e4m3 bytes", 128, torch.float32, (), 1.0, ("key_scale", "value_scale"),
               "lwm_kv8_cache_write", "lwm_kv8_cache_write_at", "lwm_attn_decode_kv8", _capi.LwmKv8DecodeArgs, True)


def _kvq_check(f, cache, scale, src):
    """(code bytes (B,S,H,head_bytes) u8, scales (B,S,H)+scale_tail, bf16 source (B,*,H,128)) with contiguous rows"""
    hb = f.head_bytes
    if not cache.is_cuda or cache.dtype != torch.uint8 or cache.dim() != 4 or not cache[0].is_contiguous():
        raise ValueError(f"cache: expected a uint8 (B,S,H,{hb}) device tensor of {f.codes} with contiguous (S,H,{hb})")
    B, rows, H, last = cache.shape
    if last != hb:
        raise ValueError(f"cache: last dimension {last}; the {f.bits} cache holds heads of 128 elements in {hb} bytes")
    sshape = (B, rows, H) + f.scale_tail
    if not scale.is_cuda or scale.dtype != f.scale_dtype or tuple(scale.shape) != sshape or not scale[0].is_contiguous():
        raise ValueError(f"scale: expected a {f.scale_dtype} device tensor of shape {sshape} with contiguous rows")
    if not src.is_cuda or src.dtype != torch.bfloat16 or src.dim() != 4 or not src[0].is_contiguous() or \
            src.shape[0] != B or tuple(src.shape[2:]) != (H, 128):
        raise ValueError(f"src: expected a bf16 device tensor (B,*,H,D) = ({B},*,{H},128) with contiguous (S,H,D) "
                         f"(the {f.bits} cache quantises bf16 rows; there is no float32 flavour)")
    return B, rows, H, 128


def _kvq_cache_write(f, cache, scale, src, *, dst_row0, src_row0=0, nrows=None):
    B, rows, H, D = _kvq_check(f, cache, scale, src)
    if nrows is None:
        nrows = src.shape[1] - src_row0
    if dst_row0 < 0 or dst_row0 + nrows > rows or src_row0 < 0 or src_row0 + nrows > src.shape[1]:
        raise ValueError(f"{f.name}_cache_write: row range out of bounds")
    L = lib()
    _capi.check(L, getattr(L, f.write)(cache.data_ptr(), src.data_ptr(), B, cache.stride(0), src.stride(0), dst_row0, src_row0,
                                       nrows, H * D, scale.data_ptr(), scale.stride(0), H, _stream_ptr()), f.write)
    return cache, scale


def _kvq_cache_write_at(f, cache, scale, src, index_dev, *, row_offset=0, src_row0=0, nrows=None):
    B, rows, H, D = _kvq_check(f, cache, scale, src)
    if not index_dev.is_cuda or index_dev.dtype != torch.int32 or index_dev.numel() != 1:
        raise ValueError("index_dev: expected a one-element int32 device tensor")
    if nrows is None:
        nrows = src.shape[1] - src_row0
    if src_row0 < 0 or src_row0 + nrows > src.shape[1]:
        raise ValueError(f"{f.name}_cache_write_at: source row range out of bounds")
    L = lib()
    _capi.check(L, getattr(L, f.write_at)(cache.data_ptr(), src.data_ptr(), B, cache.stride(0), src.stride(0),
                                          index_dev.data_ptr(), row_offset, rows, src_row0, nrows, H * D, scale.data_ptr(),
                                          scale.stride(0), H, _stream_ptr()), f.write_at)
    return cache, scale


def _kvq_attn_decode(f, q, cached_key, key_scale, cached_value, value_scale, *, k_splits, dense_mask=None, scale=None):
    who = f"attn_decode_{f.name}"
    if not torch.is_tensor(q) or q.dim() != 4:
        raise ValueError(f"{who}: q: expected a bf16 (B,1,H,D) device tensor")
    B, Sq, H, D = q.shape
    if Sq != 1 or q.dtype != torch.bfloat16:
        raise ValueError(f"{who}: expected a bf16 (B,1,H,D) query (the {f.bits} cache serves one-token decode steps)")
    if D != 128:
        raise ValueError(f"{who}: head_dim {D} (the {f.bits} decode kernel is built for 128)")
    a = f.decode_args()
    a.q = _t4(q, "q", torch.bfloat16)
    Sk = cached_key.shape[1]
    cshape, sshape = (B, Sk, H, f.head_bytes), (B, Sk, H) + f.scale_tail
    sstride = (math.prod(f.scale_tail),) + (1,) * len(f.scale_tail)         # the scales of a head and the heads of a row contiguous
    for n, c, s in (("key", cached_key, key_scale), ("value", cached_value, value_scale)):
        if not c.is_cuda or c.device != q.device or c.dtype != torch.uint8 or tuple(c.shape) != cshape or c.stride(3) != 1:
            raise ValueError(f"cached_{n}: expected a uint8 tensor of shape {cshape} on {q.device} with contiguous bytes")
        if not s.is_cuda or s.device != q.device or s.dtype != f.scale_dtype or tuple(s.shape) != sshape or \
                tuple(s.stride()[2:]) != sstride:
            raise ValueError(f"{n}_scale: expected a {f.scale_dtype} tensor of shape {sshape} on {q.device} with contiguous heads")
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
        raise ValueError(f"{who}: k_splits = {k_splits} > 4096")
    a.k_splits = k_splits
    o_parts = torch.empty((k_splits, B, 1, H, D), dtype=torch.float32, device=q.device)
    lse_parts = torch.empty((k_splits, B, H, 1), dtype=torch.float32, device=q.device)
    a.out_acc, a.lse_acc = o_parts.data_ptr(), lse_parts.data_ptr()
    L = lib()
    _capi.check(L, getattr(L, f.decode)(C.byref(a), _stream_ptr()), f.decode)
    return o_parts, lse_parts


def _kvq_attn_prefill(f, entry, args, q, cached_key, key_scale, cached_value, value_scale, *, q_start, k_splits, key_valid=None,
                      scale=None):
    """A block of queries over format f's cache through the C entry point `entry`, whose argument struct is `args`
    (kv8.attn_prefill_kv8 and kv6.attn_prefill_kv6 have the contract)."""
    who = f"attn_prefill_{f.name}"
    if not torch.is_tensor(q) or q.dim() != 4:
        raise ValueError(f"{who}: q: expected a bf16 (B,Sq,H,D) device tensor")
    B, Sq, H, D = q.shape
    if q.dtype != torch.bfloat16:
        raise ValueError(f"{who}: expected a bf16 (B,Sq,H,D) query (the {f.bits} cache holds quantised bf16 rows; there is no "
                         "float32 flavour)")
    if Sq < 1 or D != 128:
        raise ValueError(f"{who}: q of shape {tuple(q.shape)}: need Sq >= 1 and head_dim 128")
    a = args()
    a.q = _t4(q, "q", torch.bfloat16)
    if not torch.is_tensor(cached_key) or cached_key.dim() != 4:
        raise ValueError(f"cached_key: expected a uint8 device tensor of shape ({B},Sk,{H},{f.head_bytes})")
    Sk = cached_key.shape[1]
    if Sk < 1:
        raise ValueError("cached_key: expected at least one cache row")
    cshape, sshape = (B, Sk, H, f.head_bytes), (B, Sk, H) + f.scale_tail
    sstride = (math.prod(f.scale_tail),) + (1,) * len(f.scale_tail)         # the scales of a head and the heads of a row contiguous
    for n, c, s in (("key", cached_key, key_scale), ("value", cached_value, value_scale)):
        if not torch.is_tensor(c) or not c.is_cuda or c.device != q.device or c.dtype != torch.uint8 or \
                tuple(c.shape) != cshape or c.stride(3) != 1:
            raise ValueError(f"cached_{n}: expected a uint8 tensor of shape {cshape} on {q.device} with contiguous bytes")
        if not torch.is_tensor(s) or not s.is_cuda or s.device != q.device or s.dtype != f.scale_dtype or \
                tuple(s.shape) != sshape or tuple(s.stride()[2:]) != sstride:
            raise ValueError(f"{n}_scale: expected a {f.scale_dtype} tensor of shape {sshape} on {q.device} with contiguous heads")
    q_start = int(q_start)
    if q_start < 0:
        raise ValueError(f"{who}: q_start = {q_start} < 0")
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
        raise ValueError(f"{who}: k_splits = {k_splits} > 4096")
    a.k_splits = k_splits
    o_parts = torch.empty((k_splits, B, Sq, H, D), dtype=torch.float32, device=q.device)
    lse_parts = torch.empty((k_splits, B, H, Sq), dtype=torch.float32, device=q.device)
    a.out_acc, a.lse_acc = o_parts.data_ptr(), lse_parts.data_ptr()
    L = lib()
    _capi.check(L, getattr(L, entry)(C.byref(a), _stream_ptr()), entry)
    return o_parts, lse_parts


def kv8_cache_write(cache, scale, src, *, dst_row0, src_row0=0, nrows=None):
    """Quantise src[:, src_row0:src_row0+nrows] (bf16) into the 8-bit cache at row dst_row0: `cache` takes the e4m3fn
    bytes, `scale` one power-of-two f32 per (row, head) (lwm_kv8_cache_write; the format: include/lwm_hip.h)."""
    return _kvq_cache_write(KV8, cache, scale, src, dst_row0=dst_row0, src_row0=src_row0, nrows=nrows)


def kv8_cache_write_at(cache, scale, src, index_dev, *, row_offset=0, src_row0=0, nrows=None):
    """The same with the destination row `index + row_offset` read from an int32 DEVICE tensor
    (lwm_kv8_cache_write_at); rows that fall outside the cache are skipped."""
    return _kvq_cache_write_at(KV8, cache, scale, src, index_dev, row_offset=row_offset, src_row0=src_row0, nrows=nrows)


def kv8_dequant(q, scale):
    """The numbers an 8-bit cache holds, as bf16: e4m3(q) * scale, exactly (4 significant bits times a power of two).
    A torch expression for tests and debugging -- the decode kernel never materialises it."""
    return (q.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1)).to(torch.bfloat16)


def attn_decode_kv8(q, cached_key, key_scale, cached_value, value_scale, *, k_splits, dense_mask=None, scale=None):
    """One query per batch row over the 8-bit cache (lwm_attn_decode_kv8): q bf16 (B,1,H,D); the cache as written by
    kv8_cache_write; dense_mask u8 (B,1,Sk) or None.  Returns normalised partials (o_parts f32 [k_splits,B,1,H,D],
    lse_parts f32 [k_splits,B,H,1]) -- merge with attn_combine."""
    return _kvq_attn_decode(KV8, q, cached_key, key_scale, cached_value, value_scale, k_splits=k_splits, dense_mask=dense_mask,
                            scale=scale)


def bwd_stats_shape(B, H, Sq):
    """Shape of the backward's row statistics for a (B, Sq, H, D) query block: per (b, h) the rows
    [-lse * log2 e | -rowsum(dout * out)], padded to a multiple of 64 queries (lwm_attn_bwd_delta_bytes)."""
    return (B, H, 2, (Sq + 63) // 64 * 64)


def attn_bwd_delta(out, dout, lse, delta=None):
    """The row statistics the backward kernels consume (lwm_attn_bwd_delta), from out, dout and the forward's lse."""
    a = _capi.LwmAttnArgs()
    a.out = _t4(out, "out")
    B, Sq, H, D = out.shape
    if delta is None:
        delta = torch.empty(bwd_stats_shape(B, H, Sq), dtype=torch.float32, device=out.device)
    a.dout = _t4(dout, "dout", out.dtype, (B, Sq, H, D), out)
    a.B, a.H, a.Sq, a.Sk, a.D = B, H, Sq, 0, D
    a.lse = _f32(lse, "lse", (B, H, Sq), out)
    a.delta = _f32(delta, "delta", bwd_stats_shape(B, H, Sq), out)
    a.delta_bytes = delta.numel() * 4
    L = lib()
    _capi.check(L, _entry(L, "lwm_attn_bwd_delta", out.dtype)(C.byref(a), _stream_ptr()), "lwm_attn_bwd_delta")
    return delta


def _bwd_base(q, k, v, dout, lse, delta, kw):
    a = _base(q, k, v, **kw)
    B, Sq, H, D = q.shape
    a.dout = _t4(dout, "dout", q.dtype, (B, Sq, H, D), q)
    a.lse = _f32(lse, "lse", (B, H, Sq), q)
    a.delta = _f32(delta, "delta", bwd_stats_shape(B, H, Sq), q)
    a.delta_bytes = delta.numel() * 4
    return a


def _acc_shape(B, Sq, H, D, head_major):
    """dq accumulator / carry: (B,Sq,H,D), or head-major (B,H,Sq,D)."""
    return (B, H, Sq, D) if head_major else (B, Sq, H, D)


# ---- dS hand-over (include/lwm_hip.h, LwmAttnArgs::ds_ws): attn_bwd_dkdv_block stores its dS in the workspace and
# attn_bwd_dq_block, called after it with the same arguments, computes dq from them in one GEMM (ring.py allots it)
def _set_ds_ws(a, ds_ws, like):
    if ds_ws is None:
        return
    if not torch.is_tensor(ds_ws) or ds_ws.device != like.device or ds_ws.dtype != torch.uint8 or not ds_ws.is_contiguous():
        raise ValueError(f"ds_ws: expected a contiguous uint8 tensor on {like.device}")
    a.ds_ws, a.ds_ws_bytes = ds_ws.data_ptr(), ds_ws.numel()


def attn_bwd_dq_block(q, k, v, dout, lse, delta, *, q_start=0, k_start=0, causal=True,
                      seg_q=None, seg_k=None, key_valid=None, scale=None, dq=None, dq_acc=None,
                      carry_in=False, final=True, acc_head_major=False, q_piece2=None, k_piece2=None, ds_ws=None):
    """ds_ws: the workspace attn_bwd_dkdv_block has just filled for the same arguments (dS hand-over), or None"""
    B, Sq, H, D = q.shape
    a = _bwd_base(q, k, v, dout, lse, delta,
                  dict(q_start=q_start, k_start=k_start, causal=causal, seg_q=seg_q, seg_k=seg_k,
                       key_valid=key_valid, scale=scale, q_piece2=q_piece2, k_piece2=k_piece2))
    if final:
        if dq is None:
            dq = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
        a.dq = _t4(dq, "dq", q.dtype, (B, Sq, H, D), q)
    elif dq_acc is None:
        dq_acc = torch.empty(_acc_shape(B, Sq, H, D, acc_head_major), dtype=torch.float32, device=q.device)
    a.dq_acc = _f32(dq_acc, "dq_acc", _acc_shape(B, Sq, H, D, acc_head_major), q)
    a.dq_acc_head_major = int(bool(acc_head_major))
    a.carry_in = int(bool(carry_in))
    a.final_out = int(bool(final))
    _set_hints(a)
    _set_ds_ws(a, ds_ws, q)
    L = lib()
    _capi.check(L, _entry(L, "lwm_attn_bwd_dq", q.dtype)(C.byref(a), _stream_ptr()), "lwm_attn_bwd_dq")
    return dq if final else dq_acc


def attn_bwd_dkdv_block(q, k, v, dout, lse, delta, *, q_start=0, k_start=0, causal=True,
                        seg_q=None, seg_k=None, key_valid=None, scale=None, dk=None, dv=None,
                        dk_acc=None, dv_acc=None, carry_in=False, final=True, q_piece2=None, k_piece2=None, ds_ws=None):
    """ds_ws: a uint8 workspace of lwm_attn_bwd_ds_bytes bytes: the kernel also stores its dS there (dS hand-over), or None"""
    B, Sk, H, D = k.shape
    a = _bwd_base(q, k, v, dout, lse, delta,
                  dict(q_start=q_start, k_start=k_start, causal=causal, seg_q=seg_q, seg_k=seg_k,
                       key_valid=key_valid, scale=scale, q_piece2=q_piece2, k_piece2=k_piece2))
    if final:
        if dk is None:
            dk = torch.empty((B, Sk, H, D), dtype=q.dtype, device=q.device)
        if dv is None:
            dv = torch.empty((B, Sk, H, D), dtype=q.dtype, device=q.device)
        a.dk, a.dv = _t4(dk, "dk", q.dtype, (B, Sk, H, D), q), _t4(dv, "dv", q.dtype, (B, Sk, H, D), q)
    else:
        if dk_acc is None:
            dk_acc = torch.empty((B, Sk, H, D), dtype=torch.float32, device=q.device)
        if dv_acc is None:
            dv_acc = torch.empty((B, Sk, H, D), dtype=torch.float32, device=q.device)
    a.dk_acc = _f32(dk_acc, "dk_acc", (B, Sk, H, D), q)
    a.dv_acc = _f32(dv_acc, "dv_acc", (B, Sk, H, D), q)
    a.carry_in = int(bool(carry_in))
    a.final_out = int(bool(final))
    _set_hints(a)
    _set_ds_ws(a, ds_ws, q)
    L = lib()
    _capi.check(L, _entry(L, "lwm_attn_bwd_dkdv", q.dtype)(C.byref(a), _stream_ptr()), "lwm_attn_bwd_dkdv")
    return (dk, dv) if final else (dk_acc, dv_acc)


def cast_f32_to_bf16(src, dst=None):
    if not src.is_cuda or src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("cast_f32_to_bf16: expected contiguous f32 device tensor")
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    elif dst.device != src.device or dst.dtype != torch.bfloat16 or not dst.is_contiguous() or dst.numel() != src.numel():
        raise ValueError(f"cast_f32_to_bf16: dst must be a contiguous bf16 tensor of {src.numel()} elements on {src.device}")
    L = lib()
    _capi.check(L, L.lwm_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), src.numel(),
                                          _stream_ptr()), "lwm_cast_f32_to_bf16")
    return dst


def sum_f32_to_bf16(srcs, dst=None):
    """bf16(((srcs[0] + srcs[1]) + ...)) -- the owner-side reduction of returned dK/dV partials."""
    srcs = list(srcs)
    if not srcs:
        raise ValueError("sum_f32_to_bf16: expected at least one source")
    for s in srcs:
        if not s.is_cuda or s.dtype != torch.float32 or not s.is_contiguous() or s.shape != srcs[0].shape or \
                s.device != srcs[0].device:
            raise ValueError("sum_f32_to_bf16: expected same-shaped contiguous f32 tensors on one device")
    if dst is None:
        dst = torch.empty(srcs[0].shape, dtype=torch.bfloat16, device=srcs[0].device)
    elif dst.device != srcs[0].device or not dst.is_contiguous() or dst.dtype not in (torch.bfloat16, torch.float32) or \
            dst.numel() != srcs[0].numel():
        raise ValueError("sum_f32_to_bf16: dst must be a contiguous bf16 (or, the fp32 flavour, f32) tensor of the same size")
    ptrs = (C.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])
    L = lib()
    if dst.dtype == torch.float32:      # f32 operands: the same ordered sum, nothing rounded (lwm_sum_f32)
        _capi.check(L, L.lwm_sum_f32(ptrs, len(srcs), dst.data_ptr(), srcs[0].numel(), _stream_ptr()), "lwm_sum_f32")
        return dst
    _capi.check(L, L.lwm_sum_f32_to_bf16(ptrs, len(srcs), dst.data_ptr(), srcs[0].numel(), _stream_ptr()),
                "lwm_sum_f32_to_bf16")
    return dst


# ---------------------------------------------------------------- VQGAN primitives
def _f32c(t, name, shape=None, like=None):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous f32 ROCm device tensor (lwm_amd has no CPU path)")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name}: expected a tensor on {like.device}, got {t.device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr()


def conv2d_nhwc(x, w, bias=None, residual=None, *, stride=1, pad=None, up_shift=0, out_hw=None,
                clip=False, out=None):
    """flax nn.Conv on NHWC f32 (lwm_conv2d_nhwc_f32).  x (B,H,W,Cin), w (KH,KW,Cin,Cout) HWIO.
    pad=None = 'SAME' for stride 1.  Downsample: stride=2, pad=0, out_hw=(H//2, W//2);
    Upsample+conv: up_shift=1."""
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError("conv2d_nhwc: x must be (B,H,W,Cin) and w (KH,KW,Cin,Cout)")
    B, Hin, Win, Cin = x.shape
    KH, KW, Cin2, Cout = w.shape
    if Cin2 != Cin:
        raise ValueError(f"conv2d_nhwc: kernel expects {Cin2} input channels, x has {Cin}")
    if pad is None:
        pad = (KH - 1) // 2
    Hv, Wv = Hin << up_shift, Win << up_shift
    if out_hw is None:
        out_hw = ((Hv + 2 * pad - KH) // stride + 1, (Wv + 2 * pad - KW) // stride + 1)
    Ho, Wo = out_hw
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    if residual is not None and tuple(residual.shape) != tuple(out.shape):
        raise ValueError("conv2d_nhwc: residual shape mismatch")
    a = _capi.LwmConvArgs(_f32c(x, "x"), _f32c(w, "w", like=x),
                          None if bias is None else _f32c(bias, "bias", (Cout,), x),
                          None if residual is None else _f32c(residual, "residual", like=x),
                          _f32c(out, "out", (B, Ho, Wo, Cout), x), B, Hin, Win, Cin, Cout, KH, KW, stride, pad, up_shift,
                          Ho, Wo, int(bool(clip)))
    L = lib()
    _capi.check(L, L.lwm_conv2d_nhwc_f32(C.byref(a), _stream_ptr()), "lwm_conv2d_nhwc_f32")
    return out


def groupnorm_silu(x, gamma, beta, *, groups=32, eps=1e-6, silu=True, out=None, workspace=None):
    """flax nn.GroupNorm (+ nn.silu) over NHWC / (B, ..., C) f32 (lwm_groupnorm_silu_f32)."""
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc) if B else 0
    if gamma.numel() != Cc or beta.numel() != Cc:
        raise ValueError(f"groupnorm_silu: scale/bias have {gamma.numel()}/{beta.numel()} elements, x has {Cc} channels")
    if groups < 1 or Cc % groups:
        raise ValueError(f"groupnorm_silu: {Cc} channels do not split into {groups} groups")
    px, pg, pb = _f32c(x, "x"), _f32c(gamma, "gamma", like=x), _f32c(beta, "beta", like=x)
    if out is not None:
        _f32c(out, "out", x.shape, x)
    if workspace is not None and workspace.device != x.device:
        raise ValueError(f"workspace: expected a tensor on {x.device}")
    L = lib()
    need = L.lwm_groupnorm_workspace_bytes(B, HW, Cc, groups)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((max(need, 16) + 7) // 8, dtype=torch.float64, device=x.device)
    if out is None:
        out = torch.empty_like(x)
    _capi.check(L, L.lwm_groupnorm_silu_f32(px, pg, pb, out.data_ptr(), workspace.data_ptr(), B, HW, Cc, groups,
                                            float(eps), int(bool(silu)), _stream_ptr()),
                "lwm_groupnorm_silu_f32")
    return out


def vq_sqnorm(codebook):
    if codebook.dim() != 2:
        raise ValueError("codebook: expected a contiguous f32 (E, D) device tensor")
    E, D = codebook.shape
    pc = _f32c(codebook, "codebook")
    se = torch.empty(E, dtype=torch.float32, device=codebook.device)
    L = lib()
    _capi.check(L, L.lwm_vq_sqnorm_f32(pc, se.data_ptr(), E, D, _stream_ptr()),
                "lwm_vq_sqnorm_f32")
    return se


def vq_argmin(z, codebook, se=None):
    """First argmin over the codebook of the f32 squared distances (lwm_vq_argmin_f32)."""
    E, D = codebook.shape
    if z.shape[-1] != D:
        raise ValueError("vq_argmin: embed dim mismatch")
    if se is None:
        se = vq_sqnorm(codebook)
    N = z.numel() // D
    pz, pc, ps = _f32c(z, "z"), _f32c(codebook, "codebook", like=z), _f32c(se, "se", (E,), z)
    idx = torch.empty(z.shape[:-1], dtype=torch.int32, device=z.device)
    L = lib()
    _capi.check(L, L.lwm_vq_argmin_f32(pz, pc, ps,
                                       idx.data_ptr(), N, E, D, _stream_ptr()), "lwm_vq_argmin_f32")
    return idx


def vq_gather(codebook, idx, z=None):
    E, D = codebook.shape
    pc = _f32c(codebook, "codebook")
    if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.device != codebook.device:
        raise ValueError("vq_gather: idx must be a contiguous int32 tensor on the codebook's device")
    pz = None if z is None else _f32c(z, "z", tuple(idx.shape) + (D,), codebook)
    out = torch.empty(tuple(idx.shape) + (D,), dtype=torch.float32, device=codebook.device)
    L = lib()
    _capi.check(L, L.lwm_vq_gather_f32(pc, idx.data_ptr(), pz, out.data_ptr(),
                                       idx.numel(), E, D, _stream_ptr()), "lwm_vq_gather_f32")
    return out


def _check_top_p(top_p, who):
    """top_p of the samplers: None or 1.0 = off (-> 0.0, the C struct's "no filter"), 0 < top_p < 1 -> that float;
    anything else, NaN included, is refused by name"""
    if top_p is None:
        return 0.0
    top_p = float(top_p)
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"{who}: top_p = {top_p!r} must lie in (0, 1] (None or 1.0 = no nucleus filter)")
    return 0.0 if top_p == 1.0 else max(top_p, 2.0 ** -126)       # (the struct's float: never rounded to its 0 = off)


def sample_tokens(logits, *, temperature, top_k, seed, step_dev=None, step=0, step_base=0, cfg_scale=None, force_period=0,
                  force_token=0, done=None, eos=None, pad=0, tokens_out=None, copies=1, seq_out=None, top_p=None):
    """One decode step's next token per output row, drawn on the device (lwm_sample_tokens, csrc/sample.h): guidance
    over (2B, V) logits when cfg_scale (B,) is given (conditional rows first), temperature (0 = greedy), top-k (0 =
    none), top-p (None or 1.0 = none; 0 < top_p < 1: the nucleus rule of include/lwm_hip.h over the top-k survivors --
    an entry stays iff the softmax mass strictly above it is below top_p; anything outside (0, 1] is a ValueError), a
    Gumbel-max draw from the Philox stream of (seed, entry, row, step).  `step` is read from the one-element
    int32 device tensor step_dev (minus step_base) or taken from the host value.  force_period / force_token, done ((B,)
    uint8) / eos / pad, the int64 outputs tokens_out ((copies * B, 1): the next step's input ids) and seq_out ((B, n):
    column `step`) as include/lwm_hip.h documents.  Returns tokens_out -- allocated when not given; a call that is handed
    every output allocates nothing and can be captured in a hipGraph."""
    top_p = _check_top_p(top_p, "sample_tokens")
    if not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("sample_tokens: logits must be a (rows, V) f32 device tensor with contiguous rows")
    rows, V = logits.shape
    B = rows // 2 if cfg_scale is not None else rows

    def dev_ptr(t, name, dtype, n):
        if t is None:
            return None
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"sample_tokens: {name} must be a contiguous {dtype} device tensor of {n} elements")
        return t.data_ptr()

    if tokens_out is None:
        tokens_out = torch.empty((copies * B, 1), dtype=torch.int64, device=logits.device)
    a = _capi.LwmSampleArgs()
    a.logits, a.ld, a.rows, a.V = logits.data_ptr(), logits.stride(0), rows, V
    a.cfg_scale = dev_ptr(cfg_scale, "cfg_scale", torch.float32, B)
    a.temperature, a.top_k, a.top_p = float(temperature), int(top_k or 0), top_p
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.step_dev = dev_ptr(step_dev, "step_dev", torch.int32, 1)
    a.step_base, a.step = int(step_base), int(step)
    a.force_period, a.force_token = int(force_period), int(force_token)
    a.done = dev_ptr(done, "done", torch.uint8, B)
    a.eos, a.pad = -1 if eos is None else int(eos), int(pad)
    a.tokens, a.copies = dev_ptr(tokens_out, "tokens_out", torch.int64, copies * B), int(copies)
    if seq_out is not None:
        if not seq_out.is_cuda or seq_out.dtype != torch.int64 or seq_out.dim() != 2 or seq_out.shape[0] != B or \
                seq_out.stride(1) != 1:
            raise ValueError(f"sample_tokens: seq_out must be a ({B}, n) int64 device tensor with contiguous rows")
        a.seq, a.seq_ld, a.seq_cols = seq_out.data_ptr(), seq_out.stride(0), seq_out.shape[1]
    L = lib()
    _capi.check(L, L.lwm_sample_tokens(C.byref(a), _stream_ptr()), "lwm_sample_tokens")
    return tokens_out


# the bf16 flavour of conv2d_nhwc, with the pack of its kernel (lwm_conv2d_nhwc_bf16): a module of its own
from .vqgan_bf16 import ConvPackBF16, conv2d_nhwc_bf16, conv_pack_bf16      # noqa: E402,F401
