"""LWM_DECODE_ROWS / model.decode_rows: one-token steps of 5..N batch rows through lwm_gemm_rows_fused_bf16 / _w8 /
_w6 (csrc/gemm_rows.h; the 8-bit and 6-bit entries where the model holds such packs, w8.py / w6.py; 4-bit packs have no rows
entry -- the `proj.entries[1]` of their record in wpack.FORMATS is None -- and take the bf16 one over the rounded parameters)
instead of the library GEMMs.  Opt-in: the matrix pipe adds the products of a group of K in another
order than the library GEMM does, so the low bits of such a step change.  llama_ops re-exports everything here."""
import os

import torch

_ROWS_SCOPE = []


def parse_decode_rows(value, what="LWM_DECODE_ROWS"):
    """None / "" -> None (off); an integer 5..32 -> it; anything else is refused"""
    if value is None or value == "":
        return None
    try:
        n = int(value)
        if isinstance(value, float) and n != value:
            raise ValueError
    except (TypeError, ValueError):
        n = -1
    if not 5 <= n <= 32:
        raise ValueError(f"{what}={value!r}: unset (batches over 4 rows decode through the library GEMMs), or a row count "
                         f"5..32 up to which one-token steps run through the fused step and lwm_gemm_rows_fused_*")
    return n


def decode_rows_limit():
    """the row count up to which a no-grad bf16 one-token step leaves the library GEMMs: the model's decode_rows while one
    of its steps runs (decode_rows_scope), else LWM_DECODE_ROWS; None = 4, today's routing"""
    if _ROWS_SCOPE:
        return _ROWS_SCOPE[-1]
    return parse_decode_rows(os.environ.get("LWM_DECODE_ROWS"))


class decode_rows_scope:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        _ROWS_SCOPE.append(self.n)

    def __exit__(self, *exc):
        _ROWS_SCOPE.pop()



def rows_x_ok(x):
    """x as lwm_gemm_rows_fused_* reads it: 16 bytes at a time"""
    return x.data_ptr() % 16 == 0 and x.stride(0) % 8 == 0


def gemm_rows_fused(x, kernels, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """lwm_gemm_rows_fused_bf16: llama_ops.gemv_fused for 1..32 rows, the products on the matrix pipe (csrc/gemm_rows.h) --
    the same arguments, fusions and reduction; the kernels are still streamed once.  x must be 16-byte aligned with a row
    stride that is a multiple of 8 elements.  A row's result does not depend on how many rows ride with it."""
    from . import llama_ops
    return llama_ops._fused_call(llama_ops.BF16, True, x, kernels, norm, residual, want_ss, out_dtype)
