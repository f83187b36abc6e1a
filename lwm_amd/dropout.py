"""Residual and embedding dropout of the training path as one differentiable operator over the HIP kernels of
lwm_amd/csrc/dropout.h (lwm_dropout_add_* / lwm_dropout_bwd_*; the mask rule is stated in include/lwm_hip.h, "dropout").
`lwm_amd.llama_ops.dropout_add` is this module's; the sites that call it are lwm_amd/llama.py's (DropoutState).

No CPU path: tensors must be on the ROCm device, bf16 or float32."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from ._lib import lib
from .ops import _stream_ptr

_DTYPES = (torch.bfloat16, torch.float32)


def dropout_threshold(p):
    """p in [0, 1) -> (thr16, inv): thr16 = round(p * 65536), the integer the kernel compares 16 random bits against -- the
    drop probability is EXACTLY thr16 / 65536 (p = 0.1: 6554 / 65536) -- and inv = the f32 nearest to 1 / (1 - thr16 / 65536),
    from f64."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout: p = {p!r} must lie in [0, 1)")
    thr16 = int(p * 65536.0 + 0.5)
    if thr16 > 65535:
        raise ValueError(f"dropout: p = {p!r} rounds to a drop probability of 1 (the largest is 65535 / 65536)")
    return thr16, float(np.float32(1.0 / (1.0 - thr16 / 65536.0)))


def _u32(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < (1 << 32):
        raise ValueError(f"dropout_add: {what} = {v!r} must be an integer in [0, 2^32)")
    return int(v)


def _dropout_launch(kind, x, res, y, sc):
    """lwm_dropout_<kind>_bf16 / _f32 on contiguous (B, S, C) tensors; sc = (thr16, inv, key0, key1, site, s_offset)"""
    a = _capi.LwmDropoutArgs()
    a.x, a.res, a.y = x.data_ptr(), None if res is None else res.data_ptr(), y.data_ptr()
    a.B, a.S, a.C = x.shape
    a.thr16, a.inv, a.key0, a.key1, a.site, a.s_offset = sc
    L = lib()
    fn = getattr(L, f"lwm_dropout_{kind}_{'f32' if x.dtype == torch.float32 else 'bf16'}")
    _capi.check(L, fn(C.byref(a), _stream_ptr()), f"lwm_dropout_{kind}")


class _DropoutAdd(torch.autograd.Function):
    """y = residual + dropout(x).  Saves NO tensor: the mask is a function of the scalars, and the backward launches the
    backward kernel with the same ones."""

    @staticmethod
    def forward(ctx, x, residual, sc):
        y = torch.empty_like(x)
        _dropout_launch("add", x, residual, y, sc)
        ctx.sc, ctx.has_res = sc, residual is not None
        return y

    @staticmethod
    def backward(ctx, g):
        dx = None
        if ctx.needs_input_grad[0]:
            gc = g.contiguous()
            dx = torch.empty_like(gc)
            _dropout_launch("bwd", gc, None, dx, ctx.sc)
        return dx, (g if ctx.has_res else None), None


def dropout_add(x, residual, p, rng, site, s_offset=0):
    """residual + dropout(x) in one launch (residual None: dropout(x)): the residual / MLP / embedding dropout of the
    reference's training step (lwm/llama.py:423 and :618, :656-660, :998 and :1017) on contiguous (B, S, C) tensors, bf16 or
    f32, C % 8 == 0.  An element is dropped with probability thr16 / 65536, thr16 = round(p * 65536) (dropout_threshold),
    and a kept one scaled by 1 / (1 - thr16 / 65536): an f32 product, an f32 add, one rounding to the tensors' dtype.

    The mask is a function of (rng, site, b, s_offset + s, c) -- include/lwm_hip.h states the rule -- and nothing else:
    rng = (seed, step), two integers in [0, 2^32), is the Philox key as it stands; `site` (an integer in [0, 2^32)) tells
    the call sites of one step apart; s_offset is the row of the whole sequence that row 0 of x is, so a chunk of rows
    gets the bits the whole tensor would.  Nothing is saved for the backward, which regenerates the mask; the gradient of
    `residual` is the incoming gradient itself.  The masks are this build's own stream, not jax's threefry bits."""
    if not torch.is_tensor(x) or x.dim() != 3 or not x.is_cuda or x.dtype not in _DTYPES or not x.is_contiguous():
        raise ValueError("dropout_add: expected a contiguous bf16 / f32 (B, S, C) ROCm tensor")
    if x.shape[-1] % 8:
        raise ValueError(f"dropout_add: C = {x.shape[-1]} must be a multiple of 8")
    if residual is not None and (not torch.is_tensor(residual) or residual.shape != x.shape or residual.dtype != x.dtype or
                                 residual.device != x.device or not residual.is_contiguous()):
        raise ValueError(f"dropout_add: residual must be a contiguous {x.dtype} tensor of x's shape {tuple(x.shape)} on {x.device}")
    thr16, inv = dropout_threshold(p)
    try:
        seed, step = rng
    except (TypeError, ValueError):
        raise ValueError(f"dropout_add: rng = {rng!r} must be (seed, step)") from None
    sc = (thr16, inv, _u32(seed, "seed"), _u32(step, "step"), _u32(site, "site"), _u32(s_offset, "s_offset"))
    if sc[5] + x.shape[1] > (1 << 32):
        raise ValueError(f"dropout_add: s_offset + S = {sc[5] + x.shape[1]} exceeds 2^32")
    return _DropoutAdd.apply(x, residual, sc)
