"""The opt-in second precision of the VQGAN convolutions (lwm_conv2d_nhwc_bf16, csrc/vqgan_conv_bf16.h): operands
rounded to bf16, products exact, f32 accumulation.  `lwm_amd.ops` re-exports both functions; they are the mirror of
`ops.conv2d_nhwc` and apply its operator-boundary checks (tests/test_op_boundary_conv_bf16.py)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi


class ConvPackBF16:
    """A convolution kernel in the layout the bf16 kernel reads (include/lwm_hip.h): `data`, bf16 [KH*KW][Cin/8][Cout][8]
    on the device, and `shape` = (KH, KW, Cin, Cout) of the HWIO kernel it was made from."""
    __slots__ = ("data", "shape")

    def __init__(self, data, shape):
        self.data, self.shape = data, tuple(int(s) for s in shape)


def conv_pack_bf16(w):
    """HWIO f32 kernel (KH,KW,Cin,Cout) on the device -> ConvPackBF16.  A torch expression, run once when the weights are
    loaded; the rounding is torch's f32 -> bf16 cast, round to nearest even.  Cin % 32 == 0 and Cout % 32 == 0."""
    if w.dim() != 4:
        raise ValueError("conv_pack_bf16: w must be (KH,KW,Cin,Cout)")
    _ops._f32c(w, "w")
    KH, KW, Cin, Cout = w.shape
    if Cin % 32 or Cout % 32:
        raise ValueError(f"conv_pack_bf16: Cin={Cin} Cout={Cout}: the bf16 convolution needs multiples of 32 "
                         f"(conv2d_nhwc serves the rest)")
    data = w.to(torch.bfloat16).reshape(KH * KW, Cin // 8, 8, Cout).permute(0, 1, 3, 2).contiguous()
    return ConvPackBF16(data, (KH, KW, Cin, Cout))


def conv2d_nhwc_bf16(x, pack, bias=None, residual=None, *, stride=1, pad=None, up_shift=0, out_hw=None,
                     clip=False, out=None):
    """ops.conv2d_nhwc with the kernel given as a ConvPackBF16 (lwm_conv2d_nhwc_bf16): x, bias, residual and the result
    stay f32; x is rounded to bf16 inside the kernel.  Same geometry arguments, same checks."""
    if not isinstance(pack, ConvPackBF16):
        raise ValueError("conv2d_nhwc_bf16: pack must come from conv_pack_bf16")
    if x.dim() != 4:
        raise ValueError("conv2d_nhwc_bf16: x must be (B,H,W,Cin)")
    B, Hin, Win, Cin = x.shape
    KH, KW, Cin2, Cout = pack.shape
    if Cin2 != Cin:
        raise ValueError(f"conv2d_nhwc_bf16: kernel expects {Cin2} input channels, x has {Cin}")
    if pad is None:
        pad = (KH - 1) // 2
    Hv, Wv = Hin << up_shift, Win << up_shift
    if out_hw is None:
        out_hw = ((Hv + 2 * pad - KH) // stride + 1, (Wv + 2 * pad - KW) // stride + 1)
    Ho, Wo = out_hw
    px = _ops._f32c(x, "x")
    w = pack.data
    if not w.is_cuda or w.dtype != torch.bfloat16 or not w.is_contiguous() or w.device != x.device or \
            tuple(w.shape) != (KH * KW, Cin // 8, Cout, 8):
        raise ValueError(f"pack: expected a contiguous bf16 tensor of shape {(KH * KW, Cin // 8, Cout, 8)} on {x.device}")
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    if residual is not None and tuple(residual.shape) != tuple(out.shape):
        raise ValueError("conv2d_nhwc_bf16: residual shape mismatch")
    a = _capi.LwmConvArgs(px, w.data_ptr(),
                          None if bias is None else _ops._f32c(bias, "bias", (Cout,), x),
                          None if residual is None else _ops._f32c(residual, "residual", like=x),
                          _ops._f32c(out, "out", (B, Ho, Wo, Cout), x), B, Hin, Win, Cin, Cout, KH, KW, stride, pad, up_shift,
                          Ho, Wo, int(bool(clip)))
    L = _ops.lib()
    _capi.check(L, L.lwm_conv2d_nhwc_bf16(C.byref(a), _ops._stream_ptr()), "lwm_conv2d_nhwc_bf16")
    return out


from . import ops as _ops      # noqa: E402  (at the end: ops re-exports the two functions above)
