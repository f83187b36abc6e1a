"""Test helper of the bf16 convolution (lwm_conv2d_nhwc_bf16, lwm_amd/csrc/vqgan_conv_bf16.h): the pack in numpy, a ctypes
wrapper over the host-emulated library, the fp64 reference of the contract with its magnitude sum, the contract's cases
and the rounded-operand oracle of the model-level tests.  TEST INFRASTRUCTURE ONLY.

The contract (include/lwm_hip.h): with x^ = bf16_rne(x), w^ = bf16_rne(w), K = KH KW Cin and y64 the fp64 convolution of
x^ and w^ plus bias plus residual,
  1. integer data (x in [-4, 4], w in [-8, 8], bias and residual in [-300, 300]): every partial sum is an integer below
     2^24 (K 64 |x w| <= 2304 * 32 < 2^17 at the widest case here), so the output equals oracle.vqgan_ref.conv2d exactly;
  2. random data: |y - y64| <= (K + 2) 2^-23 (sum |x^ w^| + |bias| + |residual|) element by element -- one rounding of
     relative size 2^-24 per accumulation step at worst, with a factor two of room: the bound tests/_rows_cases.py holds
     lwm_gemm_rows_fused_* to on the same instruction."""
import contextlib
import ctypes as C

import numpy as np

from lwm_amd import _capi
from oracle import vqgan_ref as R
from oracle.attention_ref import round_bf16, to_bf16_bits

# (B, H, W, Cin, Cout, k, conv options, residual?): the smallest shapes at which each part can go wrong
CASES = [
    (1, 12, 12, 32, 128, 3, {}, False),                                       # ragged last pixel tile
    (2, 10, 6, 64, 160, 3, {}, False),                                        # two images in one tile, ragged Cout tile
    (1, 8, 8, 96, 32, 3, {}, False),                                          # three K steps (odd: the double buffer), narrowest Cout
    (1, 16, 16, 64, 64, 1, {}, False),                                        # 1x1
    (1, 16, 16, 32, 128, 3, dict(stride=2, pad=0, out_hw=(8, 8)), False),     # Downsample
    (1, 31, 33, 32, 128, 3, dict(stride=2, pad=0, out_hw=(15, 16)), False),   # ... with odd sizes
    (1, 6, 6, 32, 128, 3, dict(up_shift=1), False),                           # Upsample
    (3, 8, 24, 64, 128, 3, {}, True),                                         # a tile that straddles images
    (1, 16, 48, 256, 256, 3, {}, True),                                       # the widest K; 128 x 128 tiles on a small machine
    (1, 16, 24, 128, 128, 3, dict(up_shift=1), True),
]
IDS = [f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}-k{c[5]}" + "".join(f"-{k}" for k in c[6]) + ("-res" if c[7] else "") for c in CASES]


def out_shape(B, H, W, Cout, k, kw):
    up, stride = kw.get("up_shift", 0), kw.get("stride", 1)
    pad = kw.get("pad", (k - 1) // 2)
    return (B,) + tuple(kw.get("out_hw", (((H << up) + 2 * pad - k) // stride + 1, ((W << up) + 2 * pad - k) // stride + 1))) + (Cout,)


def int_case(seed, B, H, W, Cin, Cout, k, kw, res):
    """contract point 1: integer data -> (x, w, bias, residual or None)"""
    g = np.random.default_rng(seed)
    f = lambda lo, hi, shape: g.integers(lo, hi + 1, shape).astype(np.float32)
    return (f(-4, 4, (B, H, W, Cin)), f(-8, 8, (k, k, Cin, Cout)), f(-300, 300, (Cout,)),
            f(-300, 300, out_shape(B, H, W, Cout, k, kw)) if res else None)


def random_case(seed, B, H, W, Cin, Cout, k, kw, res):
    """contract point 2: x ~ N(0, 1), w ~ N(0, 1 / K) (neither representable in bf16), bias and residual ~ N(0, 1)"""
    g = np.random.default_rng(seed)
    n = lambda shape: g.standard_normal(shape).astype(np.float32)
    return (n((B, H, W, Cin)), n((k, k, Cin, Cout)) / np.float32(np.sqrt(k * k * Cin)), n((Cout,)),
            n(out_shape(B, H, W, Cout, k, kw)) if res else None)


def pack(w):
    """HWIO f32 kernel -> the documented pack, uint16 bf16 bits [KH*KW][Cin/8][Cout][8], rounded to nearest even"""
    KH, KW, Cin, Cout = w.shape
    return np.ascontiguousarray(to_bf16_bits(w).reshape(KH * KW, Cin // 8, 8, Cout).transpose(0, 1, 3, 2))


def _patches(x, KH, KW, stride, pad, up_shift, Ho, Wo):
    """im2col of the virtual input (nearest upsample, zeros outside): (B, Ho, Wo, KH*KW*Cin), taps in (kh, kw) order"""
    xv = x.repeat(1 << up_shift, axis=1).repeat(1 << up_shift, axis=2)
    B, Hv, Wv, Cin = xv.shape
    hh, ww = (Ho - 1) * stride + KH, (Wo - 1) * stride + KW
    xp = np.zeros((B, max(hh, Hv + pad), max(ww, Wv + pad), Cin), xv.dtype)
    xp[:, pad:pad + Hv, pad:pad + Wv] = xv
    cols = [xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride] for kh in range(KH) for kw in range(KW)]
    return np.concatenate(cols, axis=-1)


def ref64(x, w, bias=None, residual=None, *, stride=1, pad=None, up_shift=0, out_hw=None):
    """-> (y64, mag): the fp64 convolution of the ROUNDED operands + bias + residual, and sum |x^ w^| + |bias| + |residual|"""
    KH, KW, Cin, Cout = w.shape
    if pad is None:
        pad = (KH - 1) // 2
    Ho, Wo = out_hw if out_hw is not None else out_shape(*x.shape[:3], Cout, KH, dict(stride=stride, pad=pad, up_shift=up_shift))[1:3]
    P = _patches(round_bf16(x).astype(np.float64), KH, KW, stride, pad, up_shift, Ho, Wo)
    Wm = round_bf16(w).astype(np.float64).reshape(KH * KW * Cin, Cout)
    y, mag = P @ Wm, np.abs(P) @ np.abs(Wm)
    for t in (bias, residual):
        if t is not None:
            y, mag = y + t.astype(np.float64), mag + np.abs(t.astype(np.float64))
    return y, mag


def bound(w, mag):
    return (w.shape[0] * w.shape[1] * w.shape[2] + 2) * 2.0 ** -23 * mag


def check_contract2(y, x, w, bias=None, residual=None, **kw):
    """contract point 2 on one output; returns the worst error over its bound (for the test to print)"""
    y64, mag = ref64(x, w, bias, residual, **kw)
    assert y.shape == y64.shape
    err, lim = np.abs(y.astype(np.float64) - y64), bound(w, mag)
    worst = float((err / np.maximum(lim, 1e-300)).max())
    assert (err <= lim).all(), f"worst error / bound = {worst:.3f} at {np.unravel_index(np.argmax(err / np.maximum(lim, 1e-300)), err.shape)}"
    return worst


def guarded(a, fill, guard=4096):
    """`a` inside a larger 16-byte aligned buffer whose every other byte is `fill` -> (view of a, whole buffer bytes)"""
    a = np.ascontiguousarray(a)
    raw = np.full(a.nbytes + 2 * guard + 16, fill, np.uint8)
    off = guard + (-(raw.ctypes.data + guard)) % 16
    view = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    view[...] = a
    return view, raw, off


class DevGuarded:
    """a device tensor between two guard bands of 0xFF bytes (NaN patterns in f32 and bf16); `.t` is the tensor inside"""
    GUARD = 4096

    def __init__(self, shape, dtype, init=None):
        import torch
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n + 2 * self.GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.raw[self.GUARD:self.GUARD + n].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.raw[:self.GUARD] == 0xFF).all() and (self.raw[-self.GUARD:] == 0xFF).all())


def emu_conv(x, w, bias=None, residual=None, *, stride=1, pad=None, up_shift=0, out_hw=None, clip=False, hidden=None):
    """lwm_conv2d_nhwc_bf16 of the host-emulated library.  w: the HWIO f32 kernel (packed here).  hidden: a byte value --
    every operand then lies inside a larger buffer filled with it (0xFF: NaN patterns in f32 and in bf16) and the result
    comes back with `intact`, whether all guard bytes kept their value."""
    from tests import _emu
    L = _emu.lib()
    KH, KW, Cin, Cout = w.shape
    kw = dict(stride=stride, pad=(KH - 1) // 2 if pad is None else pad, up_shift=up_shift, **({} if out_hw is None else dict(out_hw=out_hw)))
    oshape = out_shape(x.shape[0], x.shape[1], x.shape[2], Cout, KH, kw)
    ops = [np.ascontiguousarray(x, np.float32), pack(w), None if bias is None else np.ascontiguousarray(bias, np.float32),
           None if residual is None else np.ascontiguousarray(residual, np.float32), np.zeros(oshape, np.float32)]
    raws = []
    for i, a in enumerate(ops):
        if a is None:
            continue
        if hidden is None:
            al = _emu.aligned(a.shape, a.dtype)
            al[...] = a
            ops[i] = al
        else:
            ops[i], raw, off = guarded(a, hidden)
            raws.append((raw, off, a.nbytes))
    xa, wa, ba, ra, y = ops
    a = _capi.LwmConvArgs(xa.ctypes.data, wa.ctypes.data, _emu._ptr(ba), _emu._ptr(ra), y.ctypes.data, x.shape[0], x.shape[1],
                          x.shape[2], Cin, Cout, KH, KW, stride, kw["pad"], up_shift, oshape[1], oshape[2], int(clip))
    _capi.check(L, L.lwm_conv2d_nhwc_bf16(C.byref(a), None), "lwm_conv2d_nhwc_bf16")
    if hidden is None:
        return y
    intact = all((raw[:off] == hidden).all() and (raw[off + n:] == hidden).all() for raw, off, n in raws)
    return y.copy(), intact


def rne_case():
    """contract point 3: a 1x1 identity convolution, 32 channels, over normal numbers that include bf16 ties in both
    directions (1 + 2^-8 rounds DOWN to the even 1, 1 + 3 2^-8 rounds UP to the even 1 + 2^-6) and their negatives"""
    g = np.random.default_rng(7)
    x = (g.standard_normal((1, 4, 8, 32)) * np.exp2(g.integers(-20, 20, (1, 4, 8, 32)))).astype(np.float32)
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23,
                     1 + 2.0 ** -8 - 2.0 ** -24], np.float32)
    x.reshape(-1)[:ties.size * 5:5] = ties
    x.reshape(-1)[-ties.size:] = ties * np.float32(2.0 ** 40)
    assert np.isfinite(x).all() and (np.abs(x[x != 0]) >= 2.0 ** -126).all()
    return x, np.eye(32, dtype=np.float32).reshape(1, 1, 32, 32)


@contextlib.contextmanager
def rounded_operand_oracle():
    """oracle.vqgan_ref with x and w rounded to bf16 (nearest even) in front of every convolution the bf16 route serves
    (Cin % 32 == 0 and Cout % 32 == 0); everything else -- the convolution's f32 fmaf chain, GroupNorm, SiLU, the
    quantiser -- is the oracle's own.  R.encoder / R.decoder / R.encode / R.decode inside the block are that oracle."""
    plain = R.conv2d

    def conv2d(x, w, bias=None, residual=None, **kw):
        if w.shape[2] % 32 == 0 and w.shape[3] % 32 == 0:
            x, w = round_bf16(x), round_bf16(w)
        return plain(x, w, bias, residual, **kw)
    R.conv2d = conv2d
    try:
        yield R
    finally:
        R.conv2d = plain
