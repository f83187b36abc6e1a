"""What the opt-in decode-weight formats share (w8.py, w6.py, w4.py are their public faces): the description of a format
(WeightFormat, FORMATS), the pack of one kernel (WeightPack), the quantiser call and the pack checks of the fused entries.  A
further format is one more record here and one more module of one-line wrappers."""
import importlib
import sys

import torch

from . import _capi
from .llama_ops import ProjFormat, _is_dev
from .ops import _stream_ptr


class WeightFormat:
    """The record of one format.  Every name follows from its mode: fp8 -> w8, 8-bit, W8Kernel's module lwm_amd.w8,
    lwm_w8_quantise, LwmGemvW8Args, gemv_fused_w8 ...; rows=False: no lwm_gemm_rows_fused_* entry over these packs
    (proj.entries[1] is None)."""
    __slots__ = ("mode", "tag", "bits", "pack", "quantise", "shapes", "q_words", "scale_dtype", "scale_word", "proj")

    def __init__(self, mode, pack, shapes, q_words, scale_dtype, scale_word, rows=True):
        self.mode = mode                    # "fp8": what quantize_decode_weights / LWM_DECODE_WEIGHTS take, the word of the messages
        self.tag = "w" + mode[2:]           # "w8": the format's module lwm_amd.<tag> and the suffix of its entries
        self.bits = mode[2:] + "-bit"
        self.pack = pack                    # "W8Kernel": the format's WeightPack subclass, in its module
        self.quantise = f"lwm_{self.tag}_quantise"      # the quantiser entry of the library
        self.shapes = shapes                # (K, N) -> (the shape of a pack's q -- None: no pack has this K, N --, of its scale)
        self.q_words = q_words              # (K) -> q's shape as the refusals put it
        self.scale_dtype, self.scale_word = scale_dtype, scale_word
        names = (f"gemv_fused_{self.tag}", f"gemm_rows_fused_{self.tag}" if rows else None)
        self.proj = ProjFormat(getattr(_capi, f"LwmGemvW{mode[2:]}Args"), tuple(n and "lwm_" + n for n in names), names[0], names,
                               "pack", self.pack_matrix, pack_fill, True)

    @property
    def module(self):
        """the format's module, looked up at call time: its entries can be wrapped.  (Through sys.modules where it is loaded:
        the decode step asks per token, and importlib takes the import lock for a module that is there)"""
        name = f"{__package__}.{self.tag}"
        return sys.modules.get(name) or importlib.import_module(name)

    def pack_matrix(self, i, p, x, K):
        """ProjFormat.matrix: pack i of a fused call over x (rows, K) -> N_i, or a ValueError"""
        who = self.proj.who
        if not (isinstance(p, WeightPack) and p.fmt is self):
            raise ValueError(f"{who}: packs[{i}] must be a {self.pack} (quantise_weight)")
        Kp, N = p.shape
        q, s = p.q, p.scale
        q_shape, s_shape = self.shapes(K, N)
        if Kp != K or not _is_dev(q) or q.device != x.device or q.dtype != torch.uint8 or tuple(q.shape) != q_shape or \
                not q.is_contiguous():
            raise ValueError(f"{who}: packs[{i}].q must be a contiguous uint8 {self.q_words(K)} tensor on {x.device}")
        if not _is_dev(s) or s.device != x.device or s.dtype != self.scale_dtype or tuple(s.shape) != s_shape or not s.is_contiguous():
            raise ValueError(f"{who}: packs[{i}].scale must be a contiguous {self.scale_word} ({s_shape[0]}, {N}) tensor on {x.device}")
        return int(N)


class WeightPack:
    """The pack of one (K, N) kernel: `q`, `scale` (the layouts: w8.py, w6.py, w4.py), the shape, and `stamp` = (_version,
    data_ptr) of the parameter AFTER it was rounded in place -- a pack whose parameter has changed since is stale (`check`).
    The subclasses W8Kernel, W6Kernel, W4Kernel carry their format as `fmt`."""
    __slots__ = ("q", "scale", "shape", "stamp")

    def __init__(self, q, scale, shape, stamp):
        self.q, self.scale, self.shape, self.stamp = q, scale, tuple(shape), stamp

    def check(self, kernel, name="kernel"):
        if (kernel._version, kernel.data_ptr()) != self.stamp:
            mode = self.fmt.mode
            raise RuntimeError(f"{name}: the parameter changed after its {mode} decode pack was made (the pack holds the old "
                               f"weights): call quantize_decode_weights({mode!r}) again, or drop_decode_weights()")
        return self


def quantise_weight(fmt, kernel):
    """kernel: a contiguous bf16 (K, N) ROCm tensor (K % 32 == 0, K <= 12288, N % 8 == 0), ROUNDED IN PLACE to the values its
    pack of `fmt` stands for -> that pack.  One pass over the kernel on the device."""
    if not _is_dev(kernel) or kernel.dim() != 2 or kernel.dtype != torch.bfloat16 or not kernel.is_contiguous():
        raise ValueError("quantise_weight: kernel must be a contiguous bf16 (K, N) ROCm tensor")
    K, N = kernel.shape
    if K < 32 or K % 32 or K > 12288 or N < 8 or N % 8:
        raise ValueError(f"quantise_weight: kernel of shape {(K, N)}: need K % 32 == 0, K <= 12288 and N % 8 == 0")
    q_shape, s_shape = fmt.shapes(K, N)
    q = torch.empty(q_shape, dtype=torch.uint8, device=kernel.device)
    scale = torch.empty(s_shape, dtype=fmt.scale_dtype, device=kernel.device)
    L = fmt.module.lib()                # (the module's own name for the library: what a test wraps to watch its calls)
    with torch.no_grad():
        data = kernel.detach()
        _capi.check(L, getattr(L, fmt.quantise)(data.data_ptr(), q.data_ptr(), scale.data_ptr(), data.data_ptr(), K, N, _stream_ptr()),
                    fmt.quantise)
        # (the kernel wrote behind torch's back: count it as the in-place edit it is, so that copies kept while the
        # parameter is "unchanged" -- llama_ops._as_dtype -- are made again)
        torch.autograd.graph.increment_version(data)
    return getattr(fmt.module, fmt.pack)(q, scale, (K, N), (kernel._version, kernel.data_ptr()))


def pack_fill(a, i, p):
    a.w[i], a.w_scale[i] = p.q.data_ptr(), p.scale.data_ptr()


def _mx_shapes(slot):
    """the MX formats: q (K / 4, N / 8, slot bytes), for K % 32 == 0 and N % 8 == 0 only; scale (K / 32, N)"""
    return lambda K, N: (None if K % 32 or N % 8 else (K // 4, N // 8, slot), (K // 32, N))


# (128, 32 = w8.GROUP, w6.BLOCK / w4.BLOCK; 24 = w6.SLOT)
FORMATS = {f.mode: f for f in (
    WeightFormat("fp8", "W8Kernel", lambda K, N: ((K, N), ((K + 127) // 128, N)), lambda K: f"({K}, N)", torch.float32, "f32"),
    WeightFormat("fp6", "W6Kernel", _mx_shapes(24), lambda K: f"({K // 4}, N / 8, 24)", torch.uint8, "uint8"),
    WeightFormat("fp4", "W4Kernel", _mx_shapes(16), lambda K: f"({K // 4}, N / 8, 16)", torch.uint8, "uint8", rows=False),
)}
