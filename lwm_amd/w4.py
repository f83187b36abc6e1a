"""4-bit (MXFP4: e2m1 codes, e8m0 block scales) decode weights: the torch-tensor front end of lwm_w4_quantise and
lwm_gemv_fused_w4 (include/lwm_hip.h, "4-bit decode weights"; csrc/gemv_w4.h).  As everything in lwm_amd: hand-written HIP
kernels on the current torch stream, no PyTorch / CPU fallback.  w4_dequant alone is a torch expression: the byte layout
written down, and the yardstick of the tests."""
import torch

from . import _capi
from ._lib import lib
from .kv4 import E2M1_VALUES
from .llama_ops import ProjFormat, _fused_call, _is_dev
from .ops import _stream_ptr

BLOCK = 32             # rows of K per scale byte = the rows one wave of the GEMV walks


class W4Kernel:
    """The 4-bit pack of one (K, N) kernel: `q` uint8 (K / 4, N / 8, 16) e2m1 nibble pairs (slot [k4][n8]: rows 4 k4 .. 4 k4 + 3
    of columns 8 n8 .. 8 n8 + 7, byte 4 j + b = row 4 k4 + j, column 8 n8 + 2 b low and 8 n8 + 2 b + 1 high), `scale` uint8
    (K / 32, N) e8m0 bytes, the shape, and `stamp` = (_version, data_ptr) of the parameter AFTER it was rounded in place -- a
    pack whose parameter has changed since is stale (`check`)."""
    __slots__ = ("q", "scale", "shape", "stamp")

    def __init__(self, q, scale, shape, stamp):
        self.q, self.scale, self.shape, self.stamp = q, scale, tuple(shape), stamp

    def check(self, kernel, name="kernel"):
        if (kernel._version, kernel.data_ptr()) != self.stamp:
            raise RuntimeError(f"{name}: the parameter changed after its fp4 decode pack was made (the pack holds the old "
                               f"weights): call quantize_decode_weights('fp4') again, or drop_decode_weights()")
        return self


def quantise_weight(kernel):
    """kernel: a contiguous bf16 (K, N) ROCm tensor (K % 32 == 0, K <= 12288, N % 8 == 0), ROUNDED IN PLACE to the values
    its 4-bit pack stands for, bf16(e2m1(q) * s) -> W4Kernel.  One pass over the kernel on the device."""
    if not _is_dev(kernel) or kernel.dim() != 2 or kernel.dtype != torch.bfloat16 or not kernel.is_contiguous():
        raise ValueError("quantise_weight: kernel must be a contiguous bf16 (K, N) ROCm tensor")
    K, N = kernel.shape
    if K < 32 or K % 32 or K > 12288 or N < 8 or N % 8:
        raise ValueError(f"quantise_weight: kernel of shape {(K, N)}: need K % 32 == 0, K <= 12288 and N % 8 == 0")
    q = torch.empty((K // 4, N // 8, 16), dtype=torch.uint8, device=kernel.device)
    scale = torch.empty((K // BLOCK, N), dtype=torch.uint8, device=kernel.device)
    L = lib()
    with torch.no_grad():
        data = kernel.detach()
        _capi.check(L, L.lwm_w4_quantise(data.data_ptr(), q.data_ptr(), scale.data_ptr(), data.data_ptr(), K, N, _stream_ptr()),
                    "lwm_w4_quantise")
        # (the kernel wrote behind torch's back: count it as the in-place edit it is -- w8.quantise_weight)
        torch.autograd.graph.increment_version(data)
    return W4Kernel(q, scale, (K, N), (kernel._version, kernel.data_ptr()))


def w4_dequant(q, scale, shape):
    """The numbers a 4-bit pack holds, as bf16 (K, N): e2m1(code) * 2^(scale byte - 127), exactly (2 significant bits times
    a power of two).  q uint8 (K / 4, N / 8, 16), scale uint8 (K / 32, N).  A torch table lookup for tests and debugging --
    the GEMV never materialises it."""
    K, N = shape
    if K % 32 or N % 8 or q.dtype != torch.uint8 or scale.dtype != torch.uint8 or tuple(q.shape) != (K // 4, N // 8, 16) or \
            tuple(scale.shape) != (K // BLOCK, N):
        raise ValueError(f"w4_dequant: expected uint8 nibble pairs ({K // 4}, {N // 8}, 16) and uint8 e8m0 bytes ({K // BLOCK}, {N})")
    table = torch.tensor(E2M1_VALUES, dtype=torch.float64, device=q.device)
    rows = q.reshape(K // 4, N // 8, 4, 4)                                                # [k4][n8][j][b]
    codes = torch.stack((rows & 15, rows >> 4), dim=-1)                                   # [k4][n8][j][b][nibble]: column 2 b + nibble
    codes = codes.permute(0, 2, 1, 3, 4).reshape(K, N).long()                             # row 4 k4 + j, column 8 n8 + 2 b + nibble
    s = torch.exp2(scale.to(torch.float64) - 127.0).repeat_interleave(BLOCK, dim=0)
    return (table[codes] * s).to(torch.bfloat16)


def _pack_matrix(i, p, x, K):
    if not isinstance(p, W4Kernel):
        raise ValueError(f"gemv_fused_w4: packs[{i}] must be a W4Kernel (quantise_weight)")
    Kp, N = p.shape
    q, s = p.q, p.scale
    if Kp != K or K % 32 or N % 8 or not _is_dev(q) or q.device != x.device or q.dtype != torch.uint8 or \
            tuple(q.shape) != (K // 4, N // 8, 16) or not q.is_contiguous():
        raise ValueError(f"gemv_fused_w4: packs[{i}].q must be a contiguous uint8 ({K // 4}, N / 8, 16) tensor on {x.device}")
    if not _is_dev(s) or s.device != x.device or s.dtype != torch.uint8 or tuple(s.shape) != (K // BLOCK, N) or not s.is_contiguous():
        raise ValueError(f"gemv_fused_w4: packs[{i}].scale must be a contiguous uint8 ({K // BLOCK}, {N}) tensor on {x.device}")
    return int(N)


def _pack_fill(a, i, p):
    a.w[i], a.w_scale[i] = p.q.data_ptr(), p.scale.data_ptr()


# (no lwm_gemm_rows_fused_* entry over 4-bit packs: steps of more than 4 rows stream the rounded bf16 parameters)
W4 = ProjFormat(_capi.LwmGemvW4Args, ("lwm_gemv_fused_w4", None), "gemv_fused_w4", ("gemv_fused_w4", None), "pack", _pack_matrix,
                _pack_fill, True)


def gemv_fused_w4(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemv_fused over 4-bit packs (lwm_gemv_fused_w4): x (rows <= 4, K) bf16 against 1..3 W4Kernel packs that
    share it.  norm = (ss (rows, n <= 64) f32, weight (K,) bf16, eps): RMSNorm on load; residual (rows, N) bf16 (one pack):
    y = bf16(bf16(x @ W) + residual); want_ss: also the (rows, N / 128) partial sums of squares of y.  -> [y_i] or
    ([y_i], ss).  Bit for bit gemv_fused on the rounded kernels."""
    return _fused_call(W4, False, x, packs, norm, residual, want_ss, out_dtype)
