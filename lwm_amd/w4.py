"""4-bit (MXFP4: e2m1 codes, e8m0 block scales) decode weights: the torch-tensor front end of lwm_w4_quantise and
lwm_gemv_fused_w4 (include/lwm_hip.h, "4-bit decode weights"; csrc/gemv_w4.h).  As everything in lwm_amd: hand-written HIP
kernels on the current torch stream, no PyTorch / CPU fallback.  w4_dequant alone is a torch expression: the byte layout
written down, and the yardstick of the tests."""
import torch

from . import wpack
from ._lib import lib                   # noqa: F401  (wpack.quantise_weight calls the library through this name)
from .kv4 import E2M1_VALUES
from .llama_ops import _fused_call

FORMAT = wpack.FORMATS["fp4"]
BLOCK = 32             # rows of K per scale byte = the rows one wave of the GEMV walks


class W4Kernel(wpack.WeightPack):
    """The 4-bit pack of one (K, N) kernel: `q` uint8 (K / 4, N / 8, 16) e2m1 nibble pairs (slot [k4][n8]: rows 4 k4 .. 4 k4 + 3
    of columns 8 n8 .. 8 n8 + 7, byte 4 j + b = row 4 k4 + j, column 8 n8 + 2 b low and 8 n8 + 2 b + 1 high), `scale` uint8
    (K / 32, N) e8m0 bytes, the shape, and `stamp` = (_version, data_ptr) of the parameter AFTER it was rounded in place -- a
    pack whose parameter has changed since is stale (`check`)."""
    __slots__, fmt = (), FORMAT


def quantise_weight(kernel):
    """kernel: a contiguous bf16 (K, N) ROCm tensor (K % 32 == 0, K <= 12288, N % 8 == 0), ROUNDED IN PLACE to the values
    its 4-bit pack stands for, bf16(e2m1(q) * s) -> W4Kernel.  One pass over the kernel on the device."""
    return wpack.quantise_weight(FORMAT, kernel)


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


def gemv_fused_w4(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemv_fused over 4-bit packs (lwm_gemv_fused_w4): x (rows <= 4, K) bf16 against 1..3 W4Kernel packs that
    share it.  norm = (ss (rows, n <= 64) f32, weight (K,) bf16, eps): RMSNorm on load; residual (rows, N) bf16 (one pack):
    y = bf16(bf16(x @ W) + residual); want_ss: also the (rows, N / 128) partial sums of squares of y.  -> [y_i] or
    ([y_i], ss).  Bit for bit gemv_fused on the rounded kernels."""
    return _fused_call(FORMAT.proj, False, x, packs, norm, residual, want_ss, out_dtype)
