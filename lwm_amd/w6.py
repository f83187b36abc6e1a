"""6-bit (MXFP6: e2m3 codes, e8m0 block scales) decode weights: the torch-tensor front end of lwm_w6_quantise,
lwm_gemv_fused_w6 and lwm_gemm_rows_fused_w6 (include/lwm_hip.h, "6-bit decode weights"; csrc/gemv_w6.h, csrc/gemm_rows.h).
As everything in lwm_amd: hand-written HIP kernels on the current torch stream, no PyTorch / CPU fallback.  w6_dequant alone
is a torch expression: the byte layout written down, and the yardstick of the tests."""
import torch

from . import wpack
from ._lib import lib                   # noqa: F401  (wpack.quantise_weight calls the library through this name)
from .llama_ops import _fused_call

FORMAT = wpack.FORMATS["fp6"]
BLOCK = 32             # rows of K per scale byte = the rows one wave of the GEMV walks
SLOT = 24              # bytes of one slot: 32 codes of 6 bits, four rows of eight columns


class W6Kernel(wpack.WeightPack):
    """The 6-bit pack of one (K, N) kernel: `q` uint8 (K / 4, N / 8, 24) e2m3 codes (slot [k4][n8]: rows 4 k4 .. 4 k4 + 3 of
    columns 8 n8 .. 8 n8 + 7, code 8 j + c = row 4 k4 + j, column 8 n8 + c at bits [6 i, 6 i + 6) of the slot read as one
    little-endian integer), `scale` uint8 (K / 32, N) e8m0 bytes, the shape, and `stamp` = (_version, data_ptr) of the
    parameter AFTER it was rounded in place -- a pack whose parameter has changed since is stale (`check`)."""
    __slots__, fmt = (), FORMAT


def quantise_weight(kernel):
    """kernel: a contiguous bf16 (K, N) ROCm tensor (K % 32 == 0, K <= 12288, N % 8 == 0), ROUNDED IN PLACE to the values
    its 6-bit pack stands for, bf16(e2m3(q) * s) -> W6Kernel.  One pass over the kernel on the device."""
    return wpack.quantise_weight(FORMAT, kernel)


def w6_dequant(q, scale, shape):
    """The numbers a 6-bit pack holds, as bf16 (K, N): e2m3(code) * 2^(scale byte - 127), exactly (4 significant bits times
    a power of two).  q uint8 (K / 4, N / 8, 24), scale uint8 (K / 32, N), on the device or on the host.  A torch statement
    of the byte layout for tests and debugging -- the kernels never materialise it."""
    K, N = shape
    if K % 32 or N % 8 or q.dtype != torch.uint8 or scale.dtype != torch.uint8 or tuple(q.shape) != (K // 4, N // 8, SLOT) or \
            tuple(scale.shape) != (K // BLOCK, N):
        raise ValueError(f"w6_dequant: expected uint8 e2m3 slots ({K // 4}, {N // 8}, {SLOT}) and uint8 e8m0 bytes ({K // BLOCK}, {N})")
    # four codes are three bytes, little-endian: code 4 t + i of a slot is bits [6 i, 6 i + 6) of bytes 3 t .. 3 t + 2
    b = q.reshape(K // 4, N // 8, 8, 3).to(torch.int64)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    codes = torch.stack([(w >> (6 * i)) & 63 for i in range(4)], dim=-1)                    # [k4][n8][t][i]
    codes = codes.reshape(K // 4, N // 8, 4, 8).permute(0, 2, 1, 3).reshape(K, N)          # code 8 j + c: row 4 k4 + j, column 8 n8 + c
    m = codes & 31
    mag = torch.where(m < 8, m.to(torch.float64) / 8.0, (1.0 + (m & 7).to(torch.float64) / 8.0) * torch.exp2(((m >> 3) - 1).to(torch.float64)))
    val = torch.where((codes & 32) != 0, -mag, mag)
    s = torch.exp2(scale.to(torch.float64) - 127.0).repeat_interleave(BLOCK, dim=0)
    return (val * s).to(torch.bfloat16)


def gemv_fused_w6(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemv_fused over 6-bit packs (lwm_gemv_fused_w6): x (rows <= 4, K) bf16 against 1..3 W6Kernel packs that
    share it.  norm = (ss (rows, n <= 64) f32, weight (K,) bf16, eps): RMSNorm on load; residual (rows, N) bf16 (one pack):
    y = bf16(bf16(x @ W) + residual); want_ss: also the (rows, N / 128) partial sums of squares of y.  -> [y_i] or
    ([y_i], ss).  Bit for bit gemv_fused on the rounded kernels."""
    return _fused_call(FORMAT.proj, False, x, packs, norm, residual, want_ss, out_dtype)


def gemm_rows_fused_w6(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemm_rows_fused over 6-bit packs (lwm_gemm_rows_fused_w6): gemv_fused_w6 for 1..32 rows, the products on the
    matrix pipe.  Bit for bit gemm_rows_fused on the rounded kernels.  (Callers that hold parameters check each pack
    against its parameter first: W6Kernel.check, as for gemv_fused_w6.)"""
    return _fused_call(FORMAT.proj, True, x, packs, norm, residual, want_ss, out_dtype)
