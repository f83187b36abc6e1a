"""8-bit (e4m3) decode weights: the torch-tensor front end of lwm_w8_quantise, lwm_gemv_fused_w8 and lwm_gemm_rows_fused_w8
(include/lwm_hip.h, "8-bit decode weights"; csrc/gemv_w8.h, csrc/gemm_rows.h).  As everything in lwm_amd: hand-written HIP kernels on the current torch stream,
no PyTorch / CPU fallback."""
import torch

from . import wpack
from ._lib import lib                   # noqa: F401  (wpack.quantise_weight calls the library through this name)
from .llama_ops import _fused_call

FORMAT = wpack.FORMATS["fp8"]
GROUP = 128            # rows of K per scale = the K tile of one GEMV partial


class W8Kernel(wpack.WeightPack):
    """The 8-bit pack of one (K, N) kernel: `q` uint8 (K, N) e4m3fn bytes, `scale` f32 (ceil(K / 128), N), the shape, and
    `stamp` = (_version, data_ptr) of the parameter AFTER it was rounded in place -- a pack whose parameter has changed
    since is stale (`check`)."""
    __slots__, fmt = (), FORMAT


def quantise_weight(kernel):
    """kernel: a contiguous bf16 (K, N) ROCm tensor (K % 32 == 0, K <= 12288, N % 8 == 0), ROUNDED IN PLACE to the values
    its 8-bit pack stands for, bf16(e4m3(q) * s) -> W8Kernel.  One pass over the kernel on the device."""
    return wpack.quantise_weight(FORMAT, kernel)


def gemv_fused_w8(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemv_fused over 8-bit packs (lwm_gemv_fused_w8): x (rows <= 4, K) bf16 against 1..3 W8Kernel packs that
    share it.  norm = (ss (rows, n <= 64) f32, weight (K,) bf16, eps): RMSNorm on load; residual (rows, N) bf16 (one pack):
    y = bf16(bf16(x @ W) + residual); want_ss: also the (rows, N / 128) partial sums of squares of y.  -> [y_i] or
    ([y_i], ss).  Bit for bit gemv_fused on the rounded kernels."""
    return _fused_call(FORMAT.proj, False, x, packs, norm, residual, want_ss, out_dtype)


def gemm_rows_fused_w8(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemm_rows_fused over 8-bit packs (lwm_gemm_rows_fused_w8): gemv_fused_w8 for 1..32 rows, the products on the
    matrix pipe.  Bit for bit gemm_rows_fused on the rounded kernels.  (Callers that hold parameters check each pack
    against its parameter first: W8Kernel.check, as for gemv_fused_w8.)"""
    return _fused_call(FORMAT.proj, True, x, packs, norm, residual, want_ss, out_dtype)
