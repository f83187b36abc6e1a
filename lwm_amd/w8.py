"""8-bit (e4m3) decode weights: the torch-tensor front end of lwm_w8_quantise, lwm_gemv_fused_w8 and lwm_gemm_rows_fused_w8
(include/lwm_hip.h, "8-bit decode weights"; csrc/gemv_w8.h, csrc/gemm_rows.h).  As everything in lwm_amd: hand-written HIP kernels on the current torch stream,
no PyTorch / CPU fallback."""
import torch

from . import _capi
from ._lib import lib
from .llama_ops import ProjFormat, _fused_call, _is_dev
from .ops import _stream_ptr

GROUP = 128            # rows of K per scale = the K tile of one GEMV partial


class W8Kernel:
    """The 8-bit pack of one (K, N) kernel: `q` uint8 (K, N) e4m3fn bytes, `scale` f32 (ceil(K / 128), N), the shape, and
    `stamp` = (_version, data_ptr) of the parameter AFTER it was rounded in place -- a pack whose parameter has changed
    since is stale (`check`)."""
    __slots__ = ("q", "scale", "shape", "stamp")

    def __init__(self, q, scale, shape, stamp):
        self.q, self.scale, self.shape, self.stamp = q, scale, tuple(shape), stamp

    def check(self, kernel, name="kernel"):
        if (kernel._version, kernel.data_ptr()) != self.stamp:
            raise RuntimeError(f"{name}: the parameter changed after its fp8 decode pack was made (the pack holds the old "
                               f"weights): call quantize_decode_weights('fp8') again, or drop_decode_weights()")
        return self


def quantise_weight(kernel):
    """kernel: a contiguous bf16 (K, N) ROCm tensor (K % 32 == 0, K <= 12288, N % 8 == 0), ROUNDED IN PLACE to the values
    its 8-bit pack stands for, bf16(e4m3(q) * s) -> W8Kernel.  One pass over the kernel on the device."""
    if not _is_dev(kernel) or kernel.dim() != 2 or kernel.dtype != torch.bfloat16 or not kernel.is_contiguous():
        raise ValueError("quantise_weight: kernel must be a contiguous bf16 (K, N) ROCm tensor")
    K, N = kernel.shape
    if K < 32 or K % 32 or K > 12288 or N < 8 or N % 8:
        raise ValueError(f"quantise_weight: kernel of shape {(K, N)}: need K % 32 == 0, K <= 12288 and N % 8 == 0")
    q = torch.empty((K, N), dtype=torch.uint8, device=kernel.device)
    scale = torch.empty(((K + GROUP - 1) // GROUP, N), dtype=torch.float32, device=kernel.device)
    L = lib()
    with torch.no_grad():
        data = kernel.detach()
        _capi.check(L, L.lwm_w8_quantise(data.data_ptr(), q.data_ptr(), scale.data_ptr(), data.data_ptr(), K, N, _stream_ptr()),
                    "lwm_w8_quantise")
        # (the kernel wrote behind torch's back: count it as the in-place edit it is, so that copies kept while the
        # parameter is "unchanged" -- llama_ops._as_dtype -- are made again)
        torch.autograd.graph.increment_version(data)
    return W8Kernel(q, scale, (K, N), (kernel._version, kernel.data_ptr()))


def _pack_matrix(i, p, x, K):
    if not isinstance(p, W8Kernel):
        raise ValueError(f"gemv_fused_w8: packs[{i}] must be a W8Kernel (quantise_weight)")
    Kp, N = p.shape
    q, s = p.q, p.scale
    if Kp != K or not _is_dev(q) or q.device != x.device or q.dtype != torch.uint8 or tuple(q.shape) != (K, N) or \
            not q.is_contiguous():
        raise ValueError(f"gemv_fused_w8: packs[{i}].q must be a contiguous uint8 ({K}, N) tensor on {x.device}")
    if not _is_dev(s) or s.device != x.device or s.dtype != torch.float32 or \
            tuple(s.shape) != ((K + GROUP - 1) // GROUP, N) or not s.is_contiguous():
        raise ValueError(f"gemv_fused_w8: packs[{i}].scale must be a contiguous f32 ({(K + GROUP - 1) // GROUP}, {N}) "
                         f"tensor on {x.device}")
    return int(N)


def _pack_fill(a, i, p):
    a.w[i], a.w_scale[i] = p.q.data_ptr(), p.scale.data_ptr()


W8 = ProjFormat(_capi.LwmGemvW8Args, ("lwm_gemv_fused_w8", "lwm_gemm_rows_fused_w8"), "gemv_fused_w8",
                ("gemv_fused_w8", "gemm_rows_fused_w8"), "pack", _pack_matrix, _pack_fill, True)


def gemv_fused_w8(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemv_fused over 8-bit packs (lwm_gemv_fused_w8): x (rows <= 4, K) bf16 against 1..3 W8Kernel packs that
    share it.  norm = (ss (rows, n <= 64) f32, weight (K,) bf16, eps): RMSNorm on load; residual (rows, N) bf16 (one pack):
    y = bf16(bf16(x @ W) + residual); want_ss: also the (rows, N / 128) partial sums of squares of y.  -> [y_i] or
    ([y_i], ss).  Bit for bit gemv_fused on the rounded kernels."""
    return _fused_call(W8, False, x, packs, norm, residual, want_ss, out_dtype)


def gemm_rows_fused_w8(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemm_rows_fused over 8-bit packs (lwm_gemm_rows_fused_w8): gemv_fused_w8 for 1..32 rows, the products on the
    matrix pipe.  Bit for bit gemm_rows_fused on the rounded kernels.  (Callers that hold parameters check each pack
    against its parameter first: W8Kernel.check, as for gemv_fused_w8.)"""
    return _fused_call(W8, True, x, packs, norm, residual, want_ss, out_dtype)
