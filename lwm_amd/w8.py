"""8-bit (e4m3) decode weights: the torch-tensor front end of lwm_w8_quantise, lwm_gemv_fused_w8 and lwm_gemm_rows_fused_w8
(include/lwm_hip.h, "8-bit decode weights"; csrc/gemv_w8.h, csrc/gemm_rows.h).  As everything in lwm_amd: hand-written HIP kernels on the current torch stream,
no PyTorch / CPU fallback."""
import ctypes as C

import torch

from . import _capi
from ._lib import lib
from .ops import _stream_ptr

GROUP = 128            # rows of K per scale = the K tile of one GEMV partial
_WS = {}
_DTYPES = (torch.bfloat16, torch.float32)


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


def _is_dev(t):
    return torch.is_tensor(t) and t.is_cuda


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


def _check(x, packs, out_dtype):
    """x (rows, K) bf16 with contiguous rows, 1..3 W8Kernel packs of (K, N_i) kernels on x's device -> (rows, K)"""
    if not _is_dev(x) or x.dim() != 2 or x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise ValueError("gemv_fused_w8: x must be a bf16 (rows, K) ROCm tensor with contiguous rows")
    rows, K = x.shape
    if not 1 <= len(packs) <= 3:
        raise ValueError("gemv_fused_w8: one to three packs per call")
    for i, p in enumerate(packs):
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
    if out_dtype not in _DTYPES:
        raise ValueError("gemv_fused_w8: out_dtype must be torch.bfloat16 or torch.float32")
    return rows, K


def gemv_fused_w8(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemv_fused over 8-bit packs (lwm_gemv_fused_w8): x (rows <= 4, K) bf16 against 1..3 W8Kernel packs that
    share it.  norm = (ss (rows, n <= 64) f32, weight (K,) bf16, eps): RMSNorm on load; residual (rows, N) bf16 (one pack):
    y = bf16(bf16(x @ W) + residual); want_ss: also the (rows, N / 128) partial sums of squares of y.  -> [y_i] or
    ([y_i], ss).  Bit for bit gemv_fused on the rounded kernels."""
    return _fused_call(False, x, packs, norm, residual, want_ss, out_dtype)


def gemm_rows_fused_w8(x, packs, *, norm=None, residual=None, want_ss=False, out_dtype=torch.bfloat16):
    """llama_ops.gemm_rows_fused over 8-bit packs (lwm_gemm_rows_fused_w8): gemv_fused_w8 for 1..32 rows, the products on the
    matrix pipe.  Bit for bit gemm_rows_fused on the rounded kernels.  (Callers that hold parameters check each pack
    against its parameter first: W8Kernel.check, as for gemv_fused_w8.)"""
    return _fused_call(True, x, packs, norm, residual, want_ss, out_dtype)


def _fused_call(rows_entry, x, packs, norm, residual, want_ss, out_dtype):
    rows, K = _check(x, packs, out_dtype)
    n = len(packs)
    Ns = [int(p.shape[1]) for p in packs]
    if rows_entry:
        if not 1 <= rows <= 32:
            raise ValueError(f"gemm_rows_fused_w8: {rows} rows (1..32)")
        if x.data_ptr() % 16 or x.stride(0) % 8:
            raise ValueError("gemm_rows_fused_w8: x must be 16-byte aligned with a row stride that is a multiple of 8 elements")
    on = lambda t: _is_dev(t) and t.device == x.device
    if norm is not None:
        ss, w, eps = norm
        if not on(ss) or ss.dtype != torch.float32 or not ss.is_contiguous() or ss.dim() != 2 or ss.shape[0] != rows or \
                not 1 <= ss.shape[1] <= 64:
            raise ValueError(f"gemv_fused_w8: norm ss must be a contiguous f32 ({rows}, n <= 64) tensor on {x.device}")
        if not on(w) or w.dtype != torch.bfloat16 or not w.is_contiguous() or w.numel() != K:
            raise ValueError(f"gemv_fused_w8: norm weight must be a contiguous bf16 tensor of {K} elements on {x.device}")
    if residual is not None:
        if n != 1 or not on(residual) or residual.dtype != torch.bfloat16 or tuple(residual.shape) != (rows, Ns[0]) or \
                residual.stride(1) != 1:
            raise ValueError(f"gemv_fused_w8: residual goes with ONE pack and is a bf16 tensor of its output's shape on {x.device}")
    if want_ss and (n != 1 or Ns[0] % 128 or out_dtype != torch.bfloat16):
        raise ValueError("gemv_fused_w8: want_ss goes with ONE pack, a bf16 output and N % 128 == 0")
    L = lib()
    key = (x.device, rows, K, tuple(Ns)) + (("rows",) if rows_entry else ())
    ws = _WS.get(key)
    if ws is None:                     # (one workspace per shape: a hipGraph replays with the pointers it captured)
        need = sum((L.lwm_gemm_rows_workspace_bytes if rows_entry else L.lwm_gemv_workspace_bytes)(rows, K, N) for N in Ns)
        ws = _WS[key] = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    ys = [torch.empty(rows, N, dtype=out_dtype, device=x.device) for N in Ns]
    a = _capi.LwmGemvW8Args()
    a.x, a.ldx, a.nmat, a.rows, a.K = x.data_ptr(), x.stride(0), n, rows, K
    a.workspace = ws.data_ptr()
    for i, p in enumerate(packs):
        a.w[i], a.w_scale[i], a.N[i] = p.q.data_ptr(), p.scale.data_ptr(), Ns[i]
        if out_dtype == torch.float32:
            a.y_f32[i] = ys[i].data_ptr()
        else:
            a.y[i], a.ldy[i] = ys[i].data_ptr(), Ns[i]
    if norm is not None:
        a.norm_weight, a.ss_in, a.ss_n, a.eps = w.data_ptr(), ss.data_ptr(), ss.shape[1], float(eps)
    if residual is not None:
        a.residual[0], a.ldres[0] = residual.data_ptr(), residual.stride(0)
    ss_out = None
    if want_ss:
        ss_out = torch.empty(rows, Ns[0] // 128, dtype=torch.float32, device=x.device)
        a.ss_out = ss_out.data_ptr()
    name = "lwm_gemm_rows_fused_w8" if rows_entry else "lwm_gemv_fused_w8"
    _capi.check(L, getattr(L, name)(C.byref(a), _stream_ptr()), name)
    return (ys, ss_out) if want_ss else ys
