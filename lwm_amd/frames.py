"""The frame preprocessor in front of the VQGAN tokeniser, on the device: uint8 RGB frames -> f32 (T,size,size,3) in
[-1, 1], bit for bit what `lwm_amd.cli.vision_chat._process_frame` (lwm/vision_chat.py:59-74) gets from Pillow -- the
antialiased bicubic resize of the short side to `size`, the centre crop and u / 127.5 - 1.

Pillow's 8-bit resample is integer arithmetic on 22-bit fixed-point coefficients.  `resample_tables` builds those
coefficients here, in f64 and in Pillow's order of operations (src/libImaging/Resample.c), together with the 256-entry
f32 table of the final scale; the HIP kernels (csrc/frames.h, lwm_frames_preprocess_u8) do the integer arithmetic and
nothing else.  There is no CPU path: `process_frames` needs a ROCm device.
"""
import ctypes as C
import functools
import math
import typing
import warnings

import numpy as np
import torch

from . import _capi
from ._lib import lib

PRECISION_BITS = 22
# host frames are uploaded, and device frames processed, this many raw bytes at a time (a 1020-frame 1080p clip is
# 6.3 GB: it never sits on the device whole, and the intermediate image of a chunk stays small)
CHUNK_BYTES = 512 << 20


class FrameTables(typing.NamedTuple):
    """The tables of one (h, w, size), restricted to the crop window.  Per pass: bounds (size, 2) int32 = (first input
    sample, tap count) and coeffs (size, ksize) int32; None for a pass Pillow skips (output length == input length),
    whose window is copied from column `left` / row `top` on.  scale: (256,) f32, the value of each byte."""
    nw: int
    nh: int
    left: int
    top: int
    h_bounds: typing.Optional[np.ndarray]
    h_coeffs: typing.Optional[np.ndarray]
    v_bounds: typing.Optional[np.ndarray]
    v_coeffs: typing.Optional[np.ndarray]
    scale: np.ndarray


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _pass_tables(n_in, n_out, first_out, count):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for outputs [first_out, first_out + count) of a pass from
    n_in to n_out samples; None if the pass is skipped"""
    if n_in == n_out:
        return None, None
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((count, 2), np.int32)
    coeffs = np.zeros((count, ksize), np.int32)
    for i in range(count):
        center = (first_out + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[i] = xmin, xmax
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coeffs[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


@functools.lru_cache(maxsize=None)
def resample_tables(h, w, size):
    """FrameTables of an (h, w) frame and a `size` x `size` result (cached: the arrays are read-only and live as long as
    the process, which is what the asynchronous copy of lwm_frames_preprocess_u8 asks of them)"""
    h, w, size = int(h), int(w), int(size)
    if h < 1 or w < 1 or size < 1:
        raise ValueError(f"resample_tables: h, w, size must be >= 1, got {h}, {w}, {size}")
    if w < h:
        nw, nh = size, int(size * h / w)
    else:
        nh, nw = size, int(size * w / h)
    left, top = round((nw - size) / 2), round((nh - size) / 2)
    hb, hk = _pass_tables(w, nw, left, size)
    vb, vk = _pass_tables(h, nh, top, size)
    scale = np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1)
    scale.setflags(write=False)
    return FrameTables(nw, nh, left, top, hb, hk, vb, vk, scale)


def _as_u8_frames(frames):
    """-> a (T,H,W,3) uint8 torch tensor (host or device) that shares the caller's memory"""
    if isinstance(frames, np.ndarray):
        if frames.dtype != np.uint8:
            raise ValueError(f"process_frames: expected uint8 RGB frames, got dtype {frames.dtype}")
        with warnings.catch_warnings():         # (read-only memory, a memory-mapped clip say: nothing writes here)
            warnings.simplefilter("ignore", UserWarning)
            frames = torch.from_numpy(frames)
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f"process_frames: expected a numpy array or a torch tensor, got {type(frames).__name__}")
    if frames.dtype != torch.uint8:
        raise ValueError(f"process_frames: expected uint8 RGB frames, got dtype {frames.dtype}")
    if frames.dim() == 3:
        frames = frames[None]
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError(f"process_frames: expected (T,H,W,3) or (H,W,3) RGB frames, got shape {tuple(frames.shape)}")
    return frames


def process_frames(frames, size=256, device=None):
    """uint8 RGB frames (T,H,W,3) or (H,W,3) -- numpy array or torch tensor, on the host or on the device -- -> f32
    device tensor (T,size,size,3) in [-1, 1], ready for `VQGAN.encode`: exactly `_process_frame` of every frame.
    Host frames are uploaded CHUNK_BYTES at a time.  ValueError for anything other than 8-bit RGB."""
    from .ops import _stream_ptr
    frames = _as_u8_frames(frames)
    size = int(size)
    if size < 1:
        raise ValueError(f"process_frames: size must be >= 1, got {size}")
    if frames.is_cuda:
        if device is not None and torch.device(device) != frames.device:
            raise ValueError(f"process_frames: frames are on {frames.device}, device={device}")
        dev = frames.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("process_frames needs a ROCm device (lwm_amd has no CPU path)")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"process_frames: device must be a ROCm device, got {dev}")
    T, H, W, _ = frames.shape
    out = torch.empty((T, size, size, 3), dtype=torch.float32, device=dev)
    if T == 0:
        return out
    tab = resample_tables(H, W, size)
    hks = 0 if tab.h_coeffs is None else tab.h_coeffs.shape[1]
    vks = 0 if tab.v_coeffs is None else tab.v_coeffs.shape[1]
    ptr = lambda a: None if a is None else a.ctypes.data
    per = max(1, min(T, CHUNK_BYTES // (H * W * 3)))
    L = lib()
    ws_bytes = L.lwm_frames_preprocess_workspace_bytes(per, H, size, hks, vks)
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        for t0 in range(0, T, per):
            chunk = frames[t0:t0 + per].contiguous().to(dev)
            a = _capi.LwmFramesArgs(chunk.data_ptr(), out[t0:t0 + per].data_ptr(), ws.data_ptr(), ws_bytes,
                                    ptr(tab.h_bounds), ptr(tab.h_coeffs), ptr(tab.v_bounds), ptr(tab.v_coeffs),
                                    ptr(tab.scale), chunk.shape[0], H, W, size, hks, vks, tab.left, tab.top)
            _capi.check(L, L.lwm_frames_preprocess_u8(C.byref(a), _stream_ptr()), "lwm_frames_preprocess_u8")
            # (the caching allocator reuses `chunk` only for work queued behind this kernel on the same stream)
    return out
