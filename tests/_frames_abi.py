"""lwm_frames_preprocess_u8 driven through the raw C ABI on caller-owned buffers, for tests/test_emu_frames.py (numpy
buffers, host emulation) and tests/test_gpu_frames.py (torch buffers, the product).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from lwm_amd import _capi
from lwm_amd.frames import resample_tables

GUARD = 64            # guard bytes on each side of the output
GUARD_BYTE = 0xA5


def args_for(tab, T, H, W, size, frames_ptr, out_ptr, ws_ptr, ws_bytes):
    """LwmFramesArgs from a FrameTables-like object (h_bounds, h_coeffs, v_bounds, v_coeffs, scale, left, top); the
    returned `keep` list owns the contiguous host copies the pointers refer to"""
    keep = []

    def host(a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    hks = 0 if tab.h_coeffs is None else np.shape(tab.h_coeffs)[1]
    vks = 0 if tab.v_coeffs is None else np.shape(tab.v_coeffs)[1]
    a = _capi.LwmFramesArgs(frames_ptr, out_ptr, ws_ptr, ws_bytes, host(tab.h_bounds, np.int32), host(tab.h_coeffs, np.int32),
                            host(tab.v_bounds, np.int32), host(tab.v_coeffs, np.int32), host(tab.scale, np.float32),
                            T, H, W, size, hks, vks, tab.left, tab.top)
    return a, keep


def run_torch(frames, size, tab=None, misalign=0):
    """run_numpy on the device through the product library: -> (out as numpy, return code)"""
    import torch
    from lwm_amd._lib import lib
    from lwm_amd.ops import _stream_ptr
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    T, H, W, _ = frames.shape
    tab = resample_tables(H, W, size) if tab is None else tab
    hks = 0 if tab.h_coeffs is None else np.shape(tab.h_coeffs)[1]
    vks = 0 if tab.v_coeffs is None else np.shape(tab.v_coeffs)[1]
    raw_in = torch.zeros(frames.size + 16, dtype=torch.uint8, device=dev)
    fin = raw_in[misalign:misalign + frames.size]
    fin.copy_(torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)))
    n_out = T * size * size * 3 * 4
    raw_out = torch.full((n_out + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    out = raw_out[GUARD:GUARD + n_out].view(torch.float32)
    out.fill_(float("nan"))
    ws_bytes = L.lwm_frames_preprocess_workspace_bytes(T, H, size, hks, vks)
    raw_ws = torch.full((ws_bytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    raw_ws[ws_bytes:] = GUARD_BYTE
    assert fin.data_ptr() % 4 == misalign and out.data_ptr() % 16 == 0 and raw_ws.data_ptr() % 16 == 0
    a, keep = args_for(tab, T, H, W, size, fin.data_ptr(), out.data_ptr(), raw_ws.data_ptr(), ws_bytes)
    rc = L.lwm_frames_preprocess_u8(C.byref(a), _stream_ptr())
    torch.cuda.synchronize()
    assert bool((raw_out[:GUARD] == GUARD_BYTE).all()) and bool((raw_out[GUARD + n_out:] == GUARD_BYTE).all()), \
        "wrote outside the output"
    assert bool((raw_ws[ws_bytes:] == GUARD_BYTE).all()), "wrote past the workspace"
    assert np.array_equal(fin.cpu().numpy().reshape(frames.shape), frames), "the input changed"
    return out.cpu().numpy().reshape(T, size, size, 3), rc


def run_numpy(L, frames, size, tab=None, misalign=0):
    """frames (T,H,W,3) uint8 through the library `L` on numpy buffers: the output prefilled with NaN between guard bytes,
    the workspace with 0xFF, the frames at a byte offset of `misalign` from a 16-byte boundary.  -> (out, return code);
    asserts that the guards are intact."""
    T, H, W, _ = frames.shape
    tab = resample_tables(H, W, size) if tab is None else tab
    hks = 0 if tab.h_coeffs is None else np.shape(tab.h_coeffs)[1]
    vks = 0 if tab.v_coeffs is None else np.shape(tab.v_coeffs)[1]
    raw_in = np.zeros(frames.size + 32, np.uint8)
    off = (-raw_in.ctypes.data) % 16 + misalign
    fin = raw_in[off:off + frames.size].reshape(frames.shape)
    fin[...] = frames
    n_out = T * size * size * 3 * 4
    raw_out = np.full(n_out + 2 * GUARD + 16, GUARD_BYTE, np.uint8)
    o0 = (-(raw_out.ctypes.data + GUARD)) % 16 + GUARD
    out = raw_out[o0:o0 + n_out].view(np.float32).reshape(T, size, size, 3)
    out[...] = np.nan
    ws_bytes = L.lwm_frames_preprocess_workspace_bytes(T, H, size, hks, vks)
    raw_ws = np.full(ws_bytes + 16 + GUARD, 0xFF, np.uint8)
    w0 = (-raw_ws.ctypes.data) % 16
    raw_ws[w0 + ws_bytes:] = GUARD_BYTE
    a, keep = args_for(tab, T, H, W, size, fin.ctypes.data, out.ctypes.data, raw_ws.ctypes.data + w0, ws_bytes)
    rc = L.lwm_frames_preprocess_u8(C.byref(a), None)
    assert (raw_out[:o0] == GUARD_BYTE).all() and (raw_out[o0 + n_out:] == GUARD_BYTE).all(), "wrote outside the output"
    assert (raw_ws[w0 + ws_bytes:] == GUARD_BYTE).all(), "wrote past the workspace"
    assert np.array_equal(fin, frames), "the input changed"
    return out, rc
