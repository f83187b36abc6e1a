"""The frame preprocessor's kernels (csrc/frames.h) compiled for the host and driven through lwm_frames_preprocess_u8:
bit for bit the numpy restatement of Pillow's resize + crop + scale (tests/_frames_ref.py), every output element
written and nothing else, and every malformed argument set refused before a kernel runs."""
import ctypes as C

import numpy as np
import pytest

from lwm_amd import _capi
from lwm_amd.frames import resample_tables
from tests import _emu, _frames_abi as A, _frames_ref as R


expected = R.expected


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_restatement(shape, pattern):
    h, w, size = shape
    frames = R.make_frames(h, w, pattern)
    out, rc = A.run_numpy(_emu.lib(), frames, size)
    assert rc == _capi.LWM_OK, _emu.lib().lwm_last_error()
    assert not np.isnan(out).any(), "an output element was not written"
    assert np.array_equal(out, expected(h, w, size, pattern))


def test_all_byte_values_reach_the_scale_table():
    frames = R.make_frames(16, 16, "random")
    assert len(np.unique(frames[0])) == 256
    out, rc = A.run_numpy(_emu.lib(), frames, 16)
    assert rc == _capi.LWM_OK
    assert np.array_equal(out, frames.astype(np.float32) / np.float32(127.5) - np.float32(1))


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_frames_at_any_byte_alignment(misalign):
    """the rows are fetched as aligned dwords: the first and the last dword of the buffer hang over its ends"""
    for h, w in ((37, 61), (16, 40)):
        frames = R.make_frames(h, w, "random")
        out, rc = A.run_numpy(_emu.lib(), frames, 16, misalign=misalign)
        assert rc == _capi.LWM_OK
        assert np.array_equal(out, expected(h, w, 16, "random"))


def test_stripes_drive_both_clamps():
    """the 0/255 stripes push the accumulators of each pass past 0 and past 255 in the restatement, so the kernels'
    clamps are exercised by test_kernel_equals_restatement (upscaling shape: bicubic overshoot is not averaged away)"""
    for pattern in ("row_stripes", "col_stripes"):
        frames = R.make_frames(9, 23, pattern)
        lo, hi = [], []
        for f in frames:
            _, raw = R.process_frame(f, 16, want_unclamped=True)
            assert len(raw) == 2
            lo.append(min(r.min() for r in raw))
            hi.append(max(r.max() for r in raw))
        assert min(lo) < 0 and max(hi) > 255, (pattern, lo, hi)


def test_one_pass_alone_from_caller_tables():
    """_process_frame resizes both axes or neither, but the C contract lets either pass be skipped on its own"""
    L = _emu.lib()
    frames = R.make_frames(40, 61, "random")
    full = resample_tables(40, 61, 16)
    # horizontal pass alone: rows top .. top+16 copied
    tab = full._replace(v_bounds=None, v_coeffs=None, top=7)
    out, rc = A.run_numpy(L, frames, 16, tab=tab)
    assert rc == _capi.LWM_OK, L.lwm_last_error()
    want = np.clip(R.resample_unclamped(frames[:, 7:23], full.h_bounds, full.h_coeffs, 2), 0, 255)
    assert np.array_equal(out, want.astype(np.float32) / np.float32(127.5) - np.float32(1))
    # vertical pass alone: columns left .. left+16 copied
    tab = full._replace(h_bounds=None, h_coeffs=None, left=45)
    out, rc = A.run_numpy(L, frames, 16, tab=tab)
    assert rc == _capi.LWM_OK, L.lwm_last_error()
    want = np.clip(R.resample_unclamped(frames[:, :, 45:61], full.v_bounds, full.v_coeffs, 1), 0, 255)
    assert np.array_equal(out, want.astype(np.float32) / np.float32(127.5) - np.float32(1))


def _edit(tab, name, index, value):
    a = np.array(getattr(tab, name))
    a[index] = value
    return tab._replace(**{name: a})


def test_rejected_arguments():
    """LWM_EINVAL, and no kernel has run: the NaN-filled output is untouched"""
    L = _emu.lib()
    h, w, size = 37, 61, 16
    frames = R.make_frames(h, w, "random")
    good = resample_tables(h, w, size)
    skip = resample_tables(16, 40, 16)
    bad_tables = {
        "first < 0": _edit(good, "h_bounds", (3, 0), -1),
        "window past the row": _edit(good, "h_bounds", (15, 0), w - 1),
        "window past the column": _edit(good, "v_bounds", (15, 1), h),
        "taps > ksize": _edit(good, "v_bounds", (0, 1), good.v_coeffs.shape[1] + 1),
        "taps 0": _edit(good, "h_bounds", (0, 1), 0),
        "null scale": good._replace(scale=None),
    }
    for name, tab in bad_tables.items():
        out, rc = A.run_numpy(L, frames, size, tab=tab)
        assert rc == _capi.LWM_EINVAL, name
        assert np.isnan(out).all(), name
    f40 = R.make_frames(16, 40, "random")
    for name, tab in {"skipped window past the row": skip._replace(left=25), "negative skipped window": skip._replace(top=-1)}.items():
        out, rc = A.run_numpy(L, f40, 16, tab=tab)
        assert rc == _capi.LWM_EINVAL and np.isnan(out).all(), name

    # scalar arguments and pointers, on a well-formed call
    def call(**edits):
        T = frames.shape[0]
        out = np.full((T, size, size, 3), np.nan, np.float32)
        ws_bytes = L.lwm_frames_preprocess_workspace_bytes(T, h, size, good.h_coeffs.shape[1], good.v_coeffs.shape[1])
        ws = _emu.aligned((ws_bytes,), np.uint8)
        fin = np.ascontiguousarray(frames)
        a, keep = A.args_for(good, T, h, w, size, fin.ctypes.data, out.ctypes.data, ws.ctypes.data, ws_bytes)
        for k, v in edits.items():
            setattr(a, k, v)
        rc = L.lwm_frames_preprocess_u8(C.byref(a), None)
        assert rc == _capi.LWM_OK or np.isnan(out).all()
        return rc

    assert call() == _capi.LWM_OK
    assert L.lwm_frames_preprocess_u8(None, None) == _capi.LWM_EINVAL
    for edits in (dict(frames=None), dict(out=None), dict(workspace=None), dict(T=0), dict(H=0), dict(W=0), dict(size=0),
                  dict(T=-1), dict(h_coeffs=None), dict(v_bounds=None), dict(h_ksize=0),
                  dict(workspace_bytes=L.lwm_frames_preprocess_workspace_bytes(3, h, size, good.h_coeffs.shape[1],
                                                                               good.v_coeffs.shape[1]) - 1),
                  dict(W=w // 2), dict(H=h - 1), dict(h_ksize=1), dict(v_ksize=-1)):
        assert call(**edits) == _capi.LWM_EINVAL, edits
    assert b"frames" in L.lwm_last_error()
    assert L.lwm_version() >= 600
    assert L.lwm_frames_preprocess_workspace_bytes(0, h, size, 5, 5) == 0
