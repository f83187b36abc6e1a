"""lwm_conv2d_nhwc_bf16 (lwm_amd/csrc/vqgan_conv_bf16.h) compiled for the host and run one fiber per lane through the C
ABI: the six points of its contract (include/lwm_hip.h; tests/_conv16_ref.py has the cases and the references), on the
smallest shapes at which each part of the kernel can go wrong, and the ABI checks of the new entry."""
import ctypes as C
import os

import numpy as np
import pytest

from lwm_amd import _capi
from oracle import vqgan_ref as R
from oracle.attention_ref import round_bf16
from tests import _conv16_ref as K, _emu

WIDE = [c for c in K.CASES if c[3] >= 128]      # the two widest cases again on a machine of 3 CUs: 128 x 128 tiles


def _names(capfd):
    return [l.split()[1] for l in capfd.readouterr().err.splitlines() if l.startswith("emu-launch")]


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_exact_on_integer_data(case):
    """contract point 1: taps, padding, stride, upsample, tile edges, the pack layout and the epilogue, with no tolerance"""
    *shape, kw, res = case
    x, w, b, r = K.int_case(1, *shape, kw, res)
    got = K.emu_conv(x, w, b, r, **kw)
    ref = R.conv2d(x, w, b, r, **kw)
    assert got.shape == ref.shape and np.array_equal(got, ref), np.abs(got - ref).max()


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_random_data_within_the_bound(case):
    """contract point 2"""
    *shape, kw, res = case
    x, w, b, r = K.random_case(2, *shape, kw, res)
    print("worst error / bound:", K.check_contract2(K.emu_conv(x, w, b, r, **kw), x, w, b, r, **kw))


@pytest.mark.parametrize("case", WIDE, ids=[i for i, c in zip(K.IDS, K.CASES) if c[3] >= 128])
def test_small_machine_takes_the_wide_tile(case, capfd, monkeypatch):
    """on 3 CUs the same shapes run in 128 x 128 tiles (elsewhere too few of them fill the machine: 64 x 64), whole ones
    and, for 160 output channels, one with a column block past Cout: points 1 and 2 again"""
    monkeypatch.setenv("LWM_EMU_CUS", "3")
    monkeypatch.setenv("LWM_EMU_TRACE", "1")
    *shape, kw, res = case
    x, w, b, r = K.int_case(3, *shape, kw, res)
    assert np.array_equal(K.emu_conv(x, w, b, r, **kw), R.conv2d(x, w, b, r, **kw))
    assert _names(capfd) == ["conv16_igemm_128x128"]
    x, w, b, r = K.random_case(4, *shape, kw, res)
    K.check_contract2(K.emu_conv(x, w, b, r, **kw), x, w, b, r, **kw)
    x, w, b, r = K.int_case(5, 2, 10, 16, 64, 160, 3, {}, True)
    assert np.array_equal(K.emu_conv(x, w, b, r), R.conv2d(x, w, b, r))


def test_every_tile_shape_is_what_runs(capfd, monkeypatch):
    monkeypatch.setenv("LWM_EMU_TRACE", "1")
    for Cout in (32, 64, 128):
        x, w, b, _ = K.int_case(6, 1, 8, 8, 32, Cout, 3, {}, False)
        assert np.array_equal(K.emu_conv(x, w, b), R.conv2d(x, w, b))
    assert _names(capfd) == ["conv16_igemm_128x32", "conv16_igemm_64x64", "conv16_igemm_64x64"]


def test_clip_without_bias():
    x, w, _, _ = K.random_case(8, 1, 12, 12, 32, 128, 3, {}, False)
    x *= 4.0
    got = K.emu_conv(x, w, clip=True)
    y64, mag = K.ref64(x, w)
    assert np.abs(got).max() == 1.0 and (np.abs(y64) > 1).mean() > 0.2         # the clip acts
    assert (np.abs(got - np.clip(y64, -1, 1)) <= K.bound(w, mag)).all()
    xi, wi, _, _ = K.int_case(9, 1, 12, 12, 32, 128, 3, {}, False)
    assert np.array_equal(K.emu_conv(xi, wi, clip=True), R.conv2d(xi, wi, clip=True))


def test_rounding_is_nearest_even_at_the_staging():
    """contract point 3"""
    x, w = K.rne_case()
    got = K.emu_conv(x, w)
    assert np.array_equal(got.view(np.uint32), round_bf16(x).view(np.uint32))
    assert got.reshape(-1)[0] == 1.0 and got.reshape(-1)[5] == 1 + 2.0 ** -6     # the two ties, to even


def test_hidden_memory_reaches_nothing():
    """contract point 4: every operand inside a larger buffer of NaN patterns: the same bits, the guards intact"""
    for case in (K.CASES[0], K.CASES[5], K.CASES[7]):          # ragged tile; odd Downsample; straddling tile + residual
        *shape, kw, res = case
        x, w, b, r = K.random_case(10, *shape, kw, res)
        got, intact = K.emu_conv(x, w, b, r, hidden=0xFF, **kw)
        assert intact and np.isfinite(got).all()
        assert np.array_equal(got, K.emu_conv(x, w, b, r, **kw))


def test_same_launch_same_bits_and_batch_independence():
    """contract point 5"""
    x, w, b, r = K.random_case(11, 3, 8, 24, 64, 128, 3, {}, True)
    a = K.emu_conv(x, w, b, r)
    assert np.array_equal(a, K.emu_conv(x, w, b, r))
    alone = K.emu_conv(x[1:2], w, b, r[1:2])
    assert np.array_equal(alone[0], a[1])


def _args(xa, wa, ya, Cin, Cout, k=3, **over):
    B, H, W = xa.shape[:3]
    a = _capi.LwmConvArgs(xa.ctypes.data, wa.ctypes.data, None, None, ya.ctypes.data, B, H, W, Cin, Cout, k, k, 1, 1, 0, H, W, 0)
    for n, v in over.items():
        setattr(a, n, v)
    return a


def test_refusals_by_name():
    """contract point 6: the channel rule -> LWM_EUNSUPPORTED; null, misaligned, bad dimension as the f32 entry"""
    L = _emu.lib()
    x, wp, y = _emu.aligned((1, 8, 8, 64), np.float32), _emu.aligned((9 * 64 * 64,), np.uint16), _emu.aligned((1, 8, 8, 64), np.float32)
    call = lambda a: L.lwm_conv2d_nhwc_bf16(C.byref(a), None)
    assert call(_args(x, wp, y, 40, 64)) == _capi.LWM_EUNSUPPORTED and b"Cin=40" in L.lwm_last_error()
    assert call(_args(x, wp, y, 64, 3)) == _capi.LWM_EUNSUPPORTED and b"Cout=3" in L.lwm_last_error()
    assert L.lwm_conv2d_nhwc_bf16(None, None) == _capi.LWM_EINVAL
    assert call(_capi.LwmConvArgs()) == _capi.LWM_EINVAL
    f32 = lambda a: L.lwm_conv2d_nhwc_f32(C.byref(a), None)
    for over in (dict(x=None), dict(w=None), dict(y=None), dict(x=x.ctypes.data + 4), dict(w=wp.ctypes.data + 2),
                 dict(y=y.ctypes.data + 8), dict(residual=y.ctypes.data + 4), dict(Hin=0), dict(KH=0), dict(stride=0),
                 dict(pad=-1), dict(up_shift=5), dict(Wo=0), dict(B=-1)):
        a = _args(x, wp, y, 64, 64, **over)
        assert call(a) == _capi.LWM_EINVAL, over
        msg = L.lwm_last_error()
        assert f32(a) == _capi.LWM_EINVAL and L.lwm_last_error() == msg, over
    y[...] = 7.0
    assert call(_args(x, wp, y, 64, 64, B=0)) == _capi.LWM_OK and (y == 7.0).all()      # an empty batch: nothing runs


def test_abi():
    L = _emu.lib()
    assert L.lwm_version() >= 620
    so = os.path.join(_emu.ROOT, "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    P = _capi.bind(C.CDLL(so))
    assert P.lwm_version() >= 620
    assert P.lwm_conv2d_nhwc_bf16(None, None) == _capi.LWM_EINVAL and b"null" in P.lwm_last_error()
    assert "lwm_conv2d_nhwc_bf16" in _capi.PROTOTYPES
