"""The dropout kernels (lwm_dropout_add_* / lwm_dropout_bwd_*, lwm_amd/csrc/dropout.h) in the host emulation, through the C
ABI, against the numpy restatement of tests/_dropout_ref.py -- bit for bit -- and their argument validation on the
emulated and the real library (no GPU: every bad argument is refused before a launch)."""
import ctypes as C
import os

import numpy as np
import pytest

from lwm_amd import _capi
from tests import _dropout_ref as R
from tests import _emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = dict(key0=0x5EED0001, key1=17, site=3)
THR, INV = R.thr_inv(0.1)
# (B, S, C): one vector; rows and batches of one vector; C no power of two (33 vectors a row, tiles that straddle rows
# and batches); 257 vectors a row (rows of 256 or more take the compare path: tiles that cross a row and a batch end);
# more vectors than one pass of the emulated grid (8 blocks x 24 "compute units" x 256), the last tile cut
SHAPES = [(1, 1, 8), (2, 3, 8), (2, 5, 264), (2, 3, 2056), (3, 131, 1032)]
ENTRIES = ("lwm_dropout_add_bf16", "lwm_dropout_add_f32", "lwm_dropout_bwd_bf16", "lwm_dropout_bwd_f32")


def test_the_large_shape_takes_the_grid_stride_tail():
    B, S, Cc = SHAPES[-1]
    assert "LWM_EMU_CUS" not in os.environ and B * S * Cc // 8 > 8 * 24 * 256 and (B * S * Cc // 8) % 256


def _args(x, res, y, shape, *, thr16=THR, inv=INV, s_offset=0, key0, key1, site):
    a = _capi.LwmDropoutArgs()
    a.x, a.res, a.y = x.ctypes.data, None if res is None else res.ctypes.data, y.ctypes.data
    a.B, a.S, a.C = shape
    a.s_offset, a.site, a.key0, a.key1, a.thr16, a.inv = s_offset, site, key0, key1, thr16, inv
    return a


def emu(x, res=None, *, f32, bwd=False, alias=None, **kw):
    """one emulated launch on copies of x / res (uint16 bf16 bits or float32); alias = "x" / "res": y IS that operand"""
    L = _emu.lib()
    dt = np.float32 if f32 else np.uint16
    xa = _emu.aligned(x.shape, dt)
    xa[...] = x
    ra = None
    if res is not None:
        ra = _emu.aligned(x.shape, dt)
        ra[...] = res
    y = xa if alias == "x" else ra if alias == "res" else _emu.aligned(x.shape, dt)
    if alias is None:
        y[...] = 0x7FC1 if not f32 else np.nan          # the launch must write every element
    name = f"lwm_dropout_{'bwd' if bwd else 'add'}_{'f32' if f32 else 'bf16'}"
    _capi.check(L, getattr(L, name)(C.byref(_args(xa, ra, y, x.shape, **{**RULE, **kw})), None), name)
    return y


def _inputs(shape, f32, seed=0):
    rng = np.random.default_rng(seed + shape[1] * 7 + shape[2])
    x, r = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    return (x, r) if f32 else (R.to_bf16_bits(x), R.to_bf16_bits(r))


def _ref(x, res, f32, **kw):
    kw = {**RULE, "thr16": THR, "inv": INV, **kw}
    return (R.dropout_add_f32 if f32 else R.dropout_add_bf16)(x, res, **kw)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16),
                          np.asarray(b).view(np.uint32 if b.dtype == np.float32 else np.uint16))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_and_backward_bits(shape, f32):
    x, r = _inputs(shape, f32)
    assert _same(emu(x, r, f32=f32), _ref(x, r, f32))
    assert _same(emu(x, None, f32=f32), _ref(x, None, f32))                    # res = None
    # the backward: dx = round(keep ? g * inv : 0); a `res` handed to it is not read
    assert _same(emu(x, None, f32=f32, bwd=True), _ref(x, None, f32))
    assert _same(emu(x, r, f32=f32, bwd=True), _ref(x, None, f32))
    # something was dropped and something kept (but for the shapes of a few elements, where either may fail to happen)
    if np.prod(shape) >= 48:
        kept = R.keep_mask(*shape, thr16=THR, **RULE)
        assert kept.any() and not kept.all()


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("alias", ["x", "res"])
def test_output_may_alias_an_operand(alias, f32):
    x, r = _inputs(SHAPES[2], f32, seed=5)
    assert _same(emu(x, r, f32=f32, alias=alias), _ref(x, r, f32))
    if alias == "x":
        assert _same(emu(x, None, f32=f32, alias="x"), _ref(x, None, f32))
        assert _same(emu(x, None, f32=f32, alias="x", bwd=True), _ref(x, None, f32))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_threshold_ends(f32):
    shape = SHAPES[2]
    x, r = _inputs(shape, f32, seed=9)
    # thr16 = 0 (inv = 1): nothing is dropped, the plain rounded sum, bit for bit
    y0 = emu(x, r, f32=f32, thr16=0, inv=1.0)
    plain = (x + r).astype(np.float32) if f32 else R.to_bf16_bits(R.from_bf16_bits(x) + R.from_bf16_bits(r))
    assert _same(y0, plain) and _same(y0, _ref(x, r, f32, thr16=0, inv=np.float32(1.0)))
    assert _same(emu(x, None, f32=f32, thr16=0, inv=1.0), x)
    # thr16 = 65535: an element survives with probability 2^-16, scaled by 65536
    t, inv = R.thr_inv(65535 / 65536)
    assert t == 65535 and inv == np.float32(65536.0)
    y1 = emu(x, r, f32=f32, thr16=t, inv=inv)
    assert _same(y1, _ref(x, r, f32, thr16=t, inv=inv))
    kept = R.keep_mask(*shape, thr16=t, **RULE)
    assert kept.sum() <= 3 and _same(np.where(kept, y1, r), y1)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_negative_zero_and_subnormals(f32):
    shape = (2, 5, 264)
    n = int(np.prod(shape))
    tiny = np.float32(2.0 ** -133)             # subnormal in f32 and in bf16 (a bf16 value: 2^-133 = 2^6 * 2^-139... one bit)
    vals = np.array([-0.0, 0.0, tiny, -tiny, np.float32(2.0 ** -126), 1.0, -3.5, np.float32(2.0 ** -149) if f32 else tiny * 3],
                    np.float32)
    rng = np.random.default_rng(3)
    x = vals[rng.integers(0, len(vals), n)].reshape(shape)
    r = vals[rng.integers(0, len(vals), n)].reshape(shape)
    if not f32:
        x, r = R.to_bf16_bits(x), R.to_bf16_bits(r)
    y = emu(x, r, f32=f32)
    assert _same(y, _ref(x, r, f32))
    assert _same(emu(x, None, f32=f32), _ref(x, None, f32))
    # a dropped element adds exactly +0: res = -0 comes out as +0, every other res unchanged
    kept = R.keep_mask(*shape, thr16=THR, **RULE)
    rf, yf = (r, y) if f32 else (R.from_bf16_bits(r), R.from_bf16_bits(y))
    drop = ~kept
    assert np.array_equal(yf[drop], rf[drop]) and not np.signbit(yf[drop][rf[drop] == 0]).any()
    assert (np.signbit(rf[drop]) & (rf[drop] == 0)).any()
    # without res, a dropped element is +0 and a kept -0 stays -0
    xf, y1 = (x, emu(x, None, f32=True)) if f32 else (R.from_bf16_bits(x), R.from_bf16_bits(emu(x, None, f32=False)))
    assert not np.signbit(y1[drop]).any() and (y1[drop] == 0).all()
    assert np.array_equal(np.signbit(y1[kept]), np.signbit(xf[kept]))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_chunk_invariance(f32):
    """rows [s0, s1) computed with s_offset = s0 are the slice of the whole (s0 a multiple of nothing)"""
    B, S, Cc = 2, 37, 264
    x, r = _inputs((B, S, Cc), f32, seed=11)
    whole = emu(x, r, f32=f32)
    for s0, s1 in ((0, 13), (13, 30), (30, 37)):
        xc, rc = np.ascontiguousarray(x[:, s0:s1]), np.ascontiguousarray(r[:, s0:s1])
        assert _same(emu(xc, rc, f32=f32, s_offset=s0), np.ascontiguousarray(whole[:, s0:s1])), (s0, s1)
    # and the offset matters
    assert not _same(emu(np.ascontiguousarray(x[:, 13:30]), np.ascontiguousarray(r[:, 13:30]), f32=f32, s_offset=0),
                     np.ascontiguousarray(whole[:, 13:30]))
    # an offset past 2^31: the counter word is s_offset + s modulo nothing, as 32 bits hold it
    big = 2 ** 32 - S
    assert _same(emu(x, r, f32=f32, s_offset=big), _ref(x, r, f32, s_offset=big))


def test_every_part_of_the_counter_and_key_changes_the_mask():
    shape = (2, 5, 264)
    x = np.ones(shape, np.float32)
    mask = lambda **kw: emu(x, None, f32=True, **kw) != 0
    base = mask()
    assert np.array_equal(base, R.keep_mask(*shape, thr16=THR, **RULE))
    for name, v in (("key0", RULE["key0"] + 1), ("key1", RULE["key1"] + 1), ("site", RULE["site"] + 1), ("s_offset", 1)):
        other = mask(**{name: v})
        assert not np.array_equal(base, other), name
        ref_kw = {**RULE, **({name: v} if name != "s_offset" else {})}
        assert np.array_equal(other, R.keep_mask(*shape, thr16=THR, s_offset=v if name == "s_offset" else 0, **ref_kw)), name
    assert not np.array_equal(base[0], base[1])                      # b
    assert not np.array_equal(base[0, 0], base[0, 1])                # s
    assert not np.array_equal(base[0, 0, :8], base[0, 0, 8:16])      # c / 8
    # the eight elements of one call do not share a fate: within vectors, all 8 positions see both outcomes
    v = base.reshape(-1, 8)
    assert v.any(0).all() and not v.all(0).any()


def test_keep_count():
    """2^20 elements at p = 0.1 (thr16 = 6554, drop probability 6554 / 65536 exactly): the number kept lies within 5
    sigma of its expectation, sigma^2 = n q (1 - q) -- for the restatement and, being equal to it, for the kernel"""
    shape = (4, 256, 1024)
    n = int(np.prod(shape))
    assert n == 2 ** 20 and THR == 6554
    q = THR / 65536.0
    ref = R.keep_mask(*shape, thr16=THR, **RULE)
    sigma = np.sqrt(n * q * (1 - q))
    assert abs(int(ref.sum()) - n * (1 - q)) <= 5 * sigma, (int(ref.sum()), n * (1 - q), sigma)
    got = emu(np.ones(shape, np.float32), None, f32=True) != 0
    assert np.array_equal(got, ref)
    # inv is the f32 nearest to 1 / (1 - q)
    assert INV == np.float32(1.0 / (1.0 - q)) and abs(float(INV) * (1 - q) - 1) < 2.0 ** -24


def _lib_real():
    so = os.path.join(ROOT, "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return _capi.bind(C.CDLL(so))


@pytest.mark.parametrize("which", ["emu", "real"])
def test_refusals_in_their_order(which):
    L = _emu.lib() if which == "emu" else _lib_real()
    assert L.lwm_version() >= 650
    assert L.lwm_sizeof(16) == C.sizeof(_capi.LwmDropoutArgs)
    buf = _emu.aligned((64,), np.float32)
    good, odd = buf.ctypes.data, buf.ctypes.data + 4
    for name in ENTRIES:
        fn = getattr(L, name)
        bwd = "bwd" in name

        def refused(a, word):
            assert fn(C.byref(a), None) == _capi.LWM_EINVAL, (name, word)
            assert word.encode() in L.lwm_last_error(), (name, word, L.lwm_last_error())

        assert fn(None, None) == _capi.LWM_EINVAL
        # everything wrong at once; each fix uncovers the next refusal
        a = _capi.LwmDropoutArgs()
        a.x, a.res, a.y, a.B, a.S, a.C, a.thr16, a.inv = None, odd, odd, -1, 1, 12, 65536, 0.5
        refused(a, "null")
        a.x = odd
        a.y = None
        refused(a, "null")
        a.y = odd
        refused(a, "negative")
        a.B = 1
        a.S = -1
        refused(a, "negative")
        a.S = 1
        a.C = -8
        refused(a, "negative")
        a.C = 12
        a.s_offset = -1
        refused(a, "s_offset")
        a.s_offset = 2 ** 32
        refused(a, "s_offset")
        a.s_offset = 2 ** 32 - 1
        refused(a, "multiple of 8")
        a.C = 8
        refused(a, "misaligned")
        a.x = good
        refused(a, "misaligned")
        a.y = good
        if not bwd:                     # (the backward does not read res)
            refused(a, "misaligned")
        a.res = good
        refused(a, "thr16")
        a.thr16 = 65535
        refused(a, "inv")
        for bad in (float("nan"), float("inf"), 0.99999994):
            a.inv = bad
            refused(a, "inv")
        a.inv = 1.0
        # a zero dimension: LWM_OK and nothing launched (the real library has no device to launch on here)
        for dim in ("B", "S", "C"):
            b = _capi.LwmDropoutArgs()
            C.memmove(C.byref(b), C.byref(a), C.sizeof(a))
            setattr(b, dim, 0)
            assert fn(C.byref(b), None) == _capi.LWM_OK, (name, dim)
        if which == "emu":
            a.thr16 = 0                 # legal: the plain sum
            assert fn(C.byref(a), None) == _capi.LWM_OK
