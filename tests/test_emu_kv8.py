"""The 8-bit (e4m3) KV cache on the CPU: the numpy restatement of the format against torch.float8_e4m3fn, the
quantising cache write and the decode kernel of csrc/attn_decode_kv8.h host-emulated through the C ABI, the
exactness of the bf16 yardstick, and the ABI mirror."""
import ctypes as C

import numpy as np
import pytest

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _emu, _kv8_ref as K8


def _rnd(shape, seed, mag=1.0):
    return R.round_bf16((np.random.default_rng(seed).standard_normal(shape) * mag).astype(np.float32))


def _rows(seed=0):
    """random rows over magnitudes 1e-6 .. 1e3, then the edge rows"""
    rng = np.random.default_rng(seed)
    mags = 10.0 ** rng.uniform(-6, 3, size=(96, 1))
    rnd = R.round_bf16((rng.standard_normal((96, 128)) * mags).astype(np.float32))
    return np.concatenate([rnd, K8.edge_rows(rng)])


def emu_quant_write(cache, scale, src, *, dst_row0=None, index=None, row_offset=0, src_row0=0, nrows=None):
    """cache u8 (B,S,H,128), scale f32 (B,S,H), src f32 (B,*,H,128) of bf16 values; index: the _at form"""
    L = _emu.lib()
    B, S, H, D = cache.shape
    sb = _emu.bf16_array(src)
    nrows = src.shape[1] - src_row0 if nrows is None else nrows
    if index is None:
        rc = L.lwm_kv8_cache_write(cache.ctypes.data, sb.ctypes.data, B, cache.strides[0], sb.strides[0] // 2, dst_row0, src_row0,
                                   nrows, H * D, scale.ctypes.data, scale.strides[0] // 4, H, None)
    else:
        idx = np.array([index], np.int32)
        rc = L.lwm_kv8_cache_write_at(cache.ctypes.data, sb.ctypes.data, B, cache.strides[0], sb.strides[0] // 2, idx.ctypes.data,
                                      row_offset, S, src_row0, nrows, H * D, scale.ctypes.data, scale.strides[0] // 4, H, None)
    _capi.check(L, rc, "lwm_kv8_cache_write")


def emu_cache(B, S, H):
    return _emu.aligned((B, S, H, 128), np.uint8), _emu.aligned((B, S, H), np.float32)


def emu_decode(q, kq, ks, vq, vs, mask, k_splits, scale=None):
    """-> (out f32 (B,1,H,128), lse (B,H,1)) through lwm_attn_decode_kv8 + lwm_attn_combine; scale: default 1/sqrt(D)"""
    L = _emu.lib()
    B, _, H, D = q.shape
    Sk = kq.shape[1]
    qb = _emu.bf16_array(q)
    a = _capi.LwmKv8DecodeArgs()
    a.q = _emu._t4(qb)
    a.k, a.v, a.k_scale, a.v_scale = kq.ctypes.data, vq.ctypes.data, ks.ctypes.data, vs.ctypes.data
    a.k_stride_b, a.k_stride_s, a.k_stride_h = kq.strides[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = vq.strides[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = (s // 4 for s in ks.strides[:2])
    a.v_scale_stride_b, a.v_scale_stride_s = (s // 4 for s in vs.strides[:2])
    if mask is not None:
        mask = np.ascontiguousarray(mask.reshape(B, Sk).astype(np.uint8))
        a.dense_mask, a.mask_stride_b = mask.ctypes.data, Sk
    a.B, a.Sk, a.H, a.D, a.scale, a.k_splits = B, Sk, H, D, (1.0 / np.sqrt(D) if scale is None else scale), k_splits
    P = max(1, k_splits)
    op, lp = _emu.aligned((P, B, 1, H, D), np.float32), _emu.aligned((P, B, H, 1), np.float32)
    a.out_acc, a.lse_acc = op.ctypes.data, lp.ctypes.data
    _capi.check(L, L.lwm_attn_decode_kv8(C.byref(a), None), "lwm_attn_decode_kv8")
    out, lse = _emu.aligned((B, 1, H, D), np.float32), _emu.aligned((B, H, 1), np.float32)
    _capi.check(L, L.lwm_attn_combine(op.ctypes.data, lp.ctypes.data, P, _capi.LwmTensor4(None, 0, 0, 0), out.ctypes.data,
                                      lse.ctypes.data, B, 1, H, D, None), "lwm_attn_combine")
    return out, lse, op, lp


# ---------------------------------------------------------------- the restatement itself
def test_restatement_rounds_like_torch_float8():
    import torch
    x = _rows()
    q, s = K8.quantise(x)
    y = x / s[:, None]
    assert np.abs(y).max() <= 448 and (np.abs(x).max(-1) / s <= 448).all()
    ref = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(q, ref)
    # smallest power of two: half of it no longer fits (except at the lower clamp and for all-zero rows)
    amax = np.abs(x).max(-1)
    free = (amax > 0) & (s > 2.0 ** -126)
    assert (amax[free] / (s[free] / 2) > 448).all()
    assert np.array_equal(np.frexp(s)[0], np.full(s.shape, 0.5, np.float32))          # powers of two
    # the decode table against torch, every byte
    tb = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(K8.e4m3_table(), tb, equal_nan=True)
    # and encode(decode(b)) = b for every finite byte
    b = np.array([i for i in range(256) if i & 0x7f != 0x7f], np.uint8)
    assert np.array_equal(K8.e4m3_encode(K8.e4m3_decode(b)), b)


def test_dequant_is_exact_in_bf16():
    """kv8_dequant(q, s).float() == e4m3(q) * s exactly: all 256 bytes times a spread of scales"""
    import torch
    from lwm_amd import ops
    # every scale at which all products are normal numbers: 2^-9 * s >= 2^-126 and 448 * s below the top of bf16.  (Below
    # 2^-117 -- rows whose amax is under 2^-108 -- the smallest products are subnormal and a bf16 copy holds what the
    # denormal mode of the machine leaves of them.)
    scales = 2.0 ** np.array([-117, -100, -30, -8, -1, 0, 1, 7, 40, 118], np.float64)
    q = np.tile(np.arange(256, dtype=np.uint8)[:128], (len(scales), 1)), np.tile(np.arange(256, dtype=np.uint8)[128:], (len(scales), 1))
    for half in q:
        s = scales.astype(np.float32)
        d = ops.kv8_dequant(torch.from_numpy(half), torch.from_numpy(s))
        assert d.dtype == torch.bfloat16
        want = K8.e4m3_decode(half).astype(np.float64) * scales[:, None]
        assert np.array_equal(d.float().numpy().astype(np.float64), want, equal_nan=True)
        assert np.array_equal(K8.dequant(half, s).astype(np.float64), want, equal_nan=True)


# ---------------------------------------------------------------- quantising write, bit for bit
def test_quantiser_bit_for_bit():
    x = _rows()
    n = x.shape[0]
    H = 2
    pad = (-n) % H
    x = np.concatenate([x, np.zeros((pad, 128), np.float32)])
    src = x.reshape(1, -1, H, 128)
    S = src.shape[1]
    cache, scale = emu_cache(1, S, H)
    emu_quant_write(cache, scale, src, dst_row0=0)
    q, s = K8.quantise(src)
    assert np.array_equal(scale, s)
    assert np.array_equal(cache, q)
    # negative zero keeps its sign bit
    assert (q[np.signbit(src) & (src == 0)] == 0x80).all()


@pytest.mark.parametrize("H", [1, 3, 32])
def test_write_at_equals_host_index_and_skips_outside_rows(H):
    B, S, n = 2, 12, 4
    src = _rnd((B, 6, H, 128), 5, 3.0)
    q, s = K8.quantise(src)
    fill = lambda: (np.full((B, S, H, 128), 0xAB, np.uint8), np.full((B, S, H), 7.5, np.float32))
    ch, sh = emu_cache(B, S, H)
    ch[...], sh[...] = fill()
    emu_quant_write(ch, sh, src, dst_row0=5, src_row0=1, nrows=n)
    cd, sd = emu_cache(B, S, H)
    cd[...], sd[...] = fill()
    emu_quant_write(cd, sd, src, index=3, row_offset=2, src_row0=1, nrows=n)
    assert np.array_equal(ch, cd) and np.array_equal(sh, sd)
    assert np.array_equal(ch[:, 5:9], q[:, 1:5]) and np.array_equal(sh[:, 5:9], s[:, 1:5])
    assert (ch[:, :5] == 0xAB).all() and (ch[:, 9:] == 0xAB).all() and (sh[:, :5] == 7.5).all() and (sh[:, 9:] == 7.5).all()
    # rows that fall outside [0, cache_rows) are skipped, their neighbours untouched: index 10 + rows 0..3 -> 10, 11 land
    cd[...], sd[...] = fill()
    emu_quant_write(cd, sd, src, index=10, src_row0=0, nrows=n)
    assert np.array_equal(cd[:, 10:12], q[:, 0:2]) and np.array_equal(sd[:, 10:12], s[:, 0:2])
    assert (cd[:, :10] == 0xAB).all() and (sd[:, :10] == 7.5).all()
    # "only the owning shard writes": row_offset = -rank * cache_rows puts every row below 0 -> nothing is written
    cd[...], sd[...] = fill()
    emu_quant_write(cd, sd, src, index=3, row_offset=-S, src_row0=0, nrows=n)
    assert (cd == 0xAB).all() and (sd == 7.5).all()
    emu_quant_write(cd, sd, src, index=3, row_offset=-5, src_row0=0, nrows=n)        # rows -2, -1, 0, 1
    assert np.array_equal(cd[:, 0:2], q[:, 2:4]) and (cd[:, 2:] == 0xAB).all() and (sd[:, 2:] == 7.5).all()


# ---------------------------------------------------------------- decode kernel against the fp64 oracle
def _quantised_cache(B, Sk, H, seed):
    k, v = _rnd((B, Sk, H, 128), seed, 1.5), _rnd((B, Sk, H, 128), seed + 1, 0.7)
    kq, ks = emu_cache(B, Sk, H)
    vq, vs = emu_cache(B, Sk, H)
    kq[...], ks[...] = K8.quantise(k)
    vq[...], vs[...] = K8.quantise(v)
    return kq, ks, vq, vs


@pytest.mark.parametrize("B,Sk,H,splits,cache_index", [
    (1, 300, 2, 1, 200),         # one piece; 32 key lanes per head
    (2, 520, 1, 3, 519),         # ragged last piece; 64 key lanes
    (1, 130, 4, 4, 10),          # pieces that are entirely masked
    (1, 200, 32, 2, 150),        # the LWM-7B head count: two keys per pass
    (1, 70, 3, 2, 69),           # a head count that is no power of two: one idle slot in four
    (1, 40, 65, 1, 39),          # more heads than slots: two passes over the heads
])
def test_decode_kv8_vs_oracle(B, Sk, H, splits, cache_index):
    q = _rnd((B, 1, H, 128), 1)
    kq, ks, vq, vs = _quantised_cache(B, Sk, H, 2)
    am = (np.random.default_rng(4).random((B, Sk)) > 0.1).astype(np.uint8)
    am[:, cache_index] = 1
    mask = R.decode_mask(B, 1, Sk, cache_index, am)
    out, lse, _, _ = emu_decode(q, kq, ks, vq, vs, mask, splits)
    # the oracle gets the DEQUANTISED cache: quantisation error is not in the comparison
    ro, rl = R.dense_attention(q, K8.dequant(kq, ks), K8.dequant(vq, vs), causal=False, dense_mask=mask)
    assert np.abs(out - ro).max() / np.abs(ro).max() <= 2e-2
    assert np.abs(lse - rl).max() <= 2e-3


def test_decode_kv8_mask_behaviour():
    """no mask = all visible; garbage bytes and scales (NaN patterns included) in masked rows change nothing; a row
    with nothing visible gives (0, -inf) in every piece"""
    B, Sk, H = 2, 257, 4
    q = _rnd((B, 1, H, 128), 11)
    kq, ks, vq, vs = _quantised_cache(B, Sk, H, 12)
    full, lse_full, _, _ = emu_decode(q, kq, ks, vq, vs, None, 3)
    ones, lse_ones, _, _ = emu_decode(q, kq, ks, vq, vs, np.ones((B, 1, Sk), np.uint8), 3)
    assert np.array_equal(full, ones) and np.array_equal(lse_full, lse_ones)
    mask = np.ones((B, 1, Sk), np.uint8)
    mask[0, 0, :20] = 0                  # left padding
    mask[:, 0, 100:140] = 0              # a hole
    mask[:, 0, 201:] = 0                 # the empty tail of the cache
    out, lse, _, _ = emu_decode(q, kq, ks, vq, vs, mask, 5)
    hid = np.broadcast_to((mask[:, 0] == 0)[:, :, None], (B, Sk, H))
    rng = np.random.default_rng(3)
    for fill_q, fill_s in ((0x7f, np.nan), (0xff, np.inf), (0x7e, -np.float32(3e38)), (None, None)):
        k2, s2, v2, t2 = kq.copy(), ks.copy(), vq.copy(), vs.copy()
        for c, s in ((k2, s2), (v2, t2)):
            c[hid] = rng.integers(0, 256, (int(hid.sum()), 128)).astype(np.uint8) if fill_q is None else fill_q
            s[hid] = rng.standard_normal(int(hid.sum())).astype(np.float32) * 1e30 if fill_s is None else fill_s
        (ka, sa), (va, ta) = emu_cache(B, Sk, H), emu_cache(B, Sk, H)        # (16-byte aligned copies)
        ka[...], sa[...], va[...], ta[...] = k2, s2, v2, t2
        o2, l2, _, _ = emu_decode(q, ka, sa, va, ta, mask, 5)
        assert np.array_equal(o2, out) and np.array_equal(l2, lse)
    mask[1] = 0                          # batch row 1 sees nothing
    out, lse, op, lp = emu_decode(q, kq, ks, vq, vs, mask, 5)
    assert (op[:, 1] == 0).all() and np.isneginf(lp[:, 1]).all()
    assert (out[1] == 0).all() and np.isneginf(lse[1]).all()
    assert np.isfinite(out[0]).all() and np.isfinite(lse[0]).all()


def test_product_library_abi():
    """lwm_sizeof(5) of liblwm_hip.so against the ctypes mirror, and the version that introduced the 8-bit cache"""
    import os
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    L = _capi.bind(C.CDLL(so))
    assert L.lwm_version() >= 520
    assert L.lwm_sizeof(5) == C.sizeof(_capi.LwmKv8DecodeArgs)
    assert L.lwm_attn_decode_kv8(None, None) == _capi.LWM_EINVAL


def test_decode_kv8_validation_and_abi():
    L = _emu.lib()
    assert L.lwm_version() >= 520
    assert L.lwm_sizeof(5) == C.sizeof(_capi.LwmKv8DecodeArgs)
    assert L.lwm_attn_decode_kv8(None, None) == _capi.LWM_EINVAL
    q = _rnd((1, 1, 2, 128), 1)
    kq, ks, vq, vs = _quantised_cache(1, 16, 2, 2)
    a = _capi.LwmKv8DecodeArgs()
    a.q = _emu._t4(_emu.bf16_array(q))
    a.B, a.Sk, a.H, a.D, a.scale, a.k_splits = 1, 16, 2, 64, 0.1, 1
    assert L.lwm_attn_decode_kv8(C.byref(a), None) == _capi.LWM_EUNSUPPORTED and b"head_dim" in L.lwm_last_error()
    a.D = 128
    assert L.lwm_attn_decode_kv8(C.byref(a), None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    op, lp = _emu.aligned((1, 1, 1, 2, 128), np.float32), _emu.aligned((1, 1, 2, 1), np.float32)
    a.k, a.v, a.k_scale, a.v_scale, a.out_acc, a.lse_acc = (t.ctypes.data for t in (kq, vq, ks, vs, op, lp))
    a.k_stride_b, a.k_stride_s, a.k_stride_h = kq.strides[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = vq.strides[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = a.v_scale_stride_b, a.v_scale_stride_s = 32, 2
    a.k = kq.ctypes.data + 8
    assert L.lwm_attn_decode_kv8(C.byref(a), None) == _capi.LWM_EUNSUPPORTED and b"aligned" in L.lwm_last_error()
    a.k = kq.ctypes.data
    assert L.lwm_attn_decode_kv8(C.byref(a), None) == _capi.LWM_OK
    # the write refuses rows that are not H * 128 elements
    assert L.lwm_kv8_cache_write(kq.ctypes.data, kq.ctypes.data, 1, 4096, 4096, 0, 0, 1, 200, ks.ctypes.data, 32, 2, None) == \
        _capi.LWM_EUNSUPPORTED
    assert L.lwm_kv8_cache_write(None, None, 1, 0, 0, 0, 0, 1, 256, None, 0, 2, None) == _capi.LWM_EINVAL
