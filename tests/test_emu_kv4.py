"""The 4-bit (MXFP4) KV cache on the CPU: the numpy restatement of the format checked against its own definition in
fp64, the quantising cache write and the decode kernel of csrc/attn_decode_kv4.h host-emulated through the C ABI, the
exactness of the bf16 yardstick, and the ABI mirror.

Bounds: decode against the fp64 oracle on the DEQUANTISED cache, out <= 2e-2 of max and lse <= 2e-3 -- the project's
bounds for bf16-query, f32-accumulate decode over exactly representable rows (tests/test_gpu_infer.py,
tests/test_emu_kv8.py): the arithmetic class is the same."""
import ctypes as C

import numpy as np
import pytest

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _emu, _kv4_ref as K4


def _rnd(shape, seed, mag=1.0):
    return R.round_bf16((np.random.default_rng(seed).standard_normal(shape) * mag).astype(np.float32))


def _rows(n=4096, seed=0):
    """random rows over magnitudes 1e-6 .. 1e3, then the edge rows, padded to a multiple of 32 rows"""
    rng = np.random.default_rng(seed)
    mags = 10.0 ** rng.uniform(-6, 3, size=(n, 1))
    x = np.concatenate([R.round_bf16((rng.standard_normal((n, 128)) * mags).astype(np.float32)), K4.edge_rows(rng)])
    return np.concatenate([x, np.zeros((-x.shape[0] % 32, 128), np.float32)])


def emu_quant_write(cache, scale, src, *, dst_row0=None, index=None, row_offset=0, src_row0=0, nrows=None):
    """cache u8 (B,S,H,64), scale u8 (B,S,H,4), src f32 (B,*,H,128) of bf16 values; index: the _at form"""
    L = _emu.lib()
    B, S, H, _ = cache.shape
    sb = _emu.bf16_array(src)
    nrows = src.shape[1] - src_row0 if nrows is None else nrows
    if index is None:
        rc = L.lwm_kv4_cache_write(cache.ctypes.data, sb.ctypes.data, B, cache.strides[0], sb.strides[0] // 2, dst_row0, src_row0,
                                   nrows, H * 128, scale.ctypes.data, scale.strides[0], H, None)
    else:
        idx = np.array([index], np.int32)
        rc = L.lwm_kv4_cache_write_at(cache.ctypes.data, sb.ctypes.data, B, cache.strides[0], sb.strides[0] // 2, idx.ctypes.data,
                                      row_offset, S, src_row0, nrows, H * 128, scale.ctypes.data, scale.strides[0], H, None)
    _capi.check(L, rc, "lwm_kv4_cache_write")


def emu_cache(B, S, H):
    return _emu.aligned((B, S, H, 64), np.uint8), _emu.aligned((B, S, H, 4), np.uint8)


def emu_decode(q, kq, ks, vq, vs, mask, k_splits, scale=None):
    """-> (out f32 (B,1,H,128), lse (B,H,1), partials) through lwm_attn_decode_kv4 + lwm_attn_combine"""
    L = _emu.lib()
    B, _, H, D = q.shape
    Sk = kq.shape[1]
    qb = _emu.bf16_array(q)
    a = _capi.LwmKv4DecodeArgs()
    a.q = _emu._t4(qb)
    a.k, a.v, a.k_scale, a.v_scale = kq.ctypes.data, vq.ctypes.data, ks.ctypes.data, vs.ctypes.data
    a.k_stride_b, a.k_stride_s, a.k_stride_h = kq.strides[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = vq.strides[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = ks.strides[:2]
    a.v_scale_stride_b, a.v_scale_stride_s = vs.strides[:2]
    if mask is not None:
        mask = np.ascontiguousarray(mask.reshape(B, Sk).astype(np.uint8))
        a.dense_mask, a.mask_stride_b = mask.ctypes.data, Sk
    a.B, a.Sk, a.H, a.D, a.scale, a.k_splits = B, Sk, H, D, (1.0 / np.sqrt(D) if scale is None else scale), k_splits
    P = max(1, k_splits)
    op, lp = _emu.aligned((P, B, 1, H, D), np.float32), _emu.aligned((P, B, H, 1), np.float32)
    op[...], lp[...] = np.nan, np.nan                      # the kernel must write every partial
    a.out_acc, a.lse_acc = op.ctypes.data, lp.ctypes.data
    _capi.check(L, L.lwm_attn_decode_kv4(C.byref(a), None), "lwm_attn_decode_kv4")
    out, lse = _emu.aligned((B, 1, H, D), np.float32), _emu.aligned((B, H, 1), np.float32)
    _capi.check(L, L.lwm_attn_combine(op.ctypes.data, lp.ctypes.data, P, _capi.LwmTensor4(None, 0, 0, 0), out.ctypes.data,
                                      lse.ctypes.data, B, 1, H, D, None), "lwm_attn_combine")
    return out, lse, op, lp


# ---------------------------------------------------------------- the restatement itself, in fp64
def test_restatement_self_check():
    y = np.concatenate([np.linspace(-6, 6, 48001), np.array(list(K4.TIES)), -np.array(list(K4.TIES)), K4.E2M1_MAG, -K4.E2M1_MAG])
    c = K4.e2m1_encode(y)
    got = K4.e2m1_decode(c)
    # a nearest representable magnitude, with the sign of y
    best = np.abs(np.abs(y)[:, None] - K4.E2M1_MAG).min(-1)
    assert np.array_equal(np.abs(np.abs(got) - np.abs(y)), best)
    assert np.array_equal(np.signbit(got), np.signbit(y))
    for t, want in K4.TIES.items():                       # 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 -> 0, 1, 1, 2, 2, 4, 4
        assert K4.e2m1_decode(K4.e2m1_encode(t)) == want and K4.e2m1_decode(K4.e2m1_encode(-t)) == -want
        assert K4.e2m1_encode(t) % 2 == 0
    assert [K4.TIES[t] for t in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)] == [0, 1, 1, 2, 2, 4, 4]
    assert K4.e2m1_encode(-0.0) == 8 and K4.e2m1_encode(0.0) == 0
    assert np.array_equal(K4.e2m1_encode(K4.e2m1_decode(np.arange(16, dtype=np.uint8))), np.arange(16, dtype=np.uint8))
    for k in range(-125, 120):
        assert K4.scale_for(6.0 * 2.0 ** k) == 2.0 ** k
        assert K4.scale_for(5.96875 * 2.0 ** k) == 2.0 ** k
        assert K4.scale_for(6.03125 * 2.0 ** k) == 2.0 ** (k + 1)
    assert K4.scale_exp_for(0.0) == 127 and K4.scale_exp_for(2.0 ** -133) == 1 and K4.scale_exp_for(6 * 2.0 ** -126) == 1
    assert K4.scale_exp_for(float(np.float32(3.3895e38))) <= 254
    # smallest power of two: half of it no longer fits (except at the clamp and for all-zero blocks)
    x = _rows(256)
    q, e = K4.quantise(x)
    amax = np.abs(x.astype(np.float64).reshape(-1, 4, 32)).max(-1)
    s = 2.0 ** (e.astype(np.float64) - 127)
    assert (amax / s <= 6).all()
    free = (amax > 0) & (e > 1)
    assert (amax[free] / (s[free] / 2) > 6).all()
    assert e.min() >= 1 and e.max() <= 254


def test_dequant_round_trips_through_bf16():
    """q * s is a bf16 number: the restatement's dequantised values and kv4_dequant agree exactly, for every code and a
    spread of scales at which every product is a normal number (s >= 2^-125)"""
    import torch
    from lwm_amd import kv4
    ebytes = np.array([2, 27, 97, 119, 126, 127, 128, 134, 167, 252], np.uint8)      # (6 * 2^125 is below the top of bf16)
    q = np.zeros((len(ebytes), 64), np.uint8)
    q[:] = (np.arange(64) % 16) | (((np.arange(64) // 4) % 16) << 4)
    e = np.repeat(ebytes[:, None], 4, 1)
    want = K4.dequant(q, e)
    assert np.array_equal(R.round_bf16(want.astype(np.float32)).astype(np.float64), want)
    d = kv4.kv4_dequant(torch.from_numpy(q), torch.from_numpy(e))
    assert d.dtype == torch.bfloat16 and tuple(d.shape) == (len(ebytes), 128)
    assert np.array_equal(d.float().numpy().astype(np.float64), want)
    assert np.array_equal(np.signbit(d.float().numpy()), np.signbit(want))
    # the same for quantised rows, the edge rows included, wherever the products are normal numbers below the top of bf16
    x = _rows(64)
    q, e = K4.quantise(x)
    ok = (e >= 2).all(-1) & (np.abs(x).max(-1) < 1e38)
    assert ok.sum() >= x.shape[0] - 3
    dq = K4.dequant(q[ok], e[ok])
    assert np.array_equal(R.round_bf16(dq.astype(np.float32)).astype(np.float64), dq)


# ---------------------------------------------------------------- quantising write, bit for bit
@pytest.mark.parametrize("H", [32, 1])
def test_quantiser_bit_for_bit(H):
    x = _rows()
    src = x.reshape(1, -1, H, 128)
    S = src.shape[1]
    cache, scale = emu_cache(1, S, H)
    cache[...], scale[...] = 0xAB, 0xAB
    emu_quant_write(cache, scale, src, dst_row0=0)
    q, e = K4.quantise(src)
    assert np.array_equal(scale, e), np.argwhere(scale != e)[:8]
    bad = np.argwhere(cache != q)
    assert bad.size == 0, [(tuple(i), cache[tuple(i)], q[tuple(i)]) for i in bad[:8]]
    # negative zero keeps its sign bit; byte 255 is never written; the four-block row has four different bytes
    nz = np.signbit(src) & (src == 0)
    assert nz.any() and (K4.codes(cache)[nz] == 8).all()
    assert scale.max() <= 254 and scale.min() >= 1
    assert any(len(set(r)) == 4 for r in e.reshape(-1, 4)[4096:])


@pytest.mark.parametrize("H", [1, 3, 32])
def test_write_at_equals_host_index_and_skips_outside_rows(H):
    B, S, n = 2, 12, 4
    src = _rnd((B, 6, H, 128), 5, 3.0)
    q, s = K4.quantise(src)

    def fresh():
        c, e = emu_cache(B, S, H)
        c[...], e[...] = 0xAB, 0xAB
        return c, e
    ch, sh = fresh()
    emu_quant_write(ch, sh, src, dst_row0=5, src_row0=1, nrows=n)
    cd, sd = fresh()
    emu_quant_write(cd, sd, src, index=3, row_offset=2, src_row0=1, nrows=n)
    assert np.array_equal(ch, cd) and np.array_equal(sh, sd)
    assert np.array_equal(ch[:, 5:9], q[:, 1:5]) and np.array_equal(sh[:, 5:9], s[:, 1:5])
    assert (ch[:, :5] == 0xAB).all() and (ch[:, 9:] == 0xAB).all() and (sh[:, :5] == 0xAB).all() and (sh[:, 9:] == 0xAB).all()
    # rows that fall outside [0, cache_rows) are skipped, their neighbours untouched: index 10 + rows 0..3 -> 10, 11 land
    cd, sd = fresh()
    emu_quant_write(cd, sd, src, index=10, src_row0=0, nrows=n)
    assert np.array_equal(cd[:, 10:12], q[:, 0:2]) and np.array_equal(sd[:, 10:12], s[:, 0:2])
    assert (cd[:, :10] == 0xAB).all() and (sd[:, :10] == 0xAB).all()
    # "only the owning shard writes": row_offset = -rank * cache_rows puts every row below 0 -> nothing is written
    cd, sd = fresh()
    emu_quant_write(cd, sd, src, index=3, row_offset=-S, src_row0=0, nrows=n)
    assert (cd == 0xAB).all() and (sd == 0xAB).all()
    emu_quant_write(cd, sd, src, index=3, row_offset=-5, src_row0=0, nrows=n)        # rows -2, -1, 0, 1
    assert np.array_equal(cd[:, 0:2], q[:, 2:4]) and (cd[:, 2:] == 0xAB).all() and (sd[:, 2:] == 0xAB).all()
    assert np.array_equal(sd[:, 0:2], s[:, 2:4])


# ---------------------------------------------------------------- decode kernel against the fp64 oracle
def _quantised_cache(B, Sk, H, seed):
    k, v = _rnd((B, Sk, H, 128), seed, 1.5), _rnd((B, Sk, H, 128), seed + 1, 0.7)
    # blocks of different magnitude inside a head, so that a wrong scale byte shows
    k[..., 32:64] *= 0.25
    v[..., 96:] *= 8.0
    kq, ks = emu_cache(B, Sk, H)
    vq, vs = emu_cache(B, Sk, H)
    kq[...], ks[...] = K4.quantise(k)
    vq[...], vs[...] = K4.quantise(v)
    return kq, ks, vq, vs


_DEQ = lambda q, e: K4.dequant(q, e).astype(np.float32)          # (exact: bf16 numbers)


@pytest.mark.parametrize("B,Sk,H,splits,cache_index", [
    (2, 300, 2, 3, 250),         # 64 key lanes per head, ragged pieces
    (1, 64, 32, 1, 63),          # the LWM-7B head count: four keys per pass, one piece
    (1, 130, 3, 2, 129),         # a head count that is no power of two: one idle slot in four
    (1, 40, 130, 2, 39),         # more heads than slots: two passes over the heads
])
def test_decode_kv4_vs_oracle(B, Sk, H, splits, cache_index):
    q = _rnd((B, 1, H, 128), 1)
    kq, ks, vq, vs = _quantised_cache(B, Sk, H, 2)
    am = (np.random.default_rng(4).random((B, Sk)) > 0.1).astype(np.uint8)       # random 10 % holes
    am[:, cache_index] = 1
    mask = R.decode_mask(B, 1, Sk, cache_index, am)
    out, lse, _, _ = emu_decode(q, kq, ks, vq, vs, mask, splits)
    # the oracle gets the DEQUANTISED cache: quantisation error is not in the comparison
    ro, rl = R.dense_attention(q, _DEQ(kq, ks), _DEQ(vq, vs), causal=False, dense_mask=mask)
    e_out, e_lse = np.abs(out - ro).max() / np.abs(ro).max(), np.abs(lse - rl).max()
    print(f"kv4 decode (emulated) B={B} Sk={Sk} H={H} splits={splits}: out {e_out:.3e} of max, lse {e_lse:.3e}")
    assert e_out <= 2e-2
    assert e_lse <= 2e-3


def test_decode_kv4_mask_behaviour():
    """no mask = all visible; 0xFF nibble bytes and 0xFF scale bytes (and other garbage) in masked rows change nothing; a
    row with nothing visible gives (0, -inf) in every piece; so does a piece that is entirely masked"""
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
    ro, rl = R.dense_attention(q, _DEQ(kq, ks), _DEQ(vq, vs), causal=False, dense_mask=mask)
    assert np.abs(out - ro).max() / np.abs(ro).max() <= 2e-2 and np.abs(lse - rl).max() <= 2e-3
    hid = np.broadcast_to((mask[:, 0] == 0)[:, :, None], (B, Sk, H))
    rng = np.random.default_rng(3)
    for fill_q, fill_s in ((0xFF, 0xFF), (0x77, 0xFE), (0x00, 0x00), (None, None)):
        k2, s2, v2, t2 = kq.copy(), ks.copy(), vq.copy(), vs.copy()
        for c, s in ((k2, s2), (v2, t2)):
            c[hid] = rng.integers(0, 256, (int(hid.sum()), 64)).astype(np.uint8) if fill_q is None else fill_q
            s[hid] = rng.integers(0, 256, (int(hid.sum()), 4)).astype(np.uint8) if fill_s is None else fill_s
        (ka, sa), (va, ta) = emu_cache(B, Sk, H), emu_cache(B, Sk, H)        # (16-byte aligned copies)
        ka[...], sa[...], va[...], ta[...] = k2, s2, v2, t2
        o2, l2, _, _ = emu_decode(q, ka, sa, va, ta, mask, 5)
        assert np.array_equal(o2, out) and np.array_equal(l2, lse), (fill_q, fill_s)
    # a piece that is entirely masked: the visible range [0, 200] in 5 pieces of 41; keys 82..122 are piece 2
    m2 = np.ones((B, 1, Sk), np.uint8)
    m2[:, 0, 201:] = 0
    m2[:, 0, 82:123] = 0
    _, _, op, lp = emu_decode(q, kq, ks, vq, vs, m2, 5)
    assert (op[2] == 0).all() and np.isneginf(lp[2]).all()
    assert np.isfinite(op).all() and np.isfinite(lp[[0, 1, 3, 4]]).all()
    mask[1] = 0                          # batch row 1 sees nothing
    out, lse, op, lp = emu_decode(q, kq, ks, vq, vs, mask, 5)
    assert (op[:, 1] == 0).all() and np.isneginf(lp[:, 1]).all()
    assert (out[1] == 0).all() and np.isneginf(lse[1]).all()
    assert np.isfinite(out[0]).all() and np.isfinite(lse[0]).all()


def test_decode_kv4_validation_and_abi():
    L = _emu.lib()
    assert L.lwm_version() >= 570
    assert L.lwm_sizeof(10) == C.sizeof(_capi.LwmKv4DecodeArgs)
    assert L.lwm_attn_decode_kv4(None, None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    q = _rnd((1, 1, 2, 128), 1)
    kq, ks, vq, vs = _quantised_cache(1, 16, 2, 2)
    a = _capi.LwmKv4DecodeArgs()
    a.q = _emu._t4(_emu.bf16_array(q))
    a.B, a.Sk, a.H, a.D, a.scale, a.k_splits = 1, 16, 2, 64, 0.1, 1
    assert L.lwm_attn_decode_kv4(C.byref(a), None) == _capi.LWM_EINVAL and b"head_dim" in L.lwm_last_error()
    a.D = 128
    assert L.lwm_attn_decode_kv4(C.byref(a), None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    op, lp = _emu.aligned((1, 1, 1, 2, 128), np.float32), _emu.aligned((1, 1, 2, 1), np.float32)
    a.k, a.v, a.k_scale, a.v_scale, a.out_acc, a.lse_acc = (t.ctypes.data for t in (kq, vq, ks, vs, op, lp))
    a.k_stride_b, a.k_stride_s, a.k_stride_h = kq.strides[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = vq.strides[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = a.v_scale_stride_b, a.v_scale_stride_s = ks.strides[:2]
    a.k = kq.ctypes.data + 8
    assert L.lwm_attn_decode_kv4(C.byref(a), None) == _capi.LWM_EINVAL and b"aligned" in L.lwm_last_error()
    a.k = kq.ctypes.data
    a.v_stride_s = vq.strides[1] + 4
    assert L.lwm_attn_decode_kv4(C.byref(a), None) == _capi.LWM_EINVAL and b"aligned" in L.lwm_last_error()
    a.v_stride_s = vq.strides[1]
    a.k_stride_h = 32
    assert L.lwm_attn_decode_kv4(C.byref(a), None) == _capi.LWM_EINVAL and b"strides" in L.lwm_last_error()
    a.k_stride_h = 64
    for bad in (-1, 4097):
        a.k_splits = bad
        assert L.lwm_attn_decode_kv4(C.byref(a), None) == _capi.LWM_EINVAL and b"k_splits" in L.lwm_last_error()
    a.k_splits = 1
    assert L.lwm_attn_decode_kv4(C.byref(a), None) == _capi.LWM_OK
    # the write refuses rows that are not H * 128 elements, null pointers and misaligned tensors
    src = _emu.bf16_array(_rnd((1, 1, 2, 128), 3))
    w = lambda cache, s, row_elems: L.lwm_kv4_cache_write(cache, src.ctypes.data, 1, kq.strides[0], 256, 0, 0, 1, row_elems, s,
                                                         ks.strides[0], 2, None)
    assert w(kq.ctypes.data, ks.ctypes.data, 200) == _capi.LWM_EINVAL and b"row_elems" in L.lwm_last_error()
    assert w(kq.ctypes.data + 2, ks.ctypes.data, 256) == _capi.LWM_EINVAL and b"misaligned" in L.lwm_last_error()
    assert w(None, None, 256) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    assert w(kq.ctypes.data, ks.ctypes.data, 256) == _capi.LWM_OK
    idx = np.zeros(1, np.int32)
    assert L.lwm_kv4_cache_write_at(kq.ctypes.data, src.ctypes.data, 1, kq.strides[0], 256, None, 0, 16, 0, 1, 256, ks.ctypes.data,
                                    ks.strides[0], 2, None) == _capi.LWM_EINVAL
    assert L.lwm_kv4_cache_write_at(kq.ctypes.data, src.ctypes.data, 1, kq.strides[0], 256, idx.ctypes.data, 0, 16, 0, 1, 256,
                                    ks.ctypes.data, ks.strides[0], 2, None) == _capi.LWM_OK


def test_product_library_abi():
    """lwm_sizeof(10) of liblwm_hip.so against the ctypes mirror, and the version that introduced the 4-bit cache"""
    import os
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    L = _capi.bind(C.CDLL(so))
    assert L.lwm_version() >= 570
    assert L.lwm_sizeof(10) == C.sizeof(_capi.LwmKv4DecodeArgs)
    assert L.lwm_attn_decode_kv4(None, None) == _capi.LWM_EINVAL
