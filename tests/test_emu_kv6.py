"""The 6-bit (MXFP6 e2m3) KV cache on the CPU: the numpy restatement of the format checked against its own definition in
fp64, the derived properties the format is held to, the quantising cache write, the decode kernel and the block kernel of
csrc/attn_decode_kv6.h / attn_prefill_kv6.h host-emulated through the C ABI, the exactness of the bf16 yardstick, and the
ABI mirror.

Bounds: decode and block kernel against the fp64 oracle on the DEQUANTISED cache, out <= 2e-2 of max and lse <= 2e-3 --
the project's bounds for bf16-query, f32-accumulate attention over exactly representable rows (tests/test_emu_kv4.py,
tests/test_emu_kv8_prefill.py); two routes of the same attention 1.6e-2 of max (tests/test_gpu_infer.py).  The block
kernel's partials equal the emulated lwm_attn_fwd split-K kernel's on the dequantised cache bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _emu, _kv4_ref as K4, _kv6_ref as K6


def _rnd(shape, seed, mag=1.0):
    return R.round_bf16((np.random.default_rng(seed).standard_normal(shape) * mag).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _rows(n=4096, seed=0):
    """random rows over magnitudes 1e-6 .. 1e3, then the edge rows, padded to a multiple of 32 rows (shared, read-only)"""
    rng = np.random.default_rng(seed)
    mags = 10.0 ** rng.uniform(-6, 3, size=(n, 1))
    x = np.concatenate([R.round_bf16((rng.standard_normal((n, 128)) * mags).astype(np.float32)), K6.edge_rows(rng)])
    x = np.concatenate([x, np.zeros((-x.shape[0] % 32, 128), np.float32)])
    x.flags.writeable = False
    return x


def emu_quant_write(cache, scale, src, *, dst_row0=None, index=None, row_offset=0, src_row0=0, nrows=None):
    """cache u8 (B,S,H,96), scale u8 (B,S,H,4), src f32 (B,*,H,128) of bf16 values; index: the _at form"""
    L = _emu.lib()
    B, S, H, _ = cache.shape
    sb = _emu.bf16_array(src)
    nrows = src.shape[1] - src_row0 if nrows is None else nrows
    if index is None:
        rc = L.lwm_kv6_cache_write(cache.ctypes.data, sb.ctypes.data, B, cache.strides[0], sb.strides[0] // 2, dst_row0, src_row0,
                                   nrows, H * 128, scale.ctypes.data, scale.strides[0], H, None)
    else:
        idx = np.array([index], np.int32)
        rc = L.lwm_kv6_cache_write_at(cache.ctypes.data, sb.ctypes.data, B, cache.strides[0], sb.strides[0] // 2, idx.ctypes.data,
                                      row_offset, S, src_row0, nrows, H * 128, scale.ctypes.data, scale.strides[0], H, None)
    _capi.check(L, rc, "lwm_kv6_cache_write")


def emu_cache(B, S, H):
    return _emu.aligned((B, S, H, 96), np.uint8), _emu.aligned((B, S, H, 4), np.uint8)


def _fill(a, kq, ks, vq, vs):
    a.k, a.v, a.k_scale, a.v_scale = kq.ctypes.data, vq.ctypes.data, ks.ctypes.data, vs.ctypes.data
    a.k_stride_b, a.k_stride_s, a.k_stride_h = kq.strides[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = vq.strides[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = ks.strides[:2]
    a.v_scale_stride_b, a.v_scale_stride_s = vs.strides[:2]


def emu_combine(op, lp):
    L = _emu.lib()
    P, B, Sq, H, D = op.shape
    out, lse = _emu.aligned((B, Sq, H, D), np.float32), _emu.aligned((B, H, Sq), np.float32)
    _capi.check(L, L.lwm_attn_combine(op.ctypes.data, lp.ctypes.data, P, _capi.LwmTensor4(None, 0, 0, 0), out.ctypes.data,
                                      lse.ctypes.data, B, Sq, H, D, None), "lwm_attn_combine")
    return out, lse


def emu_decode(q, kq, ks, vq, vs, mask, k_splits, scale=None):
    """-> (out f32 (B,1,H,128), lse (B,H,1), partials) through lwm_attn_decode_kv6 + lwm_attn_combine"""
    L = _emu.lib()
    B, _, H, D = q.shape
    Sk = kq.shape[1]
    qb = _emu.bf16_array(q)
    a = _capi.LwmKv6DecodeArgs()
    a.q = _emu._t4(qb)
    _fill(a, kq, ks, vq, vs)
    if mask is not None:
        mask = np.ascontiguousarray(mask.reshape(B, Sk).astype(np.uint8))
        a.dense_mask, a.mask_stride_b = mask.ctypes.data, Sk
    a.B, a.Sk, a.H, a.D, a.scale, a.k_splits = B, Sk, H, D, (1.0 / np.sqrt(D) if scale is None else scale), k_splits
    P = max(1, k_splits)
    op, lp = _emu.aligned((P, B, 1, H, D), np.float32), _emu.aligned((P, B, H, 1), np.float32)
    op[...], lp[...] = np.nan, np.nan                      # the kernel must write every partial
    a.out_acc, a.lse_acc = op.ctypes.data, lp.ctypes.data
    _capi.check(L, L.lwm_attn_decode_kv6(C.byref(a), None), "lwm_attn_decode_kv6")
    out, lse = emu_combine(op, lp)
    return out, lse, op, lp


# ---------------------------------------------------------------- the restatement itself, in fp64
def test_restatement_self_check():
    ties = np.array(list(K6.TIES))
    assert len(ties) == 31 and K6.E2M3_MAG[31] == 7.5 and (np.diff(K6.E2M3_MAG) > 0).all()
    y = np.concatenate([np.linspace(-7.5, 7.5, 60001), ties, -ties, K6.E2M3_MAG, -K6.E2M3_MAG])
    c = K6.e2m3_encode(y)
    got = K6.e2m3_decode(c)
    # a nearest representable magnitude, with the sign of y
    best = np.abs(np.abs(y)[:, None] - K6.E2M3_MAG).min(-1)
    assert np.array_equal(np.abs(np.abs(got) - np.abs(y)), best)
    assert np.array_equal(np.signbit(got), np.signbit(y))
    for t, want in K6.TIES.items():                       # every midpoint goes to the even code
        assert K6.e2m3_decode(K6.e2m3_encode(t)) == want and K6.e2m3_decode(K6.e2m3_encode(-t)) == -want
        assert K6.e2m3_encode(t) % 2 == 0 and abs(want - t) == best[np.flatnonzero(y == t)[0]]
    assert K6.e2m3_encode(-0.0) == 32 and K6.e2m3_encode(0.0) == 0
    assert np.array_equal(K6.e2m3_encode(K6.e2m3_decode(np.arange(64, dtype=np.uint8))), np.arange(64, dtype=np.uint8))
    # the packing against its definition: a block's bytes as one little-endian integer
    cd = np.random.default_rng(1).integers(0, 64, (3, 128)).astype(np.uint8)
    pk = K6.pack(cd)
    assert pk.shape == (3, 96) and np.array_equal(K6.codes(pk), cd)
    for r in range(3):
        for b in range(4):
            assert np.array_equal(K6.block_as_int(pk[r, 24 * b:24 * b + 24]), cd[r, 32 * b:32 * b + 32])
    for k in range(-120, 121):                            # 7.5 * 2^k and one bf16 ulp (2^-5 * 2^k at 7.5) either side
        assert K6.scale_for(7.5 * 2.0 ** k) == 2.0 ** k
        assert K6.scale_for(7.46875 * 2.0 ** k) == 2.0 ** k
        assert K6.scale_for(7.53125 * 2.0 ** k) == 2.0 ** (k + 1)
    assert K6.scale_exp_for(0.0) == 127 and K6.scale_exp_for(2.0 ** -133) == 1 and K6.scale_exp_for(7.5 * 2.0 ** -126) == 1
    assert K6.scale_exp_for(7.53125 * 2.0 ** -126) == 2
    assert K6.scale_exp_for(float(np.float32(3.3895e38))) <= 254
    # smallest power of two: half of it no longer fits (except at the clamp and for all-zero blocks)
    x = _rows()[:256]
    x = np.concatenate([x, _rows()[4096:]])
    q, e = K6.quantise(x)
    amax = np.abs(x.astype(np.float64).reshape(-1, 4, 32)).max(-1)
    s = 2.0 ** (e.astype(np.float64) - 127)
    assert (amax / s <= 7.5).all()
    free = (amax > 0) & (e > 1)
    assert free.sum() > 1000 and (amax[free] / (s[free] / 2) > 7.5).all()
    assert e.min() >= 1 and e.max() <= 254


def test_derived_properties():
    """what the header promises of the format, away from the lower clamp, on the random rows and the edge rows"""
    x = _rows().astype(np.float64)
    q6, e6 = K6.quantise(x)
    q4, e4 = K4.quantise(x)
    d6, d4 = K6.dequant(q6, e6), K4.dequant(q4, e4)
    xb, err6, err4 = (t.reshape(-1, 4, 32) for t in (x, np.abs(x - d6), np.abs(x - d4)))
    amax = np.abs(xb).max(-1)
    s6, s4 = 2.0 ** (e6.astype(np.float64) - 127).reshape(-1, 4), 2.0 ** (e4.astype(np.float64) - 127).reshape(-1, 4)
    free = (e6.reshape(-1, 4) > 1) & (e4.reshape(-1, 4) > 1) & (amax > 0)
    assert free.sum() > 16000 and (~free).sum() > 0
    S6, A = s6[..., None], amax[..., None]
    f = np.broadcast_to(free[..., None], xb.shape)
    assert (err6 <= S6 / 4)[f].all()                      # the widest step, in [4, 7.5], is s / 2
    assert (s6 < amax / 3.75)[free].all()
    assert (err6 < A / 15)[f].all()
    big = f & (np.abs(xb) >= S6)
    assert big.sum() > 100000 and (err6 <= 2.0 ** -4 * np.abs(xb))[big].all()
    # s6 is s4 or s4 / 2, and element by element the 6-bit error is never larger than the 4-bit one
    assert (((s6 == s4) | (s6 == s4 / 2))[free]).all() and (s6 == s4)[free].any() and (s6 == s4 / 2)[free].any()
    assert (err6 <= err4)[f].all()
    Af = np.broadcast_to(A, xb.shape)[f]
    print(f"mean |x - dq| / amax over {int(free.sum())} blocks: 6-bit {float((err6[f] / Af).mean()):.4f}, "
          f"4-bit {float((err4[f] / Af).mean()):.4f}")


def test_dequant_round_trips_through_bf16():
    """q * s is a bf16 number: the restatement's dequantised values and kv6_dequant agree exactly, for every code at
    every position of a block and a spread of scales at which every product is a normal number (byte >= 4: s >= 2^-123)"""
    import torch
    from lwm_amd import kv6
    ebytes = np.array([4, 27, 97, 119, 126, 127, 128, 134, 167, 252], np.uint8)      # (7.5 * 2^125 is below the top of bf16)
    pos = np.arange(32)
    cd = np.stack([np.tile((pos + c) % 64, 4) for c in range(64)]).astype(np.uint8)   # (64, 128): every code at every position
    q = np.repeat(K6.pack(cd)[None], len(ebytes), 0)                                  # (10, 64, 96)
    e = np.broadcast_to(ebytes[:, None, None], (len(ebytes), 64, 4)).copy()
    want = K6.dequant(q, e)
    assert np.array_equal(R.round_bf16(want.astype(np.float32)).astype(np.float64), want)
    assert np.abs(want).min() == 0 and np.abs(want[want != 0]).min() >= 2.0 ** -126
    d = kv6.kv6_dequant(torch.from_numpy(q), torch.from_numpy(e))
    assert d.dtype == torch.bfloat16 and tuple(d.shape) == (len(ebytes), 64, 128)
    assert np.array_equal(d.float().numpy().astype(np.float64), want)
    assert np.array_equal(np.signbit(d.float().numpy()), np.signbit(want))
    assert np.array_equal(kv6.kv6_codes(torch.from_numpy(q)).numpy().astype(np.uint8), np.broadcast_to(cd, (len(ebytes), 64, 128)))
    with pytest.raises(ValueError, match="kv6_dequant"):
        kv6.kv6_dequant(torch.from_numpy(q[..., :64].copy()), torch.from_numpy(e))
    # the same for quantised rows, the edge rows included, wherever the products are normal numbers below the top of bf16
    x = _rows()[4000:]
    q, e = K6.quantise(x)
    ok = (e >= 4).all(-1) & (np.abs(x).max(-1) < 1e38)
    assert ok.sum() >= x.shape[0] - 5
    dq = K6.dequant(q[ok], e[ok])
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
    q, e = K6.quantise(src)
    assert np.array_equal(scale, e), np.argwhere(scale != e)[:8]
    bad = np.argwhere(K6.codes(cache) != K6.codes(q))
    assert bad.size == 0, [(tuple(i), K6.codes(cache)[tuple(i)], K6.codes(q)[tuple(i)], src[tuple(i)]) for i in bad[:8]]
    assert np.array_equal(cache, q)
    # negative zero keeps its sign bit; byte 255 is never written; the four-block row has four different bytes
    nz = np.signbit(src) & (src == 0)
    assert nz.any() and (K6.codes(cache)[nz] == 32).all()
    assert scale.max() <= 254 and scale.min() >= 1
    assert any(len(set(r)) == 4 for r in e.reshape(-1, 4)[4096:])


@pytest.mark.parametrize("H", [1, 3, 32])
def test_write_at_equals_host_index_and_skips_outside_rows(H):
    B, S, n = 2, 12, 4
    src = _rnd((B, 6, H, 128), 5, 3.0)
    q, s = K6.quantise(src)

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
    # blocks of different magnitude inside a head, so that a wrong scale byte or block order shows
    k[..., 32:64] *= 0.25
    k[..., 64:96] *= 4.0
    v[..., :32] *= 0.125
    v[..., 96:] *= 8.0
    kq, ks = emu_cache(B, Sk, H)
    vq, vs = emu_cache(B, Sk, H)
    kq[...], ks[...] = K6.quantise(k)
    vq[...], vs[...] = K6.quantise(v)
    return kq, ks, vq, vs


_DEQ = lambda q, e: K6.dequant(q, e).astype(np.float32)          # (exact: bf16 numbers)


@pytest.mark.parametrize("B,Sk,H,splits,cache_index", [
    (2, 300, 2, 3, 250),         # 64 key lanes per head, ragged pieces
    (1, 64, 32, 1, 63),          # the LWM-7B head count: four keys per pass, one piece
    (1, 130, 3, 2, 129),         # a head count that is no power of two: one idle slot in four
    (1, 40, 130, 2, 39),         # more heads than slots: two passes over the heads
])
def test_decode_kv6_vs_oracle(B, Sk, H, splits, cache_index):
    q = _rnd((B, 1, H, 128), 1)
    kq, ks, vq, vs = _quantised_cache(B, Sk, H, 2)
    assert len(set(ks[0, 0, 0])) >= 3 and len(set(vs[0, 0, 0])) >= 3
    am = (np.random.default_rng(4).random((B, Sk)) > 0.1).astype(np.uint8)       # random 10 % holes
    am[:, cache_index] = 1
    mask = R.decode_mask(B, 1, Sk, cache_index, am)
    out, lse, _, _ = emu_decode(q, kq, ks, vq, vs, mask, splits)
    # the oracle gets the DEQUANTISED cache: quantisation error is not in the comparison
    ro, rl = R.dense_attention(q, _DEQ(kq, ks), _DEQ(vq, vs), causal=False, dense_mask=mask)
    e_out, e_lse = np.abs(out - ro).max() / np.abs(ro).max(), np.abs(lse - rl).max()
    print(f"kv6 decode (emulated) B={B} Sk={Sk} H={H} splits={splits}: out {e_out:.3e} of max, lse {e_lse:.3e}")
    assert e_out <= 2e-2
    assert e_lse <= 2e-3


def test_decode_kv6_mask_behaviour():
    """no mask = all visible; 0xFF code bytes and 0xFF scale bytes (and other garbage) in masked rows change nothing; a
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
        (ka, sa), (va, ta) = emu_cache(B, Sk, H), emu_cache(B, Sk, H)        # (16-byte aligned copies)
        ka[...], sa[...], va[...], ta[...] = kq, ks, vq, vs
        for c, s in ((ka, sa), (va, ta)):
            c[hid] = rng.integers(0, 256, (int(hid.sum()), 96)).astype(np.uint8) if fill_q is None else fill_q
            s[hid] = rng.integers(0, 256, (int(hid.sum()), 4)).astype(np.uint8) if fill_s is None else fill_s
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


# ---------------------------------------------------------------- block kernel
# (B, Q, idx, cache_rows, H, k_splits, left padding of batch row 0 in key_valid or None = no key_valid tensor): the cases
# of tests/test_emu_kv8_prefill.py, the smallest that crosses each of the 256-query tile, the 64-key tile and the splits
CASES = [
    (1, 3, 8, 32, 2, 1, 5),            # a short block behind a short prompt, one piece
    (2, 300, 70, 512, 2, 2, 9),        # two q tiles, idx off the 64 grid, ragged last key tile, batch strides, left padding
    (1, 256, 256, 1024, 8, 4, None),   # B * H a multiple of 8 (the XCD map); Sk % 64 == 0 and no key_valid: no key meta
    (1, 64, 1000, 1100, 3, 3, 5),      # B * H no multiple of 8; 6 of the 8 waves idle
    (1, 1, 500, 512, 4, 2, 5),         # one query
    (1, 5, 60, 128, 2, 4, None),       # Sk = 65: two key tiles cut into four pieces, pieces 2 and 3 walk no tile -> (0, -inf), all written
    (1, 40, 0, 64, 1, 2, 3),           # q_start = 0, one ragged tile with the diagonal inside, second piece empty, left padding
]
IDS = ["B%d-Q%d-idx%d-rows%d-H%d-splits%d" % c[:6] for c in CASES]


def emu_prefill(q, kq, ks, vq, vs, Sk, idx, key_valid, k_splits, scale=None):
    """lwm_attn_prefill_kv6 over the first Sk rows of the caches (the strides are the whole cache's); key_valid u8
    (B, cache_rows) or None -> the partials (o_parts (P,B,Sq,H,D), lse_parts (P,B,H,Sq))"""
    L = _emu.lib()
    B, Sq, H, D = q.shape
    qb = _emu.bf16_array(q)
    a = _capi.LwmKv6PrefillArgs()
    a.q = _emu._t4(qb)
    _fill(a, kq, ks, vq, vs)
    if key_valid is not None:
        assert key_valid.dtype == np.uint8 and key_valid.strides[1] == 1
        a.key_valid, a.key_valid_stride_b = key_valid.ctypes.data, key_valid.strides[0]
    a.B, a.Sq, a.Sk, a.H, a.D = B, Sq, Sk, H, D
    a.q_start, a.scale, a.k_splits = idx, (1.0 / np.sqrt(D) if scale is None else scale), k_splits
    P = max(1, k_splits)
    op, lp = _emu.aligned((P, B, Sq, H, D), np.float32), _emu.aligned((P, B, H, Sq), np.float32)
    op[...], lp[...] = np.nan, np.nan          # the call must write every element
    a.out_acc, a.lse_acc = op.ctypes.data, lp.ctypes.data
    _capi.check(L, L.lwm_attn_prefill_kv6(C.byref(a), None), "lwm_attn_prefill_kv6")
    return op, lp


def emu_fwd_parts(q, kd, vd, idx, key_valid, k_splits):
    """the emulated lwm_attn_fwd in its partials form (final_out = 0, k_splits >= 2: attn_fwd_infer_kernel) on bf16 K/V"""
    L = _emu.lib()
    B, Sq, H, D = q.shape
    qb, kb, vb = _emu.bf16_array(q), _emu.bf16_array(kd), _emu.bf16_array(vd)
    a, keep = _emu.base_args(qb, kb, vb, causal=True, q_start=idx, k_start=0, seg_q=None, seg_k=None, key_valid=key_valid,
                             scale=None)
    op, lp = _emu.aligned((k_splits, B, Sq, H, D), np.float32), _emu.aligned((k_splits, B, H, Sq), np.float32)
    a.out_acc, a.lse_acc, a.k_splits, a.final_out, a.carry_in = op.ctypes.data, lp.ctypes.data, k_splits, 0, 0
    _capi.check(L, L.lwm_attn_fwd(C.byref(a), None), "lwm_attn_fwd")
    return op, lp


@functools.lru_cache(maxsize=None)
def _case(i):
    """inputs of case i and the kernel's answer on them, computed once and shared (nothing below writes to them)"""
    B, Q, idx, rows, H, n, pad = CASES[i]
    Sk = idx + Q
    q = _rnd((B, Q, H, 128), 100 + i)
    k, v = _rnd((B, rows, H, 128), 200 + i, 1.5), _rnd((B, rows, H, 128), 300 + i, 0.7)
    k[..., 32:64] *= 0.25                      # blocks of different magnitude inside a head
    v[..., 96:] *= 8.0
    kq, ks = emu_cache(B, rows, H)
    vq, vs = emu_cache(B, rows, H)
    kq[...], ks[...] = K6.quantise(k)
    vq[...], vs[...] = K6.quantise(v)
    kv = None
    if pad is not None:
        kv = np.ones((B, rows), np.uint8)
        kv[0, :pad] = 0
    op, lp = emu_prefill(q, kq, ks, vq, vs, Sk, idx, kv, n)
    for t in (q, kq, ks, vq, vs, op, lp) + (() if kv is None else (kv,)):
        t.flags.writeable = False
    return q, kq, ks, vq, vs, kv, op, lp


def _valid(kv, Sk):
    return None if kv is None else np.ascontiguousarray(kv[:, :Sk])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv6_vs_oracle(i):
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    assert not np.isnan(op).any() and not np.isnan(lp).any()
    out, lse = emu_combine(op, lp)
    ro, rl = R.dense_attention(q, _DEQ(kq[:, :Sk], ks[:, :Sk]), _DEQ(vq[:, :Sk], vs[:, :Sk]), causal=True, q_start=idx,
                               key_valid=_valid(kv, Sk))
    none = np.isneginf(rl)              # rows that see nothing: -inf exactly (-inf minus -inf is no error, it is nan)
    assert np.array_equal(np.isneginf(lse), none)
    eo, el = np.abs(out - ro).max() / np.abs(ro).max(), np.abs(lse[~none] - rl[~none]).max()
    print(f"out {eo:.3e} of max (bound 2e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 2e-2
    assert el <= 2e-3


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[5] >= 2], ids=[IDS[i] for i, c in enumerate(CASES) if c[5] >= 2])
def test_prefill_kv6_partials_equal_the_bf16_kernel_bit_for_bit(i):
    """pins the staging, the swizzle, the block order and the scale indexing: the LDS tiles are the tiles of a bf16 copy"""
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    fo, fl = emu_fwd_parts(q, _DEQ(kq[:, :Sk], ks[:, :Sk]), _DEQ(vq[:, :Sk], vs[:, :Sk]), idx, _valid(kv, Sk), n)
    assert np.array_equal(op.view(np.uint32), fo.view(np.uint32))
    assert np.array_equal(lp.view(np.uint32), fl.view(np.uint32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv6_hidden_rows_reach_nothing(i):
    """rows at or past idx + Q and rows with key_valid == 0 hold 0xFF bytes with 0xFF scales, zero scales, or random bytes:
    the same bits come out"""
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    hid = np.zeros((B, rows), bool)
    hid[:, Sk:] = True
    if kv is not None:
        hid |= kv == 0
    assert hid.any()
    hid = np.broadcast_to(hid[:, :, None], (B, rows, H))
    rng = np.random.default_rng(3)
    for fill_q, fill_s in ((0xFF, 0xFF), (0x77, 0x00), (None, None)):
        (ka, sa), (va, ta) = emu_cache(B, rows, H), emu_cache(B, rows, H)
        ka[...], sa[...], va[...], ta[...] = kq, ks, vq, vs
        for c, s in ((ka, sa), (va, ta)):
            c[hid] = rng.integers(0, 256, (int(hid.sum()), 96)).astype(np.uint8) if fill_q is None else fill_q
            s[hid] = rng.integers(0, 256, (int(hid.sum()), 4)).astype(np.uint8) if fill_s is None else fill_s
        o2, l2 = emu_prefill(q, ka, sa, va, ta, Sk, idx, kv, n)
        assert np.array_equal(o2.view(np.uint32), op.view(np.uint32)) and np.array_equal(l2.view(np.uint32), lp.view(np.uint32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv6_a_row_that_sees_nothing(i):
    """the last batch row with key_valid all zero: out 0 and lse -inf in every partial; the other rows unchanged"""
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    kv2 = np.ones((B, rows), np.uint8) if kv is None else kv.copy()
    kv2[B - 1] = 0
    o2, l2 = emu_prefill(q, kq, ks, vq, vs, Sk, idx, kv2, n)
    assert (o2[:, B - 1] == 0).all() and np.isneginf(l2[:, B - 1]).all()
    out, lse = emu_combine(o2, l2)
    assert (out[B - 1] == 0).all() and np.isneginf(lse[B - 1]).all()
    if B > 1 and kv is not None:
        assert np.array_equal(o2[:, :B - 1], op[:, :B - 1]) and np.array_equal(l2[:, :B - 1], lp[:, :B - 1])


def test_prefill_kv6_one_query_against_the_decode_kernel():
    """Q = 1: the block kernel and the streaming decode kernel are two routes of the same attention"""
    i = [c[1] for c in CASES].index(1)
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    out, lse = emu_combine(op, lp)
    mask = R.decode_mask(B, 1, Sk, idx, kv[:, :Sk])
    (ka, sa), (va, ta) = emu_cache(B, Sk, H), emu_cache(B, Sk, H)
    ka[...], sa[...], va[...], ta[...] = kq[:, :Sk], ks[:, :Sk], vq[:, :Sk], vs[:, :Sk]
    do, dl, _, _ = emu_decode(q, ka, sa, va, ta, mask, n)
    eo, el = np.abs(out - do).max() / np.abs(do).max(), np.abs(lse - dl).max()
    print(f"block kernel against decode kernel: out {eo:.3e} of max (bound 1.6e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 1.6e-2
    assert el <= 2e-3


# ---------------------------------------------------------------- validation and the ABI
def _abi_checks(L):
    assert L.lwm_version() >= 630
    assert L.lwm_sizeof(13) == C.sizeof(_capi.LwmKv6DecodeArgs)
    assert L.lwm_sizeof(14) == C.sizeof(_capi.LwmKv6PrefillArgs)
    assert L.lwm_attn_decode_kv6(None, None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    assert L.lwm_attn_prefill_kv6(None, None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()


def _validation(L):
    """every refusal returns its code and names its reason (host-side checks: nothing is launched before the last call of
    each entry, and those launches are what the emulated library is for)"""
    _abi_checks(L)
    q = _rnd((1, 1, 2, 128), 1)
    kq, ks, vq, vs = _quantised_cache(1, 16, 2, 2)
    a = _capi.LwmKv6DecodeArgs()
    qb = _emu.bf16_array(q)                   # (kept alive with everything else the structs point at: `keep` below)
    a.q = _emu._t4(qb)
    a.B, a.Sk, a.H, a.D, a.scale, a.k_splits = 1, 16, 2, 64, 0.1, 1
    assert L.lwm_attn_decode_kv6(C.byref(a), None) == _capi.LWM_EINVAL and b"head_dim" in L.lwm_last_error()
    a.D = 128
    assert L.lwm_attn_decode_kv6(C.byref(a), None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    op, lp = _emu.aligned((1, 1, 1, 2, 128), np.float32), _emu.aligned((1, 1, 2, 1), np.float32)
    a.out_acc, a.lse_acc = op.ctypes.data, lp.ctypes.data
    _fill(a, kq, ks, vq, vs)
    a.k = kq.ctypes.data + 4
    assert L.lwm_attn_decode_kv6(C.byref(a), None) == _capi.LWM_EINVAL and b"aligned" in L.lwm_last_error()
    a.k = kq.ctypes.data
    a.v_stride_s = vq.strides[1] + 4
    assert L.lwm_attn_decode_kv6(C.byref(a), None) == _capi.LWM_EINVAL and b"aligned" in L.lwm_last_error()
    a.v_stride_s = vq.strides[1]
    a.k_stride_h = 64
    assert L.lwm_attn_decode_kv6(C.byref(a), None) == _capi.LWM_EINVAL and b"strides" in L.lwm_last_error()
    a.k_stride_h = 96
    for bad in (-1, 4097):
        a.k_splits = bad
        assert L.lwm_attn_decode_kv6(C.byref(a), None) == _capi.LWM_EINVAL and b"k_splits" in L.lwm_last_error()
    a.k_splits = 1
    # the write refuses rows that are not H * 128 elements, null pointers and misaligned tensors
    src = _emu.bf16_array(_rnd((1, 1, 2, 128), 3))
    w = lambda cache, s, row_elems: L.lwm_kv6_cache_write(cache, src.ctypes.data, 1, kq.strides[0], 256, 0, 0, 1, row_elems, s,
                                                         ks.strides[0], 2, None)
    assert w(kq.ctypes.data, ks.ctypes.data, 200) == _capi.LWM_EINVAL and b"row_elems" in L.lwm_last_error()
    assert w(kq.ctypes.data + 4, ks.ctypes.data, 256) == _capi.LWM_EINVAL and b"misaligned" in L.lwm_last_error()
    assert w(None, None, 256) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    assert L.lwm_kv6_cache_write_at(kq.ctypes.data, src.ctypes.data, 1, kq.strides[0], 256, None, 0, 16, 0, 1, 256, ks.ctypes.data,
                                    ks.strides[0], 2, None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    # the block kernel
    p = _capi.LwmKv6PrefillArgs()
    q4 = _rnd((1, 4, 2, 128), 1)
    q4b = _emu.bf16_array(q4)
    p.q = _emu._t4(q4b)
    p.B, p.Sq, p.Sk, p.H, p.D, p.q_start, p.scale, p.k_splits = 1, 4, 16, 2, 64, 12, 0.1, 1
    assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_EUNSUPPORTED and b"head_dim" in L.lwm_last_error()
    p.D = 128
    assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    op4, lp4 = _emu.aligned((1, 1, 4, 2, 128), np.float32), _emu.aligned((1, 1, 2, 4), np.float32)
    ptrs = dict(k=kq, v=vq, k_scale=ks, v_scale=vs, out_acc=op4, lse_acc=lp4)
    _fill(p, kq, ks, vq, vs)
    p.out_acc, p.lse_acc = op4.ctypes.data, lp4.ctypes.data
    for n, t in ptrs.items():                # each pointer on its own
        setattr(p, n, None)
        assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error(), n
        setattr(p, n, t.ctypes.data)
    p.k = kq.ctypes.data + 4
    assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_EUNSUPPORTED and b"aligned" in L.lwm_last_error()
    p.k = kq.ctypes.data
    p.v_stride_s = vq.strides[1] + 4
    assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_EUNSUPPORTED and b"aligned" in L.lwm_last_error()
    p.v_stride_s = vq.strides[1]
    p.v_stride_h = 64
    assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_EINVAL and b"strides" in L.lwm_last_error()
    p.v_stride_h = 96
    for field, bad in (("Sq", 0), ("Sk", 0), ("k_splits", -1), ("k_splits", 4097), ("q_start", -1)):
        good = getattr(p, field)
        setattr(p, field, bad)
        assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_EINVAL, field
        setattr(p, field, good)
    return a, p, w, (kq, ks, src), (qb, q4b, vq, vs, op, lp, op4, lp4)


def test_validation_and_abi():
    L = _emu.lib()
    a, p, w, (kq, ks, src), keep = _validation(L)
    assert L.lwm_attn_decode_kv6(C.byref(a), None) == _capi.LWM_OK
    assert L.lwm_attn_prefill_kv6(C.byref(p), None) == _capi.LWM_OK
    assert w(kq.ctypes.data, ks.ctypes.data, 256) == _capi.LWM_OK
    idx = np.zeros(1, np.int32)
    assert L.lwm_kv6_cache_write_at(kq.ctypes.data, src.ctypes.data, 1, kq.strides[0], 256, idx.ctypes.data, 0, 16, 0, 1, 256,
                                    ks.ctypes.data, ks.strides[0], 2, None) == _capi.LWM_OK


def test_product_library_validation_and_abi():
    """the same refusals from liblwm_hip.so: they are decided on the host, before anything is launched"""
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    _validation(_capi.bind(C.CDLL(so)))
