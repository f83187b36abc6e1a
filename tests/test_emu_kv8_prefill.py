"""Block attention over the 8-bit (e4m3) KV cache on the CPU: the kernel of csrc/attn_prefill_kv8.h host-emulated through
the C ABI -- against the fp64 oracle on the dequantised cache, BIT FOR BIT against the emulated lwm_attn_fwd split-K
kernel on a bf16 copy of the cache (the staged tiles are exact: q * s is a bf16 number), with garbage in every row the
mask hides, and the ABI mirror.

Bounds are the project's own: out against the oracle 2e-2 of max, lse 2e-3 (tests/test_emu_kv8.py); two routes of the
same attention 1.6e-2 of max (tests/test_gpu_infer.py).  Inputs have magnitude 0.7 .. 1.5: no row has an amax anywhere
near 2^-100, so every dequantised value is a normal bf16."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _emu, _kv8_ref as K8
from tests.test_emu_kv8 import _rnd, emu_cache, emu_decode

# (B, Q, idx, cache_rows, H, k_splits, left padding of batch row 0 in key_valid or None = no key_valid tensor)
CASES = [
    (1, 3, 8, 32, 2, 1, 5),            # the shape the unmarked cache refuses: a short block behind a short prompt
    (2, 300, 70, 512, 2, 2, 9),        # two q tiles, idx off the 64 grid, ragged last key tile, batch strides, left padding
    (1, 256, 256, 1024, 8, 4, None),   # B * H a multiple of 8 (the XCD map); Sk % 64 == 0 and no key_valid: no key meta
    (1, 64, 1000, 1100, 3, 3, 5),      # B * H no multiple of 8; 6 of the 8 waves idle
    (1, 1, 500, 512, 4, 2, 5),         # one query
    (1, 5, 60, 128, 2, 4, None),       # Sk = 65: two key tiles cut into four pieces, pieces 2 and 3 walk no tile -> (0, -inf), all written
    (1, 40, 0, 64, 1, 2, 3),           # q_start = 0, one ragged tile with the diagonal inside, second piece empty, left padding
]
IDS = ["B%d-Q%d-idx%d-rows%d-H%d-splits%d" % c[:6] for c in CASES]


def emu_prefill(q, kq, ks, vq, vs, Sk, idx, key_valid, k_splits, scale=None):
    """lwm_attn_prefill_kv8 over the first Sk rows of the caches (views: the strides are the whole cache's); key_valid u8
    (B, cache_rows) or None -> the partials (o_parts (P,B,Sq,H,D), lse_parts (P,B,H,Sq))"""
    L = _emu.lib()
    B, Sq, H, D = q.shape
    qb = _emu.bf16_array(q)
    a = _capi.LwmKv8PrefillArgs()
    a.q = _emu._t4(qb)
    a.k, a.v, a.k_scale, a.v_scale = kq.ctypes.data, vq.ctypes.data, ks.ctypes.data, vs.ctypes.data
    a.k_stride_b, a.k_stride_s, a.k_stride_h = kq.strides[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = vq.strides[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = (s // 4 for s in ks.strides[:2])
    a.v_scale_stride_b, a.v_scale_stride_s = (s // 4 for s in vs.strides[:2])
    if key_valid is not None:
        assert key_valid.dtype == np.uint8 and key_valid.strides[1] == 1
        a.key_valid, a.key_valid_stride_b = key_valid.ctypes.data, key_valid.strides[0]
    a.B, a.Sq, a.Sk, a.H, a.D = B, Sq, Sk, H, D
    a.q_start, a.scale, a.k_splits = idx, (1.0 / np.sqrt(D) if scale is None else scale), k_splits
    P = max(1, k_splits)
    op, lp = _emu.aligned((P, B, Sq, H, D), np.float32), _emu.aligned((P, B, H, Sq), np.float32)
    op[...], lp[...] = np.nan, np.nan          # the call must write every element
    a.out_acc, a.lse_acc = op.ctypes.data, lp.ctypes.data
    _capi.check(L, L.lwm_attn_prefill_kv8(C.byref(a), None), "lwm_attn_prefill_kv8")
    return op, lp


def emu_combine(op, lp):
    L = _emu.lib()
    P, B, Sq, H, D = op.shape
    out, lse = _emu.aligned((B, Sq, H, D), np.float32), _emu.aligned((B, H, Sq), np.float32)
    _capi.check(L, L.lwm_attn_combine(op.ctypes.data, lp.ctypes.data, P, _capi.LwmTensor4(None, 0, 0, 0), out.ctypes.data,
                                      lse.ctypes.data, B, Sq, H, D, None), "lwm_attn_combine")
    return out, lse


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
    kq, ks = emu_cache(B, rows, H)
    vq, vs = emu_cache(B, rows, H)
    kq[...], ks[...] = K8.quantise(k)
    vq[...], vs[...] = K8.quantise(v)
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
def test_prefill_kv8_vs_oracle(i):
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    assert not np.isnan(op).any() and not np.isnan(lp).any()
    out, lse = emu_combine(op, lp)
    # the oracle gets the DEQUANTISED cache: quantisation error is not in the comparison
    ro, rl = R.dense_attention(q, K8.dequant(kq[:, :Sk], ks[:, :Sk]), K8.dequant(vq[:, :Sk], vs[:, :Sk]), causal=True,
                               q_start=idx, key_valid=_valid(kv, Sk))
    none = np.isneginf(rl)              # rows that see nothing: -inf exactly (-inf minus -inf is no error, it is nan)
    assert np.array_equal(np.isneginf(lse), none)
    eo, el = np.abs(out - ro).max() / np.abs(ro).max(), np.abs(lse[~none] - rl[~none]).max()
    print(f"out {eo:.3e} of max (bound 2e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 2e-2
    assert el <= 2e-3


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[5] >= 2], ids=[IDS[i] for i, c in enumerate(CASES) if c[5] >= 2])
def test_prefill_kv8_partials_equal_the_bf16_kernel_bit_for_bit(i):
    """pins the staging, the swizzle and the scale indexing: the LDS tiles are the tiles of a bf16 copy of the cache"""
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    fo, fl = emu_fwd_parts(q, K8.dequant(kq[:, :Sk], ks[:, :Sk]), K8.dequant(vq[:, :Sk], vs[:, :Sk]), idx, _valid(kv, Sk), n)
    assert np.array_equal(op.view(np.uint32), fo.view(np.uint32))
    assert np.array_equal(lp.view(np.uint32), fl.view(np.uint32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv8_hidden_rows_reach_nothing(i):
    """rows at or past idx + Q and rows with key_valid == 0 hold e4m3 NaN patterns with NaN / Inf scales, or random
    bytes with scales of 1e30: the same bits come out"""
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
    for fill_q, fill_s in ((0x7f, np.nan), (0xff, np.inf), (None, None)):
        (ka, sa), (va, ta) = emu_cache(B, rows, H), emu_cache(B, rows, H)
        ka[...], sa[...], va[...], ta[...] = kq, ks, vq, vs
        for c, s in ((ka, sa), (va, ta)):
            c[hid] = rng.integers(0, 256, (int(hid.sum()), 128)).astype(np.uint8) if fill_q is None else fill_q
            s[hid] = rng.standard_normal(int(hid.sum())).astype(np.float32) * 1e30 if fill_s is None else fill_s
        o2, l2 = emu_prefill(q, ka, sa, va, ta, Sk, idx, kv, n)
        assert np.array_equal(o2.view(np.uint32), op.view(np.uint32)) and np.array_equal(l2.view(np.uint32), lp.view(np.uint32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv8_a_row_that_sees_nothing(i):
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


def test_prefill_kv8_one_query_against_the_decode_kernel():
    """Q = 1: the block kernel and the streaming decode kernel are two routes of the same attention"""
    i = [c[1] for c in CASES].index(1)
    B, Q, idx, rows, H, n, _ = CASES[i]
    Sk = idx + Q
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    out, lse = emu_combine(op, lp)
    mask = R.decode_mask(B, 1, Sk, idx, kv[:, :Sk])
    kc, sc, vc, tc = (np.ascontiguousarray(t[:, :Sk]) for t in (kq, ks, vq, vs))
    (ka, sa), (va, ta) = emu_cache(B, Sk, H), emu_cache(B, Sk, H)
    ka[...], sa[...], va[...], ta[...] = kc, sc, vc, tc
    do, dl, _, _ = emu_decode(q, ka, sa, va, ta, mask, n)
    eo, el = np.abs(out - do).max() / np.abs(do).max(), np.abs(lse - dl).max()
    print(f"block kernel against decode kernel: out {eo:.3e} of max (bound 1.6e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 1.6e-2
    assert el <= 2e-3


# ---------------------------------------------------------------- the ABI
def _abi_checks(L):
    assert L.lwm_version() >= 530
    assert L.lwm_sizeof(6) == C.sizeof(_capi.LwmKv8PrefillArgs)
    assert L.lwm_attn_prefill_kv8(None, None) == _capi.LWM_EINVAL


def test_product_library_abi():
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    _abi_checks(_capi.bind(C.CDLL(so)))


def test_prefill_kv8_validation_and_abi():
    L = _emu.lib()
    _abi_checks(L)
    q = _rnd((1, 4, 2, 128), 1)
    kq, ks = emu_cache(1, 16, 2)
    vq, vs = emu_cache(1, 16, 2)
    a = _capi.LwmKv8PrefillArgs()
    a.q = _emu._t4(_emu.bf16_array(q))
    a.B, a.Sq, a.Sk, a.H, a.D, a.q_start, a.scale, a.k_splits = 1, 4, 16, 2, 64, 12, 0.1, 1
    assert L.lwm_attn_prefill_kv8(C.byref(a), None) == _capi.LWM_EUNSUPPORTED and b"head_dim" in L.lwm_last_error()
    a.D = 128
    assert L.lwm_attn_prefill_kv8(C.byref(a), None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error()
    op, lp = _emu.aligned((1, 1, 4, 2, 128), np.float32), _emu.aligned((1, 1, 2, 4), np.float32)
    ptrs = dict(k=kq, v=vq, k_scale=ks, v_scale=vs, out_acc=op, lse_acc=lp)
    for n, t in ptrs.items():
        setattr(a, n, t.ctypes.data)
    a.k_stride_b, a.k_stride_s, a.k_stride_h = kq.strides[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = vq.strides[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = a.v_scale_stride_b, a.v_scale_stride_s = 32, 2
    for n, t in ptrs.items():                # each pointer on its own
        setattr(a, n, None)
        assert L.lwm_attn_prefill_kv8(C.byref(a), None) == _capi.LWM_EINVAL and b"null" in L.lwm_last_error(), n
        setattr(a, n, t.ctypes.data)
    a.k = kq.ctypes.data + 8
    assert L.lwm_attn_prefill_kv8(C.byref(a), None) == _capi.LWM_EUNSUPPORTED and b"aligned" in L.lwm_last_error()
    a.k = kq.ctypes.data
    a.v_stride_s = vq.strides[1] + 8
    assert L.lwm_attn_prefill_kv8(C.byref(a), None) == _capi.LWM_EUNSUPPORTED and b"aligned" in L.lwm_last_error()
    a.v_stride_s = vq.strides[1]
    for field, bad in (("Sq", 0), ("Sk", 0), ("k_splits", -1), ("k_splits", 4097), ("q_start", -1)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert L.lwm_attn_prefill_kv8(C.byref(a), None) == _capi.LWM_EINVAL, field
        setattr(a, field, good)
    assert L.lwm_attn_prefill_kv8(C.byref(a), None) == _capi.LWM_OK
