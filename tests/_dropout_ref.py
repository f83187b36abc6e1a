"""numpy restatement of the dropout kernels (lwm_amd/csrc/dropout.h; "dropout" in include/lwm_hip.h): the mask rule and
both kernels, on tests/_sample_ref.philox4x32_10 -- the reference the emulated and the device kernels are held to, bit
for bit.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle.attention_ref import from_bf16_bits, to_bf16_bits
from tests._sample_ref import philox4x32_10


def thr_inv(p):
    """p -> (thr16 = round(p * 65536), inv = the f32 nearest to 1 / (1 - thr16 / 65536), from f64)"""
    thr16 = int(np.floor(float(p) * 65536.0 + 0.5))
    assert 0 <= thr16 <= 65535, p
    return thr16, np.float32(1.0 / (1.0 - thr16 / 65536.0))


def halfwords(B, S, C, *, key0, key1, site, s_offset=0):
    """(B, S, C) uint32 in [0, 65536): the 16 bits element (b, s, c) is judged by.  One Philox call per 8 channels, key
    (key0, key1), counter (c / 8, s_offset + s, b, site); element c reads output word (c % 8) / 2, low half for even c,
    high half for odd c."""
    assert C % 8 == 0
    ctr = np.zeros((B, S, C // 8, 4), np.uint64)
    ctr[..., 0] = np.arange(C // 8, dtype=np.uint64)[None, None, :]
    ctr[..., 1] = ((np.arange(S, dtype=np.uint64) + np.uint64(s_offset)) & np.uint64(0xFFFFFFFF))[None, :, None]
    ctr[..., 2] = np.arange(B, dtype=np.uint64)[:, None, None]
    ctr[..., 3] = np.uint64(site)
    w = philox4x32_10(ctr, (int(key1) << 32) | int(key0))                        # (B, S, C/8, 4) uint32
    return np.stack((w & np.uint32(0xFFFF), w >> np.uint32(16)), axis=-1).reshape(B, S, C)


def keep_mask(B, S, C, *, thr16, **rule):
    """(B, S, C) bool: drop iff the element's half-word < thr16"""
    return halfwords(B, S, C, **rule) >= np.uint32(thr16)


def dropout_add_f32(x, res=None, *, thr16, inv, **rule):
    """res + (keep ? x * inv : +0): one f32 product, one f32 add; res None: the product alone.  Also the backward
    (x = the incoming gradient, res None)."""
    x = np.asarray(x, np.float32)
    B, S, C = x.shape
    d = np.where(keep_mask(B, S, C, thr16=thr16, **rule), x * np.float32(inv), np.float32(0.0)).astype(np.float32)
    return d if res is None else (np.asarray(res, np.float32) + d).astype(np.float32)


def dropout_add_bf16(x_bits, res_bits=None, **kw):
    """the same on bf16 bit patterns (uint16), with the one rounding to bf16 (nearest even) at the end"""
    y = dropout_add_f32(from_bf16_bits(x_bits), None if res_bits is None else from_bf16_bits(res_bits), **kw)
    return to_bf16_bits(y)
