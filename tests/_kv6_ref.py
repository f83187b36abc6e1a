"""The 6-bit (MXFP6 e2m3) KV cache format restated in numpy, from its description (include/lwm_hip.h, "6-bit KV cache"),
not from the kernel.  TEST INFRASTRUCTURE ONLY.

Per block of 32 consecutive elements of a head (bf16 values x): amax = max |x|; s = the smallest power of two with
amax / s <= 7.5, its biased exponent clamped to [1, 254], s = 1 when amax == 0; q = e2m3(x / s), round to nearest, ties to
the even code; -0 keeps its sign.  Element j of a block is bits [6j, 6j + 6) of the block's 24 bytes read as one
little-endian integer; one e8m0 byte (2^(b - 127)) per block.  Everything here is computed in float64."""
import numpy as np

E2M3_MAX = 7.5
# magnitude codes 0..31; bit 5 is the sign: c / 8 below 8, (1 + (c & 7) / 8) * 2^((c >> 3) - 1) from 8 on
E2M3_MAG = np.array([c / 8.0 if c < 8 else (1.0 + (c & 7) / 8.0) * 2.0 ** ((c >> 3) - 1) for c in range(32)], np.float64)
# midpoint of two neighbouring magnitudes -> the value of the even code of the two
TIES = {float((E2M3_MAG[c] + E2M3_MAG[c + 1]) / 2): float(E2M3_MAG[c + (c & 1)]) for c in range(31)}


def e2m3_encode(y):
    """f64 (finite, |y| <= 7.5) -> e2m3 code 0..63: the nearest magnitude; of two equally near ones the even code."""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    assert np.all(np.isfinite(a)) and np.all(a <= E2M3_MAX)
    d = np.abs(a[..., None] - E2M3_MAG)                   # distances to the 32 magnitudes: exact in f64 for bf16-derived y
    best = d.min(-1, keepdims=True)
    near = d == best                                      # one or two candidates
    even = (np.arange(32) % 2 == 0)
    code = np.where(near.sum(-1) == 2, np.argmax(near & even, -1), np.argmax(near, -1))
    return (code | np.where(np.signbit(y), 32, 0)).astype(np.uint8)


def e2m3_decode(c):
    c = np.asarray(c, np.uint8)
    return np.where(c & 32, -E2M3_MAG[c & 31], E2M3_MAG[c & 31])


def scale_exp_for(amax):
    """Biased exponent b (the e8m0 byte) of the smallest power of two 2^(b-127) with amax / 2^(b-127) <= 7.5, clamped to
    [1, 254]; 127 for amax == 0."""
    amax = np.asarray(amax, np.float64)
    with np.errstate(divide="ignore"):
        k = np.ceil(np.log2(np.where(amax > 0, amax, 1.0) / E2M3_MAX)).astype(np.int64)       # a first guess ...
    k = np.where(amax > E2M3_MAX * 2.0 ** k, k + 1, k)                                        # ... corrected exactly:
    k = np.where(amax <= E2M3_MAX * 2.0 ** (k - 1), k - 1, k)                                 # products with 2^k are exact
    b = np.clip(k + 127, 1, 254)
    return np.where(amax == 0, 127, b).astype(np.uint8)


def scale_for(amax):
    return 2.0 ** (scale_exp_for(amax).astype(np.float64) - 127)


def pack(c):
    """codes (..., 128) -> cache bytes (..., 96): four codes are three bytes, little-endian"""
    c = np.asarray(c, np.uint32).reshape(*np.shape(c)[:-1], 32, 4)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return np.stack([w & 255, (w >> 8) & 255, w >> 16], -1).astype(np.uint8).reshape(*c.shape[:-2], 96)


def codes(q):
    """cache bytes (..., 96) -> codes (..., 128), element order"""
    b = np.asarray(q, np.uint8).astype(np.uint32).reshape(*np.shape(q)[:-1], 32, 3)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return np.stack([(w >> (6 * i)) & 63 for i in range(4)], -1).astype(np.uint8).reshape(*b.shape[:-2], 128)


def block_as_int(q24):
    """the definition itself, for the self-check: a block's 24 bytes as one little-endian integer -> its 32 codes"""
    n = int.from_bytes(bytes(bytearray(np.asarray(q24, np.uint8))), "little")
    return np.array([(n >> (6 * j)) & 63 for j in range(32)], np.uint8)


def quantise(x):
    """x: (..., 128) f32 holding bf16 values -> (cache bytes uint8 (..., 96), e8m0 bytes uint8 (..., 4))."""
    x = np.asarray(x, np.float64)
    xb = x.reshape(*x.shape[:-1], 4, 32)
    e = scale_exp_for(np.abs(xb).max(-1))
    y = xb / 2.0 ** (e.astype(np.float64) - 127)[..., None]
    return pack(e2m3_encode(y).reshape(*x.shape[:-1], 128)), e


def dequant(q, e):
    """f64 (exact) value of the cache: e2m3(code) * 2^(byte - 127); (..., 128)."""
    s = 2.0 ** (np.asarray(e, np.uint8).astype(np.float64) - 127)
    return e2m3_decode(codes(q)) * np.repeat(s, 32, axis=-1)


def edge_rows(rng):
    """(n, 128) f32 rows, bf16-representable, built to hit the edges of the format."""
    from oracle.attention_ref import round_bf16
    rows = []
    base = lambda: round_bf16(rng.standard_normal(128).astype(np.float32))
    rows.append(np.zeros(128, np.float32))                               # all zero: byte 127
    z = np.zeros(128, np.float32)
    z[5], z[9], z[10], z[40] = -0.0, 1.0, -0.0, -0.0
    rows.append(z)                                                       # negative zero keeps its sign
    r = base()                                                           # four blocks, four scale bytes: independent
    for blk, top in enumerate((1e-3, 1.0, 100.0, 0.0)):
        seg = r[32 * blk:32 * blk + 32]
        seg *= 0.0 if top == 0 else top / np.abs(seg).max()
    rows.append(r)
    for k in (-20, -3, 0, 1, 9):                                         # one element exactly +-7.5 * 2^k
        for sign in (1.0, -1.0):
            r = np.clip(base(), -2.5, 2.5) * np.float32(2.0 ** k)
            r[17] = sign * 7.5 * 2.0 ** k
            rows.append(r.astype(np.float32))
    for k in (-9, 0, 6):                                                 # amax at 7.5 * 2^k and one bf16 ulp either side, and of 4 and 8
        for top in (7.5, 7.46875, 7.53125, 8.0, 7.96875, 4.0, 3.984375):
            r = np.clip(base(), -2.5, 2.5) * np.float32(2.0 ** k)
            r[3] = top * 2.0 ** k
            r[64 + 3] = -top * 2.0 ** k
            rows.append(r.astype(np.float32))
    ties = list(TIES)                                                    # 31 midpoints: all are bf16 numbers (<= 6 significant bits)
    r = np.zeros(128, np.float32)                                        # amax 7.5 (s = 1): every tie, both signs
    r[0], r[32] = 7.5, -7.5
    r[1:32], r[33:64] = ties, [-t for t in ties]
    r[64], r[96] = 7.5, -7.5                                             # the representable values themselves
    r[65:96], r[97:128] = E2M3_MAG[:31], -E2M3_MAG[:31]
    rows.append(r)
    r = np.zeros(128, np.float32)                                        # just beside the ties (bf16 neighbours)
    r[0], r[32] = 7.5, 7.5
    r[1:32] = [t * (1 + 2.0 ** -7) for t in ties]
    r[33:64] = [-t * (1 - 2.0 ** -8) for t in ties]
    rows.append(r)
    rows.append(np.full(128, 1e-30, np.float32))                         # tiny
    rows.append(np.full(128, 2.0 ** -130, np.float32))                   # below the clamp of the scale
    r = np.full(128, 2.0 ** -126, np.float32)                            # at the clamp: s = 2^-126, values on and between its steps
    r[1::2] = 2.0 ** -128
    r[2::4] = 3 * 2.0 ** -130
    rows.append(r)
    rows.append(np.full(128, 3e38, np.float32))                          # near the top of bf16
    out = round_bf16(np.stack(rows))
    assert np.isfinite(out).all()
    return out
