"""The 4-bit (MXFP4) KV cache format restated in numpy, from its description (include/lwm_hip.h, "4-bit KV cache"),
not from the kernel.  TEST INFRASTRUCTURE ONLY.

Per block of 32 consecutive elements of a head (bf16 values x): amax = max |x|; s = the smallest power of two with
amax / s <= 6, its biased exponent clamped to [1, 254], s = 1 when amax == 0; q = e2m1(x / s), round to nearest, ties to
the even code; -0 keeps its sign.  Two codes per byte (element 2i in the low nibble), one e8m0 byte (2^(b - 127)) per block.
Everything here is computed in float64."""
import numpy as np

E2M1_MAX = 6.0
E2M1_MAG = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float64)      # codes 0..7; bit 3 is the sign
TIES = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}       # midpoint -> the even code's value


def e2m1_encode(y):
    """f64 (finite, |y| <= 6) -> e2m1 code 0..15: the nearest magnitude; of two equally near ones the even code."""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    assert np.all(np.isfinite(a)) and np.all(a <= E2M1_MAX)
    d = np.abs(a[..., None] - E2M1_MAG)                   # distances to the 8 magnitudes: exact in f64 for bf16-derived y
    best = d.min(-1, keepdims=True)
    near = d == best                                      # one or two candidates
    even = (np.arange(8) % 2 == 0)
    code = np.where(near.sum(-1) == 2, np.argmax(near & even, -1), np.argmax(near, -1))
    return (code | np.where(np.signbit(y), 8, 0)).astype(np.uint8)


def e2m1_decode(c):
    c = np.asarray(c, np.uint8)
    return np.where(c & 8, -E2M1_MAG[c & 7], E2M1_MAG[c & 7])


def scale_exp_for(amax):
    """Biased exponent b (the e8m0 byte) of the smallest power of two 2^(b-127) with amax / 2^(b-127) <= 6, clamped to
    [1, 254]; 127 for amax == 0."""
    amax = np.asarray(amax, np.float64)
    with np.errstate(divide="ignore"):
        k = np.ceil(np.log2(np.where(amax > 0, amax, 1.0) / E2M1_MAX)).astype(np.int64)       # a first guess ...
    k = np.where(amax > E2M1_MAX * 2.0 ** k, k + 1, k)                                        # ... corrected exactly:
    k = np.where(amax <= E2M1_MAX * 2.0 ** (k - 1), k - 1, k)                                 # products with 2^k are exact
    b = np.clip(k + 127, 1, 254)
    return np.where(amax == 0, 127, b).astype(np.uint8)


def scale_for(amax):
    return 2.0 ** (scale_exp_for(amax).astype(np.float64) - 127)


def quantise(x):
    """x: (..., 128) f32 holding bf16 values -> (nibble bytes uint8 (..., 64), e8m0 bytes uint8 (..., 4))."""
    x = np.asarray(x, np.float64)
    xb = x.reshape(*x.shape[:-1], 4, 32)
    e = scale_exp_for(np.abs(xb).max(-1))
    y = xb / 2.0 ** (e.astype(np.float64) - 127)[..., None]
    c = e2m1_encode(y).reshape(*x.shape[:-1], 64, 2)
    return (c[..., 0] | (c[..., 1] << 4)).astype(np.uint8), e


def codes(q):
    """nibble bytes (..., 64) -> codes (..., 128), element order"""
    q = np.asarray(q, np.uint8)
    return np.stack([q & 15, q >> 4], -1).reshape(*q.shape[:-1], 128)


def dequant(q, e):
    """f64 (exact) value of the cache: e2m1(code) * 2^(byte - 127); (..., 128)."""
    s = 2.0 ** (np.asarray(e, np.uint8).astype(np.float64) - 127)
    return e2m1_decode(codes(q)) * np.repeat(s, 32, axis=-1)


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
    for k in (-20, -3, 0, 1, 9):                                         # one element exactly +-6 * 2^k
        for sign in (1.0, -1.0):
            r = np.clip(base(), -2.5, 2.5) * np.float32(2.0 ** k)
            r[17] = sign * 6.0 * 2.0 ** k
            rows.append(r.astype(np.float32))
    for k in (-9, 0, 6):                                                 # amax at the bf16 neighbours of 6 * 2^k, and of 4 and 8
        for top in (6.0, 5.96875, 6.03125, 8.0, 7.96875, 4.0, 3.984375):
            r = np.clip(base(), -2.5, 2.5) * np.float32(2.0 ** k)
            r[3] = top * 2.0 ** k
            r[64 + 3] = -top * 2.0 ** k
            rows.append(r.astype(np.float32))
    r = np.zeros(128, np.float32)                                        # amax 6 (s = 1): every tie, both signs
    r[0] = 6.0
    for i, t in enumerate(TIES):
        r[1 + i], r[10 + i] = t, -t
    r[20:28] = E2M1_MAG                                                  # and the representable values themselves
    r[32] = -6.0
    for i, t in enumerate(TIES):                                         # just beside the ties (bf16 neighbours)
        r[33 + i], r[42 + i] = t * (1 + 2.0 ** -7), -t * (1 - 2.0 ** -8)
    rows.append(r)
    rows.append(np.full(128, 1e-30, np.float32))                         # tiny
    rows.append(np.full(128, 2.0 ** -130, np.float32))                   # below the clamp of the scale
    rows.append(np.full(128, 3e38, np.float32))                          # near the top of bf16
    out = round_bf16(np.stack(rows))
    assert np.isfinite(out).all()
    return out
