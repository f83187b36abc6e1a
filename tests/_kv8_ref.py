"""The 8-bit KV cache format restated in numpy, from its description (include/lwm_hip.h, "8-bit KV cache"),
not from the kernel.  TEST INFRASTRUCTURE ONLY.

Per head of one row (128 bf16 values x): amax = max |x|; s = the smallest power of two with amax / s <= 448,
clamped to [2^-126, 2^127], s = 1 when amax == 0; q = e4m3fn(x / s), round to nearest even."""
import numpy as np

E4M3_MAX = 448.0


def e4m3_table():
    """f32 value of each of the 256 OCP e4m3fn bytes (0x7f, 0xff: NaN)."""
    t = np.empty(256, np.float32)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8) * 2.0 ** (e - 7)
        t[b] = -v if b & 0x80 else v
    return t


def e4m3_decode(q):
    return e4m3_table()[np.asarray(q, np.uint8)]


def e4m3_encode(y):
    """f32 (finite, |y| <= 448) -> e4m3fn byte, round to nearest even.  The spacing of e4m3 values is 2^-9 below
    2^-6 (subnormals) and 2^(floor(log2 |y|) - 3) above; |y| / spacing is exact in f64 and np.rint rounds ties to even --
    an even count is an even mantissa in both ranges."""
    y = np.asarray(y, np.float32)
    a = np.abs(y).astype(np.float64)
    assert np.all(np.isfinite(a)) and np.all(a <= E4M3_MAX)
    _, ex = np.frexp(a)                                   # a = mant * 2^ex, mant in [0.5, 1)
    e = np.maximum(ex - 1, -6)                            # floor(log2 a), held at the subnormal binade
    v = np.rint(a / 2.0 ** (e - 3)) * 2.0 ** (e - 3)      # the nearest representable magnitude
    _, ex = np.frexp(v)
    e = np.maximum(ex - 1, -6)
    n = (v / 2.0 ** (e - 3)).astype(np.int64)             # subnormal: 0..7; normal: 8..15
    byte = np.where(v < 2.0 ** -6, n, ((e + 7) << 3) | (n - 8))
    return (byte | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def scale_for(amax):
    """The smallest power of two s with amax / s <= 448, clamped to [2^-126, 2^127]; 1 for amax == 0."""
    amax = np.asarray(amax, np.float64)
    _, ex = np.frexp(amax)
    k = ex - 1 - 8                                        # 2^8 <= amax / 2^k < 2^9: at most one step short
    k = np.where(amax > E4M3_MAX * 2.0 ** k, k + 1, k)
    k = np.clip(k, -126, 127)
    return np.where(amax == 0, 1.0, 2.0 ** k).astype(np.float32)


def quantise(x):
    """x: (..., 128) f32 holding bf16 values -> (bytes uint8 (..., 128), scales f32 (...))."""
    x = np.asarray(x, np.float32)
    s = scale_for(np.abs(x).max(axis=-1))
    with np.errstate(under="ignore"):
        y = x / s[..., None]
    return e4m3_encode(y), s


def dequant(q, s):
    """f32 (exact) value of the cache: e4m3(q) * s."""
    return e4m3_decode(q) * np.asarray(s, np.float32)[..., None]


def edge_rows(rng):
    """(n, 128) f32 rows, bf16-representable, built to hit the edges of the format."""
    from oracle.attention_ref import round_bf16
    rows = []
    base = lambda: round_bf16(rng.standard_normal(128).astype(np.float32))
    rows.append(np.zeros(128, np.float32))                               # all zero: s = 1
    z = np.zeros(128, np.float32)
    z[5] = -0.0
    z[9] = 1.0
    z[10] = -0.0
    rows.append(z)                                                       # negative zero keeps its sign
    for k in (-20, -3, 0, 1, 9):                                         # one element exactly 448 * 2^k
        r = base() * np.float32(2.0 ** k)
        r = np.clip(r, -400 * 2.0 ** k, 400 * 2.0 ** k).astype(np.float32)
        r[17] = 448.0 * 2.0 ** k
        rows.append(r)
        r = r.copy()
        r[17] = -448.0 * 2.0 ** k
        rows.append(r)
    for k in (-9, 0, 6):                                                 # amax just above / below the boundary at 448 * 2^k
        for top in (448.0, 450.0, 446.0, 512.0, 510.0, 256.0, 255.0):    # (bf16 has 8 significant bits: 450 = 448 + ulp, 446 = 448 - ulp)
            r = (base() * np.float32(2.0 ** k)).astype(np.float32)
            r[3] = top * 2.0 ** k
            rows.append(r)
    # e4m3 subnormals and round-to-even ties: with amax = 256 (s = 1) the values m * 2^-9 are subnormal, (m + 1/2) * 2^-9
    # are ties between them, and 2^-10 is the tie between 0 and the least subnormal
    r = np.zeros(128, np.float32)
    r[0] = 256.0
    for i, m in enumerate(range(0, 17)):
        r[1 + i] = m * 2.0 ** -9
        r[20 + i] = (m + 0.5) * 2.0 ** -9
        r[40 + i] = -(m + 0.5) * 2.0 ** -9
    r[60], r[61], r[62] = 2.0 ** -10, 2.0 ** -11, -(2.0 ** -10)
    for i in range(16):                                                  # ties in a normal binade: 1 + (2i + 1) / 16
        r[64 + i] = 1.0 + (2 * i + 1) / 16.0
        r[80 + i] = -(16.0 + (2 * i + 1))
    r[100], r[101] = 15.5, 31.0                                          # ties that carry into the next binade
    rows.append(r)
    rows.append(np.full(128, 1e-30, np.float32))                         # tiny
    rows.append(np.full(128, 2.0 ** -130, np.float32))                   # below the clamp of the scale
    rows.append(np.full(128, 3e38, np.float32))                          # near the top of bf16
    out = round_bf16(np.stack(rows))
    assert np.array_equal(out[-1], out[-1]) and np.isfinite(out).all()
    return out
