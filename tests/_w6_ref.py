"""The 6-bit (MXFP6 e2m3) decode-weight format restated in numpy, from its description (include/lwm_hip.h, "6-bit decode
weights"), not from the kernel.  TEST INFRASTRUCTURE ONLY.

A bf16 kernel W (K, N), K % 32 == 0 and N % 8 == 0, becomes codes uint8 (K/4, N/8, 24) and scale bytes uint8 (K/32, N): per
block of 32 consecutive rows of K of one column, amax = max |w|; s = the smallest power of two with amax / s <= 7.5, its
exponent byte clamped to [1, 254], byte 127 when amax == 0; q = e2m3(w / s), round to nearest, ties to the even code -- the
codec and the scale rule of _kv6_ref.  Slot [k4][n8] of the codes holds rows 4 k4 .. 4 k4 + 3 of columns 8 n8 .. 8 n8 + 7 as
32 codes: code 8 j + c is row 4 k4 + j, column 8 n8 + c, and code i is bits [6 i, 6 i + 6) of the slot's 24 bytes read as one
little-endian integer."""
import numpy as np

from tests import _kv6_ref as K6

BLOCK = 32
SLOT = 24


def blocks(K):
    return K // BLOCK


def pack_codes(c):
    """codes (K, N) uint8 in 0..63 -> the byte layout (K/4, N/8, 24): four codes are three bytes, little-endian"""
    K, N = c.shape
    slots = c.reshape(K // 4, 4, N // 8, 8).transpose(0, 2, 1, 3).reshape(K // 4, N // 8, 8, 4).astype(np.uint32)   # [k4][n8][t][i]: code 4 t + i
    w = slots[..., 0] | (slots[..., 1] << 6) | (slots[..., 2] << 12) | (slots[..., 3] << 18)
    return np.stack([w & 255, (w >> 8) & 255, w >> 16], -1).astype(np.uint8).reshape(K // 4, N // 8, SLOT)


def unpack_codes(q, shape):
    """the byte layout (K/4, N/8, 24) -> codes (K, N), written out address by address (the formula of the header): W[k][n]
    is code i = 8 (k & 3) + (n & 7) of the slot at byte ((k >> 2) * (N / 8) + (n >> 3)) * 24, bits [6 i, 6 i + 6)"""
    K, N = shape
    flat = np.asarray(q, np.uint8).reshape(-1).astype(np.uint32)
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    base = ((k >> 2) * (N // 8) + (n >> 3)) * SLOT
    bit = 6 * (8 * (k & 3) + (n & 7))
    lo = base + (bit >> 3)
    hi = np.minimum(lo + 1, base + SLOT - 1)               # (the last code ends with its slot: no byte past it is needed)
    return (((flat[lo] | (flat[hi] << 8)) >> (bit & 7)) & 63).astype(np.uint8)


def check_layout(q, shape):
    """the self-check: every slot decoded through the 192-bit-integer definition equals the address formula"""
    K, N = shape
    codes = unpack_codes(q, shape)
    q = np.asarray(q, np.uint8).reshape(K // 4, N // 8, SLOT)
    for k4 in range(K // 4):
        for n8 in range(N // 8):
            want = K6.block_as_int(q[k4, n8]).reshape(4, 8)
            if not np.array_equal(codes[4 * k4:4 * k4 + 4, 8 * n8:8 * n8 + 8], want):
                return False
    return True


def quantise(w):
    """w: (K, N) f32 holding bf16 values -> (codes uint8 (K/4, N/8, 24), scale bytes uint8 (K/32, N))."""
    w = np.asarray(w, np.float64)
    K, N = w.shape
    assert K % BLOCK == 0 and N % 8 == 0
    wb = w.reshape(K // BLOCK, BLOCK, N)
    e = K6.scale_exp_for(np.abs(wb).max(1))
    y = wb / 2.0 ** (e.astype(np.float64) - 127)[:, None, :]
    return pack_codes(K6.e2m3_encode(y).reshape(K, N)), e


def dequant(q, e, shape):
    """f64 (exact) value of the pack, e2m3(code) * 2^(byte - 127); (K, N)."""
    s = 2.0 ** (np.asarray(e, np.uint8).astype(np.float64) - 127)
    return K6.e2m3_decode(unpack_codes(q, shape)) * np.repeat(s, BLOCK, axis=0)


def rounded(q, e, shape):
    """bf16(e2m3(q) * s) as f32: what the quantiser leaves in the parameter."""
    from oracle.attention_ref import round_bf16
    return round_bf16(dequant(q, e, shape).astype(np.float32))


LIMIT = 1.9375 * 2.0 ** 127           # a block whose amax reaches this is unsupported (the header): 3.875 s ties up to 4 s = 2^128


def quantiser_cases(seed=0):
    """(name, W (K, N) f32 of bf16 values): _w4_ref.quantiser_cases with 7.5 in place of 6.  Random columns over magnitudes
    2^-30 .. 2^20, one magnitude per block, in a shape with a ragged column tile (N = 528); the edge rows of
    _kv6_ref.edge_rows (four blocks of 32 each) as columns: all zero, negative zero, an element exactly +-7.5 * 2^k, amax at
    the bf16 neighbours of 7.5 * 2^k, every tie of the code, tiny blocks at the lower clamp of the scale, blocks near the top
    of bf16; the same under another block (K = 160: a short last group); the mantissa threshold 1.875 * 2^e and its bf16
    successor, the lower clamp, and the largest supported amax."""
    from oracle.attention_ref import round_bf16
    rng = np.random.default_rng(seed)
    out = []
    mags = 2.0 ** rng.uniform(-30, 20, size=(8, 1, 528))
    w = rng.standard_normal((8, 32, 528)) * mags
    out.append(("random_256x528", round_bf16(w.reshape(256, 528).astype(np.float32))))
    edge = K6.edge_rows(rng)                                      # (n, 128): four blocks of one column each
    edge = edge[np.abs(edge).max(1) < LIMIT]
    n = edge.shape[0]
    pad = (-n) % 8
    cols = np.concatenate([edge, round_bf16(rng.standard_normal((pad, 128)).astype(np.float32))])
    out.append((f"edge_128x{n + pad}", np.ascontiguousarray(cols.T)))
    top = round_bf16((rng.standard_normal((32, n + pad)) * 37.0).astype(np.float32))
    out.append((f"edge_160x{n + pad}", np.concatenate([top, cols.T])))
    # the mantissa threshold itself: amax = 1.875 * 2^e takes s = 2^(e-2), its bf16 successor (1.875 + 2^-7) * 2^e s = 2^(e-1)
    w = np.zeros((64, 16), np.float32)
    for c, e in enumerate((-100, -20, 0, 1, 40, 100)):
        w[3, c], w[32 + 7, c] = 1.875 * 2.0 ** e, -(1.875 + 2.0 ** -7) * 2.0 ** e
    w[:, 8:] = round_bf16(rng.standard_normal((64, 8)).astype(np.float32))
    w[0:32, 9] = 0.0
    w[5, 9] = -0.0
    w[0:32, 10] = 2.0 ** -127                                     # the lower clamp: s = 2^-126 whatever amax asks for,
    w[4, 10], w[6, 10], w[7, 10] = 3.0 * 2.0 ** -126, -(2.0 ** -131), -(2.0 ** -128)    # and the rounded values 3 s, -0 s, -0.25 s
    w[32:64, 11] = 2.0 ** 120                                     # the top: the largest bf16 below the stated limit, and +-7.5 s
    w[33, 11], w[34, 11], w[35, 11] = (1.9375 - 2.0 ** -7) * 2.0 ** 127, -1.875 * 2.0 ** 127, 1.875 * 2.0 ** 127
    out.append(("threshold_64x16", round_bf16(w)))
    return out


def gemv_case(rows, K, Ns, seed=0):
    """x (rows, K) and one W (K, N) per N, f32 arrays of bf16 values; W's block magnitudes spread over 2^-24 .. 2^24 (the
    scales stay between 2^-40 and 2^40: the exactness domain the header states)"""
    from oracle.attention_ref import round_bf16
    rng = np.random.default_rng(1000 * K + 10 * sum(Ns) + rows + seed)
    x = round_bf16(rng.standard_normal((rows, K)).astype(np.float32))
    ws = []
    for N in Ns:
        mags = 2.0 ** rng.integers(-24, 25, size=(blocks(K), 1, N)).astype(np.float64)
        w = rng.standard_normal((blocks(K), BLOCK, N)) * mags
        ws.append(round_bf16(w.reshape(K, N).astype(np.float32)))
    return x, ws
