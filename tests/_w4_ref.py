"""The 4-bit (MXFP4) decode-weight format restated in numpy, from its description (include/lwm_hip.h, "4-bit decode
weights"), not from the kernel.  TEST INFRASTRUCTURE ONLY.

A bf16 kernel W (K, N), K % 32 == 0 and N % 8 == 0, becomes codes uint8 (K/4, N/8, 16) and scale bytes uint8 (K/32, N): per
block of 32 consecutive rows of K of one column, amax = max |w|; s = the smallest power of two with amax / s <= 6, its
exponent byte clamped to [1, 254], byte 127 when amax == 0; q = e2m1(w / s), round to nearest, ties to the even code -- the
rule and the rounding of _kv4_ref.  Slot [k4][n8] of the codes holds rows 4 k4 .. 4 k4 + 3 of columns 8 n8 .. 8 n8 + 7: byte
4 j + b is row 4 k4 + j, column 8 n8 + 2 b in the low nibble and column 8 n8 + 2 b + 1 in the high one."""
import numpy as np

from tests import _kv4_ref as K4

BLOCK = 32


def blocks(K):
    return K // BLOCK


def pack_codes(c):
    """codes (K, N) uint8 in 0..15 -> the byte layout (K/4, N/8, 16)"""
    K, N = c.shape
    pairs = c.reshape(K // 4, 4, N // 8, 4, 2)                      # [k4][j][n8][b][nibble]
    byte = (pairs[..., 0] | (pairs[..., 1] << 4)).astype(np.uint8)
    return np.ascontiguousarray(byte.transpose(0, 2, 1, 3)).reshape(K // 4, N // 8, 16)


def unpack_codes(q, shape):
    """the byte layout (K/4, N/8, 16) -> codes (K, N), written out address by address (the formula of the header)"""
    K, N = shape
    flat = np.asarray(q, np.uint8).reshape(-1)
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    byte = flat[((k >> 2) * (N // 8) + (n >> 3)) * 16 + (k & 3) * 4 + ((n & 7) >> 1)]
    return np.where(n & 1, byte >> 4, byte & 15).astype(np.uint8)


def quantise(w):
    """w: (K, N) f32 holding bf16 values -> (codes uint8 (K/4, N/8, 16), scale bytes uint8 (K/32, N))."""
    w = np.asarray(w, np.float64)
    K, N = w.shape
    assert K % BLOCK == 0 and N % 8 == 0
    wb = w.reshape(K // BLOCK, BLOCK, N)
    e = K4.scale_exp_for(np.abs(wb).max(1))
    y = wb / 2.0 ** (e.astype(np.float64) - 127)[:, None, :]
    return pack_codes(K4.e2m1_encode(y).reshape(K, N)), e


def dequant(q, e, shape):
    """f64 (exact) value of the pack, e2m1(code) * 2^(byte - 127); (K, N)."""
    s = 2.0 ** (np.asarray(e, np.uint8).astype(np.float64) - 127)
    return K4.e2m1_decode(unpack_codes(q, shape)) * np.repeat(s, BLOCK, axis=0)


def rounded(q, e, shape):
    """bf16(e2m1(q) * s) as f32: what the quantiser leaves in the parameter."""
    from oracle.attention_ref import round_bf16
    return round_bf16(dequant(q, e, shape).astype(np.float32))


def quantiser_cases(seed=0):
    """(name, W (K, N) f32 of bf16 values).  Random columns over magnitudes 2^-30 .. 2^20, one magnitude per block; the
    edge rows of _kv4_ref.edge_rows (four blocks of 32 each) as columns: all zero, negative zero, an element exactly
    +-6 * 2^k, amax at the bf16 neighbours of 6 * 2^k -- either side of the 1.5 * 2^e mantissa threshold --, every tie of the
    code, tiny blocks at the lower clamp of the scale, blocks near the top of bf16; and a shape with a ragged column tile."""
    from oracle.attention_ref import round_bf16
    rng = np.random.default_rng(seed)
    out = []
    mags = 2.0 ** rng.uniform(-30, 20, size=(8, 1, 528))
    w = rng.standard_normal((8, 32, 528)) * mags
    out.append(("random_256x528", round_bf16(w.reshape(256, 528).astype(np.float32))))
    edge = K4.edge_rows(rng)                                      # (n, 128): four blocks of one column each
    edge = edge[np.abs(edge).max(1) <= 3.5 * 2.0 ** 126]          # (beyond: e2m1(q) * s leaves bf16 -- unsupported, the header says)
    n = edge.shape[0]
    pad = (-n) % 8
    cols = np.concatenate([edge, round_bf16(rng.standard_normal((pad, 128)).astype(np.float32))])
    out.append((f"edge_128x{n + pad}", np.ascontiguousarray(cols.T)))
    # the same edge blocks as rows 32..159 of a taller matrix, under a block of another magnitude (K = 160: a short last group)
    top = round_bf16((rng.standard_normal((32, n + pad)) * 37.0).astype(np.float32))
    out.append((f"edge_160x{n + pad}", np.concatenate([top, cols.T])))
    # the mantissa threshold itself: amax = 1.5 * 2^e takes s = 2^(e-2), its bf16 successor s = 2^(e-1)
    w = np.zeros((64, 16), np.float32)
    for c, e in enumerate((-100, -20, 0, 1, 40, 100)):
        w[3, c], w[32 + 7, c] = 1.5 * 2.0 ** e, -1.5 * (1 + 2.0 ** -6) * 2.0 ** e
    w[:, 8:] = round_bf16(rng.standard_normal((64, 8)).astype(np.float32))
    w[0:32, 9] = 0.0
    w[5, 9] = -0.0
    w[0:32, 10] = 2.0 ** -127                                     # the lower clamp: s = 2^-126 whatever amax asks for,
    w[4, 10], w[6, 10] = 3.0 * 2.0 ** -126, -(2.0 ** -128)        # and the rounded values 0.5 s and 0 s
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
