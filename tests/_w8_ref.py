"""The 8-bit decode-weight format restated in numpy, from its description (include/lwm_hip.h, "8-bit decode weights"),
not from the kernel.  TEST INFRASTRUCTURE ONLY.

A bf16 kernel W (K, N) becomes q uint8 (K, N) and scale f32 (ceil(K / 128), N): per group of 128 rows of K (the last may
be shorter) and per column, amax = max |w|; s = the smallest power of two with amax / s <= 448, clamped to
[2^-126, 2^127], s = 1 when amax == 0; q = e4m3fn(w / s), round to nearest even -- the rule of _kv8_ref."""
import numpy as np

from tests import _kv8_ref as K8

GROUP = 128


def groups(K):
    return (K + GROUP - 1) // GROUP


def quantise(w):
    """w: (K, N) f32 holding bf16 values -> (bytes uint8 (K, N), scales f32 (ceil(K / 128), N))."""
    w = np.asarray(w, np.float32)
    K, N = w.shape
    q = np.empty((K, N), np.uint8)
    s = np.empty((groups(K), N), np.float32)
    for g in range(groups(K)):
        rows = w[g * GROUP:(g + 1) * GROUP]                     # the rows that exist
        s[g] = K8.scale_for(np.abs(rows).max(axis=0))
        with np.errstate(under="ignore"):
            q[g * GROUP:(g + 1) * GROUP] = K8.e4m3_encode(rows / s[g][None, :])
    return q, s


def dequant(q, s):
    """f32 value of the pack, e4m3(q) * s (exact in f32; a bf16 value wherever it is a normal number)."""
    q = np.asarray(q, np.uint8)
    K = q.shape[0]
    return K8.e4m3_decode(q) * np.repeat(np.asarray(s, np.float32), GROUP, axis=0)[:K]


def rounded(q, s):
    """bf16(e4m3(q) * s) as f32: what the quantiser leaves in the parameter."""
    from oracle.attention_ref import round_bf16
    return round_bf16(dequant(q, s))


def quantiser_cases(seed=0):
    """(name, W (K, N) f32 of bf16 values): random columns over magnitudes 2^-30 .. 2^20; the edge groups of
    _kv8_ref.edge_rows as columns (all zero, negative zero, an element exactly +-448 * 2^k, amax one bf16 ulp either side of
    448 * 2^k, e4m3 subnormals and ties, tiny and huge groups); K = 160: a last group of only 32 rows."""
    from oracle.attention_ref import round_bf16
    rng = np.random.default_rng(seed)
    out = []
    mags = 2.0 ** rng.uniform(-30, 20, size=(2, 1, 528))          # one magnitude per (group, column)
    w = rng.standard_normal((2, 128, 528)) * mags
    out.append(("random_256x528", round_bf16(w.reshape(256, 528).astype(np.float32))))
    edge = K8.edge_rows(rng)                                      # (n, 128): one group of one column each
    n = edge.shape[0]
    pad = (-n) % 16
    cols = np.concatenate([edge, round_bf16(rng.standard_normal((pad, 128)).astype(np.float32))])
    out.append((f"edge_128x{n + pad}", np.ascontiguousarray(cols.T)))
    # the same edge groups as the SECOND group of a taller matrix, below random rows of another magnitude
    top = round_bf16((rng.standard_normal((128, n + pad)) * 37.0).astype(np.float32))
    out.append((f"edge_256x{n + pad}", np.concatenate([top, cols.T])))
    mags = 2.0 ** rng.uniform(-30, 20, size=(1, 48))
    w = round_bf16((rng.standard_normal((160, 48)) * mags).astype(np.float32))
    w[128:, 7] = 0.0                                              # a short group that is all zero
    w[128:, 8] = np.float32(448.0 * 2.0 ** -5) * np.sign(w[128:, 8] + 0.5)
    w[:128, 9] = 0.0                                              # amax of the short group must not leak upwards
    out.append(("short_last_group_160x48", w))
    return out


# the GEMV cases: (K, N) per matrix; scales stay between 2^-40 and 2^40 (the exactness domain the header states)
GEMV_SHAPES = [(32, (16,)), (160, (48,)), (128, (1040,)), (416, (2064,)), (160, (48, 16)), (416, (1040, 16, 2064)),
               (96, (40, 8))]             # (the last: the column unit itself, N % 16 != 0)


def gemv_case(rows, K, Ns, seed=0):
    """x (rows, K) and one W (K, N) per N, f32 arrays of bf16 values; W's column magnitudes spread over 2^-24 .. 2^24"""
    from oracle.attention_ref import round_bf16
    rng = np.random.default_rng(1000 * K + 10 * sum(Ns) + rows + seed)
    x = round_bf16(rng.standard_normal((rows, K)).astype(np.float32))
    ws = []
    for N in Ns:
        mags = 2.0 ** rng.integers(-24, 25, size=(groups(K), 1, N)).astype(np.float64)
        w = rng.standard_normal((groups(K), GROUP, N)) * mags
        ws.append(round_bf16(w.reshape(-1, N)[:K].astype(np.float32)))
    return x, ws
